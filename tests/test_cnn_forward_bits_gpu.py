"""The fused CNN's forward pinned bit for bit (scripts/cnn_forward_bits.py, tests/golden/cnn_forward_bits.json):
k_cnn_eval's log-probabilities, predictions and totals, and k_cnn_train's loss and flat gradient in eval mode and
with dropout, on B = 5 images of the evaluation fixture."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("cnn_forward_bits",
                                                  os.path.join(REPO, "scripts", "cnn_forward_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_forward_bits_equal_recorded(gpu):
    """Every recorded value -- predict's 5 x 10 log-probabilities and predictions, evaluate's stats words, and the
    loss, gradient digest and first 64 gradient values of one training-kernel step in eval mode and one with dropout
    from a fixed counter -- equals the golden file exactly.  The file was recorded from the build before the forward
    became one set of functions shared by k_cnn_train and k_cnn_eval; it is regenerated with
    ``scripts/cnn_forward_bits.py --write`` only by a pull request that changes the numerics on purpose."""
    bits = _script()
    want = bits.load_golden()
    got = bits.forward_bits(gpu)
    assert set(want) == {"batch", "input_set", "rng_counter", "predict", "evaluate", "train_eval", "train_drop"}
    diff = bits.differences(got, want)
    for line in diff:
        print(line)
    assert not diff, f"{len(diff)} value(s) differ from the recorded bits; first: {diff[0]}"
    assert got == want
