"""The fixture of the fused-CNN evaluation tests (cnn_eval_fixture.py) on its own, without a GPU: the mixed-precision
reference must itself leave few images near a tie, or the GPU test's "argmax equals the reference wherever the
reference margin is at least 4e-2" would exclude too much to mean anything."""
import pytest
import torch

import cnn_eval_fixture as fx


@pytest.mark.parametrize("name, cap", [("synthetic", fx.CAP_SYNTHETIC), ("random", fx.CAP_RANDOM)])
def test_reference_margin_share_within_cap(name, cap):
    """Share of images whose reference top-2 log-probability margin is below 4e-2: at most 1 % on the synthetic test
    set and 10 % on random-normal images (this recipe on the CPU: 0 % and 8.1 %; reference accuracy 100 % and about
    10.8 %)."""
    logp, arg, margin = fx.reference(name)
    _, sets = fx.fixture()
    x, y = sets[name]
    assert logp.shape == (fx.N_TEST, 10) and x.shape == (fx.N_TEST, 1, 28, 28)
    assert torch.isfinite(logp).all()
    share = (margin < fx.MARGIN).float().mean().item()
    acc = (arg == y).float().mean().item()
    print(f"{name}: share under margin {share * 100:.2f}%, reference accuracy {acc * 100:.2f}%")
    assert share <= cap, (name, share)
    if name == "synthetic":
        assert acc > 0.95, acc  # the fixture is a trained model: the synthetic set is the meaningful accuracy


def test_reference_rounds_what_the_kernel_rounds():
    """The reference is the MIXED forward: it differs from the plain fp32 forward of the same weights (bf16 operands)
    but stays within the bf16 bound of it, and rounding is applied to the input, the conv weights and r1 only."""
    sd, sets = fx.fixture()
    x = sets["synthetic"][0][:64]
    net = fx.PlainNet()
    net.load_state_dict(sd)
    with torch.no_grad():
        full = net(x)
    mixed = fx.mixed_reference_logp(sd, x)
    d = (full - mixed).abs().max().item()
    assert 0.0 < d < fx.LOGP_ATOL, d
    # bf16-exact operands: the mixed forward of already-rounded inputs and conv weights changes only through r1
    sd_b = dict(sd)
    for k in ("conv1.weight", "conv2.weight"):
        sd_b[k] = sd[k].to(torch.bfloat16).float()
    assert torch.equal(fx.mixed_reference_logp(sd_b, x.to(torch.bfloat16).float()), mixed)
