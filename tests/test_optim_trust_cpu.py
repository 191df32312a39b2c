"""FusedLAMB / FusedLARS on CPU parameters (``_cpu_step``, plain torch in fp32) against the float64 formulas, and
the elastic DDP script with ``--optimizer``."""
import pytest
import torch

from pytorch_distributed_examples_amd.ops.optim import FusedLAMB, FusedLARS
from test_optim_trust_gpu import ref64  # the float64 formulas, shared with the GPU test


@pytest.mark.parametrize("make", [
    lambda ps: FusedLAMB(ps, lr=1e-2, weight_decay=0.1, grad_scale=0.5),
    lambda ps: FusedLAMB(ps, lr=1e-2, weight_decay=0.0),
    lambda ps: FusedLARS(ps, lr=1.0, momentum=0.9, weight_decay=0.1, grad_scale=0.5),
    lambda ps: FusedLARS(ps, lr=1.0, momentum=0.0),
], ids=["lamb", "lamb-wd0", "lars", "lars-mom0"])
def test_cpu_step_follows_float64(make):
    gen = torch.Generator().manual_seed(3)
    ps = [(0.25 * torch.randn(n, generator=gen)).requires_grad_() for n in (5, 4097)] + [torch.zeros(7).requires_grad_()]
    opt = make(ps)
    p64, s64 = [p.detach().double() for p in ps], [{} for _ in ps]
    for t in (1, 2, 3):
        for i, p in enumerate(ps):
            p.grad = torch.randn(p.shape, generator=gen) + 0.1
            p64[i] = ref64(opt.KIND, opt.param_groups[0], p64[i], p.grad.double(), s64[i], t)
        opt.step()
        for i, p in enumerate(ps):
            # fp32 arithmetic on well-scaled values: 1e-5 relative of the tensor's largest value is 100 ulp
            for got, want in [(p, p64[i])] + [(opt.state[p][k], w) for k, w in s64[i].items()]:
                assert (got.detach().double() - want).abs().max() <= 1e-5 * want.abs().max(), (t, i)
            assert set(opt.state[p]) - {"step"} == set(s64[i])


@pytest.mark.parametrize("optimizer", ["lamb", "adam"])
def test_elastic_script_takes_optimizer(optimizer, tmp_path, capsys):
    from pytorch_distributed_examples_amd.apps import mnist_ddp

    mnist_ddp.main(["1", "1", "--optimizer", optimizer, "--device", "cpu", "--train_size", "256", "--test_size", "64",
                    "--snapshot_path", str(tmp_path / "snapshot.pt")])
    out = capsys.readouterr().out
    assert "Epoch 0 | Batchsize: 128 | Steps: 2" in out and "Test accuracy" in out and "Execution time" in out
