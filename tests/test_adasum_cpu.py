"""hvd.Adasum on the CPU plane: the fp64 tree (hvd/adasum.py) on analytic cases, its Gram-weight form, and the
Horovod API over gloo at worlds 2 and 4 -- allreduce, tensors fused in one cycle (per-tensor coefficients),
grouped_allreduce and DistributedOptimizer's delta semantics against a one-process emulation of the ranks."""
import pytest
import torch

from adasum_fixture import assert_not_sum_or_average, rank_data, reference
from dist_utils import spawn


def _adasum():
    from pytorch_distributed_examples_amd.hvd import adasum

    return adasum


@pytest.mark.parametrize("n_ranks", [2, 4, 8])
def test_identical_vectors_give_that_vector(n_ranks):
    v = rank_data(0, 100, 1).double()
    out = _adasum().adasum_tree([v.clone() for _ in range(n_ranks)])
    assert torch.allclose(out, v, rtol=1e-14, atol=0)


@pytest.mark.parametrize("n_ranks", [2, 4, 8])
def test_disjoint_supports_give_the_exact_sum(n_ranks):
    xs = []
    for r in range(n_ranks):
        x = torch.zeros(16 * n_ranks, dtype=torch.float64)
        x[16 * r:16 * (r + 1)] = rank_data(r, 16, 2).double()
        xs.append(x)
    assert torch.equal(_adasum().adasum_tree(xs), sum(xs))


@pytest.mark.parametrize("zero_rank", [0, 1, 3])
def test_zero_vector_is_ignored(zero_rank):
    xs = [rank_data(r, 50, 3) for r in range(4)]
    others = [x for r, x in enumerate(xs) if r != zero_rank]
    xs[zero_rank] = torch.zeros(50)
    out = _adasum().adasum_tree(xs)
    assert torch.isfinite(out).all()
    # the zero vector's partner passes through its pair unchanged: the tree of the other three, paired the same way
    a = _adasum()
    if zero_rank < 2:
        want = a.adasum_pair(others[0], a.adasum_pair(others[1], others[2]))
    else:
        want = a.adasum_pair(a.adasum_pair(others[0], others[1]), others[2])
    assert torch.allclose(out, want, rtol=1e-13, atol=0)
    assert torch.isfinite(a.adasum_tree([torch.zeros(5)] * 4)).all()


@pytest.mark.parametrize("n_ranks", [2, 4, 8])
def test_gram_weight_form_equals_the_tree(n_ranks):
    a = _adasum()
    xs = [rank_data(r, 1000, 4).double() for r in range(n_ranks)]
    X = torch.stack(xs)
    w = a.adasum_weights(X @ X.T)
    ref = a.adasum_tree(xs)
    assert_not_sum_or_average(xs, ref)
    assert torch.allclose((w[:, None] * X).sum(0), ref, rtol=1e-12, atol=1e-14)


def test_tree_needs_a_power_of_two():
    with pytest.raises(ValueError):
        _adasum().adasum_tree([torch.ones(3)] * 3)


# ---- the Horovod API over gloo ------------------------------------------------------------------------------
def _api_worker(rank, world):
    import os

    from pytorch_distributed_examples_amd import hvd

    os.environ["HOROVOD_CYCLE_TIME"] = "20"  # ms: the enqueues of one burst land in one negotiation cycle
    hvd.init(device="cpu")
    # one tensor, with pre/post scales (a uniform scale passes straight through)
    xs = [rank_data(r, 1000, 10) for r in range(world)]
    ref = reference(xs, [1000])
    assert_not_sum_or_average(xs, ref)
    out = hvd.allreduce(xs[rank], op=hvd.Adasum, name="one")
    assert out.dtype == torch.float32 and torch.allclose(out.double(), ref, rtol=1e-6, atol=1e-7)
    out = hvd.allreduce(xs[rank], op=hvd.Adasum, name="scaled", prescale_factor=0.5, postscale_factor=3.0)
    assert torch.allclose(out.double(), 1.5 * ref, rtol=1e-6, atol=1e-7)
    t = xs[rank].clone()
    hvd.allreduce_(t, op=hvd.Adasum, name="inplace")
    assert torch.allclose(t.double(), ref, rtol=1e-6, atol=1e-7)
    # several named tensors fused in ONE cycle, with different correlations: the coefficients are per tensor, not
    # over the fused buffer (a whole-buffer tree gives another result, checked on the reference)
    noises = [0.1, 0.5, 2.0]
    sizes = [300, 40, 700]
    ts = [[rank_data(r, n, 20 + i, noise=z) for i, (n, z) in enumerate(zip(sizes, noises))] for r in range(world)]
    fused = [torch.cat(t) for t in ts]
    want = reference(fused, sizes)
    whole = reference(fused, [sum(sizes)])
    assert float((want - whole).norm() / want.norm()) > 0.05
    before = hvd.engine_stats()["fused_requests"]
    hs = [hvd.allreduce_async(t, name=f"fused.{i}", op=hvd.Adasum) for i, t in enumerate(ts[rank])]
    got = torch.cat([hvd.synchronize(h) for h in hs])
    assert hvd.engine_stats()["fused_requests"] >= before + 2  # (they shared a batch)
    assert torch.allclose(got.double(), want, rtol=1e-6, atol=1e-7)
    outs = hvd.grouped_allreduce(ts[rank], name="grouped", op=hvd.Adasum)
    assert torch.allclose(torch.cat(outs).double(), want, rtol=1e-6, atol=1e-7)
    # every rank holds the same bits
    both = hvd.allgather(got[None])
    assert all(torch.equal(both[0], both[r]) for r in range(world))
    # compression with Adasum raises, here and in the optimizer
    with pytest.raises(ValueError):
        hvd.allreduce(xs[rank], op=hvd.Adasum, compression=hvd.Compression.bf16)
    with pytest.raises(ValueError):
        hvd.allreduce_async_(xs[rank].clone(), op=hvd.Adasum, compression_bf16=True)
    m = torch.nn.Linear(4, 2)
    with pytest.raises(ValueError):
        hvd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.1), op=hvd.Adasum,
                                 compression=hvd.Compression.fp16)
    hvd.shutdown()


@pytest.mark.parametrize("world", [2, 4])
def test_adasum_api_gloo(world):
    spawn(_api_worker, world)


def _model(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(12, 16), torch.nn.Tanh(), torch.nn.Linear(16, 3))


def _batch(rank, step):
    """The ranks' batches share most of their content, so their gradients (and weight deltas) are correlated."""
    c = torch.Generator().manual_seed(100 + step)
    g = torch.Generator().manual_seed(1000 + 10 * step + rank)
    return (torch.randn(8, 12, generator=c) + 0.3 * torch.randn(8, 12, generator=g),
            torch.randn(8, 3, generator=c) + 0.3 * torch.randn(8, 3, generator=g))


def _optimizer_worker(rank, world):
    from pytorch_distributed_examples_amd import hvd
    from pytorch_distributed_examples_amd.hvd import adasum

    hvd.init(device="cpu")
    m = _model(0)
    opt = hvd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9),
                                   named_parameters=m.named_parameters(), op=hvd.Adasum)
    assert not opt._hooks  # delta semantics: no gradient hooks
    # one-process emulation of every rank: local steps from the shared weights, then the fp64 tree of the deltas
    replicas = [_model(0) for _ in range(world)]
    ropts = [torch.optim.SGD(r.parameters(), lr=0.05, momentum=0.9) for r in replicas]
    for step in range(3):
        x, y = _batch(rank, step)
        opt.zero_grad()
        torch.nn.functional.mse_loss(m(x), y).backward()
        opt.step()
        start = [p.detach().clone() for p in replicas[0].parameters()]
        for r, (rep, ro) in enumerate(zip(replicas, ropts)):
            xr, yr = _batch(r, step)
            ro.zero_grad()
            torch.nn.functional.mse_loss(rep(xr), yr).backward()
            ro.step()
        with torch.no_grad():
            for k, s in enumerate(start):
                ps = [list(rep.parameters())[k] for rep in replicas]
                deltas = [(p - s).reshape(-1) for p in ps]
                new = s + adasum.adasum_tree(deltas).view_as(s).float()
                if step == 0 and s.dim() == 2:
                    assert_not_sum_or_average(deltas, adasum.adasum_tree(deltas))
                for p in ps:
                    p.copy_(new)
        for p, q in zip(m.parameters(), replicas[0].parameters()):
            assert torch.allclose(p, q, rtol=1e-5, atol=1e-7), (step, (p - q).abs().max())
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    every = hvd.allgather(flat[None])
    assert all(torch.equal(every[0], every[r]) for r in range(world))
    hvd.shutdown()


def test_adasum_distributed_optimizer_gloo():
    spawn(_optimizer_worker, 2)


def _world3_worker(rank, world):
    from pytorch_distributed_examples_amd import hvd

    hvd.init(device="cpu")
    with pytest.raises(ValueError):
        hvd.allreduce(torch.ones(4), op=hvd.Adasum)
    with pytest.raises(ValueError):
        hvd.allreduce_async_(torch.ones(4), op=hvd.Adasum)
    m = torch.nn.Linear(4, 2)
    with pytest.raises(ValueError):
        hvd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.1), op=hvd.Adasum)
    assert torch.allclose(hvd.allreduce(torch.ones(4), op=hvd.Sum), torch.full((4,), 3.0))  # the engine is intact
    hvd.shutdown()


def test_adasum_world3_raises():
    spawn(_world3_worker, 3)


def _world1_worker(rank, world):
    from pytorch_distributed_examples_amd import hvd

    hvd.init(device="cpu")
    x = rank_data(0, 33, 7)
    out = hvd.allreduce(x, op=hvd.Adasum, prescale_factor=0.5, postscale_factor=3.0)
    assert torch.allclose(out, 1.5 * x, rtol=1e-6)
    m = _model(1)
    ref = _model(1)
    opt = hvd.DistributedOptimizer(torch.optim.SGD(m.parameters(), lr=0.1), op=hvd.Adasum)
    ropt = torch.optim.SGD(ref.parameters(), lr=0.1)
    x, y = _batch(0, 0)
    for mod, o in ((m, opt), (ref, ropt)):
        o.zero_grad()
        torch.nn.functional.mse_loss(mod(x), y).backward()
        o.step()
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), ref.parameters()))
    hvd.shutdown()


def test_adasum_world1_is_the_scale():
    spawn(_world1_worker, 1)  # (its own process: the rendezvous must not outlive the test in this one)
