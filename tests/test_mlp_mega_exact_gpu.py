"""The one-launch MLP training step (``k_mlp_train``, csrc/kernels/mlp_fused.hip) through the phase replay of
mlp_mega_exact.py: every case of its table runs 3 steps (2 for case A) on fresh batches through
``MegaMLP(net, opt).step(x, y)``, each on a fresh MegaMLP (fresh barrier words, one grid per buffer set), and every
step is replayed phase by phase in float64 on the CPU.  The bounds, the exact checks and what each case reaches are
in that module's docstring; the figures measured on an MI355X in profiles/mlp_mega_exact.md.

nl = 1 (``ce_phase<true>``: the cross-entropy phase reading the fp32 images) cannot be reached through MegaMLP -- a
model always has an input and a final layer -- and is left out.
"""
import pytest
import torch

import mlp_mega_exact as mx

pytestmark = pytest.mark.gpu


def _run(name, gpu, monkeypatch):
    case = mx.CASES[name]
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    reps, geo, secs, post = mx.run_case(case, gpu)
    print("\n".join(mx.describe(name, reps, geo, secs)))
    got = geo.reach()
    assert {k: got[k] for k in case.reach} == case.reach, (geo.grid, got)
    fails = [f for rep in reps for f in rep.fails]
    assert not fails, "\n".join(fails)
    assert len(reps) == case.steps and post["t"] == case.steps
    return post


@pytest.mark.parametrize("name", mx.TABLE)
def test_every_phase_of_every_step(gpu, monkeypatch, name):
    _run(name, gpu, monkeypatch)


def test_the_shape_the_agreement_tests_use(gpu, monkeypatch):
    """Case A's model at B = 128 (test_mlp_mega_gpu.py's shape: every phase's tiles fit the grid exactly)."""
    _run("A128", gpu, monkeypatch)


def test_fused_and_read_back_forms_on_partial_tiles(gpu, monkeypatch):
    """Case B's shape (72 wide: partial 64 x 64 tiles, 8 passes) in the fused and in the ``PDE_MLP_FUSE=0`` form: both
    pass the replay, and they agree bit for bit -- loss, gradients, weights, state and both bf16 copies (biases and
    their state to an ulp: the scalar instance of the update may contract differently in the two code paths, as in
    test_mlp_mega_gpu.py's 5 x 1024 comparison)."""
    case = mx.CASES["B"]
    a = _run("B", gpu, monkeypatch)
    nofuse = case._replace(env=(("PDE_MLP_FUSE", "0"),), reach=dict(fused=False, passes=8, span=256, partial=True))
    monkeypatch.setitem(mx.CASES, "B0", nofuse)
    b = _run("B0", gpu, monkeypatch)
    assert a["loss"] == b["loss"]
    for key in ("gw", "gb", "w", "wbf"):
        for l, (ta, tb) in enumerate(zip(a[key], b[key])):
            assert torch.equal(ta, tb), (key, l)
    for l in range(1, len(a["wtbf"])):
        assert torch.equal(a["wtbf"][l], b["wtbf"][l]), l
    for l, (ta, tb) in enumerate(zip(a["b"], b["b"])):
        assert torch.allclose(ta, tb, rtol=1e-5, atol=1e-9), l
    for i, (sa, sb) in enumerate(zip(a["state"], b["state"])):
        for k in sa:
            same = torch.equal(sa[k], sb[k]) if i % 2 == 0 else torch.allclose(sa[k], sb[k], rtol=1e-5, atol=1e-9)
            assert same, (i, k)


@pytest.mark.parametrize("hl,feat,B", [(5, 1024, 160), (5, 72, 96), (2, 264, 32), (1, 64, 288)])
def test_forward_exact_on_integers(gpu, hl, feat, B):
    """The integer fixture of test_mlp_eval_gpu.py (weights +-1, 8 non-zeros per hidden row, inputs in {0, 1}) with
    FusedSGD(lr=0): every partial sum is an integer below 2^24, so every act[l] and actT[l] equals the float64
    reference bit for bit, in any accumulation order."""
    from test_mlp_eval_gpu import _integer_fixture, _load

    ws, bs, x, y, _, _ = _integer_fixture(hl, feat)
    case = mx.Case("I", hl, feat, 10, B, "sgd", dict(lr=0.0), steps=1)
    run = mx.Runner(case, gpu)
    _load(run.net, ws, bs)
    pre, post = run.step(0, (x[:B], y[:B]))
    assert all(torch.equal(w, v) for w, v in zip(pre["w"], ws)) and all(torch.equal(w, v) for w, v in zip(post["w"], ws))
    geo = run.geo()
    rep = mx.Report(geo, 0)
    _, top = mx.replay_forward(geo, pre, post, rep, exact=True)
    assert top < 2 ** 24
    assert not rep.fails, "\n".join(rep.fails)
    assert not any(torch.isnan(t.float()).any() for t in post["act"][1:] + post["actT"])
    assert post["errors"] == 0
