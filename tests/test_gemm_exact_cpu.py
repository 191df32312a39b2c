"""The exact GEMM / conv case table (gemm_exact.py) on its own, without a GPU: the exactness premise of every case,
the bf16 range of every bf16 output, and the discrimination controls -- wrong kernels modelled on the reference
alone must change at least a quarter of the outputs, so a bitwise compare cannot miss them."""
import pytest
import torch

import gemm_exact as gx

QUARTER = 0.25


def differ(a, b):
    return (a != b).double().mean().item()


def test_table_invariants():
    assert len(set(gx.NAMES)) == len(gx.NAMES)
    assert gx.FORCED_NAMES, "the forced-tile children need cases"
    for c in gx.CASES:
        assert c.expect or c.name.startswith("layout_"), c.name
        for e in c.expect:
            if c.forced:
                assert e.M >= 128 and e.N >= 128, (c.name, e)
            if e.lanes == 0:
                assert e.N % 4 != 0, (c.name, e)  # the scalar reduce is the N % 4 != 0 path
            elif e.lanes:
                assert e.N % 4 == 0 and e.lanes in (1, 4, 16), (c.name, e)
    # the forced set keeps ragged edges: some M and N that are no multiple of 128, some K no multiple of 64
    forced = [e for c in gx.CASES if c.forced for e in c.expect]
    assert any(e.M % 128 and e.N % 128 for e in forced) and any(e.K % 64 for e in forced)


@pytest.mark.parametrize("name", gx.NAMES)
def test_case_premise_and_controls(name):
    p = gx.prepare(name)
    assert p.refs and set(p.refs) == set(p.dtypes) == set(p.bounds)
    for k, ref in p.refs.items():
        # exactness premise: every fp32 partial sum, in any order, is an integer below 2^24
        assert p.bounds[k] < gx.EXACT_LIMIT, (k, p.bounds[k])
        vals = p.values[k]
        assert torch.equal(vals, vals.round()), k
        assert vals.abs().max().item() <= p.bounds[k] or p.bounds[k] == 0, k
        if p.dtypes[k] == torch.bfloat16:
            assert vals.abs().max().item() <= gx.BF16_LIMIT, (k, vals.abs().max().item())
            assert torch.equal(ref.to(torch.bfloat16).double(), ref), k  # the bf16 compare loses nothing
        else:
            assert torch.equal(ref.to(p.dtypes[k]).double(), ref), k
    for a, b in p.gemms:
        true = a @ b
        # a kernel that drops the last K group (8 elements)
        assert differ(a[:, :-8] @ b[:-8], true) >= QUARTER, "dropped K tail"
        # a kernel that writes C transposed into the same buffer
        assert differ(true.t().contiguous().view(true.shape), true) >= QUARTER, "transposed C"
    for c in p.convs:
        x, w, dy, st, pd = c["x"], c["w"], c["dy"], c["stride"], c["pad"]
        y, dx, dw = gx.conv_all(x, w, dy, st, pd)
        co, ci, r, s = w.shape
        owned = gx.conv_all(x, torch.ones_like(w), torch.ones_like(dy), st, pd)[1] > 0
        wrong = []
        if s > 1:
            wrong.append(("kw flipped", w.flip(3)))
        if r > 1:
            wrong.append(("kh flipped", w.flip(2)))
        if r > 1 and s > 1:  # k = (kh, kw, c) decomposed with the extents of kh and kw exchanged
            wrong.append(("kh / kw swapped", w.reshape(co, ci, s, r).transpose(2, 3).contiguous()))
        for what, w2 in wrong:
            y2, dx2, _ = gx.conv_all(x, w2, dy, st, pd)
            assert differ(y2, y) >= QUARTER, ("forward gather, " + what)
            # (dx: of the elements some window owns -- all of them at stride 1; at stride 2 up to three quarters
            # of dx get no tap, or the one centre tap, whatever the weights are)
            assert differ(dx2[owned], dx[owned]) >= QUARTER, ("dgrad gather, " + what)
            # the weight gradient read back through the wrong decomposition
            dwr = dw.flip(3) if what == "kw flipped" else (dw.flip(2) if what == "kh flipped" else
                                                           dw.transpose(2, 3).reshape(co, ci, r, s))
            assert differ(dwr, dw) >= QUARTER, ("wgrad gather, " + what)
        # input rows / columns past the last window belong to no window: exactly zero gradient; a dgrad that
        # anchors the windows at the far edge instead (the ownerless rows at the top) is a different result
        h, wd_ = x.shape[2], x.shape[3]
        ho, wo = y.shape[2], y.shape[3]
        last_h, last_w = (ho - 1) * st + r - pd, (wo - 1) * st + s - pd
        if last_h < h:
            assert dx[:, :, last_h:, :].abs().max().item() == 0
        if last_w < wd_:
            assert dx[:, :, :, last_w:].abs().max().item() == 0
        if last_h < h or last_w < wd_:
            far = gx.conv_all(x.flip(2, 3), w.flip(2, 3), dy.flip(2, 3), st, pd)[1].flip(2, 3)
            assert differ(far, dx) >= QUARTER, "windows anchored at the far edge"


def test_ownerless_rows_are_in_the_table():
    """One stride-2 geometry with (H + 2 pad - R) % stride != 0, one with the same in W."""
    g = gx.GEOMS["rows"]
    assert g.stride == 2 and (g.h + 2 * g.pad - g.r) % g.stride != 0
    assert any(G.stride == 2 and (G.w + 2 * G.pad - G.s) % G.stride != 0 for G in gx.GEOMS.values())
    for G in gx.GEOMS.values():
        assert G.h != G.w and G.r != G.s and G.cp != G.ci and G.cop != G.co


def test_log_checker_can_fail():
    """parse_log / path_errors on a synthetic log: the right lines pass; another tile, a missing split, another
    slab-lane class and a missing launch are each reported."""
    case = gx.BY_NAME["wgrad_lanes4"]
    line = "[gemm] single M=70 N=132 K=2048 akind=0 bkind=0 tile={t} tiles=6 split={s} gflop=0.0378\n"
    ok = "[case] other\n[gemm] skinny M=1 N=1 K=1 akind=0 bkind=0 tile=64x32 tiles=1 split=1 gflop=0.0\n" \
         "[case] wgrad_lanes4\n" + line.format(t="64x64", s=8) + "[case] -\n"
    log = gx.parse_log(ok)
    assert set(log) == {"other", "wgrad_lanes4", "-"} and len(log["wgrad_lanes4"]) == 1
    assert gx.path_errors(case, log["wgrad_lanes4"]) == []
    for t, s in (("128x128", 8), ("64x64", 1), ("64x64", 2), ("64x64", 32)):
        bad = gx.parse_log("[case] wgrad_lanes4\n" + line.format(t=t, s=s))
        assert gx.path_errors(case, bad["wgrad_lanes4"]), (t, s)
    assert gx.path_errors(case, log["other"])
    assert [gx.slab_lanes(s) for s in (2, 3, 16, 17, 64)] == [1, 4, 4, 16, 16]


def test_compare_reports_where():
    want = torch.zeros(130, 70, dtype=torch.float64)
    got = want.float().clone()
    assert gx.compare("y", got, want, torch.float32) is None
    got[129, 65] = 3.0
    m = gx.compare("y", got, want, torch.float32)
    assert m.count == 1 and m.first[0][:2] == ((129, 65), (2, 1)) and "tile (2, 1)" in str(m)
    assert gx.compare("y", got.bfloat16(), want, torch.float32) is not None  # the dtype is part of the result
