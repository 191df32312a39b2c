"""The exact BatchNorm case table (norm_exact.py) on its own, without a GPU: the integer regime's premise, the
zero-ambiguity condition of the chosen seeds, the Python geometry against hand-computed grids, and the
discrimination controls -- the kernels' arithmetic emulated on the CPU passes every bound, and each planted mistake
breaks at least one."""
import pytest
import torch

import norm_exact as nx


def test_table_invariants():
    assert len(set(nx.NAMES)) == len(nx.NAMES)
    for c in nx.CASES:
        assert c.C % 8 == 0 and c.shape[0] % c.groups == 0, c
    stems = {n.rsplit("_", 2)[0] for n in nx.NAMES}
    assert stems == {"full", "ragged", "partial_cg", "four_cg", "few_rows", "two_rows", "rc8", "stream_16",
                     "stream_17", "pivot", "grouped", "refused", "refused200"}, stems
    # every code path of the mask: none, recomputed from x, read from y (with dres) -- in both regimes
    for regime in ("int", "rand"):
        assert {(c.res, c.relu) for c in nx.CASES if c.regime == regime} == {(False, False), (False, True),
                                                                              (True, True)}


def test_geometry_against_hand_computed_grids():
    """bn_fin_grid by hand, at a resident cap of 256: (ncg, chunks, rows per chunk, blocks)."""
    assert nx.fin_grid(512, 64) == (1, 8, 64, 8)
    assert nx.fin_grid(1000, 64) == (1, 15, 67, 15)         # 14 x 67 + 62
    assert nx.fin_grid(400, 24) == (1, 6, 67, 6)
    assert nx.fin_grid(162, 200) == (4, 2, 81, 8)
    assert nx.fin_grid(32, 2048) == (32, 1, 32, 32)
    assert nx.fin_grid(2, 64) == (1, 1, 2, 1)
    assert nx.fin_grid(40000, 64) == (1, 128, 313, 128)     # 127 x 313 + 249
    assert nx.fin_grid(4000, 64, cap=4) == (1, 4, 1000, 4)
    assert nx.fin_grid(4100, 64, cap=4) == (1, 4, 1025, 4)
    assert nx.fin_grid(128, 64, groups=4) == (1, 2, 64, 8)
    assert nx.fin_grid(4096, 512, cap=4) == (8, 1, 4096, 8)  # 8 > 4: refused
    assert nx.fin_grid(1000, 64, pol=nx.Policy(chunks=8)) == (1, 8, 125, 8)
    assert nx.fin_grid(4000, 64, pol=nx.Policy(single_rows=4096)) == (1, 1, 4000, 1)
    assert [nx.variants(k)[0] for k in (1, 4, 5, 8, 9, 16, 17)] == ["<4>", "<4>", "<8>", "<8>", "<0>", "<0>", "<0>"]
    rc16 = nx.Policy(rc16=True)
    assert [nx.variants(k, rc16) for k in (16, 17)] == [("<16>", "<16>"), ("<0>", "<0>")]
    assert nx.variants(2, nx.Policy(fwd_rc=False, rc8=False)) == ("<0>", "<4>")
    assert nx.variants(5, nx.Policy(fwd_rc=False, rc8=False)) == ("<0>", "<0>")
    assert nx.blocks_3pass(1000, 64) == (4, 250, 32)


def test_depth_and_launch_counters_against_hand_computed_plans():
    """D = ceil(rpb / 64) + 64 + nrb of the grid that runs, and what one call adds to bn_one_launch's counters."""
    three, two = nx.Policy(threepass=True), nx.Policy(fused=False)
    ragged, grouped, refused = nx.BY_NAME["ragged_r_ra"], nx.BY_NAME["grouped_r_ra"], nx.BY_NAME["refused_r_ra"]
    assert nx.plan(ragged)[2:] == (2 + 64 + 15, 1, 0, 15)
    assert nx.plan(nx.BY_NAME["rc8_r_ra"])[2:] == (5 + 64 + 128, 1, 0, 128)
    assert nx.plan(nx.BY_NAME["stream_17_r_a"])[2:] == (17 + 64 + 4, 1, 0, 4)
    assert nx.plan(grouped)[:2] == ("one", (1, 2, 64, 8)) and nx.plan(grouped)[2:] == (1 + 64 + 2, 1, 0, 8)
    # refused: no resident block is left, one chunk of all 1000 rows, the call counts as multi-launch
    assert nx.plan(refused) == ("multi", (1, 1, 1000, 1), 16 + 64 + 1, 0, 1, 0)
    # PDE_BN_FUSED=0: the grouped call and each of its four per-group calls count as multi-launch
    assert nx.plan(ragged, pol=two) == ("multi", (1, 15, 67, 15), 81, 0, 1, 0)
    assert nx.plan(grouped, pol=two) == ("multi", (1, 2, 64, 2), 67, 0, 5, 0)
    # PDE_BN_3PASS: counted as one-launch before the ticket window is refused; grouped: 1 + 4 calls, the last grid
    # is a single group's.  D: ragged 4 blocks of 250 rows, 32 rows per trip: 8 + 32 + 1 + 6; grouped (128 rows per
    # group) 1 block: 4 + 32 + 1 + 6
    assert nx.plan(ragged, pol=three) == ("3pass", (1, 15, 67, 15), 47, 1, 0, 15)
    assert nx.plan(grouped, pol=three) == ("3pass", (1, 2, 64, 8), 43, 5, 0, 2)
    assert nx.plan(refused, pol=three)[3:] == (0, 1, 0)


@pytest.mark.parametrize("name", nx.NAMES)
def test_case_plan_premise_and_ambiguity(name):
    c = nx.BY_NAME[name]
    pl = nx.plan(c)
    assert pl.form == c.form, pl
    if pl.form == "one":
        assert nx.variants(pl.grid.rows_per_thread) == (c.variant, c.variant), pl
    if name.startswith("stream_"):
        assert pl.grid.nrb == 4 and pl.grid.rows_per_thread == int(name[7:9]), pl
    r = nx.reference(name)
    if c.regime == "int":
        for t in (r.x, r.dy) + ((r.res,) if c.res else ()):
            assert torch.equal(t, t.round()) and torch.equal(t.bfloat16().double(), t)
        assert r.premise < nx.EXACT_LIMIT, r.premise
        assert r.dy.abs().sum((0, 1)).max().item() < nx.EXACT_LIMIT
        assert torch.equal(r.x[:, 0, :], r.x0) and (c.pivot == 0 or r.x0.abs().max().item() >= c.pivot - c.lim)
    assert nx.ambiguous(r) == 0, "choose another seed for this case"


@pytest.mark.parametrize("name", nx.NAMES)
def test_emulated_kernel_passes(name):
    """The kernels' arithmetic in fp32 torch stays inside every bound under the default plan."""
    pl = nx.plan(nx.BY_NAME[name])
    rep = nx.verify(name, nx.emulate(name), pl)
    assert not rep.fails, "\n".join(rep.fails)
    assert all(v <= 1.0 for k, v in rep.frac.items() if k != "rsqrt_u"), rep.frac


def _broken(name, **kw):
    pl = nx.plan(nx.BY_NAME[name])
    return nx.verify(name, nx.emulate(name, pl=pl, **kw), pl).fails


@pytest.mark.parametrize("name", ["ragged_i_a", "ragged_r_a", "ragged_r_ra", "pivot_i_ra"])
def test_one_row_lost_or_counted_twice_breaks_a_bound(name):
    c = nx.BY_NAME[name]
    rpb = nx.plan(c).grid.rpb
    assert rpb == 67
    for row in (rpb - 1, rpb, c.P - 1):
        f = _broken(name, mut="drop", row=row)
        assert any(s.startswith(("save_mean", "save_invstd")) for s in f), (row, f)
        f = _broken(name, mut="twice", row=row)
        assert any(s.startswith(("save_mean", "save_invstd")) for s in f), (row, f)
    # Row 0 is the pivot: its shifted terms x[0] - x[0] are zero, so a statistics pass that leaves it out forms the
    # same sums -- there is nothing to see and nothing wrong.  The same lost row in the apply pass is seen by check 2.
    assert not _broken(name, mut="drop", row=0)
    f = _broken(name, mut="unwritten", row=0)
    assert any(s.startswith("y:") for s in f) and "row chunk 0" in " ".join(f), f


@pytest.mark.parametrize("name", ["ragged_i_ra", "ragged_r_p", "rc8_i_a", "grouped_r_a"])
def test_biased_running_var_breaks_a_bound(name):
    f = _broken(name, mut="biased")
    assert any(s.startswith("running_var") for s in f), f
    assert not any(s.startswith(("save_", "y", "dx", "running_mean")) for s in f), f


@pytest.mark.parametrize("name", ["grouped_i_a", "grouped_r_ra"])
def test_reversed_group_updates_break_a_bound(name):
    f = _broken(name, mut="reverse")
    assert any(s.startswith("running_mean") for s in f) and any(s.startswith("running_var") for s in f), f


@pytest.mark.parametrize("name", ["ragged_i_a", "ragged_r_ra", "four_cg_i_ra"])
def test_swapped_lanes_break_the_y_bound_and_are_located(name):
    c = nx.BY_NAME[name]
    rpb = nx.plan(c).grid.rpb
    f = _broken(name, mut="lanes", row=rpb)          # within row chunk 1
    y = [s for s in f if s.startswith("y:")]
    assert y and f"first (row {rpb}, " in y[0] and "row chunk 1, channel group 0, lane 0" in y[0], f


@pytest.mark.parametrize("name", ["full_i_ra", "ragged_i_ra", "grouped_i_ra"])
def test_ge_for_gt_in_the_relu_mask_breaks_dres(name):
    """Integer data with a residual: the clamped outputs are exact zeros, which ``>=`` lets through."""
    r = nx.reference(name)
    y = nx.emulate(name)["y"]
    assert (y == 0).sum().item() > r.x.numel() // 10
    f = _broken(name, mut="ge")
    assert any(s.startswith("dres") for s in f), f


def test_report_says_where():
    name = "ragged_r_ra"
    pl = nx.plan(nx.BY_NAME[name])
    out = nx.emulate(name)
    out["y"][500, 37] += 1.0
    f = nx.verify(name, out, pl).fails
    assert any(s.startswith("y: 1 of 64000 elements") and "(row 500, channel 37)" in s and "row chunk 7" in s
               and "lane 4" in s for s in f), f
    out = nx.emulate(name)
    out["dx"][999, 63] = float("nan")
    f = nx.verify(name, out, pl).fails
    assert len(f) == 1, f
    assert any(s.startswith("dx:") and "(row 999, channel 63)" in s and "row chunk 14" in s for s in f), f
    out = nx.emulate(name)
    out["dgamma"][5] += 1.0   # (also the t2 of the dx reference: channel 5 of every row)
    f = nx.verify(name, out, pl).fails
    assert any(s.startswith("dgamma: 1 of 64 channels") and "channel 5 " in s for s in f), f
    assert any(s.startswith("dx: ") and "(row 0, channel 5)" in s for s in f), f
