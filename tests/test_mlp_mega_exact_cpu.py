"""The phase replay of the one-launch MLP step (mlp_mega_exact.py) on its own, without a GPU: the table's premises
(tile counts against the grid, which cases take the multi-tile and multi-pass branches), and the discrimination
controls -- the step's arithmetic emulated on the CPU (fp32 matmuls with K split in four, bf16 hand-offs, fp32
torch.optim) passes the whole replay on every case, and each planted mistake fails it where it was planted."""
import functools

import pytest
import torch

import mlp_mega_exact as mx


def test_table_premises():
    for name, c in mx.CASES.items():
        assert c.B % 32 == 0 and c.feat % 8 == 0 and c.classes <= 16 and len(c.dims) - 1 <= 8, name
        got = mx.Geo(c).reach()
        assert {k: got[k] for k in c.reach} == c.reach, (name, got)
    r = {n: mx.Geo(mx.CASES[n]).reach() for n in mx.CASES}
    # every branch the table claims is taken by some case
    assert r["A"]["multi_fwd"] and r["A"]["multi_dgrad"] and r["A"]["fused"] and r["A"]["passes"] == 2
    assert r["B"]["passes"] == 8 and r["B"]["span"] > 32 and r["B"]["partial"] and r["B"]["fused"]
    assert r["C"]["span"] < 32 and r["C"]["partial"] and not r["C"]["fused"] and mx.CASES["C"].classes == 16
    assert r["D"]["nl"] == 2 and not r["D"]["use_m"]
    assert all(r["E"][k] for k in ("multi_fwd", "multi_dgrad", "multi_grad")) and not r["E"]["fused"]
    assert r["G"]["nl"] == 8
    assert mx.CASES["H3"].grid < 8 and r["H1"]["multi_ce"]
    assert {dict(mx.CASES[n].env).get("PDE_MLP_PRELOAD") for n in mx.CASES} == {None, "0"}
    assert {dict(mx.CASES[n].env).get("PDE_MLP_FUSE") for n in mx.CASES} == {None, "0"}
    # the shape the agreement tests use fits the grid exactly: no later tile
    assert r["A128"]["fwd_tiles"] == mx.NAT and not r["A128"]["multi_fwd"]


def test_geometry_by_hand():
    g = mx.Geo(mx.CASES["E"])
    assert g.grad_tiles == [2 * 13, 2 * 2, 1 * 2] and g.row_tiles(72) == 3 * 5
    assert "row tile 7 (rows 32.., columns 32..), workgroup 7, round 0" in g.row_tile(40, 33)
    assert "row tile 13 (rows 32.., columns 64..), workgroup 5, round 1" in g.row_tile(63, 71)
    assert "gradient tile 25 (outputs 64.., inputs 768.., 1 pass(es)" in g.grad_tile(0)(71, 783)
    assert "workgroup 1, round 3" in g.grad_tile(0)(71, 783)
    assert mx.Geo(mx.CASES["A"]).grad_tiles == [208, 256, 256, 256, 256, 256, 16]


def test_half_ulp():
    v = torch.tensor([0.0, 1.0, 1.5, 1.9999, 2.0, 0.75, 2.0 ** -20], dtype=torch.float64)
    want = torch.tensor([0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -28], dtype=torch.float64)
    assert torch.equal(mx.hulp_bf16(v), want)
    # a correctly rounded value in the lower half of a binade is up to 2^-8 |v| off: more than a flat 2^-9 |v|
    x = torch.tensor(1.0 + 2.0 ** -8 - 2.0 ** -20)
    assert abs(x.bfloat16().double() - x.double()) > 2.0 ** -9 * x.double()


@functools.lru_cache(maxsize=None)
def _last(name, steps):
    """(geo, pre of the last of ``steps`` emulated steps, with its batch)."""
    case = mx.CASES[name]
    geo = mx.Geo(case)
    pre = mx.init_pre(case)
    for s in range(steps):
        pre["x"], pre["y"] = mx.batch(case, s)
        if s == steps - 1:
            return geo, pre
        pre = mx.next_pre(mx.emulate(geo, pre))


@pytest.mark.parametrize("name", list(mx.CASES))
def test_emulated_step_passes(name):
    """Every emulated step of every case stays inside every bound and passes every exact check."""
    steps = 1 if name.startswith("A") else 2
    for rep in mx.emulate_case(mx.CASES[name], steps):
        assert not rep.fails, "\n".join(rep.fails)
        assert all(v <= 1.0 for v in rep.frac.values()), rep.frac
        assert rep.loss_rel <= mx.LOSS_REL


def _broken(name, mut, steps=2):
    geo, pre = _last(name, steps)
    return mx.verify(geo, pre, mx.emulate(geo, pre, mut), steps - 1).fails


def _positive(name, layer, r0, c0, steps=2):
    """The largest element of act[layer + 1] in row r0 at or after column c0 (an element that cancellation left near
    zero is smaller than the accumulation bound of its operands: one bf16 ulp of it cannot be seen, nor matter)."""
    geo, pre = _last(name, steps)
    a = mx.emulate(geo, pre)["act"][layer + 1]
    r0 %= a.shape[0]
    c = c0 + int(a[r0, c0:].float().argmax())
    assert a[r0, c] > 0
    return r0, c


def _differing(name, key, mut):
    """``mut`` moved along its row to the first column b >= mut.b with post[key][layer][a, b] != [a, b + 1]."""
    geo, pre = _last(name, 2)
    row = mx.emulate(geo, pre)[key][mut.layer][mut.a].float()
    b = mut.b + int((row[mut.b:-1] != row[mut.b + 1:]).nonzero()[0])
    return mut._replace(b=b)


@pytest.mark.parametrize("name,layer", [("E", 0), ("E", 1), ("C", 2), ("A128", 3)])
def test_one_act_element_one_ulp_off(name, layer):
    steps = 1 if name.startswith("A") else 2
    r, c = _positive(name, layer, 37, 21, steps)
    f = _broken(name, mx.Mut("ulp", layer, r, c), steps)
    hit = [s for s in f if f"phase F{layer} layer {layer} act[{layer + 1}]: 1 of" in s]
    assert hit and f"first (row {r}, column {c}), 32x16 row tile" in hit[0], f
    # the transposed copy was made from the same value, and nothing downstream is blamed for it
    assert all(f"phase F{layer}" in s for s in f), f


@pytest.mark.parametrize("name,mut,phase", [
    ("E", mx.Mut("swapT", 1, 50, 40), "F0"), ("B", mx.Mut("swapT", 0, 700, 1000), "F0"),
    ("E", mx.Mut("swapdT", 2, 71, 40), "dgrad2"), ("C", mx.Mut("swapdT", 1, 263, 3), "dgrad1")])
def test_two_swapped_elements_in_a_transposed_copy(name, mut, phase):
    mut = _differing(name, "actT" if mut.name == "swapT" else "dT", mut)
    f = _broken(name, mut)
    assert len(f) == 1 and f"phase {phase} " in f[0] and "^T: 2 of" in f[0], f
    assert f"first (row {mut.a}, column {mut.b})" in f[0], f


@pytest.mark.parametrize("name,mut", [
    ("E", mx.Mut("kstep", 0, 32, 64, k=24)),      # the partial last k-step of 784 (16 inputs), the partial column tile
    ("E", mx.Mut("kstep", 1, 64, 16, k=2)),       # the partial k-step of 72
    ("A", mx.Mut("kstep", 2, 128, 1008, k=31)),   # a tile of the second round (tile 319)
    ("G", mx.Mut("kstep", 5, 32, 48, k=1))])
def test_one_lost_k_step_in_one_forward_tile(name, mut):
    f = _broken(name, mut, 1 if name == "A" else 2)
    hit = [s for s in f if f"phase F{mut.layer} layer {mut.layer} act[{mut.layer + 1}]" in s]
    geo = mx.Geo(mx.CASES[name])
    assert hit and geo.row_tile(mut.a, mut.b) in hit[0], f
    assert all(f"phase F{mut.layer}" in s for s in f), f
    if name == "A":
        assert "round 1" in hit[0]


@pytest.mark.parametrize("name,mut", [("A", mx.Mut("pass", 1, 960, 960)), ("A", mx.Mut("pass", 6, 0, 64)),
                                      ("B", mx.Mut("pass", 0, 64, 768)), ("B", mx.Mut("pass", 2, 0, 64))])
def test_second_pass_missing_from_one_gradient_tile(name, mut):
    steps = 1 if name == "A" else 2
    f = _broken(name, mut, steps)
    hit = [s for s in f if f"phase wgrad{mut.layer} layer {mut.layer} weight gradient" in s]
    assert hit and mx.Geo(mx.CASES[name]).grad_tile(mut.layer)(mut.a, mut.b) in hit[0], f
    # the update is replayed from the gradient as stored: only the gradient is blamed
    assert all(f"phase wgrad{mut.layer}" in s for s in f), f


@pytest.mark.parametrize("name,mut", [("A", mx.Mut("bias8", 3, 1000, 152)), ("B", mx.Mut("bias8", 1, 71, 1016)),
                                      ("D", mx.Mut("bias8", 1, 9, 88)), ("C", mx.Mut("bias8", 0, 263, 24))])
def test_eight_batch_columns_missing_from_one_bias_gradient(name, mut):
    f = _broken(name, mut, 1 if name == "A" else 2)
    assert len(f) == 1 and f"phase wgrad{mut.layer} layer {mut.layer} bias gradient: 1 of" in f[0], f
    assert f"first (row {mut.a}, column 0), bias row of 64x64 gradient tile {mut.a // 64} " in f[0], f


@pytest.mark.parametrize("name", ["C", "E", "G"])
def test_ge_for_gt_in_the_relu_mask(name):
    f = _broken(name, mx.Mut("ge"))
    nl = mx.Geo(mx.CASES[name]).nl
    for j in range(1, nl):
        assert any(f"phase dgrad{j} layer {j} d[{j}] = 0 where act[{j}] = 0" in s for s in f), (j, f)
    assert all("phase dgrad" in s for s in f), f


@pytest.mark.parametrize("name", ["B", "D", "H1"])
def test_missing_one_over_b(name):
    f = _broken(name, mx.Mut("noB"))
    nl = mx.Geo(mx.CASES[name]).nl
    hit = [s for s in f if f"phase CE layer {nl - 1} dlog:" in s]
    assert hit and "first (row 0, column 0), 32x16 row tile 0 " in hit[0], f
    assert all("phase CE" in s for s in f), f


@pytest.mark.parametrize("name,row", [("B", 999), ("C", 30), ("H3", 32)])
def test_label_taken_from_the_next_row(name, row):
    case = mx.CASES[name]
    _, pre = _last(name, 2)
    while pre["y"][row] == pre["y"][row + 1]:
        row -= 2
    f = _broken(name, mx.Mut("label", a=row))
    hit = [s for s in f if "phase CE" in s and " dlog: 2 of" in s]
    assert hit and f"first (row {row}, column " in hit[0] and f"row tile {row // 32} " in hit[0], f
    # one wrong row of B moves the mean loss by order 1 / B: far past the loss bound
    assert any("phase CE" in s and "loss:" in s for s in f), f
    assert all("phase CE" in s for s in f) and case.B >= 32, f


@pytest.mark.parametrize("name,mut", [("E", mx.Mut("stale", 1, 64, 64)), ("B", mx.Mut("stale", 2, 0, 64)),
                                      ("A", mx.Mut("stale", 4, 960, 0))])
def test_one_stale_tile_of_the_transposed_weights(name, mut):
    f = _broken(name, mut, 1 if name == "A" else 2)
    assert len(f) == 1 and f"phase update{mut.layer} layer {mut.layer} wtbf[:, :out] = wbf^T" in f[0], f
    assert "transposed copy in " + mx.Geo(mx.CASES[name]).grad_tile(mut.layer)(mut.a, mut.b) in f[0], f


@pytest.mark.parametrize("name", ["B", "E", "G"])
def test_update_with_the_previous_steps_count(name):
    f = _broken(name, mx.Mut("count"))
    nl = mx.Geo(mx.CASES[name]).nl
    for l in range(nl):
        assert any(f"phase update{l} layer {l} weight update" in s for s in f), (l, f)
        assert any(f"phase update{l} layer {l} bias update" in s for s in f), (l, f)
    assert all("phase update" in s for s in f), f
