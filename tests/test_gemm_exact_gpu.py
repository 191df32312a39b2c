"""Every GEMM / implicit-GEMM convolution dispatch path against a float64 reference, bit for bit (gemm_exact.py:
integer-valued bf16 operands, so no accumulation order can round).  In process under the default policy, one test
per case; then the whole table again in child processes, one per dispatch policy -- the switches are read once per
process -- the first of which also checks from PDE_GEMM_LOG that every case took the path its table entry names."""
import os
import subprocess
import sys

import pytest

import gemm_exact as gx
from pytorch_distributed_examples_amd.ops import functional as OF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 120
POLICY_VARS = ("PDE_GEMM_GENERIC", "PDE_GEMM_T128_MIN", "PDE_GEMM_WIDE_MIN", "PDE_GEMM_INKERNEL_SPLITK",
               "PDE_GEMM_SKINNY", "PDE_GEMM_LOWK", "PDE_GEMM_PAIR", "PDE_GEMM_CORE", "PDE_GEMM_DMA_TILE", "PDE_DMA_S64",
               "PDE_GEMM_LOG")


_faulted = []  # the first case or child that ended by a GPU error, a signal or its timeout: nothing more is started


@pytest.mark.parametrize("name", gx.NAMES)
def test_exact(gpu, name):
    if _faulted:
        pytest.skip(f"not started: {_faulted[0]} ended by a GPU error")
    try:
        bad = gx.run_case(name, gpu)
        OF.check_device_errors(name)
    except RuntimeError:  # a HIP error is sticky: no further launch in this process, no child behind it
        _faulted.append(f"case {name}")
        raise
    for m in bad:
        print(m)
    assert not bad, "; ".join(str(m) for m in bad)


# ---- child processes ----------------------------------------------------------------------------------------------


def _child(policy, forced=False, log=False):
    """Run the table (forced: the forced-tile set) in a fresh interpreter under ``policy``; returns its
    CompletedProcess after asserting exit 0 and the OK token."""
    if _faulted:
        pytest.skip(f"not started: {_faulted[0]} ended by a fault or at its timeout")
    env = {k: v for k, v in os.environ.items() if k not in POLICY_VARS}
    env.update(policy)
    if log:
        env["PDE_GEMM_LOG"] = "1"
    cmd = [sys.executable, os.path.join(HERE, "gemm_exact.py")] + (["--forced"] if forced else [])
    try:
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT,
                             cwd=os.path.dirname(HERE))
    except subprocess.TimeoutExpired as exc:
        _faulted.append(f"child {policy}")
        err = exc.stderr.decode(errors="replace") if isinstance(exc.stderr, bytes) else (exc.stderr or "")
        pytest.fail(f"child {policy} still running after {CHILD_TIMEOUT} s:\n{err[-3000:]}")
    tail = res.stdout[-4000:] + "\n" + "\n".join(l for l in res.stderr.splitlines() if not l.startswith("[gemm]"))[-3000:]
    if res.returncode < 0 or res.returncode in (134, 139, 124, 137):
        _faulted.append(f"child {policy}")
        pytest.fail(f"child {policy} ended with status {res.returncode}:\n{tail}")
    assert res.returncode == 0 and gx.TOKEN in res.stdout, f"child {policy}: status {res.returncode}\n{tail}"
    want = len(gx.FORCED_NAMES) if forced else len(gx.NAMES)
    assert f"{gx.TOKEN} {want}" in res.stdout, res.stdout[-500:]
    return res


def test_child_default_policy_takes_the_named_paths(gpu):
    """The default policy with PDE_GEMM_LOG=1: exact, and every case on the path its table entry names (what, tile,
    split or not, slab-lane class) -- what keeps the table honest when the policy is retuned."""
    res = _child({}, log=True)
    log = gx.parse_log(res.stderr)
    errs = []
    for c in gx.CASES:
        errs += gx.path_errors(c, log.get(c.name, []))
    assert not errs, "\n".join(errs)
    whats = {x["what"] for v in log.values() for x in v}
    assert {"single", "skinny", "lowk", "pair.0", "pair.1", "pair-skinny.0", "pair-skinny.1"} <= whats, whats


@pytest.mark.parametrize("policy", [
    {"PDE_GEMM_GENERIC": "1"},
    {"PDE_GEMM_T128_MIN": "1"},
    {"PDE_GEMM_WIDE_MIN": "1"},
    {"PDE_GEMM_INKERNEL_SPLITK": "1"},
    {"PDE_GEMM_SKINNY": "0", "PDE_GEMM_LOWK": "0", "PDE_GEMM_PAIR": "0"},
], ids=["generic", "t128", "wide128x64", "inkernel_splitk", "tile_core_unpaired"])
def test_child_ring_policies(gpu, policy):
    """The ring core's other policies: generic loaders only; the 128x128 tile; the 128x64 tile; the in-launch split-K
    combine; skinny, low-K and pairing off, so the same shapes go through the tile core, unpaired."""
    res = _child(policy, log=True)
    tiles = {x["tile"] for v in gx.parse_log(res.stderr).values() for x in v if x["what"] == "single"}
    whats = {x["what"].split(".")[0] for v in gx.parse_log(res.stderr).values() for x in v}
    if "PDE_GEMM_T128_MIN" in policy:
        assert "128x128" in tiles, tiles
    if "PDE_GEMM_WIDE_MIN" in policy:
        assert "128x64" in tiles, tiles
    if "PDE_GEMM_PAIR" in policy:
        assert whats == {"single"}, whats
    if "PDE_GEMM_GENERIC" in policy:
        assert whats == {"single"}, whats  # no skinny, low-K or paired launch either


@pytest.mark.parametrize("core", ["dma", "hybrid"])
def test_child_dma_core(gpu, core):
    """The LDS-DMA core (every tile-core GEMM) and the hybrid policy (the shapes it measured faster on): exact, and
    the log shows that DMA launches -- and under ``dma`` DMA pairs -- actually ran."""
    res = _child({"PDE_GEMM_CORE": core}, log=True)
    whats = [x["what"] for v in gx.parse_log(res.stderr).values() for x in v]
    assert any(w.startswith("dma.s") for w in whats), sorted(set(whats))
    if core == "dma":
        assert any(w.startswith("dpair") for w in whats), sorted(set(whats))


@pytest.mark.parametrize("policy", [
    {"PDE_GEMM_CORE": "dma", "PDE_GEMM_DMA_TILE": "128x128"},
    {"PDE_GEMM_CORE": "dma", "PDE_GEMM_DMA_TILE": "64x64", "PDE_DMA_S64": "2"},
], ids=["dma128x128", "dma64x64_s2"])
def test_child_dma_forced_tiles(gpu, policy):
    """A forced DMA tile, on the cases with M, N >= 128 (the automatic policy never gives a 128 tile to a smaller
    problem; forcing one there is not a supported configuration)."""
    res = _child(policy, forced=True, log=True)
    dma = [x for v in gx.parse_log(res.stderr).values() for x in v if x["what"].startswith("dma.s")]
    assert dma and all(x["tile"] == policy["PDE_GEMM_DMA_TILE"] for x in dma), dma
    if "PDE_DMA_S64" in policy:
        assert all(x["what"] == "dma.s2" for x in dma), dma
