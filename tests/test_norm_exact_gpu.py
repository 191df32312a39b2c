"""Every BatchNorm dispatch path of csrc/kernels/norm_pool.hip against float64 (norm_exact.py: statistics per
channel, the apply stages per element from the kernel's own statistics, the backward per element).  In process
under the default policy, one test per case -- each asserting from bn_launch_stats the launch form and grid its
table entry names --; then the whole table again in child processes, one per PDE_BN_* policy (the switches are read
once per process), one after another.  Every wait in these kernels is bounded to 2 s and reports through the error
word, so a child that reaches its timeout is a finding: nothing is started after it."""
import json
import os
import subprocess
import sys

import pytest

import norm_exact as nx
from pytorch_distributed_examples_amd.ops import functional as OF

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD_TIMEOUT = 150

_faulted = []  # the first case or child that ended by a GPU error, a signal or its timeout: nothing more is started


def _guard(what, fn):
    if _faulted:
        pytest.skip(f"not started: {_faulted[0]} ended by a GPU error")
    try:
        rep = fn()
        OF.check_device_errors(what)
    except RuntimeError:  # a HIP error is sticky: no further launch in this process, no child behind it
        _faulted.append(f"case {what}")
        raise
    for f in rep.fails:
        print(f)
    print(what, {k: round(v, 3) for k, v in rep.frac.items()})
    assert not rep.fails, "\n".join(rep.fails)


@pytest.mark.parametrize("name", nx.NAMES)
def test_exact(gpu, name):
    _guard(name, lambda: nx.run_case(name, gpu)[0])


@pytest.mark.parametrize("name", list(nx.EVAL_CASES))
def test_eval_apply(gpu, name):
    _guard(name, lambda: nx.run_eval(name, gpu))


# ---- child processes ----------------------------------------------------------------------------------------------


def _child(policy):
    """Run the table in a fresh interpreter under ``policy`` (every inherited PDE_BN_* stripped first); returns the
    child's FRACTIONS record after asserting exit 0 and the OK token with the case count."""
    if _faulted:
        pytest.skip(f"not started: {_faulted[0]} ended by a fault or at its timeout")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PDE_BN_")}
    env.update(policy)
    cmd = [sys.executable, os.path.join(HERE, "norm_exact.py")]
    try:
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT,
                             cwd=os.path.dirname(HERE))
    except subprocess.TimeoutExpired as exc:
        _faulted.append(f"child {policy}")
        err = exc.stderr.decode(errors="replace") if isinstance(exc.stderr, bytes) else (exc.stderr or "")
        pytest.fail(f"child {policy} still running after {CHILD_TIMEOUT} s:\n{err[-3000:]}")
    tail = res.stdout[-6000:] + "\n" + res.stderr[-3000:]
    if res.returncode < 0 or res.returncode in (134, 139, 124, 137):
        _faulted.append(f"child {policy}")
        pytest.fail(f"child {policy} ended with status {res.returncode}:\n{tail}")
    if "DeviceHandoffError" in res.stderr or "HIP error" in res.stderr:
        _faulted.append(f"child {policy}")
    assert res.returncode == 0 and nx.TOKEN in res.stdout, f"child {policy}: status {res.returncode}\n{tail}"
    assert f"{nx.TOKEN} {len(nx.NAMES) + len(nx.EVAL_CASES)}" in res.stdout, res.stdout[-500:]
    line = [l for l in res.stdout.splitlines() if l.startswith("FRACTIONS ")][-1]
    rec = json.loads(line[len("FRACTIONS "):])
    print(policy or "default", rec)
    return rec


POLICIES = {
    "default": {},                                      # the tagged hand-off, <4> / <8> / <0>
    "ticket_flag": {"PDE_BN_TAGGED": "0"},              # ticket + flag, every block finalizing
    "one_finalizer": {"PDE_BN_ALLFIN": "0"},            # one finalizer publishing the coefficients, fence-free
    "fenced": {"PDE_BN_LITE": "0"},                     # one finalizer, release / acquire fences
    "two_launch": {"PDE_BN_FUSED": "0"},                # k_bn_stats_fin / k_bn_bwd_reduce_fin + apply
    "three_pass": {"PDE_BN_3PASS": "1"},                # k_bn_stats / k_bn_finalize / k_bn_apply and the backward's
    "rc16": {"PDE_BN_RC16": "1"},                       # <16> for 9..16 rows per thread
    "streamed": {"PDE_BN_FWD_RC": "0", "PDE_BN_RC8": "0"},  # forward <0> everywhere, backward <4> / <0>
    "plain_stores": {"PDE_BN_WT": "0"},                 # outputs without the write-through stores
    "chunks8": {"PDE_BN_CHUNKS": "8"},                  # at most 8 row chunks: more rows per thread everywhere
    "single_rows": {"PDE_BN_SINGLE_ROWS": "4096"},      # one chunk per channel group up to 4096 rows
    "two_launch_apply_cap": {"PDE_BN_FUSED": "0", "PDE_BN_APPLY_CAP": "2"},  # the grid-stride apply loops
}


@pytest.mark.parametrize("policy", list(POLICIES))
def test_child_policy(gpu, policy):
    """``forms`` is what the Python mirror (norm_exact.plan) says ran.  What the DEVICE side reports is asserted per
    case inside the child by run_case: the exact one_launch / multi_launch deltas and last_grid.  That pins the launch
    form and the grid of every case, PDE_BN_FUSED=0 (multi_launch rises on every case, one_launch on none) and
    PDE_BN_3PASS (a grouped call counts 1 + groups one-launch grids where the one-launch form counts one: a switch
    that was not read fails the four grouped cases).  No counter tells the <4> / <8> / <16> / <0> variants or the
    hand-off protocols (PDE_BN_TAGGED / ALLFIN / LITE / WT) apart: those children prove 'correct under the switch',
    and that the switch is read is known from the source alone."""
    rec = _child(POLICIES[policy])
    forms = set(rec["forms"])
    if policy in ("two_launch", "two_launch_apply_cap"):
        assert forms == {"multi"}, forms
    elif policy == "three_pass":
        assert forms == {"3pass"}, forms
    elif policy == "rc16":
        assert {"one<16><16>", "one<0><0>", "one<8><8>", "one<4><4>", "multi"} == forms, forms
    elif policy == "streamed":
        assert {"one<0><4>", "one<0><0>", "multi"} == forms, forms
    elif policy == "chunks8":
        assert {"one<4><4>", "one<0><0>", "multi"} == forms, forms   # rc8_*: 8 chunks of 5000 rows, 79 per thread
    else:
        assert {"one<4><4>", "one<8><8>", "one<0><0>", "multi"} <= forms, forms
