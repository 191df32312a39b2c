#!/usr/bin/env python3
"""The fused CNN's forward, bit for bit: k_cnn_eval's outputs and k_cnn_train's loss and gradient on one small
batch, against the values recorded in tests/golden/cnn_forward_bits.json.

    python scripts/cnn_forward_bits.py            # print a comparison with the recorded values
    python scripts/cnn_forward_bits.py --write    # record the current build's values

Inputs: the weights and the first B = 5 "random" images of tests/cnn_eval_fixture.py -- one full workgroup plus one
with a single real image and three empty slots (two workgroups, the clamped image / label addresses, the empty
slots' zeros; B = 4 and B = 1 are subsets).  Recorded:

  predict    FusedCNN.predict(x, logprobs=True): the 5 x 10 log-probabilities (hex float32) and the predictions
  evaluate   FusedCNN.evaluate(x, y): the four int64 words of stats.buf
  train_eval net.eval(), one forward_backward: the loss (hex float32) and the flat gradient (SHA-256 of its float32
             bytes; the first 64 values as hex float32 make a difference readable)
  train_drop net.train() with a freshly constructed FusedCNN, one forward_backward, recorded the same way (the
             dropout masks mc2 / m1 and h1d).  The dropout counter is one per process and device, seeded from
             torch's generator at first use and advanced by every step, so the case runs from RNG_COUNTER and puts
             the process's own value back afterwards.

The file is regenerated (``--write``) only by a change that alters the numerics on purpose; everything else must
reproduce it exactly.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = os.path.join(REPO, "tests", "golden", "cnn_forward_bits.json")
B = 5
RNG_COUNTER = 0x5EED0CAFE  # the dropout counter train_drop starts from (below 2^40, like a seeded one)
HEAD = 64


def _hex32(t):
    """float32 values as 8-digit hex words of their bit patterns."""
    import torch

    words = t.detach().reshape(-1).to(torch.float32).cpu().contiguous().view(torch.int32).tolist()
    return [f"{w & 0xFFFFFFFF:08x}" for w in words]


def _step(fused, x, y):
    import torch

    grads = torch.zeros_like(fused.flat)
    loss = fused.forward_backward(x, y, grad_out=grads)
    torch.cuda.synchronize()
    g = grads.detach().cpu().contiguous()
    return {"loss": _hex32(loss)[0], "grad_numel": g.numel(),
            "grad_sha256": hashlib.sha256(g.numpy().tobytes()).hexdigest(), "grad_head": _hex32(g[:HEAD])}


def forward_bits(device=None) -> dict:
    """The current build's values, in the layout of the golden file."""
    import torch

    import cnn_eval_fixture as fx
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN
    from pytorch_distributed_examples_amd.ops import functional as OF

    dev = torch.device("cuda:0") if device is None else device
    sd, sets = fx.fixture()
    x, y = sets["random"][0][:B].to(dev), sets["random"][1][:B].to(dev)

    def fresh():
        net = Net().to(dev)
        net.load_state_dict(sd)
        return net, FusedCNN(net)

    out = {"batch": B, "input_set": "random", "rng_counter": RNG_COUNTER}
    net, fused = fresh()
    pred, logp = fused.predict(x, logprobs=True)
    out["predict"] = {"logp": [_hex32(row) for row in logp], "pred": pred.cpu().tolist()}
    out["evaluate"] = {"stats_buf": fused.evaluate(x, y).buf.cpu().tolist()}
    net.eval()
    out["train_eval"] = _step(fused, x, y)
    rng = OF._rng_counter(dev)
    saved = rng.clone()
    try:
        rng.fill_(RNG_COUNTER)
        net, fused = fresh()
        net.train()
        out["train_drop"] = _step(fused, x, y)
    finally:
        rng.copy_(saved)
    return out


def load_golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)


def differences(got: dict, want: dict, path: str = "") -> list[str]:
    """One line per leaf that differs."""
    if isinstance(want, dict) and isinstance(got, dict):
        lines = []
        for k in sorted(set(want) | set(got)):
            lines += differences(got.get(k), want.get(k), f"{path}.{k}" if path else k)
        return lines
    if isinstance(want, list) and isinstance(got, list) and len(want) == len(got):
        lines = []
        for i, (g, w) in enumerate(zip(got, want)):
            lines += differences(g, w, f"{path}[{i}]")
        return lines
    return [] if got == want else [f"{path}: recorded {want!r}, now {got!r}"]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", action="store_true", help="record the current build's values in the golden file")
    ap.add_argument("--out", default=GOLDEN, help="with --write: the file to write")
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("cnn_forward_bits: needs a GPU")
    got = forward_bits()
    if args.write:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", args.out)
        return 0
    diff = differences(got, load_golden())
    for line in diff:
        print(line)
    print(f"cnn_forward_bits: {len(diff)} difference(s) from {os.path.relpath(GOLDEN, REPO)}")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
