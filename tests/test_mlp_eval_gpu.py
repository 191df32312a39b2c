"""FusedMLPEval.predict / evaluate (k_mlp_eval: the whole Linear + ReLU stack, log-softmax, argmax and the totals in
one launch) against float64 references with bf16 hand-offs, and mlp_eval_pass, the entry scripts' test pass."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 300


def _mlp(hl, feat, gpu):
    from pytorch_distributed_examples_amd.models.mlp import MLP
    from pytorch_distributed_examples_amd.models.mlp_eval import FusedMLPEval

    net = MLP(hl, feat).to(gpu)
    return net, FusedMLPEval(net)


def _layers(net):
    return [net.input_layer, *net.hidden_layers, net.final_layer]


def _reference(ws, bs, x):
    """float64 logits, relu + a bf16 hand-off between layers; also max(|h| . |W|^T + |b|) over the layers."""
    h, top = x.double(), 0.0
    for i, (w, b) in enumerate(zip(ws, bs)):
        top = max(top, (h.abs() @ w.double().abs().T + b.double().abs()).max().item())
        h = h @ w.double().T + b.double()
        if i < len(ws) - 1:
            h = torch.relu(h).float().to(torch.bfloat16).double()
    return h, top


@functools.lru_cache(maxsize=None)
def _integer_fixture(hl, feat):
    """Weights +-1 (hidden layers: 8 non-zeros per row), biases in {-1, 0, 1}, inputs in {0, 1}: every partial sum is
    an integer below 2^24, so fp32 accumulation is exact in any order.  Labels: the reference argmax on about half
    of the rows.  Returns (ws, bs, x, y, reference logits, premise)."""
    g = torch.Generator().manual_seed(0)
    dims = [784] + [feat] * (hl + 1) + [10]
    ws, bs = [], []
    for i in range(len(dims) - 1):
        w = torch.randint(0, 2, (dims[i + 1], dims[i]), generator=g).float() * 2 - 1
        if 0 < i < len(dims) - 2:
            keep = torch.rand(w.shape, generator=g).argsort(1)[:, :8]
            w = torch.zeros_like(w).scatter_(1, keep, w.gather(1, keep))
        ws.append(w)
        bs.append(torch.randint(-1, 2, (dims[i + 1],), generator=g).float())
    x = torch.randint(0, 2, (ROWS, 784), generator=g).float()
    ref, top = _reference(ws, bs, x)
    y = torch.where(torch.rand(ROWS, generator=g) < 0.5, ref.argmax(1), torch.randint(0, 10, (ROWS,), generator=g))
    return ws, bs, x, y, ref, top


def _load(net, ws, bs):
    with torch.no_grad():
        for L, w, b in zip(_layers(net), ws, bs):
            L.weight.copy_(w)
            L.bias.copy_(b)


@pytest.mark.parametrize("B", [1, 31, 32, 33, 100])
@pytest.mark.parametrize("hl,feat", [(0, 1024), (1, 64), (5, 72), (2, 264), (5, 1024)])
def test_exact_on_integers(gpu, hl, feat, B):
    ws, bs, x, y, ref, top = _integer_fixture(hl, feat)
    assert top < 2 ** 24
    net, ev = _mlp(hl, feat, gpu)
    _load(net, ws, bs)
    xg, yg = x[:B].to(gpu), y[:B].to(gpu)
    pred, logits = ev.predict(xg, logits=True)
    assert logits.shape == (B, 10) and logits.dtype == torch.float32 and pred.dtype == torch.int64
    assert torch.equal(logits.cpu().double(), ref[:B])
    assert torch.equal(pred.cpu(), ref[:B].argmax(1))  # ties: the first maximum, the kernel's lowest index
    _, correct, count = ev.evaluate(xg, yg).result()
    assert (correct, count) == (int((ref[:B].argmax(1) == y[:B]).sum()), B)


@pytest.mark.parametrize("B", [33, 300])
@pytest.mark.parametrize("hl,feat", [(5, 1024), (1, 128)])
def test_real_magnitudes(gpu, hl, feat, B):
    """Default-initialised weights, x ~ N(0, 1): logits within the project's bound for two MLP forward paths (atol =
    rtol = 5e-2) of the float64 reference with bf16 operands and hand-offs; logp within 32 x 2^-24 x max(1, max
    |logit|) of float64 log_softmax of the kernel's own logits; loss_sum within B x 2^-24 x |want| of the float64
    sum of -logp[i, y[i]]; a repeat from zeroed stats is bitwise equal and a second call doubles the counts."""
    torch.manual_seed(1)
    net, ev = _mlp(hl, feat, gpu)
    x = torch.randn(B, 784)
    y = torch.randint(0, 10, (B,))
    xg, yg = x.to(gpu), y.to(gpu)
    ws = [L.weight.detach().cpu().to(torch.bfloat16) for L in _layers(net)]
    bs = [L.bias.detach().cpu() for L in _layers(net)]
    ref, _ = _reference(ws, bs, x.to(torch.bfloat16))
    pred, logits, logp = ev.predict(xg, logits=True, logprobs=True)
    lg = logits.cpu().double()
    err = (lg - ref).abs().max().item()
    lerr = (logp.cpu().double() - torch.log_softmax(lg, 1)).abs().max().item()
    lbound = 32 * 2.0 ** -24 * max(1.0, lg.abs().max().item())
    print(f"MLP({hl},{feat}) B={B}: max |logits - reference| = {err:.3e}; max |logp - log_softmax| = {lerr:.3e} "
          f"(bound {lbound:.3e})")
    torch.testing.assert_close(lg, ref, atol=5e-2, rtol=5e-2)
    assert lerr <= lbound
    assert torch.equal(pred, logits.argmax(1))
    stats, logp_e = ev.evaluate(xg, yg, logprobs=True)
    assert torch.equal(logp_e, logp)
    loss_sum, correct, count = stats.result()
    want = float((-logp.cpu().double()[torch.arange(B), y]).sum())
    assert abs(loss_sum - want) <= B * 2.0 ** -24 * abs(want), (loss_sum, want)
    assert (correct, count) == (int((pred.cpu() == y).sum()), B)
    bits = stats.buf.clone()
    ev.evaluate(xg, yg, stats.zero_())
    assert torch.equal(stats.buf, bits)
    ev.evaluate(xg, yg, stats)
    assert stats.result()[1:] == (2 * correct, 2 * B) and int(stats.buf[3]) == 0


def test_sees_training_writes_nothing(gpu):
    """After two eager MegaMLP steps the evaluator reads the weights training wrote (logits bitwise those of a fresh
    model loaded from the state_dict), and evaluate leaves weights, gradients, optimiser state, the device step
    counter and the weight generation as they were."""
    from pytorch_distributed_examples_amd.models.mlp_mega import MegaMLP
    from pytorch_distributed_examples_amd.ops import functional as OF
    from pytorch_distributed_examples_amd.ops.optim import FusedAdam

    torch.manual_seed(2)
    net, ev = _mlp(1, 128, gpu)
    before = ev.predict(torch.ones(32, 784, device=gpu), logits=True)[1]
    opt = FusedAdam(net.parameters(), lr=1e-2)
    mega = MegaMLP(net, opt)
    x, y = torch.randn(32, 784, device=gpu), torch.randint(0, 10, (32,), device=gpu)
    for _ in range(2):
        mega.step(x, y)
    params = list(net.parameters())

    def snapshot():
        step = opt._group_dev(0, opt.param_groups[0], params)["step"]
        state = [v for p in params for v in opt.state[p].values() if torch.is_tensor(v)]
        return [t.clone() for t in [*params, *[p.grad for p in params], *state, step]], OF.weight_generation()

    snap, gen = snapshot()
    _, logits = ev.predict(x, logits=True)
    ev.evaluate(x, y)
    snap2, gen2 = snapshot()
    assert gen2 == gen and len(snap) == len(snap2) and all(torch.equal(a, b) for a, b in zip(snap, snap2))
    fresh, fev = _mlp(1, 128, gpu)
    fresh.load_state_dict(net.state_dict())
    assert torch.equal(logits, fev.predict(x, logits=True)[1])
    assert not torch.equal(ev.predict(torch.ones(32, 784, device=gpu), logits=True)[1], before)  # training moved them


@pytest.mark.parametrize("mode", ["1", "0"])
def test_scripts_pass(gpu, monkeypatch, mode):
    """mlp_eval_pass over a ShardedLoader (batch 128) on the 300-row integer fixture: the reference's (correct, 300)
    on the fused route and, with PDE_MLP_EVAL=0, through the layer path (which returns no loss)."""
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader
    from pytorch_distributed_examples_amd.models import mlp_eval

    class Set:
        def __len__(self):
            return ROWS

    ws, bs, x, y, ref, _ = _integer_fixture(1, 64)
    net, _ = _mlp(1, 64, gpu)
    _load(net, ws, bs)
    ds = Set()
    ds.images, ds.labels = x.to(gpu), y.to(gpu)
    monkeypatch.setenv("PDE_MLP_EVAL", mode)
    calls = []
    evaluate = mlp_eval.FusedMLPEval.evaluate
    monkeypatch.setattr(mlp_eval.FusedMLPEval, "evaluate", lambda *a, **k: calls.append(1) or evaluate(*a, **k))
    correct, total, loss_sum = mlp_eval.mlp_eval_pass(net, ShardedLoader(ds, 128, 1, 0, shuffle=False), gpu)
    assert (correct, total) == (int((ref.argmax(1) == y).sum()), ROWS)
    assert (len(calls) == 1 and loss_sum > 0.0) if mode == "1" else (not calls and loss_sum is None)
