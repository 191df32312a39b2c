"""FusedCNN.predict / FusedCNN.evaluate (k_cnn_eval: the fused training kernel's forward, eval mode, one launch) on
trained weights: against the mixed-precision reference, against itself, against the training kernel's loss, and
through the entry script.  Fixture and reference: cnn_eval_fixture.py."""
import re

import pytest
import torch

import cnn_eval_fixture as fx

pytestmark = pytest.mark.gpu


def _net(gpu):
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.models.cnn_fused import FusedCNN

    net = Net().to(gpu)
    net.load_state_dict(fx.fixture()[0])
    return net, FusedCNN(net)


@pytest.fixture(scope="module")
def trained(gpu):
    """(net, fused, {name: (x, y) on the GPU}) with the fixture weights; tests that write weights build their own."""
    net, fused = _net(gpu)
    sets = {k: (x.to(gpu), y.to(gpu)) for k, (x, y) in fx.fixture()[1].items()}
    return net, fused, sets


def _batch(label: str) -> int:
    from pytorch_distributed_examples_amd import _native

    n = _native.C().cnn_eval_images_per_workgroup()
    return {"n-1": n - 1, "n": n, "n+1": n + 1}.get(label) or int(label)


@pytest.mark.parametrize("name", ["synthetic", "random"])
@pytest.mark.parametrize("blabel", ["1", "3", "n-1", "n", "n+1", "67", "1003"])
def test_eval_matches_mixed_reference(trained, name, blabel):
    """logp within atol 2e-2 of the mixed reference (measured maximum over all cases on MI355X: 2.9e-6, synthetic
    set at B = 1003; each case prints its own); pred equals the reference argmax wherever the reference's top-2
    margin is at least 4e-2 (twice the bound: no in-tolerance error can flip it), and the excluded share stays within
    the fixture's caps.  Batches around the images-per-workgroup count n cover a full, a partly filled and a
    just-started last workgroup."""
    _, fused, sets = trained
    B = _batch(blabel)
    x, y = sets[name][0][:B], sets[name][1][:B]
    ref_logp, ref_arg, margin = (t[:B] for t in fx.reference(name))
    pred, logp = fused.predict(x, logprobs=True)
    stats, logp_e = fused.evaluate(x, y, logprobs=True)
    assert pred.shape == (B,) and pred.dtype == torch.int64 and logp.shape == (B, 10) and logp.dtype == torch.float32
    assert torch.equal(logp, logp_e)  # predict and evaluate are one kernel
    err = (logp.cpu() - ref_logp).abs().max().item()
    print(f"{name} B={B}: max |logp - reference| = {err:.3e}")
    assert err <= fx.LOGP_ATOL, err
    clear = margin >= fx.MARGIN
    assert torch.equal(pred.cpu()[clear], ref_arg[clear])
    if B == fx.N_TEST:
        cap = fx.CAP_SYNTHETIC if name == "synthetic" else fx.CAP_RANDOM
        assert 1.0 - clear.float().mean().item() <= cap
    assert stats.result()[2] == B


@pytest.mark.parametrize("name", ["synthetic", "random"])
@pytest.mark.parametrize("B", [1, 5, 259, 1003])
def test_eval_self_consistency(trained, name, B):
    """Exact relations between the kernel's own outputs: pred is an argmax of logp, correct counts pred == y, count
    is B, loss_sum is the sum of -logp[i, y[i]] (to the fp32 summation bound B * 2^-24), and a repeated call from
    a zeroed stats reproduces loss_sum bit for bit."""
    _, fused, sets = trained
    x, y = sets[name][0][:B], sets[name][1][:B]
    stats, logp = fused.evaluate(x, y, logprobs=True)
    pred = fused.predict(x)
    loss_sum, correct, count = stats.result()
    idx = torch.arange(B, device=x.device)
    assert torch.equal(logp[idx, pred], logp.max(dim=1).values)
    assert torch.equal(pred, logp.argmax(1))  # argmax: the first maximum, like the kernel's lowest index
    assert correct == int((pred == y).sum().item()) and count == B
    want = float((-logp[idx, y]).double().sum().item())
    assert abs(loss_sum - want) <= B * 2.0 ** -24 * abs(want), (loss_sum, want)
    bits = stats.buf.clone()
    fused.evaluate(x, y, stats.zero_())
    assert torch.equal(stats.buf, bits)
    fused.evaluate(x, y, stats)  # running totals: a second batch adds
    l2, c2, n2 = stats.result()
    assert (c2, n2) == (2 * correct, 2 * B) and abs(l2 - 2 * loss_sum) <= 1e-12 * abs(loss_sum)


@pytest.mark.parametrize("B", [1, 4, 300])
def test_eval_loss_equals_training_kernel_loss(trained, B):
    """Same numbers as k_cnn_train in eval mode: its batch-mean loss equals loss_sum / B to the project's bound for
    two fused paths computing one loss (rtol 1e-4, atol 1e-5); measured difference on MI355X: 0 at all three
    batch sizes (the stages keep the training kernel's accumulation order; printed)."""
    net, fused, sets = trained
    x, y = sets["random"][0][:B], sets["random"][1][:B]
    net.eval()
    loss = fused.forward_backward(x, y)
    loss_sum, _, count = fused.evaluate(x, y).result()
    got = torch.tensor(loss_sum / count, dtype=torch.float32)
    print(f"B={B}: training-kernel loss {loss.item():.9g}, eval loss_sum / B {got.item():.9g}, "
          f"difference {abs(loss.item() - got.item()):.3e}")
    torch.testing.assert_close(got, loss.cpu(), rtol=1e-4, atol=1e-5)


def test_eval_has_no_side_effects(gpu):
    """Three fused training steps (dropout on, fused SGD) with and without evaluate calls in between, from the same
    dropout counter: bitwise-equal weights, equal final counter; evaluate itself changes neither the flat weights
    nor the weight generation."""
    from pytorch_distributed_examples_amd.ops import functional as OF
    from pytorch_distributed_examples_amd.ops.optim import FusedSGD

    sets = fx.fixture()[1]
    x, y = sets["synthetic"][0][:256].to(gpu), sets["synthetic"][1][:256].to(gpu)
    xe, ye = sets["random"][0][:67].to(gpu), sets["random"][1][:67].to(gpu)
    rng = OF._rng_counter(x.device)
    rng0 = rng.clone()
    runs = []
    for with_eval in (False, True):
        rng.copy_(rng0)
        net, fused = _net(gpu)
        net.train()
        opt = FusedSGD(net.parameters(), lr=0.05)
        buf = fused.grad_buffer()
        for _ in range(3):
            fused.forward_backward(x, y, grad_out=buf, sgd=opt)
            if with_eval:
                flat, gen = fused.flat.clone(), OF.weight_generation()
                fused.evaluate(xe, ye)
                fused.predict(xe)
                assert torch.equal(fused.flat, flat) and OF.weight_generation() == gen
                assert net.training  # eval mode is the kernel's, the module is left alone
        torch.cuda.synchronize()
        runs.append((fused.flat.clone(), rng.clone()))
    (w0, r0), (w1, r1) = runs
    assert torch.equal(w0, w1) and torch.equal(r0, r1)
    assert not torch.equal(r0, rng0)  # the training steps did advance the counter


def test_eval_fragment_currency(gpu):
    """evaluate reads the conv weights from the bf16 fragment image, which must be current: after fused SGD steps
    (refreshed by the reduction kernel, no prep launch), after load_state_dict + invalidate(), and with always_prep
    after an in-place write nobody announced -- each time logp matches the mixed reference of the weights the
    module holds now (and those differ from the previous ones by far more than the bound)."""
    from pytorch_distributed_examples_amd.ops import functional as OF
    from pytorch_distributed_examples_amd.ops.optim import FusedSGD

    sets = fx.fixture()[1]
    xc, yc = sets["synthetic"][0][:259], sets["synthetic"][1][:259]
    x, y = xc.to(gpu), yc.to(gpu)
    net, fused = _net(gpu)
    net.train()
    opt = FusedSGD(net.parameters(), lr=0.05)
    buf = fused.grad_buffer()
    ref0 = fx.mixed_reference_logp(net.state_dict(), xc)

    def check(prev):
        ref = fx.mixed_reference_logp(net.state_dict(), xc)
        assert (ref - prev).abs().max().item() > 10 * fx.LOGP_ATOL  # stale fragments would be seen
        _, logp = fused.evaluate(x, y, logprobs=True)
        assert (logp.cpu() - ref).abs().max().item() <= fx.LOGP_ATOL
        return ref

    for _ in range(3):
        fused.forward_backward(x, y, grad_out=buf, sgd=opt)
    assert fused._frag_gen == OF.weight_generation()  # current without a prep launch
    ref1 = check(ref0)
    assert fused._frag_gen == OF.weight_generation()
    net.load_state_dict(fx.fixture()[0])
    fused.invalidate()
    ref2 = check(ref1)
    fused.always_prep = True
    with torch.no_grad():
        net.conv2.weight.mul_(0.5)
        net.conv1.weight.mul_(0.75)
    check(ref2)


def test_eval_in_hipgraph(trained):
    """evaluate over two batches (256 and 259 images) captured into one stats: two replays give bitwise the same
    totals as the same four calls run eagerly from zero (the ticket is reset by the kernel itself)."""
    from pytorch_distributed_examples_amd.models.cnn_fused import CnnEvalStats

    _, fused, sets = trained
    x, y = sets["random"]
    xa, ya, xb, yb = x[:256], y[:256], x[256:515], y[256:515]
    eager = CnnEvalStats(x.device)
    for _ in range(2):
        fused.evaluate(xa, ya, eager)
        fused.evaluate(xb, yb, eager)
    stats = CnnEvalStats(x.device)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(graph):
        fused.evaluate(xa, ya, stats)
        fused.evaluate(xb, yb, stats)
    torch.cuda.current_stream().wait_stream(s)
    stats.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(stats.buf, eager.buf), (stats.result(), eager.result())
    assert stats.result()[2] == 1030 and int(stats.buf[3].item()) == 0


def test_entry_test_pass_runs_fused_eval(gpu, tmp_path, capsys, monkeypatch):
    """apps/mnist_ddp.py --model cnn: the per-epoch test pass through FusedCNN.evaluate (default) and through the
    layer path (PDE_CNN_EVAL=0) print the same lines, and their accuracies differ by no more than the number of
    test images whose layer-path top-2 log-probability margin is under 4e-2 (measured on MI355X: 219 and 217 correct
    of 1003 after this one short epoch, 767 images under the margin; the figures move with the process's dropout seed).

    One epoch on purpose.  The layer pass reads cached bf16 weight copies, which hipGraph replays of the training step
    do not invalidate: from the first replay-only epoch on it scores the weights of the last capture (the same
    command with 4 epochs: 222, 566, 571, 576 correct on the layer path against 223, 568, 867, 903 through
    evaluate, which reads the fp32 weights and the fragment image the training kernels keep current; a layer pass
    repeated after ``bump_weight_generation()`` agrees with evaluate again, 82.55 % against 50.65 % in epoch 3)."""
    from pytorch_distributed_examples_amd.apps import mnist_ddp
    from pytorch_distributed_examples_amd.models import cnn_fused
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.ops import functional as OF

    layer_logp, calls = [], {"evaluate": 0}
    net_forward, evaluate = Net.forward, cnn_fused.FusedCNN.evaluate

    def recording_forward(self, x):
        out = net_forward(self, x)
        if not self.training:
            layer_logp.append(out.detach().float())
        return out

    def counting_evaluate(self, *a, **k):
        calls["evaluate"] += 1
        return evaluate(self, *a, **k)

    monkeypatch.setattr(Net, "forward", recording_forward)
    monkeypatch.setattr(cnn_fused.FusedCNN, "evaluate", counting_evaluate)
    rng = OF._rng_counter(gpu)
    rng0 = rng.clone()
    epochs, correct = 1, {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PDE_CNN_EVAL", mode)
        torch.manual_seed(0)
        rng.copy_(rng0)  # the same dropout stream: both runs train the same weights
        before = calls["evaluate"]
        mnist_ddp.main([str(epochs), str(epochs), "--model", "cnn", "--train_size", "4096", "--test_size", "1003",
                        "--batch_size", "64", "--snapshot_path", str(tmp_path / f"snap{mode}.pt")])
        out = capsys.readouterr().out
        assert out.count("Global test accuracy") == epochs
        accs = [float(v) for v in re.findall(r"Test accuracy: ([0-9.]+)%", out)]
        assert len(accs) == epochs
        correct[mode] = [round(a / 100.0 * 1003) for a in accs]
        ran = calls["evaluate"] - before
        assert (ran > 0 and not layer_logp) if mode == "1" else (ran == 0 and layer_logp), (mode, ran)
    logp = torch.cat(layer_logp).reshape(epochs, 1003, 10)  # the layer path's passes, one per epoch
    near = [int((fx.top2_margin(lp) < fx.MARGIN).sum().item()) for lp in logp]
    print(f"correct per epoch: fused {correct['1']}, layer {correct['0']}; layer-path images under the margin: {near}")
    for cf, cl, n in zip(correct["1"], correct["0"], near):
        assert abs(cf - cl) <= n, (correct, near)
