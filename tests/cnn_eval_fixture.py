"""Shared fixture of the fused-CNN evaluation tests (test_cnn_eval_inputs_cpu.py, test_cnn_eval_gpu.py): a small
trained copy of ``Net`` built in code, two input sets and the mixed-precision reference forward.  Everything here
runs on the CPU in fp32 and is computed once per session."""
import functools

import torch
import torch.nn.functional as F
from torch import nn

MARGIN = 4e-2        # twice the log-probability bound: no in-tolerance error can flip an argmax with this margin
LOGP_ATOL = 2e-2     # log-probabilities between two bf16 paths (test_models_gpu.py: trained-weights eval check)
CAP_SYNTHETIC = 0.01  # share of images under MARGIN the reference itself may have: synthetic test set
CAP_RANDOM = 0.10     # ... random-normal images
N_TEST = 1003


class PlainNet(nn.Module):
    """``models/cnn.py::Net`` in plain torch.nn, layers created in the order conv1, conv2, fc1, fc2."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 10, kernel_size=5)
        self.conv2 = nn.Conv2d(10, 20, kernel_size=5)
        self.fc1 = nn.Linear(320, 50)
        self.fc2 = nn.Linear(50, 10)

    def forward(self, x):  # eval mode: no dropout
        x = F.relu(F.max_pool2d(self.conv1(x), 2))
        x = F.relu(F.max_pool2d(self.conv2(x), 2))
        x = F.relu(self.fc1(x.flatten(1)))
        return F.log_softmax(self.fc2(x), dim=1)


def _bf(t):
    return t.to(torch.bfloat16).float()


@torch.no_grad()
def mixed_reference_logp(sd, x):
    """The mixed-precision forward of test_models_gpu.py::_mixed_reference_loss (no dropout) up to the
    log-probabilities: the input, the conv weights and r1 rounded to bf16, everything else fp32.
    ``sd``: a Net / PlainNet state_dict; CPU fp32."""
    sd = {k: v.detach().float().cpu() for k, v in sd.items()}
    x = x.detach().float().cpu()
    c1 = F.conv2d(_bf(x), _bf(sd["conv1.weight"]), sd["conv1.bias"])
    r1 = _bf(F.relu(F.max_pool2d(c1, 2)))
    c2 = F.conv2d(r1, _bf(sd["conv2.weight"]), sd["conv2.bias"])
    r2 = F.relu(F.max_pool2d(c2, 2)).flatten(1)
    h = F.relu(F.linear(r2, sd["fc1.weight"], sd["fc1.bias"]))
    return F.log_softmax(F.linear(h, sd["fc2.weight"], sd["fc2.bias"]), 1)


def top2_margin(logp):
    top = logp.float().topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


@functools.lru_cache(maxsize=None)
def fixture():
    """``(state_dict, {"synthetic": (x, y), "random": (x, y)})``: 80 steps of fp32 SGD (lr 0.05, batch 256, no
    dropout) on 4096 synthetic digits from ``torch.manual_seed(0)``; the 1003 synthetic test images, and 1003
    random-normal images with the same labels."""
    from pytorch_distributed_examples_amd.data.synthetic import mnist_splits

    torch.manual_seed(0)
    net = PlainNet()
    train, test = mnist_splits(train=4096, test=N_TEST)
    xs, ys = train.images.float().reshape(-1, 1, 28, 28), train.labels.long()
    opt = torch.optim.SGD(net.parameters(), lr=0.05)
    for step in range(80):
        o = (step * 256) % (4096 - 256)
        opt.zero_grad()
        F.nll_loss(net(xs[o:o + 256]), ys[o:o + 256]).backward()
        opt.step()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    xt, yt = test.images.float().reshape(-1, 1, 28, 28).clone(), test.labels.long().clone()
    xr = torch.randn(N_TEST, 1, 28, 28, generator=torch.Generator().manual_seed(1))
    return sd, {"synthetic": (xt, yt), "random": (xr, yt)}


@functools.lru_cache(maxsize=None)
def reference(name):
    """``(logp, argmax, margin)`` of the mixed reference on input set ``name`` (all 1003 images; the forward
    treats images independently, so a test on the first B images takes the first B rows)."""
    sd, sets = fixture()
    logp = mixed_reference_logp(sd, sets[name][0])
    return logp, logp.argmax(1), top2_margin(logp)
