"""The fused CNN update's optimiser policy (fused_update_mode), and the entry scripts' --momentum / --weight_decay
flags, without a GPU."""
import pytest
import torch


def _params():
    return [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]


@pytest.mark.parametrize("kind,kw,mode", [
    ("sgd", dict(lr=0.1), 0),
    ("sgd", dict(lr=0.1, momentum=0.0, weight_decay=0.0), 0),
    ("sgd", dict(lr=0.1, momentum=0.9), 1),
    ("sgd", dict(lr=0.1, weight_decay=1e-2), 1),
    ("sgd", dict(lr=0.1, momentum=0.5, weight_decay=1e-4), 1),
    ("adam", dict(lr=1e-3), 2),
    ("adam", dict(lr=1e-3, weight_decay=1e-2), 2),
    ("adamw", dict(lr=1e-3), 3),
    ("adamw", dict(lr=1e-3, weight_decay=0.0), 3),
])
def test_fused_update_mode(kind, kw, mode):
    from pytorch_distributed_examples_amd.models.cnn_fused import fused_update_mode
    from pytorch_distributed_examples_amd.ops.optim import FusedAdam, FusedAdamW, FusedSGD

    cls = {"sgd": FusedSGD, "adam": FusedAdam, "adamw": FusedAdamW}[kind]
    assert fused_update_mode(cls(_params(), **kw)) == mode
    # two parameter groups: the fused update applies one set of hyper-parameters
    a, b = _params()
    assert fused_update_mode(cls([{"params": [a]}, {"params": [b]}], **kw)) is None


def test_fused_update_mode_rejects_other_optimisers():
    from pytorch_distributed_examples_amd.models.cnn_fused import fused_update_mode

    assert fused_update_mode(torch.optim.SGD(_params(), lr=0.1, momentum=0.9)) is None
    assert fused_update_mode(torch.optim.AdamW(_params(), lr=0.1)) is None
    assert fused_update_mode(None) is None


def test_fused_update_mode_follows_group_changes():
    """The mode is read from the group at call time: momentum switched on later selects the stateful update."""
    from pytorch_distributed_examples_amd.models.cnn_fused import fused_update_mode
    from pytorch_distributed_examples_amd.ops.optim import FusedSGD

    opt = FusedSGD(_params(), lr=0.1)
    assert fused_update_mode(opt) == 0
    opt.param_groups[0]["momentum"] = 0.9
    assert fused_update_mode(opt) == 1


def test_opt_in_reduce_switch(monkeypatch):
    from pytorch_distributed_examples_amd.models.cnn_fused import opt_in_reduce_enabled

    monkeypatch.setenv("PDE_CNN_OPT_IN_REDUCE", "0")
    assert opt_in_reduce_enabled() is False
    monkeypatch.setenv("PDE_CNN_OPT_IN_REDUCE", "1")
    assert opt_in_reduce_enabled() is True


def test_entry_parsers_accept_momentum_and_weight_decay():
    from pytorch_distributed_examples_amd.apps import mnist_ddp, mnist_hvd

    a = mnist_ddp.build_parser().parse_args(["1", "1"])
    assert a.momentum == 0.0 and a.weight_decay == 0.0
    a = mnist_ddp.build_parser().parse_args(["1", "1", "--model", "cnn", "--momentum", "0.9", "--weight_decay", "1e-4"])
    assert a.momentum == 0.9 and a.weight_decay == 1e-4
    h = mnist_hvd.build_parser().parse_args([])
    assert h.momentum == 0.0 and h.weight_decay == 0.0
    h = mnist_hvd.build_parser().parse_args(["--momentum", "0.5", "--weight-decay", "1e-4"])
    assert h.momentum == 0.5 and h.weight_decay == 1e-4


def test_load_train_objs_defaults_to_plain_sgd():
    from pytorch_distributed_examples_amd.apps.mnist_ddp import load_train_objs
    from pytorch_distributed_examples_amd.models.cnn_fused import fused_update_mode

    _, _, model, make_opt, _ = load_train_objs("cnn", torch.device("cpu"), 64, 16)
    g = make_opt(model.parameters()).param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (0.01, 0.0, 0.0)
    _, _, model, make_opt, _ = load_train_objs("cnn", torch.device("cpu"), 64, 16, None, 0.9, 1e-4)
    opt = make_opt(model.parameters())
    assert fused_update_mode(opt) == 1 and opt.param_groups[0]["momentum"] == 0.9


def test_mnist_ddp_cpu_epoch_with_momentum_matches_torch_sgd(tmp_path, monkeypatch):
    """apps/mnist_ddp.py --device cpu --model cnn --momentum 0.9 --weight_decay 1e-4: one epoch, and the trained
    weights match a plain-torch loop with torch.optim.SGD over the same batches (eval-free: Dropout draws from
    torch's generator, seeded the same for both runs)."""
    from pytorch_distributed_examples_amd.apps import mnist_ddp
    from pytorch_distributed_examples_amd.data.loader import ShardedLoader
    from pytorch_distributed_examples_amd.data.mnist import mnist_datasets
    from pytorch_distributed_examples_amd.models.cnn import Net
    from pytorch_distributed_examples_amd.ops import functional as OF

    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        monkeypatch.delenv(k, raising=False)
    snap = tmp_path / "snapshot.pt"
    torch.manual_seed(0)
    mnist_ddp.main(["1", "1", "--device", "cpu", "--model", "cnn", "--momentum", "0.9", "--weight_decay", "1e-4",
                    "--train_size", "256", "--test_size", "64", "--snapshot_path", str(snap)])
    trained = torch.load(str(snap), weights_only=False)
    weights = trained["MODEL_STATE"]
    assert any("momentum_buffer" in s for s in trained["OPTIMIZER_STATE"]["state"].values())
    # the same epoch in plain torch
    torch.manual_seed(0)
    dev = torch.device("cpu")
    train_set, _ = mnist_datasets(dev, 256, 64, None)
    model = Net()
    opt = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    loader = ShardedLoader(train_set, 128, 1, 0, shuffle=True)
    loader.set_epoch(0)
    model.train()
    for x, y in loader:
        opt.zero_grad()
        OF.nll_loss(model(x), y).backward()
        opt.step()
    ref = model.state_dict()
    assert set(ref) == set(weights)
    for k in ref:
        torch.testing.assert_close(weights[k], ref[k], rtol=1e-5, atol=1e-6)
