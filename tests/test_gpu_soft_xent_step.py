"""Soft targets through the training step: ``CrossEntropyLoss(label_smoothing=)`` on a ``MixedTarget`` behind the
native ResNet's logits -- the one-launch loss, the cross-entropy backward fused into the head backward (option
xent_fuse) against the separate launch, graph replay against eager, the direct NativeLoss chain against the
autograd path, the reduction to today's index-label step, and DataParallel's gathered logits."""
from importlib import import_module

import numpy as np
import pytest
import torch

from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

B = 8


def _setup(dtc, cuda, batch=B, seed=16):
    """The existing step tests' model and batch (torch seed 42, numpy seed `seed`) plus a second label array and
    a per-row lam that includes the exact end points and one row whose two labels coincide."""
    torch.manual_seed(42)
    model = dtc.ResNet18().to(cuda)
    g = np.random.default_rng(seed)
    x = torch.from_numpy(g.standard_normal((batch, 3, 32, 32)).astype(np.float32)).to(cuda)
    ya = g.integers(0, 100, batch)
    yb = g.integers(0, 100, batch)
    yb[batch - 1] = ya[batch - 1]
    lam = g.random(batch).astype(np.float32)
    lam[0], lam[1] = 1.0, 0.0
    t = dtc.MixedTarget(torch.from_numpy(ya).to(cuda), torch.from_numpy(yb).to(cuda), torch.from_numpy(lam).to(cuda))
    return model, x, t


@pytest.fixture
def options(dtc):
    """Set library options for one test; every one is restored afterwards."""
    lib = dtc._native.lib
    saved = {}

    def set_option(name, value):
        saved.setdefault(name, lib.dtc_get_option(name))
        lib.dtc_set_option(name, int(value))

    try:
        yield set_option
    finally:
        for name, value in saved.items():
            lib.dtc_set_option(name, value)


@pytest.mark.parametrize("head_fused", [1, 0])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_soft_xent_fused_into_head_backward_bit_identical(dtc, cuda, options, head_fused, precision):
    """xent_fuse 1 (the soft-target instantiation of the head backward kernel) against 0 (dtc_xent_soft_bwd into
    the executor's dlogits buffer, then the backward): every gradient and the dlogits buffer, bit for bit, under a
    GradScaler-scaled loss."""
    options(b"head_fused", head_fused)
    model, x, t = _setup(dtc, cuda)
    crit = dtc.CrossEntropyLoss(label_smoothing=0.1)
    scaler = dtc.GradScaler(init_scale=256.0)
    out = {}
    for fuse in (1, 0):
        options(b"xent_fuse", fuse)
        with dtc.autocast(enabled=precision == "bf16"):
            loss = crit(model(x), t)
        assert isinstance(loss, dtc.nn.NativeLoss)
        scaler.scale(loss).backward()
        exe = model.executor(B, 32, 32, precision)
        torch.cuda.synchronize()
        out[fuse] = (model.flat.grads.clone(), exe.dlogits_buffer().clone())
    assert torch.equal(out[1][1], out[0][1])
    assert torch.equal(out[1][0], out[0][0])
    assert float(out[1][1].abs().sum()) > 0 and torch.isfinite(out[1][0]).all().item()
    # the buffer holds the soft gradient: dtc_xent_soft_bwd of the same logits at the scaler's scale
    with dtc.autocast(enabled=precision == "bf16"):
        logits = model(x).detach()
    _, lse, _ = dtc.ops.xent_soft_fwd(logits, t.labels_a, t.labels_b, t.lam, 0.1)
    ref = dtc.ops.xent_soft_bwd(logits, t.labels_a, t.labels_b, t.lam, 0.1, lse, torch.tensor([256.0], device=cuda))
    assert torch.equal(out[1][1], ref)


@pytest.mark.parametrize("head_fused", [1, 0])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_soft_step_graph_replay_matches_eager(dtc, cuda, options, head_fused, precision):
    options(b"head_fused", head_fused)
    crit = dtc.CrossEntropyLoss(label_smoothing=0.1)
    res = {}
    for graphs in (0, 1):
        options(b"graphs", graphs)
        model, x, t = _setup(dtc, cuda)
        steps = []
        for _ in range(2):  # graphs: capture, then replay
            with dtc.autocast(enabled=precision == "bf16"):
                loss = crit(model(x), t)
            loss.backward()
            torch.cuda.synchronize()
            steps.append((float(loss), model.flat.grads.clone()))
        res[graphs] = steps
    for (le, ge), (lg, gg) in zip(res[0], res[1]):
        assert le == lg and torch.equal(ge, gg)
    assert torch.equal(res[0][0][1], res[0][1][1])  # and run to run


@pytest.mark.parametrize("head_fused", [1, 0])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_soft_native_loss_backward_matches_autograd(dtc, cuda, options, head_fused, precision):
    options(b"head_fused", head_fused)
    nnmod = import_module(dtc.__name__ + ".nn")
    model, x, t = _setup(dtc, cuda, seed=11)
    crit = dtc.CrossEntropyLoss(label_smoothing=0.1)
    scaler = dtc.GradScaler()
    out = {}
    for fast in (True, False):
        nnmod._FAST_BACKWARD[0] = fast
        try:
            with dtc.autocast(enabled=precision == "bf16"):
                loss = crit(model(x), t)
            assert isinstance(loss, nnmod.NativeLoss)
            loss.backward()
            g_plain = model.flat.grads.clone()
            with dtc.autocast(enabled=precision == "bf16"):
                loss = crit(model(x), t)
            scaled = scaler.scale(loss)
            assert isinstance(scaled, nnmod.NativeLoss)
            assert abs(float(scaled) - float(loss) * 65536.0) < 1e-3 * float(scaled)
            scaled.backward()
            g_scaled = model.flat.grads.clone()
        finally:
            nnmod._FAST_BACKWARD[0] = True
        torch.cuda.synchronize()
        out[fast] = (g_plain, g_scaled)
    assert rel_err(out[True][0].cpu().numpy(), out[False][0].cpu().numpy()) < 1e-5
    assert rel_err(out[True][1].cpu().numpy(), out[False][1].cpu().numpy()) < 1e-5
    assert float(out[True][0].norm()) > 0
    with dtc.autocast(enabled=precision == "bf16"):
        loss = crit(model(x), t)
    assert type(loss * 2.0) is torch.Tensor  # arithmetic on the loss leaves the fast path


@pytest.mark.parametrize("head_fused", [1, 0])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_zero_smoothing_on_index_labels_is_todays_step(dtc, cuda, options, head_fused, precision):
    """label_smoothing=0 with a plain label tensor runs the index-label kernels: gradients torch.equal to a model
    stepped through CrossEntropyLoss(); and the soft kernels at eps = 0 without labels_b (reached through the
    executor call directly) write those same bits."""
    options(b"head_fused", head_fused)
    grads, losses = [], []
    for crit in (dtc.CrossEntropyLoss(), dtc.CrossEntropyLoss(label_smoothing=0.0)):
        model, x, t = _setup(dtc, cuda)
        with dtc.autocast(enabled=precision == "bf16"):
            logits = model(x)
            loss = crit(logits, t.labels_a)
        loss.backward()
        torch.cuda.synchronize()
        grads.append(model.flat.grads.clone())
        losses.append(float(loss))
    assert torch.equal(grads[0], grads[1]) and losses[0] == losses[1]
    # the soft executor call at eps = 0, no labels_b, fused and separate
    for fuse in (1, 0):
        options(b"xent_fuse", fuse)
        model, x, t = _setup(dtc, cuda)
        with dtc.autocast(enabled=precision == "bf16"):
            logits = model(x)
        ld = logits.detach()
        sl, lse, _ = dtc.ops.xent_soft_fwd(ld, t.labels_a, None, None, 0.0)
        exe = model.executor(B, 32, 32, precision)
        exe.consume(exe.generation)
        exe.xent_soft_backward(ld, dtc.nn._Soft(t.labels_a, None, None, 0.0), lse, None, 1.0, None)
        torch.cuda.synchronize()
        assert float(sl) == losses[0]
        assert torch.equal(model.flat.grads, grads[0]), fuse


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_soft_loss_item_equals_device_value(dtc, cuda, precision):
    model, x, t = _setup(dtc, cuda)
    crit = dtc.CrossEntropyLoss(label_smoothing=0.1)
    scaler = dtc.GradScaler(init_scale=128.0)
    scaler.scale(torch.zeros((), device=cuda))  # initialise the scaler: the loss launch pre-multiplies its scale
    with dtc.autocast(enabled=precision == "bf16"):
        logits = model(x)
        loss = crit(logits, t)
    assert getattr(loss, "_dtc_host", None) is not None
    v = loss.item()
    torch.cuda.synchronize()
    assert v == float(loss.detach().cpu()) and np.isfinite(v)
    ref, _, _ = dtc.ops.xent_soft_fwd(logits.detach(), t.labels_a, t.labels_b, t.lam, 0.1)
    assert v == float(ref)
    s = scaler.scale(loss)
    assert float(s) == float(np.float32(v) * np.float32(128.0))
    # label smoothing alone, and a MixedTarget without smoothing, are soft losses too
    for c, tt in ((crit, t.labels_a), (dtc.CrossEntropyLoss(), t)):
        with dtc.autocast(enabled=precision == "bf16"):
            l2 = c(model(x), tt)
        assert isinstance(l2, dtc.nn.NativeLoss) and l2.item() == float(l2.detach().cpu()) and l2.item() != v


def test_soft_loss_under_data_parallel(dtc, cuda):
    """DataParallel device_ids=[0, 0]: the MixedTarget is not scattered, the loss sees the gathered logits
    (ops.xent_soft_bwd, then the replicas' backward); gradients are finite and equal the autograd path's."""
    nnmod = import_module(dtc.__name__ + ".nn")
    model, x, t = _setup(dtc, cuda)
    dp = dtc.DataParallel(model, device_ids=[0, 0])
    crit = dtc.CrossEntropyLoss(label_smoothing=0.1)
    out = {}
    for fast in (True, False):
        nnmod._FAST_BACKWARD[0] = fast
        try:
            dp.zero_grad()
            with dtc.autocast():
                loss = crit(dp(x), t)
            assert isinstance(loss, nnmod.NativeLoss) and np.isfinite(loss.item())
            loss.backward()
            torch.cuda.synchronize()
            out[fast] = model.flat.grads.clone()
        finally:
            nnmod._FAST_BACKWARD[0] = True
    assert torch.isfinite(out[True]).all().item() and float(out[True].norm()) > 0
    assert rel_err(out[True].cpu().numpy(), out[False].cpu().numpy()) < 1e-5
