"""A non-finite training step through the whole network: what a flagged BatchNorm does to the step.

A BN whose statistics saw a non-finite (or out-of-range) partial is flagged (csrc/common.h) and yields NaN
coefficients; the fused ReLU keeps NaN (csrc/common.h relu_nan), so the NaN reaches the loss as it does in torch and in
the oracle. Two triggers whose reference outcome is unambiguous -- oracle.resnet.forward_backward on the same state
gives a non-finite loss, asserted here on the CPU first, so the expectation is the reference's and not the code's:

  (a) one NaN pixel in one input image: flags the stem BN;
  (b) one +inf element in layer3.0.conv1.weight: flags a deep BN, followed by add-ReLU and dual-BN blocks and the head.

Smallest sizes: batch 4 at 8x8, seeded as tests/test_gpu_resnet.py::_setup.

AMP (bf16 under autocast, GradScaler, SGD; eager and captured graphs): the loss is NaN, found_inf is raised, the
parameters, the momentum and the bf16 shadow are bit-unchanged, the scale backs off. A clean step afterwards is
bit-equal -- logits, loss, parameters, momentum -- to the same step of a twin model that never saw the bad one and
whose scaler starts at the backed-off scale: the flag and the slots are cleared every step, inside captured graphs
too. Running statistics are NOT compared: those of a flagged BN are NaN from then on, as torch's are after a
non-finite batch.

fp32 (no autocast, no GradScaler): loss and logits of the bad step are NaN -- with a ReLU that turned NaN into 0 the
loss came out finite over a network whose BN coefficients were NaN.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import resnet as R
from tests.test_gpu_resnet import _setup, _split_state

pytestmark = pytest.mark.gpu

BATCH, HW = 4, 8
WEIGHT, ELEMENT = "layer3.0.conv1.weight", 7
INIT_SCALE = 2.0 ** 10


def _poison_input(x):
    x = x.copy()
    x[1, 2, 3, 4] = np.nan
    return x


@functools.lru_cache(maxsize=None)
def _oracle_loss(trigger, bf16_mode):
    """The reference's loss on the poisoned state (CPU, float64 oracle with the executor's rounding points)."""
    torch.manual_seed(42)
    import dtc_import
    dtc = dtc_import.load()
    sd = {k: v.detach().numpy().copy() for k, v in dtc.ResNet18().state_dict().items()}
    g = np.random.default_rng(0)
    x = g.standard_normal((BATCH, 3, HW, HW)).astype(np.float32)
    y = g.integers(0, 100, BATCH)
    if trigger == "input":
        x = _poison_input(x)
    else:
        sd[WEIGHT].reshape(-1)[ELEMENT] = np.inf
    params, bufs = _split_state(sd)
    with np.errstate(all="ignore"):
        ref = R.forward_backward(params, bufs, x, y, bf16_mode=bf16_mode, train=True)
    return float(ref["loss"]), bool(np.isfinite(ref["logits"]).all())


def _weight_slot(model):
    p = next(p for p in model.flat.layout.params if p.name == WEIGHT)
    return p.offset + ELEMENT


def _set_weight(model, value):
    """One element of the fp32 master weight and of its bf16 shadow (what an optimizer step would keep in step)."""
    i = _weight_slot(model)
    old = float(model.flat.params[i].item())
    model.flat.params[i] = value
    model.flat.params_bf16[i] = value
    return old


class _Graphs:
    def __init__(self, dtc, mode):
        self.lib, self.mode = dtc._native.lib, int(mode)

    def __enter__(self):
        self.prev = self.lib.dtc_get_option(b"graphs")
        self.lib.dtc_set_option(b"graphs", self.mode)

    def __exit__(self, *exc):
        self.lib.dtc_set_option(b"graphs", self.prev)


def _amp_model(dtc, cuda, scale):
    model, _, x, y = _setup(dtc, cuda, BATCH, hw=HW)
    opt = dtc.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    opt.attach(model)
    return model, opt, dtc.GradScaler(init_scale=scale), x, y


def _amp_step(dtc, model, opt, scaler, xd, yd):
    crit = dtc.CrossEntropyLoss()
    opt.zero_grad()
    with dtc.autocast():
        logits = model(xd)
        loss = crit(logits, yd)
    scaler.scale(loss).backward()
    scaler.step(opt)
    found = int(scaler.found_inf.item())  # between step() and update(), as a consumer of the word reads it
    scaler.update()
    torch.cuda.synchronize()
    return logits.detach().float().cpu().numpy().copy(), float(loss), found


def _state(model, opt):
    return [t.detach().clone() for t in (model.flat.params, opt._mom, model.flat.params_bf16)]


@pytest.mark.parametrize("graphs", [0, 1])
@pytest.mark.parametrize("trigger", ["input", "weight"])
def test_amp_bad_step_is_skipped_and_leaves_no_trace(dtc, cuda, trigger, graphs):
    loss_ref, logits_finite = _oracle_loss(trigger, True)
    assert not np.isfinite(loss_ref) and not logits_finite  # the reference: a non-finite loss
    with _Graphs(dtc, graphs):
        model, opt, scaler, x, y = _amp_model(dtc, cuda, INIT_SCALE)
        yd = torch.from_numpy(y).to(cuda)
        x_clean, x_bad = torch.from_numpy(x).to(cuda), torch.from_numpy(_poison_input(x)).to(cuda)
        before = _state(model, opt)
        if trigger == "weight":
            old = _set_weight(model, float("inf"))
        logits, loss, found = _amp_step(dtc, model, opt, scaler, x_bad if trigger == "input" else x_clean, yd)
        if trigger == "weight":
            assert _set_weight(model, old) == float("inf")  # the skipped step left the poisoned element in place
        assert np.isnan(loss), f"loss {loss} after a flagged BN (reference: {loss_ref})"
        assert np.isnan(logits).all()
        assert found != 0
        for name, a, b in zip(("params", "momentum", "bf16 shadow"), before, _state(model, opt)):
            assert torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                               b.view(torch.int32 if b.dtype == torch.float32 else torch.int16)), name
        assert scaler.get_scale() == INIT_SCALE * 0.5
        # one clean step, against a twin that never saw the bad one
        logits1, loss1, found1 = _amp_step(dtc, model, opt, scaler, x_clean, yd)
        twin, topt, tscaler, _, _ = _amp_model(dtc, cuda, INIT_SCALE * 0.5)
        logits2, loss2, found2 = _amp_step(dtc, twin, topt, tscaler, x_clean, yd)
        assert found1 == 0 and found2 == 0 and np.isfinite(loss1) and 2.0 < loss1 < 8.0
        np.testing.assert_array_equal(logits1, logits2)
        assert np.float32(loss1).tobytes() == np.float32(loss2).tobytes()
        for name, a, b in zip(("params", "momentum", "bf16 shadow"), _state(model, opt), _state(twin, topt)):
            assert torch.equal(a, b) and bool(torch.isfinite(a.float()).all()), name
        assert float((before[0] - model.flat.params).abs().sum()) > 0  # the clean step was applied
        assert scaler.get_scale() == tscaler.get_scale() == INIT_SCALE * 0.5


@pytest.mark.parametrize("trigger", ["input", "weight"])
def test_fp32_bad_step_shows_nan(dtc, cuda, trigger):
    """No autocast, no GradScaler: nothing skips the step, so the NaN has to show in the loss and the logits."""
    loss_ref, logits_finite = _oracle_loss(trigger, False)
    assert not np.isfinite(loss_ref) and not logits_finite
    model, _, x, y = _setup(dtc, cuda, BATCH, hw=HW)
    model.precision = "fp32"
    if trigger == "weight":
        _set_weight(model, float("inf"))
    else:
        x = _poison_input(x)
    with dtc.autocast(enabled=False):
        logits = model(torch.from_numpy(x).to(cuda))
        loss = dtc.CrossEntropyLoss()(logits, torch.from_numpy(y).to(cuda))
    loss.backward()
    torch.cuda.synchronize()
    assert np.isnan(float(loss)), f"loss {float(loss)} (reference: {loss_ref})"
    assert bool(torch.isnan(logits).all())
    assert not bool(torch.isfinite(model.flat.grads).all())


def test_sync_bn_bad_step_shows_nan(dtc, cuda):
    """SyncBatchNorm over the one-rank loopback communicator: the header (with the flag) travels with slot 0 through
    bn_fold_slots and the collective, and the consumers behind them still see it."""
    assert not np.isfinite(_oracle_loss("input", True)[0])
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 1.0, world=1)
    try:
        model, _, x, y = _setup(dtc, cuda, BATCH, hw=HW)
        model = dtc.SyncBatchNorm.convert_sync_batchnorm(model)
        model.set_sync_bn(comm)
        with dtc.autocast():
            logits = model(torch.from_numpy(_poison_input(x)).to(cuda))
            loss = dtc.CrossEntropyLoss()(logits, torch.from_numpy(y).to(cuda))
        loss.backward()
        torch.cuda.synchronize()
        assert len(comm.log()) > 0
        assert np.isnan(float(loss)) and bool(torch.isnan(logits.float()).all())
        assert not bool(torch.isfinite(model.flat.grads).all())
        model.set_sync_bn(None)
    finally:
        comm.close()
