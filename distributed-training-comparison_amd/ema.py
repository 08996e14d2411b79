"""Exponential moving average of a native model's weights, kept on its flat buffers.

What ``timm.utils.ModelEmaV2`` / torchvision's ``--model-ema`` / ``torch.optim.swa_utils.AveragedModel`` keep as
a second module is here a second set of the model's flat buffers -- fp32 parameters, their bf16 shadow in GEMM
operand layout, the BatchNorm running statistics -- updated by ONE native launch per step (behind a one-thread
tick; include/dtc.h ``dtc_ema_update``) and evaluated in place by the model's own executors
(``dtc_rn18_eval_batch_weights``): nothing is copied into the model and back. A GradScaler-skipped step is not
an update: the kernel reads the scaler's device-side ``found_inf`` itself, so no host synchronisation is needed.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import ops
from ._native import NativeError
from .nn import EvalResult, ResNet


class ModelEma:
    """``ema = decay * ema + (1 - decay) * model`` over every parameter and running statistic of `model` (a native
    ResNet on the GPU, or a DDP / DataParallel wrapper of one: its ``module``). ``warmup=True`` ramps the decay
    as ``min(decay, (1 + t) / (10 + t))`` over the updates t = 1, 2, ... (tf.train.ExponentialMovingAverage /
    timm's ModelEma warm-up). The object has ``params``, ``params_bf16`` and ``bufs`` tensors in the model's
    layout, which is what ``ResNet.evaluate(weights=)`` asks for."""

    def __init__(self, model, decay: float = 0.9998, warmup: bool = False):
        if not isinstance(model, ResNet) and isinstance(getattr(model, "module", None), ResNet):
            model = model.module
        if not isinstance(model, ResNet):
            raise NativeError("ModelEma: only the native ResNet (or a DDP / DataParallel wrapper of it) is supported")
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"decay = {decay} must lie in [0, 1)")
        flat = model.flat  # refuses a model that was not moved to the GPU
        self.model = model
        self.decay = float(decay)
        self.warmup = bool(warmup)
        self.params = flat.params.clone()            # device-to-device copies
        self.params_bf16 = flat.params_bf16.clone()  # the model's own shadow, not a re-rounding
        self.bufs = flat.bufs.clone()
        self.state = ops.ema_state(flat.device)

    def update(self, found_inf=None) -> None:
        """One update from the model's current weights, enqueued on the current stream: the parameters (with the
        bf16 copy) and the running mean / var in one launch. `found_inf`: GradScaler.found_inf between
        ``scaler.step`` and ``scaler.update`` -- a skipped optimizer step leaves the EMA and its count unchanged."""
        flat = self.model.flat
        ops.ema_update(((self.params, flat.params, self.params_bf16), (self.bufs, flat.bufs, None)), self.state,
                       self.decay, self.warmup, found_inf)

    @property
    def num_updates(self) -> int:
        """Updates applied so far (skipped steps excluded). Reads the device count: a host synchronisation, for
        logging and tests only."""
        return int(self.state[0].item())

    def evaluate(self, batches, topk: int = 5) -> EvalResult:
        """``model.evaluate`` on the EMA weights (the model's own stay bound and untouched)."""
        return self.model.evaluate(batches, topk, weights=self)

    def _views(self):
        layout = self.model.flat.layout
        out = {q.name: torch.as_strided(self.params, q.shape, q.stride, q.offset) for q in layout.params}
        for bn in layout.bns:
            out[bn.prefix + ".running_mean"] = self.bufs.narrow(0, bn.mean_offset, bn.channels)
            out[bn.prefix + ".running_var"] = self.bufs.narrow(0, bn.var_offset, bn.channels)
        return out

    def state_dict(self):
        """The model's keys in the model's order, so ``model.load_state_dict(ema.state_dict())`` works: views over
        the EMA buffers (conv weights as strided [K,C,R,S] views), ``num_batches_tracked`` taken from the model."""
        views = self._views()
        out = OrderedDict()
        for key, val in self.model.state_dict().items():
            out[key] = views.get(key, val)
        return out

    def load_state_dict(self, state_dict) -> None:
        """Copy the parameters and running statistics of `state_dict` (the model's keys; ``num_batches_tracked``
        is the model's and is ignored) into the EMA buffers and refresh the bf16 copy."""
        views = self._views()
        missing = [k for k in views if k not in state_dict]
        unexpected = [k for k in state_dict if k not in views and not k.endswith("num_batches_tracked")]
        if missing or unexpected:
            raise KeyError(f"ModelEma.load_state_dict: missing {missing}, unexpected {unexpected}")
        with torch.no_grad():
            for key, view in views.items():
                view.copy_(state_dict[key])
        ops.cast_f32_bf16(self.params, self.params_bf16)

    def train_state(self) -> dict:
        """What a resumed run needs beyond ``state_dict()``: the weights and the update count, which the warm-up
        decay depends on (a host synchronisation). The bf16 copy is not stored: every update writes it as the
        rounding of the fp32 EMA, which ``load_state_dict`` repeats."""
        return {"weights": self.state_dict(), "num_updates": self.num_updates}

    def load_train_state(self, state) -> None:
        """Load ``train_state()``: the weights as ``load_state_dict`` and word 0 of the device record (the tick
        kernel writes the rest ahead of every update)."""
        n = int(state["num_updates"])
        if n < 0:
            raise ValueError(f"ModelEma.load_train_state: num_updates = {n}")
        self.load_state_dict(state["weights"])
        self.state[:1].copy_(torch.tensor([n], dtype=torch.int32))

    def copy_to(self, model=None) -> None:
        """Copy the EMA parameters, bf16 copy and running statistics into `model` (default: the tracked one)."""
        if model is None:
            model = self.model
        elif not isinstance(model, ResNet):
            model = getattr(model, "module", model)
        flat = model.flat
        if flat.params.shape != self.params.shape or flat.bufs.shape != self.bufs.shape:
            raise NativeError("ModelEma.copy_to: the model's layout differs from the EMA's")
        with torch.no_grad():
            flat.params.copy_(self.params)
            flat.params_bf16.copy_(self.params_bf16)
            flat.bufs.copy_(self.bufs)
