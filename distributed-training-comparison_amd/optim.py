"""optim.SGD / Adam / AdamW mirrors, LARS and the SAM wrapper running fused flat-buffer kernels, and clip_grad_norm_.

Reference: ``optim.SGD(self.model.parameters(), lr, weight_decay, momentum=0.9, nesterov=True)``
(src/ddp/trainer.py:92-98) stepped through ``GradScaler.step`` (trainer.py:158); the reference's README
invites users to swap the optimizer in ``configure_optimizers`` ("e.g. using ADAM optimizer"). The classes
subclass ``torch.optim.Optimizer`` so ``optim.lr_scheduler.StepLR`` (trainer.py:101-105) drives
``param_groups[0]['lr']`` unchanged; ``step()`` enqueues ONE update kernel over the model's flat
parameter / gradient / state buffers that also refreshes the bf16 weight shadow (Adam: plus a one-thread
tick that advances the device-side step count).

``clip_grad_norm_`` computes the global gradient norm and the clip coefficient on the device and DEFERS
the clip: the multiplier is handed to the next ``optimizer.step()``, which applies it to the gradients as it
reads them. ``p.grad`` keeps showing the unclipped gradients.
"""
from __future__ import annotations

import copy

import torch
from torch.optim import Optimizer

from . import ops
from ._native import NativeError


def _model_of(params, who: str):
    """The native ResNet whose flat buffers hold `params` (every parameter view carries a weak reference)."""
    ref = getattr(params[0], "_dtc_model", None) if params else None
    model = ref() if ref is not None else None
    if model is None:
        raise NativeError(f"{who} parameters do not belong to a native ResNet moved to the GPU "
                          f"(create the optimizer after model.to('cuda'))")
    return model


def _check_owns_all(params, flat, who: str):
    ids = {p.data_ptr() for p in params}
    if len(ids) != len(flat.layout.params):
        raise NativeError(f"{who} must own every parameter of the model (flat-buffer update)")


class _FlatOptimizer(Optimizer):
    """What the fused optimizers share: one parameter group that owns every parameter of one native model,
    lazy binding to its FlatState, the no-op zero_grad, and a step() that hands the kernel the device-side
    gradient multiplier (GradScaler's inv_scale, or a pending clip_grad_norm_ multiplier) and found_inf."""

    def __init__(self, params, defaults):
        params = list(params)
        if params and isinstance(params[0], dict):
            raise NotImplementedError("per-parameter groups are not used by the reference (trainer.py:92-98)")
        super().__init__(params, defaults)
        self._flat = None

    def attach(self, model):
        """Bind to the model's flat buffers (done lazily on the first step)."""
        flat = model.flat
        _check_owns_all(self.param_groups[0]["params"], flat, type(self).__name__)
        self._flat = flat
        self._init_state(flat)

    def _find_flat(self):
        return _model_of(self.param_groups[0]["params"], type(self).__name__)

    def _init_state(self, flat):
        raise NotImplementedError

    def _update(self, flat, group, grad_mult, found_inf):
        raise NotImplementedError

    def zero_grad(self, set_to_none: bool = True):
        # The native backward WRITES every gradient (it never accumulates), which is exactly
        # the state zero_grad() + backward() produces in the reference; nothing to clear.
        return None

    # ------------------------------------------------------------------ state_dict, in torch's format
    # (key of torch's per-parameter state, attribute holding the flat fp32 buffer), per subclass
    _STATE_BUFFERS = ()

    def _check_group(self, group) -> None:
        """Refuse hyperparameters the fused kernel does not implement (load_state_dict takes them from a file)."""

    def _get_step(self):
        """The step count torch keeps per parameter (Adam), or None for optimizers that keep none."""
        return None

    def _set_step(self, step: int) -> None:
        pass

    def _param_infos(self, flat):
        """The layout entry of every parameter of the group, in the group's order (the order of
        ``named_parameters()`` for ``model.parameters()``), found by the address of the parameter's view."""
        base = flat.params.data_ptr()
        by_ptr = {base + 4 * q.offset: q for q in flat.layout.params}
        return [by_ptr[p.data_ptr()] for p in self.param_groups[0]["params"]]

    @staticmethod
    def _view(buf, q):
        return torch.as_strided(buf, q.shape, q.stride, q.offset)

    def state_dict(self):
        """torch's ``Optimizer.state_dict()``: ``state[i]`` of the i-th parameter holds views of the flat state
        buffers in the parameter's logical shape (conv weights: strided [K,C,R,S] views over the KRSC storage),
        under ``torch.optim``'s keys, so the dict loads into ``torch.optim`` over the reference model and back.
        Adam's ``step`` is read from the device record: one host synchronisation. Before the first step (nothing
        attached): torch's shell with an empty ``state``."""
        out = super().state_dict()
        if self._flat is None:
            return out
        step = self._get_step()
        state = {}
        for i, q in enumerate(self._param_infos(self._flat)):
            entry = {} if step is None else {"step": torch.tensor(float(step), dtype=torch.float32)}
            for key, attr in self._STATE_BUFFERS:
                entry[key] = self._view(getattr(self, attr), q)
            state[i] = entry
        out["state"] = state
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        """torch's ``Optimizer.load_state_dict()`` on the flat buffers: binds to the model first (parameters of no
        native model: NativeError), copies every per-parameter entry into its view of the state buffer -- the
        alignment padding between the parameters is never written -- and takes the hyperparameters of
        ``param_groups``. The group dicts are updated IN PLACE: SAM shares the list, schedulers hold the optimizer.
        An empty ``state`` (saved before the first step) resets the buffers. Everything is checked before anything
        is written."""
        who = type(self).__name__
        if self._flat is None:
            self.attach(self._find_flat())
        flat = self._flat
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"{who}.load_state_dict: {len(groups)} parameter groups, expected 1")
        infos = self._param_infos(flat)
        if len(groups[0]["params"]) != len(infos):
            raise ValueError(f"{who}.load_state_dict: the state holds {len(groups[0]['params'])} parameters, the "
                             f"model has {len(infos)}")
        new_group = {k: copy.deepcopy(v) for k, v in groups[0].items() if k != "params"}
        self._check_group({**self.param_groups[0], **new_group})
        saved = state_dict["state"]
        ids = list(groups[0]["params"])  # torch's packed ids: position i holds the key of parameter i
        copies, step = [], None
        for i, q in enumerate(infos if len(saved) else ()):
            if ids[i] not in saved:
                raise KeyError(f"{who}.load_state_dict: no state for parameter {i} ({q.name})")
            entry = saved[ids[i]]
            for key, attr in self._STATE_BUFFERS:
                if key not in entry:
                    raise KeyError(f"{who}.load_state_dict: parameter {i} ({q.name}) has no {key!r}")
                t = entry[key]
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(q.shape):
                    raise ValueError(f"{who}.load_state_dict: {key!r} of parameter {i} ({q.name}) has shape "
                                     f"{tuple(getattr(t, 'shape', ()))}, expected {tuple(q.shape)}")
                copies.append((attr, q, t))
            if self._get_step() is not None:
                if "step" not in entry:
                    raise KeyError(f"{who}.load_state_dict: parameter {i} ({q.name}) has no 'step'")
                s = float(entry["step"])  # a tensor or a number
                if s < 0 or s != int(s) or (step is not None and s != step):
                    raise ValueError(f"{who}.load_state_dict: 'step' of parameter {i} ({q.name}) is {s}; the fused "
                                     f"kernel keeps one non-negative integer count for all parameters")
                step = s
        if not len(saved):
            for _, attr in self._STATE_BUFFERS:
                getattr(self, attr).zero_()
            step = 0
        for attr, q, t in copies:
            self._view(getattr(self, attr), q).copy_(t)
        self._set_step(int(step or 0))
        self.param_groups[0].update(new_group)

    @torch.no_grad()
    def step(self, closure=None, inv_scale=None, found_inf=None):
        if closure is not None:
            raise NotImplementedError("closures are not used by the reference")
        if self._flat is None:
            self.attach(self._find_flat())
        flat = self._flat
        if flat.clip_pending:  # clip_grad_norm_ ran since the last step: its multiplier includes inv_scale
            inv_scale = flat.grad_mult
            flat.clip_pending = False
        self._update(flat, self.param_groups[0], inv_scale, found_inf)
        return None


class SGD(_FlatOptimizer):
    def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)
        if not nesterov or dampening != 0.0 or momentum <= 0.0:
            raise NotImplementedError("the fused kernel implements SGD(momentum>0, dampening=0, nesterov=True) "
                                      "as used by the reference (trainer.py:92-98)")
        self._mom = None

    _STATE_BUFFERS = (("momentum_buffer", "_mom"),)

    def _check_group(self, g):
        if not g["nesterov"] or g["dampening"] != 0.0 or g["momentum"] <= 0.0 or g.get("maximize", False):
            raise NotImplementedError("the fused kernel implements SGD(momentum>0, dampening=0, nesterov=True, "
                                      "maximize=False)")

    def _init_state(self, flat):
        self._mom = torch.zeros_like(flat.params)

    def _update(self, flat, g, grad_mult, found_inf):
        ops.sgd_nesterov_flat(flat.params, flat.grads, self._mom, flat.params_bf16, g["lr"], g["weight_decay"],
                              g["momentum"], grad_mult, found_inf)


class Adam(_FlatOptimizer):
    """torch.optim.Adam (amsgrad=False, maximize=False) on the fused flat-buffer kernel. The step count lives
    on the device and does not advance on a step GradScaler skips, as torch's ``state['step']``."""

    _decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 maximize=False):
        if amsgrad or maximize:
            raise NotImplementedError("the fused kernel implements amsgrad=False, maximize=False")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps} (the fused kernel needs eps > 0)")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        super().__init__(params, defaults)
        self._exp_avg = self._exp_avg_sq = self._step_state = None

    _STATE_BUFFERS = (("exp_avg", "_exp_avg"), ("exp_avg_sq", "_exp_avg_sq"))

    def _check_group(self, g):
        if g.get("amsgrad", False) or g.get("maximize", False):
            raise NotImplementedError("the fused kernel implements amsgrad=False, maximize=False")

    def _get_step(self):
        """Word 0 of the device record (a host synchronisation); 0 before the record exists."""
        return 0 if self._step_state is None else int(self._step_state[0].item())

    def _set_step(self, step: int) -> None:
        # only the count: the tick kernel recomputes the factors that depend on it ahead of every update
        self._step_state[:1].copy_(torch.tensor([step], dtype=torch.int32))

    def _init_state(self, flat):
        self._exp_avg = torch.zeros_like(flat.params)
        self._exp_avg_sq = torch.zeros_like(flat.params)
        self._step_state = ops.adam_state(flat.params.device)

    def _update(self, flat, g, grad_mult, found_inf):
        ops.adam_flat(flat.params, flat.grads, self._exp_avg, self._exp_avg_sq, flat.params_bf16, self._step_state,
                      g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self._decoupled,
                      grad_mult, found_inf)


class AdamW(Adam):
    """torch.optim.AdamW: Adam with decoupled weight decay (p *= 1 - lr * weight_decay)."""

    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False,
                 maximize=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         maximize=maximize)


class LARS(_FlatOptimizer):
    """LARS (You et al. 2017): SGD with momentum whose step is scaled per parameter tensor by the trust ratio
    ``trust_coef * ||p|| / (||g|| + weight_decay * ||p|| + eps)``; with ``trust_clip`` (LARC's "clip" mode) by
    ``min(ratio / lr, 1)``. The ratio and the weight decay apply to parameters with more than one dimension (conv
    and linear weights); BatchNorm weights / biases and ``linear.bias`` take the plain momentum step. The norms are
    recomputed on the device at every step (three launches, no host synchronisation, bit-reproducible)."""

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, nesterov=False, trust_coef=1e-3, eps=1e-8,
                 trust_clip=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 < trust_coef:
            raise ValueError(f"Invalid trust_coef value: {trust_coef}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                        trust_coef=trust_coef, eps=eps, trust_clip=trust_clip)
        super().__init__(params, defaults)
        self._mom = self._plan = self._norms = None

    _STATE_BUFFERS = (("momentum_buffer", "_mom"),)  # (_norms is rewritten whole by every step)

    def _init_state(self, flat):
        self._mom = torch.zeros_like(flat.params)
        self._plan = ops.seg_plan(flat.layout, flat.device)  # the handle keeps its device memory (plan.mem)
        self._norms = torch.zeros(self._plan.nseg, 3, dtype=torch.float32, device=flat.device)

    def _update(self, flat, g, grad_mult, found_inf):
        ops.lars_flat(self._plan, flat.params, flat.grads, self._mom, flat.params_bf16, g["lr"], g["weight_decay"],
                      g["momentum"], g["nesterov"], g["trust_coef"], g["eps"], g["trust_clip"], grad_mult, found_inf,
                      self._norms)

    def layer_norms(self):
        """(norms, names): the last step's fp32 [n, 3] device tensor of (||p||, ||g|| of the unscaled, clipped
        gradient, trust ratio applied) per parameter -- both norms taken before the update -- and the parameter
        names, in flat-buffer order. No synchronisation: the tensor is the one the next step overwrites (clone to
        keep)."""
        if self._plan is None:
            raise NativeError("LARS.layer_norms: no step has run yet")
        return self._norms, self._plan.names


class SAM(Optimizer):
    """Sharpness-aware minimisation (Foret et al. 2021; ``adaptive=True``: ASAM, Kwon et al. 2021, typical rho 0.5
    to 2.0) around one of the fused optimizers above. One optimizer step is two passes over the same batch:

        loss = criterion(model(x), y)                 # at w: the loss worth logging
        with model.local_grads():                     # this rank's own gradient: not reduced, not accumulated
            loss.backward()
        optimizer.first_step(scaler)                  # w <- w + e(w): three launches (include/dtc.h dtc_sam_perturb)
        criterion(model(x), y).backward()             # the gradient at w + e, all-reduced as ever
        optimizer.step()                              # w restored bit for bit (one launch), then the base's step

    (under AMP the two backwards run on ``scaler.scale(loss)`` and the last line is ``scaler.step(optimizer)``).
    ``param_groups`` IS the base optimizer's list, so LR schedulers built on either drive the same ``lr``; ``_flat``,
    ``attach``, ``_find_flat`` and ``zero_grad`` are the base's, so ``GradScaler.unscale_ / step`` and
    ``clip_grad_norm_`` take the wrapper unchanged. The BatchNorm running statistics and batch counts the second
    forward updates again are put back by the restore: one SAM step moves them as one plain step does.

    A first gradient that is not finite moves nothing. With a scaler the restore raises its ``found_inf`` word on
    the device, so the step is skipped and ``update()`` backs the scale off; without one the step is the plain step
    at the unperturbed weights. ``rho = 0`` is legal: the perturbation is then zero."""

    def __init__(self, base_optimizer, rho=0.05, adaptive=False, eps=1e-12):
        if not isinstance(base_optimizer, _FlatOptimizer):
            raise TypeError("SAM wraps one of this package's fused optimizers (SGD, Adam, AdamW, LARS), not "
                            f"{type(base_optimizer).__name__}")
        if not 0.0 <= rho:
            raise ValueError(f"Invalid rho value: {rho}")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        self.base = base_optimizer
        self.rho, self.adaptive, self.eps = float(rho), bool(adaptive), float(eps)
        super().__init__(base_optimizer.param_groups[0]["params"], dict(base_optimizer.defaults))
        self.param_groups = base_optimizer.param_groups  # shared, not copied: one lr for schedulers to drive
        self._perturbed = False
        self._saved = None  # (flat, p_saved, bufs_saved, nbt_saved), allocated by the first first_step()
        self._state = self._ws = None

    @property
    def _flat(self):
        return self.base._flat

    def attach(self, model):
        self.base.attach(model)

    def _find_flat(self):
        return self.base._find_flat()

    def zero_grad(self, set_to_none: bool = True):
        return self.base.zero_grad(set_to_none)

    def _refuse_perturbed(self, what: str) -> None:
        if self._perturbed:
            raise NativeError(f"SAM.{what}: the weights are perturbed between first_step() and step(); call it "
                              "after step()")

    def state_dict(self):
        """The base optimizer's (SAM keeps no state of its own across steps)."""
        self._refuse_perturbed("state_dict")
        return self.base.state_dict()

    def load_state_dict(self, state_dict) -> None:
        self._refuse_perturbed("load_state_dict")
        self.base.load_state_dict(state_dict)

    def _keep(self, flat):
        _, _, bufs_saved, nbt_saved = self._saved
        return [(flat.bufs, bufs_saved), (flat.nbt, nbt_saved)]

    @property
    def grad_norm(self) -> torch.Tensor:
        """The L2 norm of the last first_step()'s gradient (unscaled; ASAM: of p * g) as a 0-dim fp32 view of the
        device record: no synchronisation, overwritten by the next first_step() (clone to keep)."""
        if self._state is None:
            raise NativeError("SAM.grad_norm: no first_step() has run yet")
        return self._state.view(torch.float32)[1]

    @torch.no_grad()
    def first_step(self, scaler=None):
        """After the first backward: save the weights and the BatchNorm running state, move to w + e(w)."""
        if self._perturbed:
            raise NativeError("SAM.first_step: the weights are already perturbed (step() must follow first_step())")
        if self.base._flat is None:
            self.base.attach(self.base._find_flat())
        flat = self.base._flat
        if self._saved is None or self._saved[0] is not flat:
            self._saved = (flat, torch.empty_like(flat.params), torch.empty_like(flat.bufs),
                           torch.empty_like(flat.nbt))
            self._state = ops.sam_state(flat.device)
            self._ws = ops.sam_workspace(flat.params.numel(), flat.device)
        gmul = None
        if scaler is not None and scaler.is_enabled():
            scaler._lazy_init(flat.device)
            gmul = scaler._inv_scale
        ops.sam_perturb(flat.params, flat.grads, self._saved[1], flat.params_bf16, self._state, self.rho,
                        self.adaptive, self.eps, gmul, self._keep(flat), self._ws)
        self._perturbed = True

    @torch.no_grad()
    def step(self, closure=None, inv_scale=None, found_inf=None):
        if closure is not None:
            raise NotImplementedError("closures are not used: run the two passes and first_step() explicitly")
        if not self._perturbed:
            raise NativeError("SAM.step: no first_step() since the last step (the two-pass loop: backward inside "
                              "model.local_grads(), first_step(), a second forward / backward, step())")
        flat = self.base._flat
        ops.sam_restore(flat.params, self._saved[1], flat.params_bf16, self._state, self._keep(flat), found_inf)
        self._perturbed = False
        return self.base.step(inv_scale=inv_scale, found_inf=found_inf)


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, scaler=None) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ for a native model: one read pass over the flat gradient buffer and a
    tiny finalize, nothing leaves the GPU.

    ``parameters`` must be all parameters of one native ResNet. With ``scaler`` (a GradScaler, after its
    ``unscale_`` -- which here only checks for inf/NaN and leaves the gradients loss-scaled) the scaler's
    device-side 1/scale is folded in. Returns the total norm of the unscaled gradients as a 0-dim device
    tensor, without a host synchronisation.

    Deviation from torch: the gradients are NOT rewritten. The multiplier is stored on the model's
    FlatState and the next ``step()`` of SGD / Adam / AdamW / LARS applies it where it would apply ``inv_scale``
    (no extra read-modify-write pass over the gradients); ``p.grad`` keeps showing the unclipped values.
    """
    if float(norm_type) != 2.0:
        raise NotImplementedError("only the L2 norm (norm_type=2) is implemented")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = list(parameters)
    flat = _model_of(params, "clip_grad_norm_").flat
    _check_owns_all(params, flat, "clip_grad_norm_")
    if flat.grad_mult is None:
        flat.grad_mult = torch.empty(1, dtype=torch.float32, device=flat.device)
        flat.norm_ws = ops.grad_norm_workspace(flat.grads.numel(), flat.device)
    inv_scale = None
    if scaler is not None and scaler.is_enabled():
        scaler._lazy_init(flat.device)
        inv_scale = scaler._inv_scale
    # a fresh word per call (an allocation, not a launch): norms the caller kept stay valid
    total_norm = torch.empty(1, dtype=torch.float32, device=flat.device)
    ops.grad_norm_clip(flat.grads, max_norm, inv_scale, flat.norm_ws, total_norm, flat.grad_mult)
    flat.clip_pending = True
    return total_norm.reshape(())
