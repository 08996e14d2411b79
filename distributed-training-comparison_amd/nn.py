"""ResNet-18 and CrossEntropyLoss modules backed by the native executor.

Mirror of the reference's operator boundary (src/ddp/net.py, trainer.py:40):

* ``ResNet18()`` builds the module tree with the SAME ``nn.Conv2d`` / ``nn.BatchNorm2d`` /
  ``nn.Linear`` constructors in the SAME order as net.py:86-105 and net.py:16-38, so a given
  ``torch.manual_seed`` yields bit-identical initial parameters and ``state_dict()`` keys
  (``layer2.0.shortcut.0.weight`` ...). Construction is ordinary PyTorch on the host.
* ``.to('cuda')`` moves those parameters into one flat fp32 device buffer laid out by the
  native executor (reverse registration order, KRSC conv filters exposed as strided
  [K,C,R,S] views) plus its bf16 shadow; gradients are views into a flat grad buffer.
* ``forward`` runs the whole network through ``dtc_rn18_forward`` and ``backward`` through
  ``dtc_rn18_backward`` (one autograd node). Nothing falls back to torch compute: the module
  refuses to run on the CPU.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import threading
import weakref
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from ._native import NativeError, call, lib, ptr, require_cuda, stream_ptr


# ----------------------------------------------------------------------------- autocast state
# torch semantics: inside `autocast()` (trainer.py:153, the --amp path) the network computes in reduced
# precision (bf16 here, fp16 in the reference), outside it in fp32 (trainer.py:160-165 without --amp).
# amp.autocast flips this thread-local flag; ResNet.forward picks the executor precision from it
# unless the module's `precision` attribute forces one ("bf16" / "fp32").
_AUTOCAST = threading.local()


def is_autocast_enabled() -> bool:
    return bool(getattr(_AUTOCAST, "enabled", False))


def set_autocast_enabled(enabled: bool) -> None:
    _AUTOCAST.enabled = bool(enabled)


PRECISIONS = ("bf16", "fp32")
GRAD_COMPRESSIONS = (None, "bf16", "powersgd")  # ResNet.grad_compression


# ----------------------------------------------------------------------------- layout
@dataclass
class ParamInfo:
    name: str
    offset: int
    numel: int
    shape: Tuple[int, ...]
    stride: Tuple[int, ...]


@dataclass
class BNInfo:
    prefix: str
    channels: int
    mean_offset: int
    var_offset: int


class Layout:
    """Batch-independent parameter / buffer / bucket layout reported by the executor."""

    def __init__(self, num_classes: int = 100, bucket_cap_mb: float = 25.0):
        h = C.c_void_p()
        call("dtc_rn18_create", C.byref(h), 1, 32, 32, num_classes, float(bucket_cap_mb))
        try:
            self.params: List[ParamInfo] = []
            for i in range(lib.dtc_rn18_num_params(h)):
                name = C.c_char_p()
                off, numel = C.c_int64(), C.c_int64()
                nd = C.c_int()
                shp = (C.c_int64 * 4)()
                strd = (C.c_int64 * 4)()
                call("dtc_rn18_param_info", h, i, C.byref(name), C.byref(off), C.byref(numel), C.byref(nd), shp, strd)
                self.params.append(ParamInfo(name.value.decode(), off.value, numel.value,
                                             tuple(shp[: nd.value]), tuple(strd[: nd.value])))
            self.bns: List[BNInfo] = []
            for i in range(lib.dtc_rn18_num_bn(h)):
                pre = C.c_char_p()
                ch = C.c_int()
                mo, vo = C.c_int64(), C.c_int64()
                call("dtc_rn18_bn_info", h, i, C.byref(pre), C.byref(ch), C.byref(mo), C.byref(vo))
                self.bns.append(BNInfo(pre.value.decode(), ch.value, mo.value, vo.value))
            self.flat_numel = lib.dtc_rn18_flat_numel(h)
            self.bufs_numel = lib.dtc_rn18_bufs_numel(h)
            self.buckets = []
            for i in range(lib.dtc_rn18_num_buckets(h)):
                o, n = C.c_int64(), C.c_int64()
                call("dtc_rn18_bucket_info", h, i, C.byref(o), C.byref(n))
                self.buckets.append((o.value, n.value))
        finally:
            lib.dtc_rn18_destroy(h)


class FlatState:
    """Device buffers shared by every executor of one model."""

    def __init__(self, layout: Layout, device: torch.device):
        self.layout = layout
        self.device = device
        self.params = torch.zeros(layout.flat_numel, dtype=torch.float32, device=device)
        self.grads = torch.zeros(layout.flat_numel, dtype=torch.float32, device=device)
        self.params_bf16 = torch.zeros(layout.flat_numel, dtype=torch.bfloat16, device=device)
        self.bufs = torch.zeros(layout.bufs_numel, dtype=torch.float32, device=device)
        self.nbt = torch.zeros(len(layout.bns), dtype=torch.int64, device=device)
        # optim.clip_grad_norm_: the device-side gradient multiplier the next optimizer step applies
        self.grad_mult = None
        self.norm_ws = None
        self.clip_pending = False
        self._grad_acc = None
        self._grad_c16 = None
        self._grad_err = None

    @property
    def grad_err(self) -> torch.Tensor:
        """The error-feedback buffer of PowerSGD (ResNet.grad_compression = "powersgd"): the layout of `grads`,
        zeros, allocated on first use. It holds what the low-rank approximations have left out so far."""
        if self._grad_err is None:
            self._grad_err = torch.zeros_like(self.grads)
        return self._grad_err

    @property
    def grad_c16(self) -> torch.Tensor:
        """The bf16 staging buffer of gradient compression (ResNet.grad_compression): `grads`' element layout in
        bf16, allocated on first use. The bucket all-reduces of a compressed backward run on it."""
        if self._grad_c16 is None:
            self._grad_c16 = torch.zeros(self.grads.numel(), dtype=torch.bfloat16, device=self.device)
        return self._grad_c16

    @property
    def grad_acc(self) -> torch.Tensor:
        """The gradient-accumulation buffer (ResNet.accumulate): the layout of `grads`, allocated on first use."""
        if self._grad_acc is None:
            self._grad_acc = torch.zeros_like(self.grads)
        return self._grad_acc

    def refresh_bf16(self):
        ops.cast_f32_bf16(self.params, self.params_bf16)


def _check_weights(flat: FlatState, weights) -> None:
    """`weights` must hold params / params_bf16 / bufs tensors shaped and placed as `flat`'s."""
    for attr in ("params", "params_bf16", "bufs"):
        t, own = getattr(weights, attr, None), getattr(flat, attr)
        if not isinstance(t, torch.Tensor) or t.dtype != own.dtype or t.shape != own.shape or t.device != own.device:
            raise NativeError(f"weights.{attr} must be a {own.dtype} tensor of {own.numel()} elements on {own.device} "
                              "(the model's flat layout)")


class Executor:
    """One native executor (plan + workspace) for a fixed (batch, height, width)."""

    def __init__(self, flat: FlatState, batch: int, height: int, width: int, num_classes: int, bucket_cap_mb: float,
                 capture: bool = False, precision: str = "bf16"):
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
        self.handle = C.c_void_p()
        call("dtc_rn18_create", C.byref(self.handle), batch, height, width, num_classes, float(bucket_cap_mb))
        self.precision = precision
        if precision == "fp32":
            call("dtc_rn18_set_precision", self.handle, 1)
        if capture:
            call("dtc_rn18_enable_capture", self.handle)
        nbytes = lib.dtc_rn18_workspace_bytes(self.handle)
        # 256-byte aligned workspace (the caching allocator returns 512-byte aligned blocks)
        self.workspace = torch.empty(nbytes + 256, dtype=torch.uint8, device=flat.device)
        base = self.workspace.data_ptr()
        self.ws_ptr = (base + 255) // 256 * 256
        self.flat = flat
        self.batch, self.height, self.width, self.num_classes = batch, height, width, num_classes
        self.generation = 0
        self._bwd_gen = 0  # generation whose forward a backward has consumed (one backward per forward)
        self._dlogits = None
        self._accum_mode = ops.ACCUM_OFF  # dtc_rn18_bind leaves the executor there
        self._compress_mode = ops.COMPRESS_OFF  # (likewise)
        call("dtc_rn18_bind", self.handle, self.ws_ptr, ptr(flat.params), ptr(flat.grads), ptr(flat.params_bf16),
             ptr(flat.bufs), ptr(flat.nbt), stream_ptr())

    def forward(self, x: torch.Tensor, logits: torch.Tensor, train: bool) -> int:
        call("dtc_rn18_forward", self.handle, ptr(x), ptr(logits), int(bool(train)), stream_ptr())
        self.generation += 1
        return self.generation

    def eval_batch(self, x: torch.Tensor, labels: torch.Tensor, n_valid: int, topk: int, rec: torch.Tensor,
                   logits: Optional[torch.Tensor] = None, weights=None) -> int:
        """One evaluation batch (dtc_rn18_eval_batch): the eval-mode forward of the first `n_valid` images of
        x (fp32 NCHW, contiguous) and their loss / top-1 / top-k counts against `labels` (int64) into `rec`
        (a contiguous int32 [4] device tensor, see ops.eval_metrics), enqueued with no host synchronisation.
        `logits` (fp32 [batch, num_classes]) receives the logits when given. The call overwrites the
        BatchNorm statistics a training forward saved, so it starts a new generation: a backward still
        pending on an earlier training forward is refused by consume(). `weights` (anything with `params`,
        `params_bf16` and `bufs` tensors of the model's layout on its device, e.g. a ModelEma) evaluates those
        instead of the bound buffers (dtc_rn18_eval_batch_weights), which stay bound and untouched."""
        if weights is not None:
            _check_weights(self.flat, weights)
            ops.eval_batch_weights(self.handle, weights.params, weights.params_bf16, weights.bufs, x, labels, n_valid,
                                   topk, rec, logits)
        else:
            call("dtc_rn18_eval_batch", self.handle, ptr(x), ptr(labels), int(n_valid), int(topk), ptr(logits),
                 ptr(rec), stream_ptr())
        self.generation += 1
        return self.generation

    def consume(self, gen: int) -> None:
        """Claim the forward of generation `gen` for one backward. The kernels WRITE gradients, which
        equals the reference's zero_grad() + backward(); a second backward over the same forward
        (retain_graph=True) would have to ACCUMULATE into .grad in torch, so it is refused instead of
        silently returning the first backward's gradients."""
        if gen != self.generation:
            raise NativeError("ResNet backward: the executor ran another forward since this graph was built "
                              "(one forward per backward is supported)")
        if gen == self._bwd_gen:
            raise NativeError("ResNet backward: this forward was already back-propagated (a second backward "
                              "would accumulate gradients in torch; the native kernels write them): run "
                              "the forward again")
        self._bwd_gen = gen

    def set_grad_accum(self, mode: int) -> None:
        """The accumulation mode of the next backwards (dtc_rn18_set_grad_accum, sticky), on the model's
        `flat.grad_acc`; the library is called only when the mode changes."""
        if mode != self._accum_mode:
            call("dtc_rn18_set_grad_accum", self.handle, None if mode == ops.ACCUM_OFF else ptr(self.flat.grad_acc),
                 int(mode))
            self._accum_mode = mode

    def set_grad_compress(self, mode: int) -> None:
        """The gradient-compression mode of the next backwards (dtc_rn18_set_grad_compress, sticky), staged in the
        model's `flat.grad_c16`; the library is called only when the mode changes."""
        if mode != self._compress_mode:
            call("dtc_rn18_set_grad_compress", self.handle,
                 None if mode == ops.COMPRESS_OFF else ptr(self.flat.grad_c16), int(mode))
            self._compress_mode = mode

    def backward(self, dlogits: torch.Tensor, grad_scale: float, comm) -> None:
        call("dtc_rn18_backward", self.handle, ptr(dlogits), float(grad_scale), comm.handle if comm else None,
             stream_ptr())

    def xent_backward(self, logits, labels, lse, gscale, grad_scale: float, comm) -> None:
        """CrossEntropy backward into the executor's dlogits buffer + the network backward, one call.
        Runs right after the per-step barrier, when the GPU is idle until it returns: the current
        stream is read with torch's raw-stream call (torch.cuda.current_stream() builds a Stream object
        through several Python device lookups)."""
        call("dtc_rn18_xent_backward", self.handle, logits.data_ptr(), labels.data_ptr(), lse.data_ptr(),
             None if gscale is None else gscale.data_ptr(), float(grad_scale), comm.handle if comm else None,
             _raw_stream(logits.device.index))

    def xent_soft_backward(self, logits, soft, lse, gscale, grad_scale: float, comm) -> None:
        """xent_backward for a soft target (`soft`: a _Soft): dtc_rn18_xent_soft_backward."""
        call("dtc_rn18_xent_soft_backward", self.handle, logits.data_ptr(), soft.labels_a.data_ptr(),
             None if soft.labels_b is None else soft.labels_b.data_ptr(),
             None if soft.lam is None else soft.lam.data_ptr(), soft.smoothing, lse.data_ptr(),
             None if gscale is None else gscale.data_ptr(), float(grad_scale), comm.handle if comm else None,
             _raw_stream(logits.device.index))

    def dlogits_buffer(self) -> torch.Tensor:
        """fp32 [batch, num_classes] view of the executor's own dlogits buffer: a loss gradient
        written here is consumed by backward() without the copy-in."""
        if self._dlogits is None:
            off = C.c_size_t()
            call("dtc_rn18_dlogits_buffer", self.handle, C.byref(off))
            start = self.ws_ptr - self.workspace.data_ptr() + off.value
            nbytes = self.batch * self.num_classes * 4
            self._dlogits = self.workspace[start:start + nbytes].view(torch.float32).view(self.batch,
                                                                                         self.num_classes)
        return self._dlogits

    def activations(self, captures: bool = False) -> Dict[str, torch.Tensor]:
        """Views of the per-layer activations the last forward left in the workspace (NHWC); with
        captures=True the backward intermediates recorded by a capture-enabled executor."""
        base = self.ws_ptr - self.workspace.data_ptr()
        out = {}
        count = lib.dtc_rn18_num_captures if captures else lib.dtc_rn18_num_activations
        info = "dtc_rn18_capture_info" if captures else "dtc_rn18_activation_info"
        for i in range(count(self.handle)):
            name = C.c_char_p()
            off = C.c_size_t()
            shp = (C.c_int * 4)()
            call(info, self.handle, i, C.byref(name), C.byref(off), shp)
            nm = name.value.decode()
            dt = torch.float32 if (nm.endswith("_f32") or self.precision == "fp32") else torch.bfloat16
            numel = shp[0] * shp[1] * shp[2] * shp[3]
            nbytes = numel * (4 if dt == torch.float32 else 2)
            o = base + off.value
            out[nm] = self.workspace[o:o + nbytes].view(dt).view(shp[0], shp[1], shp[2], shp[3])
        return out

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            lib.dtc_rn18_destroy(h)
            self.handle = None


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_stream(index) -> int:
    """Current HIP stream of device `index` (same value as stream_ptr() on that device)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(index if index is not None else torch.cuda.current_device())
    return stream_ptr()


# ----------------------------------------------------------------------------- PowerSGD
class PowerSGD:
    """PowerSGD on a model's flat gradients (ResNet.grad_compression = "powersgd"; set up by
    DistributedDataParallel.register_comm_hook). `state` is a parallel.PowerSGDState or torch's, read by attribute
    name; its `iter` counts the reducing backwards, as torch's hook does: the first `start_powerSGD_iter` of them
    take the native Reducer, every later one runs the executor without a communicator and then `step()`: five
    launches and two small collectives on the caller's stream (ops.psgd_step). The plan, the staging / Q buffers
    (Q drawn once on the CPU from the state's seed) and `flat.grad_err` are made at the first compressed step;
    after it nothing is allocated, copied from the host or waited for.

    A non-finite step writes NaN into the compressed gradients (GradScaler then skips the step on every rank) and
    leaves the error buffer and the warm-start Q as they were. A change of the loss scale leaves the error buffer
    in the old scale for one step, as in torch."""

    def __init__(self, state, flat: Optional["FlatState"] = None):
        rank = getattr(state, "matrix_approximation_rank")
        if not isinstance(rank, int) or not 1 <= rank <= ops.PSGD_MAX_RANK:
            raise ValueError(f"matrix_approximation_rank must be an integer in [1, {ops.PSGD_MAX_RANK}] (the "
                             f"kernels' maximum), not {rank!r}")
        if not getattr(state, "warm_start", True):
            raise NotImplementedError("PowerSGD with warm_start=False is not supported: it would draw a new Q on the "
                                      "host at every step")
        self.state = state
        self.rank = rank
        self.start = int(state.start_powerSGD_iter)
        self.min_compression_rate = state.min_compression_rate
        self.error_feedback = bool(state.use_error_feedback)
        self.eps = float(getattr(state, "orthogonalization_epsilon", 0.0))
        seed = getattr(state, "random_seed", None)
        if seed is None:  # torch's state keeps only a numpy RandomState seeded with it: draw the seed as its hook does
            seed = int(state.rng.randint(1_000_000_000))
        self.seed = int(seed)
        if not hasattr(state, "iter"):
            state.iter = 0
        self.plan = self.staging = self.q = self.dev_state = None
        self.flat = flat  # the model's flat buffers: given here, or known from the first compressed step

    def take(self) -> bool:
        """Count one reducing backward; True when it is a compressed one."""
        compress = self.state.iter >= self.start
        self.state.iter += 1
        return compress

    def _setup(self, flat: "FlatState") -> None:
        self.flat = flat
        self.plan = ops.psgd_plan(flat.layout, self.rank, self.min_compression_rate, flat.device)
        self.staging, self.q, self.dev_state = ops.psgd_buffers(self.plan, self.seed, flat.device)
        if self.error_feedback:
            flat.grad_err  # noqa: B018 - allocated here, not inside a later step

    def _shape(self) -> dict:
        """The hyperparameters that shape the plan and the buffers: a saved state loads only under the same ones."""
        return {"matrix_approximation_rank": self.rank, "min_compression_rate": self.min_compression_rate,
                "use_error_feedback": self.error_feedback, "random_seed": self.seed}

    def state_dict(self) -> dict:
        """What a resumed run needs: ``iter`` and, once a compressed step has run, the plan-shaping hyperparameters,
        both copies of Q (``q``), the device record that says which copy is the warm start (``dev_state``) and,
        with error feedback, THIS RANK's ``flat.grad_err`` -- the only entry that differs between the ranks. The
        tensors are the live device buffers (copy to keep). ``staging`` is scratch: every step writes it whole
        before reading it (csrc/powersgd.hip, steps 2 and 3)."""
        out = {"iter": int(self.state.iter)}
        if self.plan is None:
            return out
        out.update(self._shape(), q=self.q, dev_state=self.dev_state)
        if self.error_feedback:
            out["grad_err"] = self.flat.grad_err
        return out

    @torch.no_grad()
    def load_state_dict(self, state, flat: Optional["FlatState"] = None) -> None:
        """Load ``state_dict()``. A state saved after a compressed step builds the plan and the buffers first (on
        `flat`, or the buffers already known) and is refused under other plan-shaping
        hyperparameters; one saved before it only sets ``iter``."""
        if "q" in state:
            diff = {k: (state.get(k), v) for k, v in self._shape().items() if state.get(k) != v}
            if diff:
                raise ValueError("PowerSGD.load_state_dict: the state was saved under other hyperparameters: "
                                 + ", ".join(f"{k} = {a!r} (now {b!r})" for k, (a, b) in diff.items()))
            flat = flat if flat is not None else self.flat
            if flat is None:
                raise NativeError("PowerSGD.load_state_dict: the model's flat buffers are not known yet (load "
                                  "through DistributedDataParallel.load_comm_hook_state_dict)")
            if self.error_feedback and "grad_err" not in state:
                raise KeyError("PowerSGD.load_state_dict: use_error_feedback is on but the state has no 'grad_err'")
            if self.plan is None:
                self._setup(flat)
            pairs = [(self.q, state["q"], "q"), (self.dev_state, state["dev_state"], "dev_state")]
            if self.error_feedback:
                pairs.append((flat.grad_err, state["grad_err"], "grad_err"))
            for own, t, name in pairs:
                if tuple(t.shape) != tuple(own.shape) or t.dtype != own.dtype:
                    raise ValueError(f"PowerSGD.load_state_dict: {name!r} is {t.dtype} {tuple(t.shape)}, expected "
                                     f"{own.dtype} {tuple(own.shape)}")
            for own, t, _ in pairs:
                own.copy_(t)
        self.state.iter = int(state["iter"])

    def step(self, flat: "FlatState", comm) -> None:
        if self.plan is None:
            self._setup(flat)
        world = comm.world if comm is not None else 1
        ops.psgd_step(self.plan, flat.grads, flat.grad_err if self.error_feedback else None, self.staging, self.q,
                      self.dev_state, 1.0 / world, self.eps, comm.allreduce_sum_ if comm is not None else None)


# ----------------------------------------------------------------------------- autograd nodes
class _NetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, model, exe):
        logits = torch.empty(x.shape[0], model.num_classes, dtype=torch.float32, device=x.device)
        ctx.gen = exe.forward(x, logits, model.training)
        ctx.model, ctx.exe = model, exe
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        model, exe = ctx.model, ctx.exe
        if model._pre_backward is not None:
            model._pre_backward()
        exe.consume(ctx.gen)
        grad_scale, comm = model._begin_backward(exe)
        exe.backward(dlogits.contiguous().float(), grad_scale, comm)
        model._end_backward()
        model._ensure_grads()
        return None, None, None, None


class _HostWords:
    """A ring of pinned host words the loss launch writes its value into (the item() read). The ring is
    owned here, not by torch's pinned-memory cache: a word a kernel may still write is never handed to
    another tensor. Reusing a slot first waits for the event of the step that last wrote it, and bumps
    the slot's generation: a loss that still holds the slot's earlier generation (kept past N newer
    losses) sees the mismatch in item() and reads its own device value instead."""

    N = 256

    def __init__(self):
        self.buf = torch.empty(self.N, dtype=torch.float32, pin_memory=True)
        self.events = [None] * self.N
        self.gens = [0] * self.N
        self.i = 0
        self.mu = threading.Lock()  # rank threads of the thread-group communicator share the ring

    def take(self):
        with self.mu:
            k = self.i % self.N
            self.i += 1
            ev = self.events[k]
            self.events[k] = None
            self.gens[k] += 1
            gen = self.gens[k]
        if ev is not None:
            ev.synchronize()
        return k, self.buf[k], gen

    def owns(self, k, gen):
        """True while slot k still holds the value of the loss that took it as generation `gen`."""
        return self.gens[k] == gen

    def done(self, k, ev):
        self.events[k] = ev


_HOST_WORDS: List[Optional[_HostWords]] = [None]


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        loss, lse = ops.xent_fwd(logits, labels)
        ctx.save_for_backward(logits, labels, lse)
        ctx.lse = lse
        return loss

    @staticmethod
    def backward(ctx, gloss):
        logits, labels, lse = ctx.saved_tensors
        g = gloss.reshape(1).float().contiguous()
        return ops.xent_bwd(logits, labels, lse, g), None


class MixedTarget:
    """The target of a Mixup / CutMix batch (data.DeviceLoader yields it in place of the label tensor): row b's
    target is lam[b] * onehot(labels_a[b]) + (1 - lam[b]) * onehot(labels_b[b]). labels_a, labels_b: int64 [n],
    lam: fp32 [n], all on the device already -- ``.to()`` returns the object itself (the trainer calls
    ``label.to(device)`` on whatever the loader yields)."""

    def __init__(self, labels_a: torch.Tensor, labels_b: torch.Tensor, lam: torch.Tensor):
        self.labels_a, self.labels_b, self.lam = labels_a, labels_b, lam

    def to(self, *args, **kwargs) -> "MixedTarget":
        return self


class _Soft:
    """A soft target as the kernels take it: labels_a, optional (labels_b, lam), the launch-wide smoothing. It
    travels in the `labels` slot of a NativeLoss's direct backward chain."""

    __slots__ = ("labels_a", "labels_b", "lam", "smoothing")

    def __init__(self, labels_a, labels_b, lam, smoothing: float):
        self.labels_a, self.labels_b, self.lam, self.smoothing = labels_a, labels_b, lam, float(smoothing)


class _XentSoftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, soft):
        loss, lse, _ = ops.xent_soft_fwd(logits, soft.labels_a, soft.labels_b, soft.lam, soft.smoothing)
        ctx.save_for_backward(logits, lse)
        ctx.soft = soft
        ctx.lse = lse
        return loss

    @staticmethod
    def backward(ctx, gloss):
        logits, lse = ctx.saved_tensors
        sf = ctx.soft
        g = gloss.reshape(1).float().contiguous()
        return ops.xent_soft_bwd(logits, sf.labels_a, sf.labels_b, sf.lam, sf.smoothing, lse, g), None


class NativeLoss(torch.Tensor):
    """Scalar loss of ``CrossEntropyLoss`` applied directly to the native ResNet's logits (and its
    ``GradScaler.scale`` product). Its ``backward()`` runs the known chain
    xent-backward -> network backward as two native calls, without the autograd engine's thread
    hand-off and the per-node Python/elementwise launches in between (this runs right after the
    reference's per-step ``dist.barrier()``, when the GPU queue is empty, so every host
    microsecond there is GPU idle time). Gradients are identical to the autograd path, which is
    still taken for any other use (explicit ``gradient``, ``create_graph``, ``inputs``), and any
    arithmetic on the loss returns a plain autograd tensor."""

    __torch_function__ = torch._C._disabled_torch_function_impl

    @property
    def _dtc_graph(self):
        """The autograd form of this loss (built on first use: the fast path never needs it)."""
        g = self.__dict__.get("_dtc_graph_t")
        if g is None:
            g = self._dtc_graph_fn()
            self.__dict__["_dtc_graph_t"] = g
        return g

    def backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
        fast = self._dtc_fast
        if fast is None or gradient is not None or create_graph or inputs is not None or not _FAST_BACKWARD[0]:
            return self._dtc_graph.backward(gradient, retain_graph, create_graph, inputs)
        node, logits, labels, lse, gscale = fast
        if isinstance(node, _NetFn._backward_cls):
            model, exe = node.model, node.exe
            if model._pre_backward is not None:
                model._pre_backward()
            exe.consume(node.gen)
            grad_scale, comm = model._begin_backward(exe)
            if isinstance(labels, _Soft):
                exe.xent_soft_backward(logits, labels, lse, gscale, grad_scale, comm)
            else:
                exe.xent_backward(logits, labels, lse, gscale, grad_scale, comm)
            model._end_backward()
            model._ensure_grads()
        else:  # DataParallel's gathered logits: xent backward, then the replicas' backward + reduce-add
            from .parallel import _DPFn

            if isinstance(labels, _Soft):
                dl = ops.xent_soft_bwd(logits, labels.labels_a, labels.labels_b, labels.lam, labels.smoothing, lse,
                                       gscale)
            else:
                dl = ops.xent_bwd(logits, labels, lse, gscale)
            _DPFn.backward(node, dl)
        if not retain_graph:
            self._dtc_fast = None
        return None

    # loss * c, c * loss, loss / c (e.g. the `loss / N` of a hand-written accumulation loop): the autograd form, so
    # the product back-propagates (the value held here has no history of its own)
    def __mul__(self, other):
        return self._dtc_graph * other

    __rmul__ = __mul__

    def __truediv__(self, other):
        return self._dtc_graph / other

    def item(self):
        """The loss value from the pinned host copy enqueued right after the loss kernel: waits
        for the loss, not for the whole stream (a plain ``Tensor.item()`` also waits for the
        backward and optimizer step issued since). Same value either way."""
        hc = getattr(self, "_dtc_host", None)
        if hc is None:
            return super().item()
        h, ev, ring = hc[0], hc[1], hc[2:]
        if ring and not ring[0].owns(ring[1], ring[2]):  # the slot went to a newer loss: own device value
            self._dtc_host = None
            return super().item()
        ev.synchronize()
        return h.item()

    def __float__(self):
        return float(self.item())


_FAST_BACKWARD = [True]  # tests flip this to compare against the autograd-engine path


def _wrap_loss(value: torch.Tensor, graph_fn, fast, host_copy: bool = False) -> torch.Tensor:
    """NativeLoss holding `value` (no autograd history of its own); graph_fn() builds the autograd
    form on demand (the fallback backward path)."""
    out = torch.Tensor._make_subclass(NativeLoss, value.detach(), False)
    out._dtc_graph_fn = graph_fn
    out._dtc_fast = fast
    if host_copy:
        h = torch.empty((), dtype=value.dtype, pin_memory=True)
        h.copy_(value.detach(), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        out._dtc_host = (h, ev)
    return out


# The GradScaler most recently initialised (amp.GradScaler._lazy_init): the loss kernel's call also
# enqueues loss * scale for it, while the GPU is still busy with the forward, so the scaler.scale(loss)
# after the per-step barrier -- when the GPU queue is empty -- needs no launch of its own.
_PRESCALER = [None]


def _prescaler():
    """The live GradScaler whose scale the loss kernel's call pre-multiplies, or None."""
    ref = _PRESCALER[0]
    sc = ref() if ref is not None else None
    if sc is None or sc._scale is None or not sc._enabled:
        return None
    return sc


def prescale(loss: "NativeLoss", scaled: Optional[torch.Tensor] = None, sc=None) -> None:
    """Enqueue loss * scale AND build its NativeLoss wrapper now, while the GPU is busy with the
    forward: scaler.scale(loss) after the per-step barrier then only looks it up (the wrapper's
    Tensor._make_subclass and closures cost 10-30 us of host time, all of it GPU idle time there).
    `scaled`: the product already computed by the loss launch (dtc_xent_fwd_ex) for scaler `sc`."""
    sc = sc if scaled is not None else _prescaler()
    if sc is None:
        return
    scale = sc._scale
    f = loss._dtc_fast
    wrapped = _wrap_loss(scaled if scaled is not None else ops.amp_scale(loss.detach(), scale),
                         lambda: loss._dtc_graph * scale, None if f is None else (f[0], f[1], f[2], f[3], scale))
    loss._dtc_prescaled = (wrapped, scale, sc._version)


def scaled_loss(loss: torch.Tensor, scale: torch.Tensor, version: int = -1) -> torch.Tensor:
    """loss * scale (GradScaler.scale); keeps the direct backward chain of a NativeLoss. `version` is
    the scaler's state version: a product enqueued with the loss for this very scale tensor and state
    is reused (same value: the scale only changes in update(), which bumps the version)."""
    if isinstance(loss, NativeLoss):
        f = loss._dtc_fast
        pre = loss.__dict__.get("_dtc_prescaled")
        if pre is not None and pre[1] is scale and pre[2] == version and pre[0]._dtc_fast is not None:
            # the wrapper built by prescale() (same value, same backward chain) until a backward has
            # consumed its direct chain; after that a fresh wrapper is built below
            return pre[0]
        # the value on the native kernel (GradScaler K9: no torch elementwise launch in the step)
        return _wrap_loss(ops.amp_scale(loss.detach(), scale), lambda: loss._dtc_graph * scale,
                          None if f is None else (f[0], f[1], f[2], f[3], scale))
    return loss * scale


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss() with mean reduction (reference trainer.py:40) on the native kernel.
    ``label_smoothing`` and a ``MixedTarget`` (Mixup / CutMix) make the target of a row the distribution
    (1 - eps) * (lam * onehot(ya) + (1 - lam) * onehot(yb)) + eps / ncls, on the soft-target kernels through
    the same routes; with neither, the index-label kernels run exactly as without the keyword. Class weights,
    ``ignore_index``, other reductions and probability-tensor targets are not built."""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None,
                 reduction: str = "mean", label_smoothing: float = 0.0):
        super().__init__()
        if weight is not None:
            raise NotImplementedError("CrossEntropyLoss: class weights are not built natively")
        if ignore_index != -100:
            raise NotImplementedError("CrossEntropyLoss: ignore_index is not built natively")
        if reduction != "mean" or size_average is not None or reduce is not None:
            raise NotImplementedError("CrossEntropyLoss: only the mean reduction is built natively")
        if not 0.0 <= float(label_smoothing) <= 1.0:
            raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing}")
        self.label_smoothing = float(label_smoothing)

    def _forward_soft(self, logits: torch.Tensor, target) -> torch.Tensor:
        if isinstance(target, MixedTarget):
            la, lb, lam = target.labels_a, target.labels_b, target.lam
            require_cuda(logits, la, lb, lam)
            soft = _Soft(la.long().contiguous(), lb.long().contiguous(), lam.float().contiguous(),
                         self.label_smoothing)
        else:
            if target.is_floating_point():
                raise NotImplementedError("CrossEntropyLoss: probability-tensor targets are not built natively "
                                          "(pass class indices or a MixedTarget)")
            require_cuda(logits, target)
            soft = _Soft(target.long().contiguous(), None, None, self.label_smoothing)
        if logits.dtype != torch.float32:
            logits = logits.float()
        logits = logits.contiguous()
        node = logits.grad_fn
        if torch.is_grad_enabled() and node is not None:
            from .parallel import _DPFn

            if isinstance(node, (_NetFn._backward_cls, _DPFn._backward_cls)):
                if logits.shape[0] <= 4096:  # the one-launch loss, as the index-label path below
                    sc = _prescaler()
                    if _HOST_WORDS[0] is None:
                        _HOST_WORDS[0] = _HostWords()
                    ring = _HOST_WORDS[0]
                    slot, host, gen = ring.take()
                    loss, lse, scaled = ops.xent_soft_fwd(logits, soft.labels_a, soft.labels_b, soft.lam,
                                                          soft.smoothing, None if sc is None else sc._scale, host)
                    ev = torch.cuda.Event()
                    ev.record()
                    ring.done(slot, ev)
                    out = _wrap_loss(loss, lambda: _XentSoftFn.apply(logits, soft), (node, logits, soft, lse, None))
                    out._dtc_host = (host, ev, ring, slot, gen)
                    if sc is not None:
                        prescale(out, scaled, sc)
                    return out
                loss = _XentSoftFn.apply(logits, soft)
                out = _wrap_loss(loss, lambda: loss, (node, logits, soft, loss.grad_fn.lse, None), host_copy=True)
                prescale(out)
                return out
        return _XentSoftFn.apply(logits, soft)

    def forward(self, logits: torch.Tensor, labels) -> torch.Tensor:
        if isinstance(labels, MixedTarget) or self.label_smoothing > 0.0:
            return self._forward_soft(logits, labels)
        if labels.is_floating_point():
            raise NotImplementedError("CrossEntropyLoss: probability-tensor targets are not built natively "
                                      "(pass class indices or a MixedTarget)")
        require_cuda(logits, labels)
        if logits.dtype != torch.float32:
            logits = logits.float()
        logits = logits.contiguous()
        labels = labels.long().contiguous()
        node = logits.grad_fn
        if torch.is_grad_enabled() and node is not None:
            from .parallel import _DPFn

            if isinstance(node, (_NetFn._backward_cls, _DPFn._backward_cls)):
                if logits.shape[0] <= 4096:
                    # loss + lse + scaled loss + host copy: one launch, called directly (no autograd node:
                    # the direct backward chain below needs none; the autograd form of the loss -- the
                    # same kernel's value -- is built only if a fallback backward asks for it)
                    sc = _prescaler()
                    if _HOST_WORDS[0] is None:
                        _HOST_WORDS[0] = _HostWords()
                    ring = _HOST_WORDS[0]
                    slot, host, gen = ring.take()
                    n, ncls = logits.shape
                    dev = logits.device
                    loss = torch.empty((), dtype=torch.float32, device=dev)
                    lse = torch.empty(n, dtype=torch.float32, device=dev)
                    scaled = torch.empty((), dtype=torch.float32, device=dev) if sc is not None else None
                    call("dtc_xent_fwd_ex", logits.data_ptr(), labels.data_ptr(), n, ncls, loss.data_ptr(),
                         lse.data_ptr(), None if sc is None else sc._scale.data_ptr(),
                         None if scaled is None else scaled.data_ptr(), host.data_ptr(), _raw_stream(dev.index))
                    ev = torch.cuda.Event()
                    ev.record()
                    ring.done(slot, ev)
                    out = _wrap_loss(loss, lambda: _XentFn.apply(logits, labels), (node, logits, labels, lse, None))
                    out._dtc_host = (host, ev, ring, slot, gen)
                    if sc is not None:
                        prescale(out, scaled, sc)
                    return out
                loss = _XentFn.apply(logits, labels)
                out = _wrap_loss(loss, lambda: loss, (node, logits, labels, loss.grad_fn.lse, None), host_copy=True)
                prescale(out)
                return out
        return _XentFn.apply(logits, labels)


# ----------------------------------------------------------------------------- evaluation result
class EvalResult:
    """Per-batch metrics of ``ResNet.evaluate``: arrays ``loss`` (fp32 mean cross-entropy of each batch), ``n``
    (rows), ``top1`` and ``topk`` (rows whose label ranks < 1 / < k, int32), in batch order; ``k`` is the
    top-k that was asked for."""

    def __init__(self, loss, n, top1, topk, k: int):
        import numpy as np

        self.loss = np.asarray(loss, dtype=np.float32)
        self.n = np.asarray(n, dtype=np.int32)
        self.top1 = np.asarray(top1, dtype=np.int32)
        self.topk = np.asarray(topk, dtype=np.int32)
        self.k = int(k)

    @classmethod
    def from_records(cls, records: torch.Tensor, k: int) -> "EvalResult":
        """records: an int32 [batches, 4] host tensor of dtc_eval_record words."""
        r = records.contiguous().numpy().reshape(-1, 4)
        return cls(r[:, 0].copy().view("float32"), r[:, 1], r[:, 2], r[:, 3], k)

    def __len__(self) -> int:
        return int(self.n.shape[0])

    def reference_meters(self) -> Dict[str, float]:
        """What the reference's validate / test report (trainer.py:170-215): an ``AverageMeter`` fed each
        batch's mean loss and each batch's ``accuracy`` value -- the fp32 product count * (100 / n), as
        utils.py:18-31 forms it -- with weight 1 per batch, so a short last batch counts as much as a full
        one. Keys: loss, top1, topk (0.0 for an empty evaluation, the meter's initial value)."""
        import numpy as np

        def avg(vals):
            s, cnt = 0.0, 0
            for v in vals:  # AverageMeter.update(v): sum += v * 1; avg = sum / count
                s += float(v) * 1
                cnt += 1
            return s / cnt if cnt else 0.0

        scale = (100.0 / self.n.astype(np.float64)).astype(np.float32)  # mul_(100.0 / batch_size) on an fp32 tensor
        return {"loss": avg(self.loss), "top1": avg(self.top1.astype(np.float32) * scale),
                "topk": avg(self.topk.astype(np.float32) * scale)}

    def totals(self) -> Dict[str, float]:
        """Sample-weighted totals over all rows: mean loss, top-1 / top-k accuracy in percent, row count."""
        import numpy as np

        rows = int(self.n.sum())
        if rows == 0:
            return {"loss": 0.0, "top1": 0.0, "topk": 0.0, "n": 0}
        return {"loss": float(np.dot(self.loss.astype(np.float64), self.n) / rows),
                "top1": 100.0 * int(self.top1.sum()) / rows, "topk": 100.0 * int(self.topk.sum()) / rows, "n": rows}


# ----------------------------------------------------------------------------- modules
class BasicBlock(nn.Module):
    """Parameter container with reference net.py:13-38's construction order and names."""

    expansion = 1

    def __init__(self, in_planes, planes, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.shortcut = nn.Sequential()
        if stride != 1 or in_planes != self.expansion * planes:
            self.shortcut = nn.Sequential(
                nn.Conv2d(in_planes, self.expansion * planes, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(self.expansion * planes),
            )

    def forward(self, x):  # pragma: no cover - the network runs as a whole in ResNet.forward
        raise NativeError("BasicBlock runs inside the native ResNet executor; call the ResNet module")


class ResNet(nn.Module):
    """CIFAR ResNet (net.py:86-116) whose forward/backward run on the MI355X executor."""

    def __init__(self, block=BasicBlock, num_blocks=(2, 2, 2, 2), num_classes=100, bucket_cap_mb: float = 25.0):
        super().__init__()
        if block is not BasicBlock or tuple(num_blocks) != (2, 2, 2, 2):
            raise NotImplementedError("only ResNet18 (BasicBlock, [2,2,2,2]) is built natively (reference main.py:26)")
        self.in_planes = 64
        self.num_classes = num_classes
        self.conv1 = nn.Conv2d(3, 64, kernel_size=3, stride=1, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.layer1 = self._make_layer(block, 64, num_blocks[0], stride=1)
        self.layer2 = self._make_layer(block, 128, num_blocks[1], stride=2)
        self.layer3 = self._make_layer(block, 256, num_blocks[2], stride=2)
        self.layer4 = self._make_layer(block, 512, num_blocks[3], stride=2)
        self.linear = nn.Linear(512 * block.expansion, num_classes)
        self._flat: Optional[FlatState] = None
        self._layout: Optional[Layout] = None
        self._executors: Dict[Tuple[int, int, int], Executor] = {}
        self._anchor: Optional[torch.Tensor] = None
        self._comm = None
        self._grad_scale = 1.0
        self._pre_backward = None  # set by DistributedDataParallel: runs before every native backward
        # gradient accumulation: the micro-batches per optimizer step (divides the executor's grad_scale, so a
        # window's gradient is the mean over its micro-batches), the nesting depth of accumulate() and whether a
        # window is open (flat.grad_acc holds the sum of the backwards run inside accumulate() so far)
        self.grad_accum_steps = 1
        # gradient compression of the bucket all-reduces: None, or "bf16" (torch's bf16_compress_hook; set by
        # DistributedDataParallel.register_comm_hook / gradient_compression=). Only a backward that all-reduces
        # compresses anything; the gradients the optimizer reads stay fp32.
        # "powersgd" (torch's powerSGD_hook) needs a state and so comes only through register_comm_hook, which
        # also sets `_powersgd`; it runs after the native backward, not inside the Reducer.
        self.grad_compression = None
        self._powersgd: Optional[PowerSGD] = None
        self._psgd_pending = False  # the backward that is running is followed by a PowerSGD step
        self._accum_depth = 0
        self._accum_open = False
        self._local_depth = 0  # nesting depth of local_grads()
        self._bucket_cap_mb = float(bucket_cap_mb)
        self._capture = False
        self._sync_bn = False  # SyncBatchNorm.convert_sync_batchnorm marks the module
        self._sync_comm = None  # communicator the executors all-reduce BN sums over
        # None: follow autocast (bf16 inside, fp32 outside, as torch); "bf16" / "fp32": force
        self.precision: Optional[str] = None

    def _make_layer(self, block, planes, num_blocks, stride):
        strides = [stride] + [1] * (num_blocks - 1)
        layers = []
        for s in strides:
            layers.append(block(self.in_planes, planes, s))
            self.in_planes = planes * block.expansion
        return nn.Sequential(*layers)

    # ------------------------------------------------------------------ device placement
    def _apply(self, fn, recurse=True):
        if self._flat is not None:
            return self  # parameters are pinned in the flat device buffers
        out = super()._apply(fn, recurse)
        dev = self.conv1.weight.device
        if dev.type == "cuda":
            self._materialize(dev)
        return out

    def _resolve(self, dotted: str):
        parts = dotted.split(".")
        mod = self
        for p in parts[:-1]:
            mod = getattr(mod, p)
        return mod, parts[-1]

    def _materialize(self, device: torch.device):
        layout = Layout(self.num_classes, self._bucket_cap_mb)
        names = [n for n, _ in self.named_parameters()]
        if names != [p.name for p in layout.params]:
            raise NativeError("module parameters do not match the executor layout")
        flat = FlatState(layout, device)
        with torch.no_grad():
            for info in layout.params:
                mod, attr = self._resolve(info.name)
                old = getattr(mod, attr)
                view = torch.as_strided(flat.params, info.shape, info.stride, info.offset)
                view.copy_(old.detach().to(device))
                newp = nn.Parameter(view, requires_grad=old.requires_grad)
                newp._dtc_model = weakref.ref(self)
                mod._parameters[attr] = newp
            for i, bn in enumerate(layout.bns):
                mod, _ = self._resolve(bn.prefix + ".x")
                rm = flat.bufs.narrow(0, bn.mean_offset, bn.channels)
                rv = flat.bufs.narrow(0, bn.var_offset, bn.channels)
                rm.copy_(mod.running_mean.to(device))
                rv.copy_(mod.running_var.to(device))
                flat.nbt[i].copy_(mod.num_batches_tracked.to(device))
                mod._buffers["running_mean"] = rm
                mod._buffers["running_var"] = rv
                mod._buffers["num_batches_tracked"] = flat.nbt[i]
        self._layout = layout
        self._flat = flat
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self._attach_grads()
        flat.refresh_bf16()

    def _attach_grads(self):
        for info in self._layout.params:
            mod, attr = self._resolve(info.name)
            mod._parameters[attr].grad = torch.as_strided(self._flat.grads, info.shape, info.stride, info.offset)

    def _ensure_grads(self):
        if self.linear.bias.grad is None or self.conv1.weight.grad is None:
            self._attach_grads()

    @property
    def flat(self) -> FlatState:
        if self._flat is None:
            raise NativeError("ResNet must be moved to a GPU (`.to('cuda')`) before use")
        return self._flat

    def sync_weights(self):
        """Re-derive the bf16 shadow after parameters were modified outside the native SGD."""
        self.flat.refresh_bf16()

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        if assign:
            raise NotImplementedError("assign=True would detach parameters from the flat buffer")
        res = super().load_state_dict(state_dict, strict=strict)
        if self._flat is not None:
            self._flat.refresh_bf16()
        return res

    def buckets(self):
        """Gradient buckets [(flat offset, numel)] in the order backward completes them."""
        return Layout(self.num_classes, self._bucket_cap_mb).buckets

    def set_bucket_cap_mb(self, mb: float):
        self._bucket_cap_mb = float(mb)
        self._executors.clear()

    def compute_precision(self) -> str:
        """The precision the next forward runs in: `self.precision` when set ("bf16" / "fp32"),
        else torch's rule -- bf16 inside `autocast()`, fp32 outside (trainer.py:152-165)."""
        if self.precision is not None:
            if self.precision not in PRECISIONS:
                raise ValueError(f"precision must be None or one of {PRECISIONS}, not {self.precision!r}")
            return self.precision
        return "bf16" if is_autocast_enabled() else "fp32"

    def executor(self, batch: int, height: int, width: int, precision: Optional[str] = None) -> Executor:
        precision = precision or self.compute_precision()
        key = (batch, height, width, precision)
        exe = self._executors.get(key)
        if exe is None:
            exe = Executor(self.flat, batch, height, width, self.num_classes, self._bucket_cap_mb,
                           capture=self._capture, precision=precision)
            if self._sync_comm is not None:
                call("dtc_rn18_set_sync_bn", exe.handle, self._sync_comm.handle)
            self._executors[key] = exe
        return exe

    def set_sync_bn(self, comm) -> None:
        """Synchronise training-mode BN statistics over `comm` (a parallel.Comm of its own, not the
        Reducer's); None restores per-rank statistics. Applies to existing and new executors."""
        self._sync_comm = comm
        for exe in self._executors.values():
            call("dtc_rn18_set_sync_bn", exe.handle, comm.handle if comm is not None else None)

    def enable_capture(self, on: bool = True):
        """Keep backward intermediates for per-layer parity tests (new executors only)."""
        self._capture = on
        self._executors.clear()

    # ------------------------------------------------------------------ gradient accumulation
    @contextlib.contextmanager
    def accumulate(self):
        """Accumulate gradients over micro-batches: the standard N x (forward, backward), one optimizer.step()
        loop. The native kernels write gradients, so the sum is kept in ``flat.grad_acc``. A backward inside
        this context adds its gradients there (the first of a window stores them) and all-reduces nothing --
        under DistributedDataParallel this is ``no_sync()``. The first backward OUTSIDE the context closes the
        window: its gradients plus the accumulated sum land in ``.grad`` / ``flat.grads`` ahead of each bucket's
        all-reduce, so the collective (and then GradScaler's finiteness check, clipping and the optimizer) sees
        the whole window. With no window open a backward is exactly the plain one.

            model.grad_accum_steps = N                    # gradients become the mean over the N micro-batches
            for i, (x, y) in enumerate(micro_batches):
                with model.accumulate() if i < N - 1 else contextlib.nullcontext():
                    criterion(model(x), y).backward()
            optimizer.step()

        ``grad_accum_steps`` divides the gradient scale of every backward, so the loss needs no ``/ N`` (and
        ``NativeLoss.backward`` keeps its direct path); with ``grad_accum_steps = 1`` a ``(loss / N).backward()``
        through autograd gives the same mean. ``.grad`` between the backwards of a window shows the last
        micro-batch's gradients, not the running sum."""
        self._accum_depth += 1
        try:
            yield self
        finally:
            self._accum_depth -= 1

    def reset_accumulation(self) -> None:
        """Drop an open accumulation window: the next backward outside accumulate() is a plain one."""
        self._accum_open = False

    @contextlib.contextmanager
    def local_grads(self):
        """Backwards inside this context write this rank's own gradients and nothing else: no communicator
        (nothing is all-reduced or compressed, whatever wrapper the model is in) and accumulation mode OFF. It is
        SAM's first backward (optim.SAM): under DistributedDataParallel every rank then perturbs along its own
        un-reduced gradient. Refused while an accumulation window is open or with ``grad_accum_steps != 1`` -- the
        local gradient would be neither the window's nor a whole step's. Outside the context nothing changes."""
        self._check_local_grads()
        self._local_depth += 1
        try:
            yield self
        finally:
            self._local_depth -= 1

    def _check_local_grads(self) -> None:
        if self._accum_open or self._accum_depth > 0:
            raise NativeError("local_grads(): a gradient-accumulation window is open (accumulate() / no_sync())")
        if self.grad_accum_steps != 1:
            raise NativeError(f"local_grads() needs grad_accum_steps == 1, not {self.grad_accum_steps!r}")

    def _begin_backward(self, exe: Executor):
        """(grad_scale, comm) of the native backward about to run on `exe`, whose accumulation mode is set
        from the window's state: STORE / ADD without a communicator inside accumulate(), FINISH for the backward
        that closes a window, OFF otherwise; its compression mode from `grad_compression`. Inside local_grads():
        OFF and no communicator. With PowerSGD armed, a reducing backward past the state's start iteration also runs
        without a communicator (its accumulation mode as usual: FINISH still folds the window's sum in) and
        _end_backward() runs the PowerSGD step on the gradients it left."""
        if self.grad_compression not in GRAD_COMPRESSIONS:
            raise ValueError(f"grad_compression must be one of {GRAD_COMPRESSIONS}, not {self.grad_compression!r}")
        steps = self.grad_accum_steps
        if not isinstance(steps, int) or steps < 1:
            raise ValueError(f"grad_accum_steps must be an integer >= 1, not {steps!r}")
        comm = self._comm
        if self._local_depth > 0:
            self._check_local_grads()  # (an accumulate() entered inside the context)
            mode, comm = ops.ACCUM_OFF, None
        elif self._accum_depth > 0:
            mode, comm = (ops.ACCUM_ADD if self._accum_open else ops.ACCUM_STORE), None
        else:
            mode = ops.ACCUM_FINISH if self._accum_open else ops.ACCUM_OFF
            if self.grad_compression == "powersgd":
                if self._powersgd is None:
                    raise NativeError('grad_compression = "powersgd" needs a state: use DistributedDataParallel.'
                                      'register_comm_hook(PowerSGDState(...), powerSGD_hook)')
                if self._powersgd.take():
                    self._psgd_pending, comm = True, None
        exe.set_grad_accum(mode)
        exe.set_grad_compress(ops.COMPRESS_BF16 if self.grad_compression == "bf16" else ops.COMPRESS_OFF)
        return self._grad_scale / steps, comm

    def _end_backward(self) -> None:
        self._accum_open = self._accum_depth > 0
        if self._psgd_pending:
            self._psgd_pending = False
            self._powersgd.step(self.flat, self._comm)

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        flat = self.flat
        require_cuda(x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [N,3,H,W] input, got {tuple(x.shape)}")
        if x.dtype != torch.float32 or not x.is_contiguous():
            x = x.float().contiguous()
        exe = self.executor(x.shape[0], x.shape[2], x.shape[3])
        return _NetFn.apply(x, self._anchor, self, exe)

    # ------------------------------------------------------------------ evaluation
    def evaluate(self, batches, topk: int = 5, weights=None) -> EvalResult:
        """The reference's validate / test loop (trainer.py:170-215) on the device: for every (images, labels)
        batch one native call enqueues the eval-mode forward and the batch's loss / top-1 / top-k counts into
        the next slot of one device record buffer -- no host synchronisation per batch -- and ONE
        device-to-host copy at the end brings all records back. Runs under no_grad semantics (nothing is
        recorded for autograd, running statistics are used and left untouched, whatever ``self.training``
        says) in the current ``compute_precision()``. The executor is the one for the first batch's size; a
        smaller batch (the short last one) runs on it through ``n_valid``, a larger one takes the executor
        of its own size. `batches` needs a length (a list or a loader), else it is materialised first.
        `weights` (see Executor.eval_batch; e.g. a ModelEma) evaluates other weights of this model's layout in
        place of its own, which are left untouched."""
        flat = self.flat
        if weights is not None:
            _check_weights(flat, weights)
        if not hasattr(batches, "__len__"):
            batches = list(batches)
        precision = self.compute_precision()
        dev = flat.device
        cap = len(batches)
        recs = torch.empty(max(cap, 1), 4, dtype=torch.int32, device=dev)
        first = None
        i = 0
        with torch.no_grad():
            for x, y in batches:
                if i >= cap:
                    raise NativeError(f"evaluate: the loader yielded more than its len() = {cap} batches")
                x = x.to(dev, non_blocking=True)
                y = y.to(dev, non_blocking=True)
                if x.dim() != 4 or x.shape[1] != 3:
                    raise ValueError(f"expected [N,3,H,W] input, got {tuple(x.shape)}")
                if x.dtype != torch.float32 or not x.is_contiguous():
                    x = x.float().contiguous()
                if y.dtype != torch.int64 or not y.is_contiguous():
                    y = y.long().contiguous()
                n, h, w = x.shape[0], x.shape[2], x.shape[3]
                if y.dim() != 1 or y.shape[0] != n:
                    raise ValueError(f"expected {n} labels, got {tuple(y.shape)}")
                if first is None:
                    first = self.executor(n, h, w, precision)
                exe = first
                if n > exe.batch or (h, w) != (exe.height, exe.width):
                    exe = self.executor(n, h, w, precision)
                exe.eval_batch(x, y, n, topk, recs[i], weights=weights)
                i += 1
        return EvalResult.from_records(recs[:i].cpu(), topk)  # the one device-to-host copy (and wait)


class SyncBatchNorm:
    """``nn.SyncBatchNorm.convert_sync_batchnorm`` for the native ResNet (README.md:40 recommends
    it; the reference trainers do not call it). The BN modules stay where they are (same
    state_dict keys); the model is marked, and ``DistributedDataParallel`` gives it a second RCCL
    communicator over which every training-mode BN all-reduces its per-channel sums
    (include/dtc.h ``dtc_rn18_set_sync_bn``). As in torch, a one-rank group keeps local statistics."""

    @staticmethod
    def convert_sync_batchnorm(module, process_group=None):
        if not isinstance(module, ResNet):
            raise NotImplementedError("convert_sync_batchnorm: only the native ResNet18 is supported")
        module._sync_bn = True
        module._sync_bn_group = process_group
        return module


def ResNet18(num_classes: int = 100) -> ResNet:
    """net.py:119-120."""
    return ResNet(BasicBlock, [2, 2, 2, 2], num_classes=num_classes)
