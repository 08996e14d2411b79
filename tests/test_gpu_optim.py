"""Fused Adam / AdamW and the device-side gradient-norm clip against torch itself.

The reference of every numeric check is the installed torch on the CPU in float64 (torch.optim.Adam / AdamW,
torch.nn.utils.clip_grad_norm_) on the same seeded inputs. Bound for the optimizer state: with p64 torch's
float64 run and p32 torch's own float32 run of the same steps,

    max|p_gpu - p64| <= 2 * max|p32 - p64|

(the factor 2 allows for FMA contraction and a different, equally valid fp32 operation order), the same for
exp_avg and exp_avg_sq. Sizes: 4 (one float4), 4096 (one partial block of the last trip) and 2,098,180 =
2048 * 256 * 4 + 1028, just past one full trip of the update kernel's capped grid.

Measured on an MI355X: the kernel follows the operation order of torch's CPU kernels, so max|gpu - f64| equals
torch's own max|f32 - f64| on 116 of the 117 printed checks; the other one (Adam, wd = 1e-4, lr = 0.1,
g * 1e-3, n = 4, p) is at 1.47x.
"""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [4, 4096, 2_098_180]
KINDS = [("adam", 0.0), ("adam", 1e-4), ("adamw", 1e-2)]


def _inputs(n, gscale, steps, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * gscale for _ in range(steps)]
    return p0, grads


def _torch_adam(kind, wd, lr, p0, grads, dtype):
    p = torch.nn.Parameter(p0.to(dtype).clone())
    cls = torch.optim.AdamW if kind == "adamw" else torch.optim.Adam
    opt = cls([p], lr=lr, weight_decay=wd, foreach=False)
    for g in grads:
        p.grad = g.to(dtype).clone()
        opt.step()
    st = opt.state[p]
    return p.detach().double(), st["exp_avg"].double(), st["exp_avg_sq"].double()


class _GpuAdam:
    """The flat kernel driven the way GradScaler drives it: gradients pre-multiplied by 4, inv_scale = 0.25
    (both exact in fp32), found_inf on the device."""

    def __init__(self, dtc, dev, kind, wd, lr, p0):
        self.ops, self.kind, self.wd, self.lr = dtc.ops, kind, wd, lr
        self.p = p0.to(dev)
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.pb = torch.zeros(p0.numel(), dtype=torch.bfloat16, device=dev)
        self.state = dtc.ops.adam_state(dev)
        self.inv = torch.full((1,), 0.25, device=dev)
        self.found = torch.zeros(1, dtype=torch.int32, device=dev)

    def step(self, g):
        self.ops.adam_flat(self.p, (g * 4).to(self.p.device), self.m, self.v, self.pb, self.state, self.lr, 0.9,
                           0.999, 1e-8, self.wd, self.kind == "adamw", self.inv, self.found)

    def snapshot(self):
        return [t.clone() for t in (self.p, self.m, self.v, self.pb)]


def _assert_within_twice_fp32(got, ref32, ref64, what):
    for name, a, b32, b64 in zip(("p", "exp_avg", "exp_avg_sq"), got, ref32, ref64):
        err = float((a.double().cpu() - b64).abs().max())
        err32 = float((b32 - b64).abs().max())
        print(f"{what} {name}: max|gpu - f64| = {err:.3e}, torch fp32 max|f32 - f64| = {err32:.3e}")
        assert err <= 2 * err32, (what, name, err, err32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gscale", [1.0, 1e-3])
@pytest.mark.parametrize("lr", [1e-3, 1e-1])
@pytest.mark.parametrize("kind,wd", KINDS)
def test_adam_flat_matches_torch(dtc, cuda, kind, wd, lr, gscale, n):
    p0, grads = _inputs(n, gscale, 5, seed=n % 1000 + int(lr * 1000))
    ref64 = _torch_adam(kind, wd, lr, p0, grads, torch.float64)
    ref32 = _torch_adam(kind, wd, lr, p0, grads, torch.float32)
    a = _GpuAdam(dtc, cuda, kind, wd, lr, p0)
    for g in grads:
        a.step(g)
    _assert_within_twice_fp32((a.p, a.m, a.v), ref32, ref64, f"{kind} wd={wd} lr={lr} g*{gscale} n={n}")
    assert torch.equal(a.pb.float(), a.p.bfloat16().float())  # the bf16 shadow, bit for bit
    assert int(a.state[0]) == 5


@pytest.mark.parametrize("kind,wd", KINDS)
def test_adam_flat_skipped_step_leaves_everything(dtc, cuda, kind, wd):
    """found_inf = 1 ahead of the second of three steps: nothing moves, and the result is torch's after TWO
    steps -- the device-side step count (the bias corrections) did not advance on the skipped one."""
    n, lr = 4096, 1e-3
    p0, grads = _inputs(n, 1.0, 3, seed=11)
    a = _GpuAdam(dtc, cuda, kind, wd, lr, p0)
    a.step(grads[0])
    before = a.snapshot()
    a.found.fill_(1)
    a.step(grads[1])
    for was, now in zip(before, a.snapshot()):
        assert torch.equal(was, now)
    assert int(a.state[0]) == 1
    a.found.zero_()
    a.step(grads[2])
    two = [grads[0], grads[2]]
    _assert_within_twice_fp32((a.p, a.m, a.v), _torch_adam(kind, wd, lr, p0, two, torch.float32),
                              _torch_adam(kind, wd, lr, p0, two, torch.float64), f"{kind} skipped")
    assert int(a.state[0]) == 2


def test_adam_flat_is_repeatable(dtc, cuda):
    p0, grads = _inputs(2_098_180, 1.0, 3, seed=5)
    runs = []
    for _ in range(2):
        a = _GpuAdam(dtc, cuda, "adamw", 1e-2, 1e-3, p0)
        for g in grads:
            a.step(g)
        runs.append(a.snapshot())
    for x, y in zip(*runs):
        assert torch.equal(x, y)


def test_adam_flat_rejects_bad_arguments(dtc, cuda):
    """n = 6, a 4-byte-offset view, eps = 0 and beta2 = 1: an error with a message, and nothing launched (the
    parameters and the step count are untouched)."""
    ops = dtc.ops

    def bufs(n):
        return [torch.ones(n, device=cuda) for _ in range(4)] + [torch.zeros(n, dtype=torch.bfloat16, device=cuda)]

    state = ops.adam_state(cuda)
    good = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=False)
    p, g, m, v, pb = bufs(8)
    base = torch.ones(12, device=cuda)
    cases = [
        (bufs(6), good, "multiple of 4"),
        ([base[1:9], g, m, v, pb], good, "aligned"),
        ([p, g, m, v, pb], dict(good, eps=0.0), "eps"),
        ([p, g, m, v, pb], dict(good, beta2=1.0), "betas"),
    ]
    for (cp, cg, cm, cv, cpb), kw, word in cases:
        with pytest.raises(dtc.NativeError, match=word):
            ops.adam_flat(cp, cg, cm, cv, cpb, state, **kw)
    assert int(state[0]) == 0
    assert torch.equal(p, torch.ones(8, device=cuda)) and torch.equal(base, torch.ones(12, device=cuda))


# ---------------------------------------------------------------------------------------- grad_norm_clip
def _norm_input(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    if kind == "normal":
        return x, None
    if kind == "zeros":
        return torch.zeros(n), None
    if kind == "loss_scaled":
        return x * 2.0 ** 16, 2.0 ** -16
    if kind == "tiny":  # squares underflow in fp32
        return x * 1e-30, None
    z = torch.zeros(n)  # "huge": the square overflows fp32, the norm itself (1e25) does not
    z[n // 2] = 1e25
    return z, None


def _torch_clip(x, inv_scale, max_norm):
    """(total norm, clip coefficient) from torch.nn.utils.clip_grad_norm_ in float64 on the unscaled gradient; the
    coefficient is read back from what torch did to the largest element."""
    p = torch.nn.Parameter(torch.zeros(x.numel(), dtype=torch.float64))
    orig = x.double() * (1.0 if inv_scale is None else inv_scale)
    p.grad = orig.clone()
    norm = float(torch.nn.utils.clip_grad_norm_([p], max_norm, foreach=False))
    j = int(orig.abs().argmax())
    return norm, float(p.grad[j] / orig[j])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["normal", "zeros", "loss_scaled", "tiny", "huge"])
def test_grad_norm_clip_matches_torch(dtc, cuda, kind, n):
    x, inv_scale = _norm_input(kind, n, seed=n % 1000 + 7)
    xd = x.to(cuda)
    inv = None if inv_scale is None else torch.full((1,), inv_scale, device=cuda)
    isf = 1.0 if inv_scale is None else inv_scale
    ws = dtc.ops.grad_norm_workspace(n, cuda)
    if kind == "zeros":
        tn, gm = dtc.ops.grad_norm_clip(xd, 1.0, inv, ws)
        assert float(tn) == 0.0 and float(gm) == isf
        return
    ref_norm = _torch_clip(x, inv_scale, 1.0)[0]
    for factor in (0.5, 2.0):  # the first clips, the second does not
        max_norm = factor * ref_norm
        norm64, coef64 = _torch_clip(x, inv_scale, max_norm)
        tn, gm = dtc.ops.grad_norm_clip(xd, max_norm, inv, ws)
        tn2, _ = dtc.ops.grad_norm_clip(xd, max_norm, inv, ws)
        tn, gm, tn2 = tn.cpu(), gm.cpu(), tn2.cpu()
        print(f"{kind} n={n} x{factor}: norm {float(tn):.9e} vs {norm64:.9e}, mult {float(gm):.9e} vs "
              f"{coef64 * isf:.9e}")
        assert abs(float(tn.double()) - norm64) <= 2.0 ** -22 * norm64
        assert abs(float(gm.double()) - coef64 * isf) <= 2.0 ** -21 * coef64 * isf
        if kind != "tiny":  # (there torch's "+ 1e-6" dwarfs the norm and both values of max_norm clip)
            assert (coef64 < 1.0) == (factor < 1.0)
        assert torch.equal(tn.view(torch.int32), tn2.view(torch.int32))  # bit-equal from run to run


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_grad_norm_clip_nonfinite_gradient(dtc, cuda, bad):
    x = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    x[1234] = bad
    tn, _ = dtc.ops.grad_norm_clip(x.to(cuda), 1.0)
    assert not math.isfinite(float(tn))


# ---------------------------------------------------------------------------------------- through the model
def _padding_mask(flat):
    """True where the flat buffer holds no parameter element (slot alignment and row padding)."""
    mask = torch.ones(flat.layout.flat_numel, dtype=torch.bool, device=flat.params.device)
    for info in flat.layout.params:
        torch.as_strided(mask, info.shape, info.stride, info.offset).fill_(False)
    return mask


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "amp"])
def test_adamw_with_clip_through_the_model(dtc, cuda, amp):
    """Two training steps of the native ResNet18 (B = 2, 32x32) with optim.AdamW and clip_grad_norm_ (max_norm =
    half the first step's norm). After each backward the executor's own p.grad goes into torch AdamW +
    torch clip_grad_norm_ over detached copies of the parameters, in float64 and in float32."""
    torch.manual_seed(42)
    model = dtc.ResNet18().to(cuda)
    crit = dtc.CrossEntropyLoss()
    opt = dtc.optim.AdamW(model.parameters(), lr=1e-3)
    scaler = dtc.GradScaler() if amp else None
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 32, 32, generator=g).to(cuda)
    y = torch.randint(0, 100, (2,), generator=g).to(cuda)
    names = [k for k, _ in model.named_parameters()]
    refs = {}
    for dt in (torch.float64, torch.float32):
        ps = [torch.nn.Parameter(p.detach().cpu().to(dt).clone()) for _, p in model.named_parameters()]
        refs[dt] = (ps, torch.optim.AdamW(ps, lr=1e-3, foreach=False))
    mask = _padding_mask(model.flat)
    assert int(mask.sum()) == model.flat.layout.flat_numel - 11_220_132
    max_norm = None
    for step in range(2):
        opt.zero_grad()
        if amp:
            with dtc.autocast():
                loss = crit(model(x), y)
            scaler.scale(loss).backward()
            scale = scaler.get_scale()
        else:
            loss = crit(model(x), y)
            loss.backward()
            scale = 1.0
        assert not bool(model.flat.grads[mask].any())  # the backward leaves the gradient padding zero
        grads = [p.grad.detach().cpu().double() / scale for _, p in model.named_parameters()]
        if max_norm is None:
            max_norm = 0.5 * math.sqrt(sum(float((gr * gr).sum()) for gr in grads))
        norms = {}
        for dt, (ps, ropt) in refs.items():
            for p, gr in zip(ps, grads):
                p.grad = gr.to(dt).clone()
            norms[dt] = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
            ropt.step()
        if amp:
            scaler.unscale_(opt)
            tn = dtc.optim.clip_grad_norm_(model.parameters(), max_norm, scaler=scaler)
            scaler.step(opt)
            scaler.update()
        else:
            tn = dtc.optim.clip_grad_norm_(model.parameters(), max_norm)
            opt.step()
        assert tn.dim() == 0 and tn.is_cuda
        assert abs(float(tn) - norms[torch.float64]) <= 2.0 ** -22 * norms[torch.float64]
        assert model.flat.clip_pending is False
        for k, p, p64, p32 in zip(names, model.parameters(), refs[torch.float64][0], refs[torch.float32][0]):
            err = float((p.detach().cpu().double() - p64.detach()).abs().max())
            err32 = float((p32.detach().double() - p64.detach()).abs().max())
            assert err <= 2 * err32, (step, k, err, err32)
    flat = model.flat
    assert int(opt._step_state[0]) == 2
    for buf in (flat.params, flat.grads, opt._exp_avg, opt._exp_avg_sq):
        assert not bool(buf[mask].any())  # padding: p = g = 0 -> m = v = 0 and an update of 0 / (0 + eps)
    assert torch.equal(flat.params_bf16.float(), flat.params.bfloat16().float())


_TRAINER_ARGS = ["--max-steps", "2", "--epoch", "1", "--synthetic-train", "64", "--synthetic-test", "16",
                 "--batch-size", "8", "--workers", "0"]


def _run_trainer(dtc, args, ckpt):
    dtc.data.fix_seed(42)
    t = dtc.trainer.Trainer(dtc.trainer.load_config(_TRAINER_ARGS + args + ["--ckpt-path", str(ckpt)], "single"),
                            dtc.ResNet18(), None)
    t.fit()
    return t


def test_trainer_adamw_with_clip_runs(dtc, cuda, tmp_path):
    t = _run_trainer(dtc, ["--optimizer", "adamw", "--clip-grad-norm", "1"], tmp_path)
    assert isinstance(t.optimizer, dtc.optim.AdamW) and t.global_step == 2
    assert int(t.optimizer._step_state[0]) == 2 and t.model.flat.clip_pending is False
    rows = [json.loads(line) for line in open(os.path.join(t.save_path, "scalars.jsonl"))]
    losses = [r for r in rows if r["tag"] == "loss/epoch"]
    assert len(losses) == 1 and math.isfinite(losses[0]["train"]) and math.isfinite(losses[0]["val"])


def test_trainer_default_sgd_path_is_unchanged_and_repeatable(dtc, cuda, tmp_path):
    """With both new flags at their defaults the trainer builds the same SGD and never touches the clip state;
    two runs of the same two steps give identical parameters."""
    a = _run_trainer(dtc, [], tmp_path / "a")
    b = _run_trainer(dtc, [], tmp_path / "b")
    assert type(a.optimizer) is dtc.optim.SGD and a.optimizer.defaults["nesterov"] is True
    assert a.model.flat.grad_mult is None and a.model.flat.clip_pending is False
    assert torch.equal(a.model.flat.params, b.model.flat.params)
    assert torch.equal(a.optimizer._mom, b.optimizer._mom)
