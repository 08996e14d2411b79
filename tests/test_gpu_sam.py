"""SAM / ASAM: the perturb / restore kernels (dtc_sam_perturb, dtc_sam_restore), ResNet.local_grads(), optim.SAM and
its two-pass step.

The reference of the kernels is include/dtc.h's formula written with torch on the CPU,

    t = g | p * g ;  S = sum t^2 (double) ;  gn = |m| sqrt(S) ;  coef = rho m / (gn + eps) ;  e = coef g | (coef g)(p p)

evaluated in float64 (p64 = p + e64) and again in float32 (the norm still summed in double, coef rounded once to
fp32; p32). Bounds, for every size: per element |p_gpu - p64| <= 2^-21 (|p| + |e64|) -- an element sees at most five
fp32 roundings (coef, coef g, p p, their product, the sum) of quantities no larger than that, 5 * 2^-24 < 2^-21 --
and for sizes from 1020 on, where the fp32 evaluation's worst error is not zero, max|p_gpu - p64| <= 2 max|p32 - p64|,
the project's usual allowance for an equally valid fp32 operation order. Everything else here (what is saved, what
the restore brings back, the shadow, the sentinels, the model-level steps) is bit-exact.

Measured on an MI355X: the per-element ratio is at most 0.18 of its bound; max|p_gpu - p64| equals the float32
formula's in 18 of the 24 cases and is below it in the other six (all adaptive).

Every test in this file fails on the code before the feature: ops.sam_perturb, ResNet.local_grads and optim.SAM do
not exist there.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# sam.hip / kernels.h: the update and restore kernels take DTC_SAM_THREADS * DTC_SAM_UNROLL float4 rows per workgroup
# trip on a grid capped at DTC_SAM_MAX_BLOCKS; the norm pass strides 256 workgroups of 1024 threads (1 Mi elements)
THREADS, UNROLL, MAX_BLOCKS = 256, 4, 1024
CHUNK = THREADS * UNROLL * 4  # fp32 elements of one workgroup trip
# one float4; the smallest size with a non-zero fp32 error; one chunk, + 4, three chunks - 4; one grid trip of the
# capped update grid plus three chunks and a ragged one (the norm pass wraps its own grid four times there)
SIZES = [4, 1020, CHUNK, CHUNK + 4, 3 * CHUNK - 4, (MAX_BLOCKS + 3) * CHUNK + 1028]
MODES = [("plain", False, 0.05), ("adaptive", True, 2.0)]
EPS = 1e-12
BASE = 64  # elements in front of and behind every range of an arena
SENT32 = 0x7FC0DEAD  # a NaN bit pattern nothing here computes
SENT16 = 0x7FDE
KEEP_F32, KEEP_I64 = 9600, 20  # the model's BatchNorm running statistics and batch counts


def _formula(p0, g, rho, adaptive, m, dtype):
    """(p + e, e, gn, coef) of the header's formula with the element-wise part in `dtype`."""
    p, gg = p0.to(dtype), g.to(dtype)
    t = p * gg if adaptive else gg
    s = float((t.double() ** 2).sum())
    gn = abs(m) * math.sqrt(s)
    coef = rho * m / (gn + EPS)
    if dtype == torch.float32:
        coef = float(np.float32(coef))
    c = torch.tensor(coef, dtype=dtype)
    e = (c * gg) * (p * p) if adaptive else c * gg
    return (p + e).double(), e.double(), gn, coef


class _Arena:
    """p, g, p_saved (fp32) and the shadow (bf16) of n elements, each between two bands of sentinel words."""

    def __init__(self, cuda, p0, g, shadow=None):
        n = p0.numel()
        self.n = n

        def f32(vals):
            a = torch.full((n + 2 * BASE,), SENT32, dtype=torch.int32)
            if vals is not None:
                a[BASE:BASE + n] = vals.view(torch.int32)
            return a.to(cuda).view(torch.float32)

        self.p, self.g, self.saved = f32(p0), f32(g), f32(None)
        pb = torch.full((n + 2 * BASE,), SENT16, dtype=torch.int16)
        if shadow is not None:
            pb[BASE:BASE + n] = shadow.view(torch.int16)
        self.pb = pb.to(cuda).view(torch.bfloat16)
        self.state = torch.full((4,), -1, dtype=torch.int32, device=cuda)

    def rng(self, t):
        return t[BASE:BASE + self.n]

    def bands_intact(self):
        for t, word in ((self.p, SENT32), (self.g, SENT32), (self.saved, SENT32), (self.pb, SENT16)):
            w = t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
            if not (bool((w[:BASE] == word).all()) and bool((w[BASE + self.n:] == word).all())):
                return False
        return True

    def perturb(self, dtc, rho, adaptive, gmul=None, keep=None):
        dtc.ops.sam_perturb(self.rng(self.p), self.rng(self.g), self.rng(self.saved), self.rng(self.pb), self.state,
                            rho, adaptive, EPS, gmul, keep)

    def restore(self, dtc, keep=None, found_inf=None):
        dtc.ops.sam_restore(self.rng(self.p), self.rng(self.saved), self.rng(self.pb), self.state, keep, found_inf)

    def coef(self):
        return float(self.state.view(torch.float32)[0])

    def norm(self):
        return float(self.state.view(torch.float32)[1])

    def skipped(self):
        return int(self.state[2])


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=gen), torch.randn(n, generator=gen)


def _within_elementwise(p_gpu, p64, p0, e64, what):
    err = (p_gpu.double() - p64).abs()
    bound = 2.0 ** -21 * (p0.double().abs() + e64.abs())
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst |p_gpu - p64| / (2^-21 (|p| + |e|)) = {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


# ----------------------------------------------------------------------------- 1. perturb against float64
@pytest.mark.parametrize("scaled", [False, True], ids=["gmul-null", "gmul-0.25"])
@pytest.mark.parametrize("mode,adaptive,rho", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("n", SIZES)
def test_perturb_matches_float64(dtc, cuda, n, mode, adaptive, rho, scaled):
    p0, g = _inputs(n, seed=n % 1000 + 7 * adaptive)
    m = 1.0
    gmul = None
    if scaled:  # what GradScaler hands over: gradients times 4 and the device word 1 / 4, both exact
        g, m = g * 4, 0.25
        gmul = torch.full((1,), m, device=cuda)
    p64, e64, gn64, _ = _formula(p0, g, rho, adaptive, m, torch.float64)
    p32 = _formula(p0, g, rho, adaptive, m, torch.float32)[0]
    a = _Arena(cuda, p0, g)
    a.perturb(dtc, rho, adaptive, gmul)
    torch.cuda.synchronize()
    got = a.rng(a.p).cpu()
    what = f"{mode} n={n} gmul={m}"
    _within_elementwise(got, p64, p0, e64, what)
    err, err32 = float((got.double() - p64).abs().max()), float((p32 - p64).abs().max())
    print(f"{what}: max|p_gpu - p64| = {err:.3e}, fp32 formula max|p32 - p64| = {err32:.3e}")
    if n >= 1020:
        assert err32 > 0 and err <= 2 * err32, (what, err, err32)
    assert abs(a.norm() - gn64) <= 2.0 ** -22 * gn64, (what, a.norm(), gn64)
    assert a.skipped() == 0 and int(a.state[3]) == 0
    assert _same_bits(a.rng(a.saved).cpu(), p0)
    assert _same_bits(a.rng(a.pb).cpu(), got.bfloat16())
    assert _same_bits(a.rng(a.g).cpu(), g)
    assert a.bands_intact()
    b = _Arena(cuda, p0, g)  # a second run from the same inputs: the same bits
    b.perturb(dtc, rho, adaptive, gmul)
    for x, y in ((a.p, b.p), (a.saved, b.saved), (a.pb, b.pb), (a.state, b.state)):
        assert _same_bits(x, y)


# ----------------------------------------------------------------------------- 2. restore
@pytest.mark.parametrize("mode,adaptive,rho", MODES, ids=[m[0] for m in MODES])
def test_restore_brings_everything_back(dtc, cuda, mode, adaptive, rho):
    n = 3 * CHUNK - 4
    p0, g = _inputs(n, seed=23)
    shadow0 = p0.bfloat16()
    a = _Arena(cuda, p0, g, shadow0)
    gen = torch.Generator().manual_seed(29)
    live_f = torch.randn(KEEP_F32, generator=gen).to(cuda)
    live_i = torch.randint(0, 1 << 40, (KEEP_I64,), generator=gen).to(cuda)
    was_f, was_i = live_f.clone(), live_i.clone()
    keep = [(live_f, torch.empty_like(live_f)), (live_i, torch.empty_like(live_i))]
    found = torch.zeros(1, dtype=torch.int32, device=cuda)
    a.perturb(dtc, rho, adaptive, None, keep)
    assert torch.equal(keep[0][1], was_f) and torch.equal(keep[1][1], was_i)  # saved <- live
    assert torch.equal(live_f, was_f) and torch.equal(live_i, was_i)
    assert not torch.equal(a.rng(a.p).cpu(), p0)
    live_f.mul_(3.0).add_(1.0)  # what a second forward does to them
    live_i.add_(1)
    a.restore(dtc, keep, found)
    assert _same_bits(a.rng(a.p).cpu(), p0) and _same_bits(a.rng(a.pb).cpu(), shadow0)
    assert _same_bits(live_f, was_f) and torch.equal(live_i, was_i)
    assert int(found) == 0  # a clean perturb raises nothing
    found.fill_(1)
    a.perturb(dtc, rho, adaptive, None, keep)
    a.restore(dtc, keep, found)
    assert int(found) == 1  # and never clears the word
    assert _same_bits(a.rng(a.p).cpu(), p0) and a.bands_intact()


# ----------------------------------------------------------------------------- 3. non-finite and degenerate gradients
@pytest.mark.parametrize("mode,adaptive,rho", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_non_finite_gradient_moves_nothing(dtc, cuda, bad, mode, adaptive, rho):
    n = CHUNK + 4
    p0, g = _inputs(n, seed=31)
    g_bad = g.clone()
    g_bad[n // 2] = bad
    shadow0 = torch.randn(n).bfloat16()  # not bf16(p0): a rewritten shadow would show
    a = _Arena(cuda, p0, g_bad, shadow0)
    found = torch.zeros(1, dtype=torch.int32, device=cuda)
    a.perturb(dtc, rho, adaptive)
    assert a.skipped() == 1 and a.coef() == 0.0
    assert _same_bits(a.rng(a.p).cpu(), p0) and _same_bits(a.rng(a.pb).cpu(), shadow0)
    assert _same_bits(a.rng(a.saved).cpu(), p0)
    a.restore(dtc, None, found)
    assert int(found) == 1
    assert _same_bits(a.rng(a.p).cpu(), p0) and a.bands_intact()
    a.rng(a.g).copy_(g.to(cuda))  # a following clean call clears the mark
    a.perturb(dtc, rho, adaptive)
    assert a.skipped() == 0 and a.coef() > 0.0
    assert not torch.equal(a.rng(a.p).cpu(), p0)


def test_non_finite_gmul_moves_nothing(dtc, cuda):
    p0, g = _inputs(1020, seed=37)
    a = _Arena(cuda, p0, g)
    a.perturb(dtc, 0.05, False, torch.full((1,), float("inf"), device=cuda))
    assert a.skipped() == 1 and _same_bits(a.rng(a.p).cpu(), p0) and _same_bits(a.rng(a.saved).cpu(), p0)


def test_huge_finite_gradient_is_not_skipped(dtc, cuda):
    """+-3e38 among the gradients: their squares overflow fp32, the sum of squares (1.8e77) is an ordinary double.
    The norm 4.2e38 is beyond fp32, so state.norm reads inf, but the step is taken: coef = 0.05 / 4.2e38 = 1.2e-40 is
    an fp32 DENORMAL, whose spacing 2^-149 makes its rounding error up to 2^-150 instead of 2^-24 coef. The
    per-element bound of the other tests therefore gains the term e * 2^-150 / coef (a flush of the coefficient to
    zero would be off by e itself)."""
    n, rho = 1020, 0.05
    p0, g = _inputs(n, seed=41)
    g[3], g[700] = 3e38, -3e38
    p64, e64, gn64, coef64 = _formula(p0, g, rho, False, 1.0, torch.float64)
    assert math.isfinite(gn64) and gn64 > 3.4028235e38 and 0 < coef64 < 1.17549435e-38
    a = _Arena(cuda, p0, g)
    a.perturb(dtc, rho, False)
    got = a.rng(a.p).cpu()
    assert a.skipped() == 0 and math.isinf(a.norm())
    assert abs(a.coef() - coef64) <= 2.0 ** -150
    err = (got.double() - p64).abs()
    bound = 2.0 ** -21 * (p0.double().abs() + e64.abs()) + e64.abs() * (2.0 ** -150 / coef64)
    print(f"huge gradient: worst |p_gpu - p64| / bound = {float((err / bound).max()):.3f}, e at the two: "
          f"{float(e64[3]):.4f}, {float(e64[700]):.4f}")
    assert bool((err <= bound).all())
    assert abs(float(got[3]) - float(p0[3])) > 0.03  # it did move: e = 0.05 * 3e38 / 4.2e38
    assert _same_bits(a.rng(a.saved).cpu(), p0) and a.bands_intact()


@pytest.mark.parametrize("mode,adaptive,rho", MODES, ids=[m[0] for m in MODES])
def test_zero_gradient_and_zero_rho_move_nothing(dtc, cuda, mode, adaptive, rho):
    n = CHUNK + 4
    p0, g = _inputs(n, seed=43)
    p0[5], p0[6] = 0.0, -0.0
    a = _Arena(cuda, p0, torch.zeros(n))
    a.perturb(dtc, rho, adaptive)
    assert a.skipped() == 0 and a.norm() == 0.0 and a.coef() > 0  # rho / eps
    assert _same_bits(a.rng(a.p).cpu(), p0) and _same_bits(a.rng(a.pb).cpu(), p0.bfloat16())
    b = _Arena(cuda, p0, g)
    b.perturb(dtc, 0.0, adaptive)
    assert b.skipped() == 0 and b.coef() == 0.0 and b.norm() > 0
    assert _same_bits(b.rng(b.p).cpu(), p0) and _same_bits(b.rng(b.saved).cpu(), p0)


# ----------------------------------------------------------------------------- the model
def _model(dtc, cuda, cap_mb=None):
    torch.manual_seed(42)
    m = dtc.ResNet18().to(cuda)
    if cap_mb is not None:
        m.set_bucket_cap_mb(cap_mb)
    return m


def _batches(cuda, n, batch=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(batch, 3, 32, 32, generator=g).to(cuda) for _ in range(n)]
    ys = [torch.randint(0, 100, (batch,), generator=g).to(cuda) for _ in range(n)]
    return xs, ys


def _sgd(dtc, model):
    return dtc.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)


def _loss(dtc, model, crit, x, y):
    with dtc.autocast():
        return crit(model(x), y)


def _sam_step(dtc, model, sam, crit, x, y, scaler=None):
    """the two-pass step of the SAM docstring"""
    scale = (lambda l: scaler.scale(l)) if scaler is not None else (lambda l: l)
    with model.local_grads():
        scale(_loss(dtc, model, crit, x, y)).backward()
    sam.first_step(scaler)
    scale(_loss(dtc, model, crit, x, y)).backward()
    if scaler is not None:
        scaler.step(sam)
        scaler.update()
    else:
        sam.step()


def _state(model, opt):
    f = model.flat
    return {"params": f.params, "momentum": opt._mom, "shadow": f.params_bf16, "bufs": f.bufs, "nbt": f.nbt}


# ----------------------------------------------------------------------------- 4. rho = 0 is the plain step
def test_rho_zero_equals_plain_sgd(dtc, cuda):
    xs, ys = _batches(cuda, 3)
    crit = dtc.CrossEntropyLoss()
    plain = _model(dtc, cuda)
    opt = _sgd(dtc, plain)
    for x, y in zip(xs, ys):
        _loss(dtc, plain, crit, x, y).backward()
        opt.step()
    model = _model(dtc, cuda)
    base = _sgd(dtc, model)
    sam = dtc.SAM(base, rho=0.0)
    for x, y in zip(xs, ys):
        _sam_step(dtc, model, sam, crit, x, y)
        assert float(sam.grad_norm) > 0
    torch.cuda.synchronize()
    want, got = _state(plain, opt), _state(model, base)
    assert bool(torch.isfinite(want["params"]).all()) and int(want["nbt"][0]) == 3
    for key in want:
        assert torch.equal(got[key], want[key]), key


# ----------------------------------------------------------------------------- 5. rho > 0 against existing pieces
@pytest.mark.parametrize("mode,adaptive,rho", MODES, ids=[m[0] for m in MODES])
def test_sam_step_against_an_emulation(dtc, cuda, mode, adaptive, rho):
    (x,), (y,) = _batches(cuda, 1, seed=13)
    crit = dtc.CrossEntropyLoss()
    model = _model(dtc, cuda)
    base = _sgd(dtc, model)
    sam = dtc.SAM(base, rho=rho, adaptive=adaptive)
    with model.local_grads():
        _loss(dtc, model, crit, x, y).backward()
    p0, g = model.flat.params.clone(), model.flat.grads.clone()
    sam.first_step()
    assert torch.equal(sam._saved[1], p0)
    perturbed = model.flat.params.clone()
    p64, e64, gn64, _ = _formula(p0.cpu(), g.cpu(), rho, adaptive, 1.0, torch.float64)
    _within_elementwise(perturbed.cpu(), p64, p0.cpu(), e64, f"model {mode}")
    assert abs(float(sam.grad_norm) - gn64) <= 2.0 ** -22 * gn64
    assert float((perturbed - p0).abs().max()) > 0
    # the gradient at the perturbed weights, from a second model holding them
    other = _model(dtc, cuda)
    other.flat.params.copy_(perturbed)
    other.flat.refresh_bf16()
    assert torch.equal(other.flat.params_bf16, model.flat.params_bf16)
    _loss(dtc, other, crit, x, y).backward()
    # one plain training forward and one plain SGD step at the original weights with that gradient
    ref = _model(dtc, cuda)
    ref_opt = _sgd(dtc, ref)
    _loss(dtc, ref, crit, x, y).backward()
    assert torch.equal(ref.flat.grads, g)
    ref.flat.grads.copy_(other.flat.grads)
    ref_opt.step()
    # the SAM step itself
    _loss(dtc, model, crit, x, y).backward()
    assert torch.equal(model.flat.grads, other.flat.grads)
    sam.step()
    torch.cuda.synchronize()
    want, got = _state(ref, ref_opt), _state(model, base)
    assert int(want["nbt"][0]) == 1
    for key in want:
        assert torch.equal(got[key], want[key]), key


# ----------------------------------------------------------------------------- 6. AMP skip
def test_amp_skip_without_a_host_synchronisation(dtc, cuda):
    xs, ys = _batches(cuda, 2, seed=17)
    crit = dtc.CrossEntropyLoss()
    scaler = dtc.GradScaler()
    model = _model(dtc, cuda)
    base = _sgd(dtc, model)
    sam = dtc.SAM(base, rho=0.05)
    _sam_step(dtc, model, sam, crit, xs[0], ys[0], scaler)  # a clean step: momentum and a scale to halve
    assert scaler.get_scale() == 65536.0 and int(scaler.found_inf) == 0
    before = {k: v.clone() for k, v in _state(model, base).items()}
    with model.local_grads():
        scaler.scale(_loss(dtc, model, crit, xs[1], ys[1])).backward()
    model.flat.grads[12345] = float("inf")
    after_first_forward = model.flat.bufs.clone()
    assert not torch.equal(after_first_forward, before["bufs"])
    sam.first_step(scaler)
    assert int(sam._state[2]) == 1
    scaler.scale(_loss(dtc, model, crit, xs[1], ys[1])).backward()
    assert bool(torch.isfinite(model.flat.grads).all())  # the second gradient alone would not skip the step
    scaler.step(sam)
    assert int(scaler.found_inf) == 1
    scaler.update()
    torch.cuda.synchronize()
    got = _state(model, base)
    for key in ("params", "momentum", "shadow"):
        assert _same_bits(got[key], before[key]), key
    assert scaler.get_scale() == 32768.0
    assert torch.equal(model.flat.bufs, after_first_forward)
    assert torch.equal(model.flat.nbt, before["nbt"] + 1)


# ----------------------------------------------------------------------------- 7. one set of collectives per step
def test_one_set_of_collectives_per_step(dtc, cuda):
    (x,), (y,) = _batches(cuda, 1, seed=19)
    crit = dtc.CrossEntropyLoss()
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 1.0, world=2)
    try:
        model = _model(dtc, cuda, cap_mb=1.0)
        model._comm = comm
        model.grad_compression = "bf16"  # the local backward must not compress either
        buckets = model.buckets()
        assert len(buckets) >= 6
        base = _sgd(dtc, model)
        sam = dtc.SAM(base, rho=0.05)
        comm.clear_log()
        with model.local_grads():
            _loss(dtc, model, crit, x, y).backward()
        torch.cuda.synchronize()
        assert [e for e in comm.log() if e[2]] == []  # nothing reduced by the first backward
        # nor compressed: a gradient that went through bf16 has no bit set in any low half
        assert bool((model.flat.grads.view(torch.int32) & 0xFFFF).any())
        sam.first_step()
        model.grad_compression = None
        _loss(dtc, model, crit, x, y).backward()
        sam.step()
        torch.cuda.synchronize()
        g0 = model.flat.grads.data_ptr()
        log = [((a - g0) // 4, n) for a, n, is_bucket in comm.log() if is_bucket]
        assert log == buckets  # exactly the bucket all-reduces of one plain step, by the second backward
    finally:
        comm.close()


# ----------------------------------------------------------------------------- 8. refusals
def test_refusals(dtc, cuda):
    (x,), (y,) = _batches(cuda, 1, seed=21)
    crit = dtc.CrossEntropyLoss()
    model = _model(dtc, cuda)
    with model.accumulate():
        _loss(dtc, model, crit, x, y).backward()
    assert model._accum_open
    with pytest.raises(dtc.NativeError, match="accumulation window"):
        with model.local_grads():
            pass
    model.reset_accumulation()
    model.grad_accum_steps = 2
    with pytest.raises(dtc.NativeError, match="grad_accum_steps"):
        with model.local_grads():
            pass
    model.grad_accum_steps = 1
    with model.local_grads():  # an accumulate() entered inside it is refused by the backward
        with model.accumulate():
            loss = _loss(dtc, model, crit, x, y)
            with pytest.raises(dtc.NativeError, match="accumulation window"):
                loss.backward()
    sam = dtc.SAM(_sgd(dtc, model))
    with pytest.raises(dtc.NativeError, match="first_step"):
        sam.step()
    with model.local_grads():
        _loss(dtc, model, crit, x, y).backward()
    sam.first_step()
    with pytest.raises(dtc.NativeError, match="already perturbed"):
        sam.first_step()
    _loss(dtc, model, crit, x, y).backward()
    sam.step()
    with pytest.raises(dtc.NativeError, match="first_step"):
        sam.step()
    some = list(model.parameters())[:-1]
    partial = dtc.SAM(dtc.SGD(some, lr=0.1, momentum=0.9, nesterov=True))
    with pytest.raises(dtc.NativeError, match="every parameter"):
        partial.first_step()
