"""Segmented norms and fused LARS (dtc_seg_norms / dtc_lars_flat, optim.LARS) against a float64 reference.

Neither torch nor this package's oracle has a LARS, so the reference of every numeric check is `_ref_step` below:
the formulas of include/dtc.h written with torch on the CPU, run in float64. It is paired with the same code run
in float32 (norms still summed in double and the ratio rounded once to fp32, as specified). Bound for the optimizer
state, test_gpu_optim.py's, taken over all segment elements of the buffer:

    max|p_gpu - p64| <= 2 * max|p32 - p64|

(the factor 2 allows for FMA contraction and a different, equally valid fp32 operation order), the same for the
momentum buffer. Single segments may exceed 2x (a ratio that rounds to the neighbouring fp32 value moves a whole
tensor), so the bound is not asserted per segment.

Synthetic layout: segments at 64-element aligned offsets, as in the model's flat buffer, of 4, 10, 64, 100, 1728,
36864 elements, exactly one chunk, one chunk + 4 and three chunks - 6 (not a multiple of 4); the 10- and
64-element ones without ADAPT. The gradient's padding is NaN, the padding of the other buffers a sentinel.

Measured on an MI355X (printed by the tests): the worst ratio over the whole buffer is 1.665, see
test_lars_flat_matches_reference's docstring; the segments without ADAPT are bit-equal to dtc_sgd_nesterov_flat's.
"""
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

P_SENTINEL, BUF_SENTINEL, BF_SENTINEL = 1234.5, -4321.25, -7.0
HYPER = dict(wd=1e-4, mu=0.9, tc=1e-3, eps=1e-8)


def _layout(sizes_adapt):
    """[(offset, numel, adapt)] at 64-aligned offsets behind 64 elements of leading padding, and the buffer length
    (64 more elements of padding behind the last segment)."""
    segs, off = [], 64
    for n, adapt in sizes_adapt:
        segs.append((off, n, adapt))
        off = (off + n + 63) // 64 * 64
    return segs, off + 64


def _synthetic(dtc):
    ch = int(dtc._native.lib.dtc_segplan_chunk_elems())
    return _layout([(4, True), (10, False), (64, False), (100, True), (1728, True), (36864, True), (ch, True),
                    (ch + 4, True), (3 * ch - 6, True)])


def _seg_mask(segs, total):
    m = torch.zeros(total, dtype=torch.bool)
    for off, n, _ in segs:
        m[off:off + n] = True
    return m


def _ref_norms(p, g, segs, mult):
    """float64 (||p_s||, |mult| ||g_s||) per segment."""
    return [(math.sqrt(float((p[o:o + n].double() ** 2).sum())),
             abs(mult) * math.sqrt(float((g[o:o + n].double() ** 2).sum()))) for o, n, _ in segs]


def _ref_step(p, g, buf, segs, mult, lr, nesterov, clip, wd, mu, tc, eps):
    """One LARS step in place on p and buf (their dtype is the arithmetic's; g in the same dtype, still multiplied
    by 1 / mult). Returns the fp32-rounded ratios."""
    ratios = []
    for (off, n, adapt), (wn, gn) in zip(segs, _ref_norms(p, g, segs, mult)):
        ratio = 1.0
        if adapt and wn > 0 and gn > 0:
            ratio = tc * wn / (gn + wd * wn + eps)
            if clip:
                ratio = min(ratio / lr, 1.0)
        ratio = float(torch.tensor(ratio, dtype=torch.float64).float())  # rounded once to fp32
        ratios.append(ratio)
        ps, gs, bs = p[off:off + n], g[off:off + n], buf[off:off + n]
        d = (gs * mult + ps * (wd if adapt else 0.0)) * ratio
        bs.mul_(mu).add_(d)
        ps.sub_((d + bs * mu if nesterov else bs) * lr)
    return ratios


class _GpuLars:
    """The flat kernel driven the way GradScaler drives it: gradients pre-multiplied by 4, inv_scale = 0.25 (both
    exact in fp32), found_inf on the device; padding poisoned."""

    def __init__(self, dtc, dev, segs, total, p0, lr, nesterov, clip):
        self.ops, self.segs, self.total, self.dev = dtc.ops, segs, total, dev
        self.lr, self.nesterov, self.clip = lr, nesterov, clip
        self.mask = _seg_mask(segs, total)
        self.plan = dtc.ops.seg_plan(segs, dev)
        self.p = torch.where(self.mask, p0, torch.tensor(P_SENTINEL)).to(dev)
        self.buf = torch.where(self.mask, torch.tensor(0.0), torch.tensor(BUF_SENTINEL)).to(dev)
        self.pb = torch.full((total,), BF_SENTINEL, dtype=torch.bfloat16, device=dev)
        self.inv = torch.full((1,), 0.25, device=dev)
        self.found = torch.zeros(1, dtype=torch.int32, device=dev)
        self.out = torch.zeros(len(segs), 3, device=dev)

    def grad(self, g):
        return torch.where(self.mask, g * 4, torch.tensor(float("nan"))).to(self.dev)

    def step(self, g):
        self.ops.lars_flat(self.plan, self.p, self.grad(g), self.buf, self.pb, self.lr, HYPER["wd"], HYPER["mu"],
                           self.nesterov, HYPER["tc"], HYPER["eps"], self.clip, self.inv, self.found, self.out)

    def snapshot(self):
        return [t.clone() for t in (self.p, self.buf, self.pb)]

    def check_padding_and_shadow(self):
        pad = ~self.mask.to(self.dev)
        assert bool((self.p[pad] == P_SENTINEL).all()) and bool((self.buf[pad] == BUF_SENTINEL).all())
        assert bool((self.pb[pad].float() == BF_SENTINEL).all())
        m = self.mask.to(self.dev)
        assert torch.equal(self.pb[m].view(torch.int16), self.p[m].bfloat16().view(torch.int16))  # bit for bit


def _inputs(total, gscale, steps, seed):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(total, generator=g)
    return p0, [torch.randn(total, generator=g) * gscale for _ in range(steps)]


def _reference(segs, p0, grads, lr, nesterov, clip, dtype):
    p, buf = p0.to(dtype).clone(), torch.zeros_like(p0, dtype=dtype)
    ratios = None
    for g in grads:
        ratios = _ref_step(p, (g * 4).to(dtype), buf, segs, 0.25, lr, nesterov, clip, **HYPER)
    return p.double(), buf.double(), ratios


def _assert_within_twice_fp32(got, ref32, ref64, mask, what):
    worst = 0.0
    for name, a, b32, b64 in zip(("p", "buf"), got, ref32, ref64):
        err = float((a.double().cpu() - b64)[mask].abs().max())
        err32 = float((b32 - b64)[mask].abs().max())
        print(f"{what} {name}: max|gpu - f64| = {err:.3e}, fp32 reference max|f32 - f64| = {err32:.3e}, "
              f"ratio {err / err32 if err32 > 0 else float('nan'):.3f}")
        assert err <= 2 * err32, (what, name, err, err32)
        worst = max(worst, err / err32 if err32 > 0 else 0.0)
    return worst


def test_seg_norms_match_float64(dtc, cuda):
    """Each norm within relative 2^-22 of the float64 norm: double accumulation of <= 2^22 squares errs below 1e-9,
    one fp32 rounding is 2^-24, the factor 4 is slack. All values finite despite the NaN padding of g."""
    segs, total = _synthetic(dtc)
    p0, (g0,) = _inputs(total, 1e-3, 1, seed=1)
    mask = _seg_mask(segs, total)
    plan = dtc.ops.seg_plan(segs, cuda)
    p = torch.where(mask, p0, torch.tensor(float("nan"))).to(cuda)
    g = torch.where(mask, g0, torch.tensor(float("nan"))).to(cuda)
    gmul = torch.full((1,), -0.5, device=cuda)
    out = dtc.ops.seg_norms(plan, p, g, gmul).cpu()
    assert out.shape == (len(segs), 3) and bool(torch.isfinite(out).all())
    for (off, n, adapt), (wn, gn), row in zip(segs, _ref_norms(p0, g0, segs, -0.5), out.double().tolist()):
        print(f"n={n}: ||p|| {row[0]:.9e} vs {wn:.9e}, ||g|| {row[1]:.9e} vs {gn:.9e}")
        assert abs(row[0] - wn) <= 2.0 ** -22 * wn and abs(row[1] - gn) <= 2.0 ** -22 * gn
        assert abs(row[2] - (wn / gn if adapt else 1.0)) <= 2.0 ** -22 * (wn / gn if adapt else 1.0)
    assert torch.equal(out, dtc.ops.seg_norms(plan, p, g, gmul).cpu())  # bit-equal from run to run
    none = dtc.ops.seg_norms(plan, p, g).cpu()  # gmul = NULL: 1
    assert torch.equal(none[:, 0], out[:, 0]) and torch.equal(none[:, 1], out[:, 1] * 2)


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("clip", [False, True], ids=["lars", "larc"])
@pytest.mark.parametrize("gscale", [1.0, 1e-3])
@pytest.mark.parametrize("lr", [0.1, 1.0])
def test_lars_flat_matches_reference(dtc, cuda, lr, gscale, clip, nesterov):
    """Five steps. Measured on an MI355X over the 16 cases, max|gpu - f64| / max|f32 - f64| over the whole buffer:
    1.000 for p and the momentum buffer in the 12 cases with lr = 0.1 or gradients * 1e-3; with lr = 1.0 and
    gradients * 1 the worst is 1.665 (plain momentum) and 1.334 (Nesterov), with and without trust_clip."""
    segs, total = _synthetic(dtc)
    p0, grads = _inputs(total, gscale, 5, seed=int(lr * 10) + int(gscale * 1000))
    ref64 = _reference(segs, p0, grads, lr, nesterov, clip, torch.float64)
    ref32 = _reference(segs, p0, grads, lr, nesterov, clip, torch.float32)
    a = _GpuLars(dtc, cuda, segs, total, p0, lr, nesterov, clip)
    for g in grads:
        a.step(g)
    what = f"lr={lr} g*{gscale} clip={clip} nesterov={nesterov}"
    worst = _assert_within_twice_fp32((a.p, a.buf), ref32, ref64, a.mask, what)
    print(f"{what}: worst ratio {worst:.3f}")
    a.check_padding_and_shadow()
    out = a.out.cpu()
    assert bool(torch.isfinite(out).all())
    for (off, n, adapt), r64, r in zip(segs, ref64[2], out[:, 2].tolist()):
        assert (r == 1.0) if not adapt else abs(r - r64) <= 1e-5 * r64, (n, r, r64)


def test_lars_degenerate_norms_give_ratio_one(dtc, cuda):
    """An ADAPT segment with p = 0 and one with g = 0: ratio exactly 1.0 (with and without trust_clip), and the
    update is the reference's."""
    segs, total = _layout([(100, True), (1728, True), (36864, True), (10, False)])
    p0, grads = _inputs(total, 1.0, 2, seed=3)
    p0[segs[0][0]:segs[0][0] + segs[0][1]] = 0.0
    for g in grads:
        g[segs[1][0]:segs[1][0] + segs[1][1]] = 0.0
    for clip in (False, True):
        a = _GpuLars(dtc, cuda, segs, total, p0, 0.1, True, clip)
        a.step(grads[0])
        ratios = a.out[:, 2].cpu().tolist()
        assert ratios[0] == 1.0 and ratios[1] == 1.0 and ratios[3] == 1.0 and 0.0 < ratios[2] < 1.0
        assert a.out[0, 0].item() == 0.0 and a.out[1, 1].item() == 0.0
        a.step(grads[1])  # the p = 0 segment has moved: its ratio adapts now; the g = 0 one still holds 1
        ratios = a.out[:, 2].cpu().tolist()
        assert 0.0 < ratios[0] < 1.0 and ratios[1] == 1.0
        _assert_within_twice_fp32((a.p, a.buf), _reference(segs, p0, grads, 0.1, True, clip, torch.float32),
                                  _reference(segs, p0, grads, 0.1, True, clip, torch.float64), a.mask,
                                  f"degenerate clip={clip}")
        a.check_padding_and_shadow()


def test_lars_without_adapt_is_nesterov_sgd(dtc, cuda):
    """Segments without ADAPT against dtc_sgd_nesterov_flat with weight_decay = 0 on the same data."""
    segs, total = _synthetic(dtc)
    lr = 0.1
    p0, grads = _inputs(total, 1.0, 5, seed=4)
    a = _GpuLars(dtc, cuda, segs, total, p0, lr, True, False)
    sp, sm = p0.to(cuda), torch.zeros(total, device=cuda)
    spb = torch.zeros(total, dtype=torch.bfloat16, device=cuda)
    for g in grads:
        a.step(g)
        dtc.ops.sgd_nesterov_flat(sp, (g * 4).to(cuda), sm, spb, lr, 0.0, HYPER["mu"], a.inv, a.found)
    off_mask = _seg_mask([s for s in segs if not s[2]], total)
    assert int(off_mask.sum()) == 74
    ref64 = _reference(segs, p0, grads, lr, True, False, torch.float64)
    ref32 = _reference(segs, p0, grads, lr, True, False, torch.float32)
    for name, x, y, b32, b64 in zip(("p", "buf"), (a.p, a.buf), (sp, sm), ref32, ref64):
        diff = float((x.cpu().double() - y.cpu().double())[off_mask].abs().max())
        err32 = float((b32 - b64)[off_mask].abs().max())
        print(f"no ADAPT {name}: max|lars - sgd| = {diff:.3e}, fp32 reference max|f32 - f64| = {err32:.3e}")
        assert diff <= 2 * err32


def test_lars_skipped_step_leaves_everything(dtc, cuda):
    """found_inf = 1 ahead of the second of three steps: all three buffers stay bit-unchanged, and the end state is
    the reference's after the two real steps."""
    segs, total = _synthetic(dtc)
    p0, grads = _inputs(total, 1.0, 3, seed=5)
    a = _GpuLars(dtc, cuda, segs, total, p0, 0.1, True, True)
    a.step(grads[0])
    before = a.snapshot()
    a.found.fill_(1)
    a.step(grads[1])
    for was, now in zip(before, a.snapshot()):
        assert torch.equal(was.view(torch.int16), now.view(torch.int16))
    a.found.zero_()
    a.step(grads[2])
    two = [grads[0], grads[2]]
    _assert_within_twice_fp32((a.p, a.buf), _reference(segs, p0, two, 0.1, True, True, torch.float32),
                              _reference(segs, p0, two, 0.1, True, True, torch.float64), a.mask, "skipped")
    a.check_padding_and_shadow()


def test_lars_is_repeatable_on_the_model_layout(dtc, cuda):
    """Two runs of three steps over the model's own flat layout (11.2 M elements, 62 segments): bit-identical."""
    layout = dtc.nn.Layout()
    n = layout.flat_numel
    gen = torch.Generator().manual_seed(6)
    p0 = torch.randn(n, generator=gen).to(cuda)
    g0 = (torch.randn(n, generator=gen) * 1e-2).to(cuda)
    runs = []
    for _ in range(2):
        plan = dtc.ops.seg_plan(layout, cuda)
        assert plan.nseg == 62
        p, buf = p0.clone(), torch.zeros_like(p0)
        pb = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
        out = torch.zeros(62, 3, device=cuda)
        for k in range(3):
            dtc.ops.lars_flat(plan, p, g0 * (k + 1), buf, pb, 0.1, 1e-4, 0.9, True, 1e-3, 1e-8, False, None, None, out)
        runs.append((p, buf, pb, out))
    for x, y in zip(*runs):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
    assert bool(torch.isfinite(runs[0][3]).all()) and bool((runs[0][0] != p0).any())


def test_lars_through_the_model(dtc, cuda):
    """dtc.LARS on ResNet18 at batch 8 under GradScaler with clip_grad_norm_, three steps. Ahead of each step the
    flat parameters, gradients, momentum buffer and the clip multiplier (which carries the scaler's 1 / scale) are
    copied; the reference takes one step from the copy, in float64 and in float32."""
    torch.manual_seed(42)
    model = dtc.ResNet18().to(cuda)
    crit = dtc.CrossEntropyLoss()
    hp = dict(lr=0.1, nesterov=True, clip=True, wd=1e-4, mu=0.9, tc=1e-3, eps=1e-8)
    opt = dtc.LARS(model.parameters(), lr=hp["lr"], momentum=hp["mu"], weight_decay=hp["wd"], nesterov=True,
                   trust_coef=hp["tc"], eps=hp["eps"], trust_clip=True)
    scaler = dtc.GradScaler()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(8, 3, 32, 32, generator=gen).to(cuda)
    y = torch.randint(0, 100, (8,), generator=gen).to(cuda)
    flat = model.flat
    segs = sorted((q.offset, q.numel, len(q.shape) > 1) for q in flat.layout.params)
    mask = _seg_mask(segs, flat.layout.flat_numel)
    max_norm = None
    for step in range(3):
        opt.zero_grad()
        with dtc.autocast():
            loss = crit(model(x), y)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        if max_norm is None:  # half the first step's norm: the clip is active
            max_norm = 0.5 * float(dtc.clip_grad_norm_(model.parameters(), 1e30, scaler=scaler))
        tn = dtc.clip_grad_norm_(model.parameters(), max_norm, scaler=scaler)
        p, g, buf = flat.params.cpu(), flat.grads.cpu(), opt._mom.cpu()
        mult, inv = float(flat.grad_mult), float(scaler._inv_scale)
        assert math.isfinite(float(tn)) and 0.0 < mult <= inv and (step > 0 or mult < 0.51 * inv)
        scaler.step(opt)
        scaler.update()
        assert flat.clip_pending is False
        refs = {}
        for dt in (torch.float64, torch.float32):
            rp, rb = p.to(dt), buf.to(dt)
            ratios = _ref_step(rp, g.to(dt), rb, segs, mult, **hp)
            refs[dt] = (rp.double(), rb.double(), ratios)
        assert bool((flat.params.cpu() != p)[mask].any())  # the step was not skipped
        _assert_within_twice_fp32((flat.params, opt._mom), refs[torch.float32], refs[torch.float64], mask,
                                  f"model step {step}")
        norms, names = opt.layer_norms()
        assert norms.is_cuda and tuple(norms.shape) == (62, 3) and len(names) == 62
        shapes = {q.name: q.shape for q in flat.layout.params}
        for name, (wn, gn, r), r64 in zip(names, norms.cpu().tolist(), refs[torch.float64][2]):
            if len(shapes[name]) > 1:
                assert 0.0 < r <= 1.0 and abs(r - r64) <= 1e-5 * r64, (name, r, r64)
            else:
                assert r == 1.0, (name, r)
            assert math.isfinite(wn) and math.isfinite(gn) and wn >= 0.0  # (BatchNorm biases start at zero)
        assert sum(len(s) == 1 for s in shapes.values()) == 41  # BN weights / biases and linear.bias
    assert torch.equal(flat.params_bf16[mask.to(cuda)].view(torch.int16),
                       flat.params[mask.to(cuda)].bfloat16().view(torch.int16))
    assert not bool(flat.params[~mask.to(cuda)].any()) and not bool(opt._mom[~mask.to(cuda)].any())  # padding kept


_TRAINER_ARGS = ["--max-steps", "2", "--epoch", "1", "--synthetic-train", "64", "--synthetic-test", "16",
                 "--batch-size", "8", "--workers", "0"]


def test_trainer_lars_with_warmup_runs(dtc, cuda, tmp_path):
    dtc.data.fix_seed(42)
    init = dtc.ResNet18().state_dict()["linear.weight"].clone()
    dtc.data.fix_seed(42)
    t = dtc.trainer.main(_TRAINER_ARGS + ["--amp", "--optimizer", "lars", "--warmup-epochs", "1", "--ckpt-path",
                                          str(tmp_path)], "single")
    assert isinstance(t.optimizer, dtc.optim.LARS) and t.global_step == 2
    assert t.optimizer.defaults["nesterov"] is True and t.optimizer.defaults["momentum"] == 0.9
    assert isinstance(t.lr_scheduler, torch.optim.lr_scheduler.LambdaLR)
    rows = [json.loads(line) for line in open(os.path.join(t.save_path, "scalars.jsonl"))]
    losses = [r for r in rows if r["tag"] == "loss/epoch"]
    assert len(losses) == 1 and math.isfinite(losses[0]["train"]) and math.isfinite(losses[0]["val"])
    assert [r["lr"] for r in rows if r["tag"] == "lr"] == [0.1]  # one warm-up epoch: lr * 1 / 1
    now = t.model.state_dict()["linear.weight"].cpu()
    assert bool(torch.isfinite(now).all()) and not torch.equal(now, init.cpu())  # the parameters moved
    norms, names = t.optimizer.layer_norms()
    assert bool(torch.isfinite(norms).all()) and "linear.weight" in names
