"""Fused LAMB (dtc_lamb_flat, optim.LAMB) against `_ref_step`: the formulas of include/dtc.h written with torch on the
CPU, run in float64 and paired with the same code in float32 (norms still summed in double, the ratio rounded once to
fp32). Bound for p, exp_avg and exp_avg_sq over all segment elements, as test_gpu_lars.py:

    max|gpu - f64| <= 2 * max|f32 - f64|

Layout, poisoned padding and the GradScaler-style driving (gradients * 4, inv_scale = 0.25) are test_gpu_lars.py's.
Measured on an MI355X (printed by the tests): worst ratio 1.016 over the flat cases, 1.362 through the model (v)."""
import math

import pytest
import torch

from tests.test_gpu_lars import _inputs, _layout, _seg_mask, _synthetic

pytestmark = pytest.mark.gpu

SENTINELS = (1234.5, -4321.25, 77.0, -7.0)  # padding of p, m, v, p_bf16
HYPER = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-6, wd=0.01)
F64, F32 = torch.float64, torch.float32


def _same_bits(xs, ys):
    return all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(xs, ys))


def _ref_step(p, g, m, v, segs, mult, t, bc, max_trust, lr, b1, b2, eps, wd):
    """One LAMB step in place on p, m, v, in their dtype; t counts this step. Returns the fp32-rounded ratios."""
    bc1, bc2 = (1 - b1 ** t, 1 - b2 ** t) if bc else (1.0, 1.0)
    ratios = []
    for off, n, adapt in segs:
        ps, ms, vs, gs = p[off:off + n], m[off:off + n], v[off:off + n], g[off:off + n] * mult
        ms.add_((gs - ms) * (1 - b1))
        vs.mul_(b2).add_(gs * gs * (1 - b2))
        u = (ms / bc1) / (vs.sqrt() / math.sqrt(bc2) + eps) + ps * (wd if adapt else 0.0)
        wn, un = math.sqrt(float((ps.double() ** 2).sum())), math.sqrt(float((u.double() ** 2).sum()))
        ratio = wn / un if adapt and wn > 0 and un > 0 else 1.0
        if adapt and max_trust > 0:
            ratio = min(ratio, max_trust)
        ratios.append(float(torch.tensor(ratio, dtype=F64).float()))  # rounded once to fp32
        ps.sub_(u * (lr * ratios[-1]))
    return ratios


def _reference(segs, p0, grads, bc, max_trust, dtype, hyper):
    p, m, v = p0.to(dtype).clone(), torch.zeros_like(p0, dtype=dtype), torch.zeros_like(p0, dtype=dtype)
    ratios = None
    for t, g in enumerate(grads, 1):
        ratios = _ref_step(p, (g * 4).to(dtype), m, v, segs, 0.25, t, bc, max_trust, **hyper)
    return p.double(), m.double(), v.double(), ratios


def _within_twice_fp32(got, ref32, ref64, mask, what):
    worst = 0.0
    for name, a, b32, b64 in zip("pmv", got, ref32, ref64):
        err, err32 = float((a.double().cpu() - b64)[mask].abs().max()), float((b32 - b64)[mask].abs().max())
        print(f"{what} {name}: max|gpu - f64| = {err:.3e}, max|f32 - f64| = {err32:.3e}, ratio {err / err32:.3f}")
        assert err <= 2 * err32, (what, name, err, err32)
        worst = max(worst, err / err32)
    return worst


def _run(dtc, dev, segs, total, p0, grads, what, bc=True, max_trust=0.0, hyper=HYPER, skip=None):
    """The flat kernel over `grads` (found_inf = 1 ahead of step `skip`, which must change no bit), then the bound
    against the references over the real steps, the padding, the shadow and the step word."""
    mask = _seg_mask(segs, total)
    plan, on = dtc.ops.seg_plan(segs, dev), mask.to(dev)
    zeros = torch.zeros(total)
    p, m, v = (torch.where(mask, x, torch.tensor(s)).to(dev) for x, s in zip((p0, zeros, zeros), SENTINELS))
    pb = torch.full((total,), SENTINELS[3], dtype=torch.bfloat16, device=dev)
    state, inv, found = dtc.ops.lamb_state(dev), torch.full((1,), 0.25, device=dev), torch.zeros(1, dtype=torch.int32)
    out = torch.zeros(len(segs), 3, device=dev)
    for k, g in enumerate(grads):
        before = [t.clone() for t in (p, m, v, pb, state)]
        g = torch.where(mask, g * 4, torch.tensor(float("nan"))).to(dev)
        dtc.ops.lamb_flat(plan, p, g, m, v, pb, state, hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"], hyper["wd"],
                          bc, max_trust, inv, (found + (k == skip)).to(dev), out)
        assert k != skip or _same_bits(before, (p, m, v, pb, state))
    real = [g for k, g in enumerate(grads) if k != skip]
    ref64, ref32 = (_reference(segs, p0, real, bc, max_trust, dt, hyper) for dt in (F64, F32))
    print(f"{what}: worst ratio {_within_twice_fp32((p, m, v), ref32, ref64, mask, what):.3f}")
    for buf, s in zip((p, m, v, pb.float()), SENTINELS):
        assert bool((buf[~on] == s).all())
    assert torch.equal(pb[on].view(torch.int16), p[on].bfloat16().view(torch.int16))  # bit for bit
    assert int(state[0]) == len(real) and bool(torch.isfinite(out).all())
    return (p, m, v), out.cpu(), ref64, ref32


@pytest.mark.parametrize("max_trust", [0.0, 0.375])
@pytest.mark.parametrize("bc", [True, False], ids=["bias_corr", "no_bias_corr"])
@pytest.mark.parametrize("gscale", [1.0, 1e-3])
def test_lamb_flat_matches_reference(dtc, cuda, gscale, bc, max_trust):
    """Five steps; max_trust = 0.375 clamps in every case (the float64 ratios of the larger segments: 0.97 to 2.25 with
    bias correction, 0.31 to 0.41 without). Measured on an MI355X, worst max|gpu - f64| / max|f32 - f64|: 1.016."""
    segs, total = _synthetic(dtc)
    p0, grads = _inputs(total, gscale, 5, seed=int(gscale * 1000) + 2 * bc + (max_trust > 0))
    _, out, ref64, _ = _run(dtc, cuda, segs, total, p0, grads, f"g*{gscale} bc={bc} clamp={max_trust}", bc, max_trust)
    assert max_trust == 0 or any(r == max_trust for (_, _, adapt), r in zip(segs, ref64[3]) if adapt)  # clamp active
    for (_, n, adapt), want, r in zip(segs, ref64[3], out[:, 2].tolist()):
        assert (r == 1.0) if not adapt else abs(r - want) <= 1e-5 * want, (n, r, want)


def test_lamb_degenerate_norms_give_ratio_one(dtc, cuda):
    """ADAPT segments with p = 0 and (weight_decay = 0) with g = 0, so u = 0: ratio exactly 1.0, the reference's update.
    After a step the p = 0 segment has moved and adapts; the u = 0 one still holds 1."""
    segs, total = _layout([(100, True), (1728, True), (9000, True), (10, False)])
    p0, grads = _inputs(total, 1.0, 2, seed=3)
    p0[segs[0][0]:segs[0][0] + 100] = 0.0
    for g in grads:
        g[segs[1][0]:segs[1][0] + 1728] = 0.0
    for steps in (1, 2):
        out = _run(dtc, cuda, segs, total, p0, grads[:steps], f"degenerate {steps}", hyper=dict(HYPER, wd=0.0))[1]
        r = out[:, 2].tolist()
        assert (r[0] == 1.0) == (steps == 1) and r[1] == 1.0 and r[3] == 1.0 and r[2] not in (0.0, 1.0)
        assert (out[0, 0].item() == 0.0) == (steps == 1) and out[1, 1].item() == 0.0


def test_lamb_skipped_step_leaves_everything(dtc, cuda):
    """found_inf = 1 ahead of the second of three steps: no bit changes, and the end state is the reference's after the
    two real steps (t was not advanced)."""
    segs, total = _synthetic(dtc)
    _run(dtc, cuda, segs, total, *_inputs(total, 1.0, 3, seed=5), "skipped", skip=1)


def test_lamb_without_adapt_is_adam(dtc, cuda):
    """Segments without ADAPT against dtc_adam_flat (coupled, weight_decay = 0) on the same data, within the bound."""
    segs, total = _synthetic(dtc)
    p0, grads = _inputs(total, 1.0, 5, seed=4)
    got, _, ref64, ref32 = _run(dtc, cuda, segs, total, p0, grads, "no ADAPT")
    adam = [p0.to(cuda), torch.zeros(total, device=cuda), torch.zeros(total, device=cuda)]
    pb, st = torch.zeros(total, dtype=torch.bfloat16, device=cuda), dtc.ops.adam_state(cuda)
    for g in grads:
        dtc.ops.adam_flat(adam[0], (g * 4).to(cuda), adam[1], adam[2], pb, st, HYPER["lr"], HYPER["b1"], HYPER["b2"],
                          HYPER["eps"], 0.0, False, torch.full((1,), 0.25, device=cuda))
    off = _seg_mask([s for s in segs if not s[2]], total)
    assert int(off.sum()) == 74
    for name, x, y, b32, b64 in zip("pmv", got, adam, ref32, ref64):
        diff, err32 = float((x - y).cpu()[off].abs().max()), float((b32 - b64)[off].abs().max())
        print(f"no ADAPT {name}: max|lamb - adam| = {diff:.3e}, max|f32 - f64| = {err32:.3e}")
        assert diff <= 2 * err32


def test_lamb_is_repeatable_on_the_model_layout(dtc, cuda):
    """Two runs of three steps over the model's own flat layout (11.2 M elements, 62 segments): bit-identical."""
    layout = dtc.nn.Layout()
    gen = torch.Generator().manual_seed(6)
    p0 = torch.randn(layout.flat_numel, generator=gen).to(cuda)
    g0 = (torch.randn(layout.flat_numel, generator=gen) * 1e-2).to(cuda)
    runs = []
    for _ in range(2):
        plan = dtc.ops.seg_plan(layout, cuda)
        p, m, v, pb = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros_like(p0).bfloat16()
        st, out = dtc.ops.lamb_state(cuda), torch.zeros(62, 3, device=cuda)
        for k in range(3):
            dtc.ops.lamb_flat(plan, p, g0 * (k + 1), m, v, pb, st, 0.01, 0.9, 0.999, 1e-6, 0.01, True, 0.0, None, None,
                              out)
        runs.append((p, m, v, pb, out))
    assert _same_bits(*runs) and bool(torch.isfinite(runs[0][4]).all()) and bool((runs[0][0] != p0).any())


def test_lamb_through_the_model(dtc, cuda):
    """dtc.LAMB on ResNet18 under GradScaler with an active clip_grad_norm_: two steps, each against a one-step
    reference from copies of the flat buffers; then state_dict() into a fresh LAMB on a cloned model, one more step on
    both: bit-equal."""
    torch.manual_seed(42)
    model, crit = dtc.ResNet18().to(cuda), dtc.CrossEntropyLoss()
    hp = dict(lr=2e-3, b1=0.9, b2=0.999, eps=1e-6, wd=0.01)
    mk = lambda m: dtc.LAMB(m.parameters(), lr=hp["lr"], weight_decay=hp["wd"], max_trust=10.0)  # noqa: E731
    opt, scaler = mk(model), dtc.GradScaler()
    gen = torch.Generator().manual_seed(7)
    x, y = torch.randn(8, 3, 32, 32, generator=gen).to(cuda), torch.randint(0, 100, (8,), generator=gen).to(cuda)
    flat = model.flat
    segs = sorted((q.offset, q.numel, len(q.shape) > 1) for q in flat.layout.params)
    mask = _seg_mask(segs, flat.layout.flat_numel)

    def step(model, opt, scaler, max_norm):
        with dtc.autocast():
            loss = crit(model(x), y)
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        if max_norm is None:  # half the first step's norm: the clip is active
            max_norm = 0.5 * float(dtc.clip_grad_norm_(model.parameters(), 1e30, scaler=scaler))
        dtc.clip_grad_norm_(model.parameters(), max_norm, scaler=scaler)
        before = model.flat.params.cpu(), model.flat.grads.cpu(), float(model.flat.grad_mult)
        scaler.step(opt)
        scaler.update()
        return max_norm, before

    max_norm = None
    for t in (1, 2):
        state = [torch.zeros_like(flat.params).cpu()] * 2 if t == 1 else [opt._exp_avg.cpu(), opt._exp_avg_sq.cpu()]
        max_norm, (p, g, mult) = step(model, opt, scaler, max_norm)
        assert 0.0 < mult < (0.51 if t == 1 else 1.01) * float(scaler._inv_scale)
        refs = []
        for dt in (F64, F32):
            rp, rm, rv = (b.to(dt, copy=True) for b in (p, *state))
            ratios = _ref_step(rp, g.to(dt), rm, rv, segs, mult, t, True, 10.0, **hp)
            refs.append((rp.double(), rm.double(), rv.double(), ratios))
        assert bool((flat.params.cpu() != p)[mask].any()) and opt._get_step() == t  # the step was not skipped
        _within_twice_fp32((flat.params, opt._exp_avg, opt._exp_avg_sq), refs[1], refs[0], mask, f"model step {t}")
        for (_, _, adapt), r, want in zip(segs, opt.layer_norms()[0][:, 2].tolist(), refs[0][3], strict=True):
            assert (r == 1.0) if not adapt else abs(r - want) <= 1e-5 * want
    assert not bool(flat.params[~mask.to(cuda)].any()) and not bool(opt._exp_avg_sq[~mask.to(cuda)].any())  # padding
    twin = dtc.ResNet18().to(cuda)
    twin.load_state_dict(model.state_dict())
    opt2, scaler2 = mk(twin), dtc.GradScaler()
    opt2.load_state_dict(opt.state_dict())
    scaler2.load_state_dict(scaler.state_dict())
    step(model, opt, scaler, max_norm)
    step(twin, opt2, scaler2, max_norm)
    assert opt2._get_step() == 3 and _same_bits(
        (flat.params, flat.params_bf16, opt._exp_avg, opt._exp_avg_sq),
        (twin.flat.params, twin.flat.params_bf16, opt2._exp_avg, opt2._exp_avg_sq))
