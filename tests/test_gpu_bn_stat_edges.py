"""The BN statistic accumulator (csrc/common.h: stat_add1 / stat_total) at the edges of its contract, and NaN
through the fused ReLU.

common.h promises: sums are exact and independent of the order of the adds; bits of a partial below 2^-52 are
dropped; a partial that is non-finite or not below 2^40 in magnitude sets the header flag; a flagged accumulator
gives NaN in every consumer. Three parts:

A  every PRODUCER (conv epilogues on each route, the split-K reductions, the stem, the BN backward reductions)
   on inputs whose fp32 partial sums are exact whatever the tiling: x is non-zero on input channel 0 only, small
   integers; the filter is non-zero at the centre tap of channel 0 only, a power of two 2^j per output channel.
   Then y = x0 * 2^j exactly and every partial sum is an integer times 2^j far below 2^24 units: no fp32 add
   rounds, so the totals must EQUAL the exact sums of y (Fractions; no tolerance), run to run bit-identical.
   j cycles through -26..14: squares have no bits below 2^-52, and 512 * (2 * 2^14)^2 = 2^39 < 2^40 cannot flag.
   With j <= -30 the squares lose bits: exact - M * 2^-52 <= total <= exact (floor per partial, at most M
   partials). With one output of 2^20 (square 2^40), or one +inf input, the flag must rise and every total be NaN.
B  every CONSUMER on hand-written slot words (tests/stat_words.py) in five encodings of the same totals, against
   a float64 reference from the exact totals; and with the flag word 1 and 2.
C  NaN (a NaN coefficient, NaN / inf data) must come out of the fused ReLU as NaN, as torch.relu and the oracle's
   np.maximum give it.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import bounds as B
from tests import stat_words as W
from tests.test_conv_route import Options
from tests.test_gpu_bn_affine import _affine, _bf, _f

pytestmark = pytest.mark.gpu

N, HW, M, K = 2, 16, 512, 64
GSCALE = 0.125


def _exps(lo, hi, step, n=K):
    span = hi - lo + 1
    return np.array([lo + (step * k) % span for k in range(n)])


J_IN = _exps(-26, 14, 7)       # both ends occur (k = 0 and k = 35)
J_IN2 = _exps(-26, 14, 11)     # the shortcut filter of the fused projection forward
J_DROP = -30 - (np.arange(K) % 3)
assert J_IN.min() == -26 and J_IN.max() == 14 and J_IN2.min() == -26 and J_IN2.max() == 14


# --------------------------------------------------------------------------------------------- A: producers
# name: (entry, input channels, (r, s, stride, pad), options, route the query must report)
CONV_PRODUCERS = {
    "halo": ("fwd", 64, (3, 3, 1, 1), {}, dict(kernel="HALO", splits=1)),
    "c64": ("fwd", 64, (3, 3, 1, 1), {"conv_c64": 2}, dict(kernel="C64")),
    "gemm": ("fwd", 64, (3, 3, 1, 1), {"halo_conv": 0, "conv_c64": 0}, dict(kernel="GEMM", splits=1)),
    "halo_split_in_kernel": ("fwd", 128, (3, 3, 1, 1), {"halo_split": 2},
                             dict(kernel="HALO", splits=2, reduce_in_kernel=1)),
    "halo_split_reduce_launch": ("fwd", 128, (3, 3, 1, 1), {"halo_split": 2, "splitk_ink": 0},
                                 dict(kernel="HALO", splits=2, reduce_in_kernel=0)),
    "gemm_split_reduce": ("fwd", 64, (3, 3, 1, 1), {"igemm_split": 2, "halo_conv": 0, "conv_c64": 0},
                          dict(kernel="GEMM", splits=2)),
    "halo_s2": ("fwd", 64, (3, 3, 2, 1), {}, dict(kernel="HALO", splits=1)),
    "gemm_1x1_s2": ("fwd", 64, (1, 1, 2, 0), {}, dict(kernel="GEMM", splits=1)),
    "fwd_sc": ("fwd_sc", 64, (3, 3, 2, 1), {}, dict(kernel="HALO", sc_ok=1)),
    "stem_wlds1": ("stem", 3, (3, 3, 1, 1), {"stem_wlds": 1}, None),
    "stem_wlds0": ("stem", 3, (3, 3, 1, 1), {"stem_wlds": 0}, None),
}
PRODUCERS = list(CONV_PRODUCERS)


@functools.lru_cache(maxsize=None)
def _ints(stride):
    """Channel 0 of the input, values in {-2, ..., 2} (fixed seed), [N, HW * stride, HW * stride]; the pixel under
    output (0, 0, 0) holds a 2 (the flag-threshold launches need one output of full magnitude)."""
    g = np.random.default_rng(5 + stride)
    xi = g.integers(-2, 3, (N, HW * stride, HW * stride)).astype(np.float32)
    xi[0, 0, 0] = 2.0
    xi.setflags(write=False)
    return xi


def _produce(dtc, dev, name, jexp, jexp2=J_IN2, xi=None):
    """Run producer `name` with per-output-channel filter exponents jexp. Returns [(y [M, K] float32 numpy,
    expected y, accumulator tensor)] -- two entries for the fused projection forward."""
    entry, C, (r, s, st, pad), opts, route = CONV_PRODUCERS[name]
    lib = dtc._native.lib
    xi = _ints(st) if xi is None else xi
    wv = (2.0 ** np.asarray(jexp, np.float64)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        exp = (xi[:, ::st, ::st, None] * wv).reshape(M, K)
    with Options(lib, opts):
        if entry == "stem":
            x = np.zeros((N, 3, HW, HW), np.float32)
            x[:, 0] = xi
            w27 = np.zeros((K, 27), np.float32)
            w27[:, (1 * 3 + 1) * 3 + 0] = wv  # KRSC: centre tap, input channel 0
            stats = dtc.ops.new_stats(K, dev)
            y = dtc.ops.stem_fwd(_f(x, dev), _bf(w27, dev), stats=stats)
            torch.cuda.synchronize()
            return [(y.float().cpu().numpy().reshape(M, K), exp, stats)]
        H = HW * st
        d = dtc.ops.conv_desc(N, H, H, C, K, r, s, st, pad)
        nb = lib.dtc_conv2d_workspace_size(d, 0)
        info = dtc.ops.conv_route_info(d, 0, sc=entry == "fwd_sc", ws=(1 << 20) if nb else None, ws_bytes=nb)
        assert not info["refused"] and {k: info[k] for k in route} == route, (name, info)
        x = np.zeros((N, H, H, C), np.float32)
        x[..., 0] = xi
        w = np.zeros((K, r, s, C), np.float32)
        w[:, r // 2, s // 2, 0] = wv
        stats = dtc.ops.new_stats(K, dev)
        if entry == "fwd":
            y = dtc.ops.conv2d_fwd(_bf(x, dev), _bf(w, dev), st, pad, stats=stats)
            torch.cuda.synchronize()
            return [(y.float().cpu().numpy().reshape(M, K), exp, stats)]
        wv2 = (2.0 ** np.asarray(jexp2, np.float64)).astype(np.float32)
        wsc = np.zeros((K, C), np.float32)
        wsc[:, 0] = wv2
        stats_sc = dtc.ops.new_stats(K, dev)
        y, ysc = dtc.ops.conv2d_fwd_sc(_bf(x, dev), _bf(w, dev), _bf(wsc, dev), stats=stats, stats_sc=stats_sc)
        torch.cuda.synchronize()
        with np.errstate(invalid="ignore"):
            exp2 = (xi[:, ::2, ::2, None] * wv2).reshape(M, K)
        return [(y.float().cpu().numpy().reshape(M, K), exp, stats),
                (ysc.float().cpu().numpy().reshape(M, K), exp2, stats_sc)]


def _exact_sums(y, jexp):
    """Exact per-channel (sum y, sum y^2) of y[:, k] = integer * 2^jexp[k], as Fractions, from the tensor read back."""
    s, q = [], []
    for k in range(y.shape[1]):
        ints = y[:, k].astype(np.float64) * 2.0 ** -int(jexp[k])
        assert np.array_equal(ints, np.round(ints)) and np.abs(ints).max() <= 2
        ints = ints.astype(np.int64)
        u = Fraction(2) ** int(jexp[k])
        s.append(int(ints.sum()) * u)
        q.append(int((ints * ints).sum()) * u * u)
    return s, q


def _assert_totals_equal(dtc, stats, exact, what):
    tot = dtc.ops.stat_totals(stats, len(exact[0])).numpy()
    for j in range(2):
        for c, e in enumerate(exact[j]):
            assert Fraction(float(tot[j, c])) == e, f"{what}: statistic {j} channel {c}: {tot[j, c]!r} != {float(e)!r}"


def _assert_flagged(dtc, stats, C, what):
    assert int(stats[0].item()) != 0, f"{what}: header flag not set"
    assert np.isnan(dtc.ops.stat_totals(stats, C).numpy()).all(), what


@pytest.mark.parametrize("name", PRODUCERS)
def test_producer_sums_exact(dtc, cuda, name):
    """In range: y bit-exact, totals EQUAL to the exact sums of the read-back y, flag clear, two runs the same words."""
    runs = [_produce(dtc, cuda, name, J_IN) for _ in range(2)]
    for i, (y, exp, stats) in enumerate(runs[0]):
        jexp = (J_IN, J_IN2)[i]
        np.testing.assert_array_equal(y, exp, err_msg=f"{name} output {i}")
        assert int(stats[0].item()) == 0
        _assert_totals_equal(dtc, stats, _exact_sums(y, jexp), f"{name} output {i}")
        assert torch.equal(stats, runs[1][i][2]), f"{name} output {i}: words differ between two runs"
        assert int(stats.abs().sum().item()) > 0


@pytest.mark.parametrize("name", PRODUCERS)
def test_producer_dropped_bits(dtc, cuda, name):
    """Filter exponents -30..-32: the sums of y are still exact (integers * 2^j, j >= -32); every partial of the
    squares loses its bits below 2^-52 towards minus infinity (stat_add1: floor), and there are at most M partials:
    exact - M * 2^-52 <= total <= exact. Bit-identical between two runs."""
    runs = [_produce(dtc, cuda, name, J_DROP, jexp2=J_DROP - 1) for _ in range(2)]
    for i, (y, exp, stats) in enumerate(runs[0]):
        jexp = (J_DROP, J_DROP - 1)[i]
        np.testing.assert_array_equal(y, exp, err_msg=f"{name} output {i}")
        assert int(stats[0].item()) == 0
        s, q = _exact_sums(y, jexp)
        tot = dtc.ops.stat_totals(stats, K).numpy()
        lost = 0
        for k in range(K):
            assert Fraction(float(tot[0, k])) == s[k], (name, i, k)
            got = Fraction(float(tot[1, k]))
            assert q[k] - M * W.UNIT <= got <= q[k], (name, i, k, float(q[k] - got) * 2.0 ** 52)
            lost += got != q[k]
        print(f"{name} output {i}: {lost} of {K} sums of squares below the exact value")
        assert torch.equal(stats, runs[1][i][2]), f"{name} output {i}: words differ between two runs"


@pytest.mark.parametrize("name", PRODUCERS)
def test_producer_flag_threshold(dtc, cuda, name):
    """One channel's filter raised to 2^19: the output under the input's 2 is 2^20, its square alone 2^40 -- the
    partial that holds it is out of range in every partition. Flag set, every total NaN, y still exact."""
    jexp = J_IN.copy()
    jexp[37] = 19
    jexp2 = J_IN2.copy()
    jexp2[5] = 19
    for i, (y, exp, stats) in enumerate(_produce(dtc, cuda, name, jexp, jexp2=jexp2)):
        assert np.abs(exp).max() == 2.0 ** 20
        np.testing.assert_array_equal(y, exp, err_msg=f"{name} output {i}")
        _assert_flagged(dtc, stats, K, f"{name} output {i}")


@pytest.mark.parametrize("name", ["halo", "stem_wlds1"])
def test_producer_flag_on_inf_input(dtc, cuda, name):
    xi = _ints(1).copy()
    xi[1, 5, 9] = np.inf
    for i, (y, exp, stats) in enumerate(_produce(dtc, cuda, name, J_IN, xi=xi)):
        assert np.isinf(y[(1 * HW + 5) * HW + 9]).all()
        _assert_flagged(dtc, stats, K, f"{name} with +inf")


# ---- the backward reductions
A_EXP = _exps(-13, 7, 5)   # dy = integer * 2^a, x = integer * 2^b: dz * xhat = integer * 2^(a + b), a + b in -26..14
B_EXP = _exps(-13, 7, 11)
B2_EXP = _exps(-13, 7, 13)


@functools.lru_cache(maxsize=None)
def _bwd_data(big):
    g = np.random.default_rng(77)
    dyi, x1i, x2i = (g.integers(-2, 3, (M, K)).astype(np.float64) for _ in range(3))
    bits = g.random((M, K)) < 0.6
    dy, x1, x2 = dyi * 2.0 ** A_EXP, x1i * 2.0 ** B_EXP, x2i * 2.0 ** B2_EXP
    if big:  # dz * xhat = 2^40 at one element
        dy[3, 9] = x1[3, 9] = x2[3, 9] = 2.0 ** 20
        bits[3, 9] = True
    for a in (dy, x1, x2):
        assert np.array_equal(O.bf16(a), a.astype(np.float32))
    dz = np.where(bits, dy, 0.0)
    fr = lambda col, e: int(round(col.sum() * 2.0 ** -int(e))) * Fraction(2) ** int(e)
    sd = [fr(dz[:, c], A_EXP[c]) for c in range(K)]
    sx1 = [fr(dz[:, c] * x1[:, c], A_EXP[c] + B_EXP[c]) for c in range(K)]
    sx2 = [fr(dz[:, c] * x2[:, c], A_EXP[c] + B2_EXP[c]) for c in range(K)]
    return dict(dy=dy, x1=x1, x2=x2, bits=bits, dz=dz, sd=sd, sx1=sx1, sx2=sx2)


def _bwd_operands(dev, D, dual):
    gam = np.random.default_rng(3)
    gamma1, gamma2 = _affine(K, gam)[0], _affine(K, gam)[0]
    zero, one = torch.zeros(K, device=dev), torch.ones(K, device=dev)
    sec = dict(x2=_bf(D["x2"], dev), mean2=zero, invstd2=one) if dual else {}
    return gamma1, gamma2, zero, one, sec


@pytest.mark.parametrize("dual", [False, True])
def test_bwd_reduce_sums_exact(dtc, cuda, dual):
    """dtc_bn_bwd_reduce (bn_bwd_reduce_kernel<MASK>): mean = 0 and invstd = 1 make xhat = x exactly; sum dz and
    sum dz * xhat EQUAL the exact sums, for one BN and for two sharing dz; dtc_bn_bwd_finalize then gives dgamma /
    dbeta = float32(total * gscale) exactly (gscale a power of two) and re-zeroes the slots."""
    D = _bwd_data(False)
    g1, g2, zero, one, sec = _bwd_operands(cuda, D, dual)
    ym = _bf(D["bits"].astype(np.float32), cuda)
    runs = [dtc.ops.bn_bwd_reduce(_bf(D["dy"], cuda), ym, _bf(D["x1"], cuda), zero, one, **sec) for _ in range(2)]
    torch.cuda.synchronize()
    dz, acc1, acc2 = runs[0]
    np.testing.assert_array_equal(dz.float().cpu().numpy(), D["dz"].astype(np.float32))
    for acc, other, sx, gamma in ((acc1, runs[1][1], D["sx1"], g1),) + (((acc2, runs[1][2], D["sx2"], g2),) if dual else ()):
        assert int(acc[0].item()) == 0 and torch.equal(acc, other)
        _assert_totals_equal(dtc, acc, (D["sd"], sx), f"bn_bwd_reduce dual={dual}")
        dgamma, dbeta, _ = dtc.ops.bn_bwd_finalize(acc, M, _f(gamma, cuda), zero, one, gscale=GSCALE)
        np.testing.assert_array_equal(dgamma.cpu().numpy(), np.float32(W.f64(sx) * GSCALE))
        np.testing.assert_array_equal(dbeta.cpu().numpy(), np.float32(W.f64(D["sd"]) * GSCALE))
        assert int(acc.abs().sum().item()) == 0


@pytest.mark.parametrize("dual", [False, True])
def test_bwd_mask_two_pass_sums_exact(dtc, cuda, dual):
    """dtc_bn_bwd_mask(one_launch=0): the reduction (bn_bwd_reduce_kernel<MB>) leaves the exact sums in `acc`; the
    apply half (bn_bwd_fin_apply_kernel) folds exactly those: dgamma / dbeta = float32(total * gscale) exactly, dx
    against the float64 oracle within tests/bounds.py's bn_bwd_tol."""
    D = _bwd_data(False)
    g1, g2, zero, one, sec = _bwd_operands(cuda, D, dual)
    if dual:
        sec["gamma2"] = _f(g2, cuda)
    mask = torch.from_numpy(np.packbits(D["bits"], axis=-1, bitorder="little").reshape(-1)).to(cuda)
    words = int(dtc._native.lib.dtc_bn_stat_words(K))
    runs = []
    for _ in range(2):
        acc = torch.zeros((2 if dual else 1) * words, dtype=torch.int64, device=cuda)
        runs.append(dtc.ops.bn_bwd_mask(_bf(D["dy"], cuda), mask, _bf(D["x1"], cuda), _f(g1, cuda), zero, one, count=M,
                                        gscale=GSCALE, one_launch=False, acc=acc, **sec))
    torch.cuda.synchronize()
    r = runs[0]
    assert torch.equal(r["acc"], runs[1]["acc"])
    for j, (sx, gamma, x) in enumerate(((D["sx1"], g1, D["x1"]),) + (((D["sx2"], g2, D["x2"]),) if dual else ())):
        acc = r["acc"][j * words:(j + 1) * words]
        assert int(acc[0].item()) == 0
        _assert_totals_equal(dtc, acc, (D["sd"], sx), f"bn_bwd_mask dual={dual} BN {j}")
        np.testing.assert_array_equal(r[f"dgamma{j + 1}"].cpu().numpy(), np.float32(W.f64(sx) * GSCALE))
        np.testing.assert_array_equal(r[f"dbeta{j + 1}"].cpu().numpy(), np.float32(W.f64(D["sd"]) * GSCALE))
        dx_ref, _, _ = O.bn_train_bwd(D["dz"], x, gamma.astype(np.float64), np.zeros(K), np.ones(K))
        tol = B.bn_bwd_tol(dx_ref, D["dz"], x, gamma, np.zeros(K), np.ones(K))
        ratio = B.assert_within(r[f"dx{j + 1}"].float().cpu().numpy(), dx_ref, tol, f"bn_bwd_mask dual={dual} dx{j + 1}")
        print(f"bn_bwd_mask dual={dual} dx{j + 1}: worst |err|/tol {ratio:.3f}")


@pytest.mark.parametrize("dual", [False, True])
def test_bwd_producers_flag_threshold(dtc, cuda, dual):
    """dy = x = 2^20 at one element: that partial of sum dz * xhat is 2^40. Both reductions flag; the finalize and
    the apply half then give NaN for every channel's dgamma, dbeta, coefficients and dx."""
    D = _bwd_data(True)
    g1, g2, zero, one, sec = _bwd_operands(cuda, D, dual)
    ym = _bf(D["bits"].astype(np.float32), cuda)
    dz, acc1, acc2 = dtc.ops.bn_bwd_reduce(_bf(D["dy"], cuda), ym, _bf(D["x1"], cuda), zero, one, **sec)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dz.float().cpu().numpy(), D["dz"].astype(np.float32))
    for acc in (acc1, acc2) if dual else (acc1,):
        _assert_flagged(dtc, acc, K, f"bn_bwd_reduce dual={dual}")
        for t in dtc.ops.bn_bwd_finalize(acc, M, _f(g1, cuda), zero, one, gscale=GSCALE):
            assert bool(torch.isnan(t).all())
    if dual:
        sec["gamma2"] = _f(g2, cuda)
    mask = torch.from_numpy(np.packbits(D["bits"], axis=-1, bitorder="little").reshape(-1)).to(cuda)
    words = int(dtc._native.lib.dtc_bn_stat_words(K))
    acc = torch.zeros((2 if dual else 1) * words, dtype=torch.int64, device=cuda)
    r = dtc.ops.bn_bwd_mask(_bf(D["dy"], cuda), mask, _bf(D["x1"], cuda), _f(g1, cuda), zero, one, count=M,
                            gscale=GSCALE, one_launch=False, acc=acc, **sec)
    torch.cuda.synchronize()
    for j in range(2 if dual else 1):
        _assert_flagged(dtc, acc[j * words:(j + 1) * words], K, f"bn_bwd_mask dual={dual} BN {j}")
        for k in (f"dgamma{j + 1}", f"dbeta{j + 1}", f"dx{j + 1}"):
            assert bool(torch.isnan(r[k].float()).all()), k


# --------------------------------------------------------------------------------------------- B: consumers
C_B, M_B = 64, 32
SENTINEL = 0x5A5A5A5A5A5A  # in the unused header words: a consumer that re-zeroes slots must not touch the header


@functools.lru_cache(maxsize=None)
def _fwd_case(which):
    """One BatchNorm's targets, fp32 operands, float64 reference and a tiny bf16 x drawn around the targets' mean."""
    s, q = W.forward_targets(C_B, seed=11 + 10 * which)
    g = np.random.default_rng(100 + which)
    gamma, beta = _affine(C_B, g)
    rm0 = (g.standard_normal(C_B) * 0.1).astype(np.float32)
    rv0 = g.uniform(0.5, 2.0, C_B).astype(np.float32)
    ref = W.forward_reference(s, q, W.COUNT, gamma, beta, rm0, rv0)
    x = O.bf16((ref["mean"] + np.sqrt(ref["var"]) * g.standard_normal((M_B, C_B))).astype(np.float32))
    return dict(s=s, q=q, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, ref=ref, x=x)


def _device_words(dtc, dev, name, s, q, flag=0):
    words = W.encoded(dtc._native.lib, name, s, q, flag)
    hdr, _ = W.layout(dtc._native.lib)
    words[1:hdr] = SENTINEL
    return torch.from_numpy(words).to(dev), words


def _check_fwd_side(case, mean, invstd, rm, rv, what):
    """One float rounding of a double expression whose own error is a few 2^-53 (times 2^20 in the cancellation
    channel): within 1 fp32 ulp of the float64 reference rounded to fp32."""
    ref = case["ref"]
    for k, got in (("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rv)):
        u = W.ulps32(got.cpu().numpy(), ref[k])
        print(f"{what}: {k} worst {u.max():.2f} ulp")
        assert u.max() <= 1.0, (what, k, int(u.argmax()), float(u.max()))


def _all_nan(*tensors):
    return all(bool(torch.isnan(t.float()).all()) for t in tensors)


def test_fwd_finalize_encodings(dtc, cuda):
    """dtc_bn_fwd_finalize on the five encodings: mean, invstd and the running statistics within 1 ulp; scale =
    fp32(gamma * invstd) and shift = fp32(beta - fp32(mean) * scale) go through one / two more fp32 operations:
    within 2 ulp, shift's ulp taken at its larger term (the subtraction cancels in the constant channels). Slots
    zero afterwards, header untouched; all encodings bit-identical. Flag 1 / 2: everything NaN."""
    case = _fwd_case(0)
    hdr, _ = W.layout(dtc._native.lib)
    seen = None
    for name in W.ENCODINGS:
        for flag in (0, 1, 2):
            stats, words = _device_words(dtc, cuda, name, case["s"], case["q"], flag)
            rm, rv = _f(case["rm0"], cuda), _f(case["rv0"], cuda)
            nbt = torch.full((1,), 5, dtype=torch.int64, device=cuda)
            out = dtc.ops.bn_fwd_finalize(stats, W.COUNT, _f(case["gamma"], cuda), _f(case["beta"], cuda), rm, rv, nbt)
            torch.cuda.synchronize()
            after = stats.cpu().numpy()
            assert not after[hdr:].any() and np.array_equal(after[:hdr], words[:hdr]), (name, flag)
            assert int(nbt.item()) == 6
            if flag:
                assert _all_nan(*out, rm, rv), (name, flag)
                continue
            mean, invstd, scale, shift = out
            _check_fwd_side(case, mean, invstd, rm, rv, f"bn_fwd_finalize {name}")
            ref = case["ref"]
            us = W.ulps32(scale.cpu().numpy(), ref["scale"])
            uh = W.ulps32(shift.cpu().numpy(), ref["shift"], at=np.maximum(np.abs(case["beta"]), np.abs(ref["mean"] * ref["scale"])))
            print(f"bn_fwd_finalize {name}: scale worst {us.max():.2f} ulp, shift {uh.max():.2f} ulp")
            assert us.max() <= 2.0 and uh.max() <= 2.0, (name, float(us.max()), float(uh.max()))
            got = [t.cpu().numpy() for t in (mean, invstd, scale, shift, rm, rv)]
            if seen is not None:
                for a, b in zip(got, seen):
                    np.testing.assert_array_equal(a, b, err_msg=name)
            seen = got
    assert seen[1][0] == np.float32(1.0 / np.sqrt(float(np.float32(1e-5))))  # the constant channel: var == 0 exactly


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_fin_apply_encodings(dtc, cuda, mode):
    """dtc_bn_fin_apply (fold_sums / fa_fwd_coef_from in every workgroup): saved and running statistics within 1
    ulp, y on M = 32 rows against the float64 oracle within tests/bounds.py's bn_apply bound, the words left as
    they were, all encodings bit-identical. In mode 3 the second BN has other targets in another encoding."""
    c1, c2 = _fwd_case(0), _fwd_case(1)
    g = np.random.default_rng(9)
    res = O.bf16(g.standard_normal((M_B, C_B)).astype(np.float32))
    x2 = res if mode == 2 else c2["x"]
    z1, dz1 = B.bn_z(c1["x"], c1["gamma"], c1["beta"], c1["ref"]["mean"], c1["ref"]["invstd"])
    if mode == 1:
        ref, tol = B.bn_apply_ref_tol(z1, dz1)
    elif mode == 2:
        ref, tol = B.bn_apply_ref_tol(z1, dz1, res=res)
    else:
        z2, dz2 = B.bn_z(c2["x"], c2["gamma"], c2["beta"], c2["ref"]["mean"], c2["ref"]["invstd"])
        ref, tol = B.bn_apply_ref_tol(z1, dz1, z2=z2, dz2=dz2)
    assert (ref > 0).any() and (ref == 0).any()
    seen = None
    for i, name in enumerate(W.ENCODINGS):
        name2 = W.ENCODINGS[(i + 2) % len(W.ENCODINGS)]
        st1, w1 = _device_words(dtc, cuda, name, c1["s"], c1["q"])
        st2, w2 = _device_words(dtc, cuda, name2, c2["s"], c2["q"])
        rm, rv, rm2, rv2 = (_f(a, cuda) for a in (c1["rm0"], c1["rv0"], c2["rm0"], c2["rv0"]))
        nbt, nbt2 = (torch.full((1,), v, dtype=torch.int64, device=cuda) for v in (7, 3))
        bn2 = dict(stats=st2, gamma=_f(c2["gamma"], cuda), beta=_f(c2["beta"], cuda), running_mean=rm2, running_var=rv2,
                   nbt=nbt2) if mode == 3 else None
        y, mask, (mean, invstd), second = dtc.ops.bn_fin_apply(
            mode, _bf(c1["x"], cuda), st1, W.COUNT, _f(c1["gamma"], cuda), _f(c1["beta"], cuda), rm, rv, nbt,
            x2=None if mode == 1 else _bf(x2, cuda), bn2=bn2)
        torch.cuda.synchronize()
        assert np.array_equal(st1.cpu().numpy(), w1) and np.array_equal(st2.cpu().numpy(), w2), name
        _check_fwd_side(c1, mean, invstd, rm, rv, f"bn_fin_apply mode {mode} {name}")
        got = [y.float().cpu().numpy(), mean.cpu().numpy(), invstd.cpu().numpy(), rm.cpu().numpy(), rv.cpu().numpy()]
        if mode == 3:
            _check_fwd_side(c2, *second, rm2, rv2, f"bn_fin_apply mode 3 second BN {name2}")
            got += [t.cpu().numpy() for t in (*second, rm2, rv2)]
            assert int(nbt2.item()) == 4
        assert int(nbt.item()) == 8
        ratio = B.assert_within(got[0], ref, tol, f"bn_fin_apply mode {mode} {name}")
        print(f"bn_fin_apply mode {mode} {name}: y worst |err|/tol {ratio:.3f}")
        assert torch.equal(mask, dtc.ops.bn_mask_bits(y).reshape(-1))
        if seen is not None:
            for a, b in zip(got, seen):
                np.testing.assert_array_equal(a, b, err_msg=name)
        seen = got


def test_bwd_finalize_encodings(dtc, cuda):
    """dtc_bn_bwd_finalize: dgamma / dbeta (one rounding of total * gscale) within 1 ulp, coef[3][C] (one rounding
    of a double expression of fp32 inputs) within 2 ulp of the float64 reference; acc re-zeroed, header untouched,
    encodings bit-identical; flag 1 / 2: all NaN."""
    sd, sx = W.backward_targets(C_B)
    g = np.random.default_rng(31)
    gamma, _ = _affine(C_B, g)
    mean = (g.standard_normal(C_B) * 3).astype(np.float32)
    invstd = g.uniform(0.2, 4.0, C_B).astype(np.float32)
    ref = W.backward_reference(sd, sx, W.COUNT, gamma, mean, invstd, GSCALE)
    hdr, _ = W.layout(dtc._native.lib)
    seen = None
    for name in W.ENCODINGS:
        for flag in (0, 1, 2):
            acc, words = _device_words(dtc, cuda, name, sd, sx, flag)
            out = dtc.ops.bn_bwd_finalize(acc, W.COUNT, _f(gamma, cuda), _f(mean, cuda), _f(invstd, cuda), gscale=GSCALE)
            torch.cuda.synchronize()
            after = acc.cpu().numpy()
            assert not after[hdr:].any() and np.array_equal(after[:hdr], words[:hdr]), (name, flag)
            if flag:
                assert _all_nan(*out), (name, flag)
                continue
            got = [t.cpu().numpy() for t in out]
            ud, ub, uc = W.ulps32(got[0], ref["dgamma"]), W.ulps32(got[1], ref["dbeta"]), W.ulps32(got[2], ref["coef"])
            print(f"bn_bwd_finalize {name}: dgamma {ud.max():.2f} dbeta {ub.max():.2f} coef {uc.max():.2f} ulp")
            assert ud.max() <= 1.0 and ub.max() <= 1.0 and uc.max() <= 2.0, name
            if seen is not None:
                for a, b in zip(got, seen):
                    np.testing.assert_array_equal(a, b, err_msg=name)
            seen = got


@pytest.mark.parametrize("flag", [1, 2])
@pytest.mark.parametrize("mode,flagged", [(1, "first"), (2, "first"), (3, "first"), (3, "second")])
def test_fin_apply_flagged(dtc, cuda, mode, flagged, flag):
    """A flagged accumulator (header 1, or 2 as a two-rank sum of flags leaves it): every saved and running statistic
    of that BN and EVERY output element NaN -- the ReLU must not turn the NaN pre-activation into 0 (part C)."""
    c1, c2 = _fwd_case(0), _fwd_case(1)
    st1, _ = _device_words(dtc, cuda, "slot0", c1["s"], c1["q"], flag if flagged == "first" else 0)
    st2, _ = _device_words(dtc, cuda, "hi_cancel", c2["s"], c2["q"], flag if flagged == "second" else 0)
    rm, rv, rm2, rv2 = (_f(a, cuda) for a in (c1["rm0"], c1["rv0"], c2["rm0"], c2["rv0"]))
    bn2 = dict(stats=st2, gamma=_f(c2["gamma"], cuda), beta=_f(c2["beta"], cuda), running_mean=rm2,
               running_var=rv2) if mode == 3 else None
    y, _, first, second = dtc.ops.bn_fin_apply(mode, _bf(c1["x"], cuda), st1, W.COUNT, _f(c1["gamma"], cuda),
                                               _f(c1["beta"], cuda), rm, rv, x2=None if mode == 1 else _bf(c2["x"], cuda),
                                               bn2=bn2)
    torch.cuda.synchronize()
    assert _all_nan(y), f"{int((~torch.isnan(y.float())).sum())} of {y.numel()} outputs are not NaN"
    if flagged == "first":
        assert _all_nan(*first, rm, rv)
        if mode == 3:
            assert all(bool(torch.isfinite(t).all()) for t in (*second, rm2, rv2))
    else:
        assert _all_nan(*second, rm2, rv2) and all(bool(torch.isfinite(t).all()) for t in (*first, rm, rv))


# --------------------------------------------------------------------------------------------- C: NaN through the ReLU
M_C, C_C = 40, 64
U = 2.0 ** -24


def _assert_nan_aware(got, ref, tol, what):
    """NaN exactly where the reference is NaN, equal where it is infinite, within tol elsewhere."""
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), \
        f"{what}: NaN in {int(np.isnan(got).sum())} places, the reference in {int(nan.sum())}; " \
        f"{int((nan & ~np.isnan(got)).sum())} reference NaNs came out as numbers"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), what
    ok = ~(nan | inf)
    return B.assert_within(got[ok], ref[ok], tol[ok], what)


@functools.lru_cache(maxsize=None)
def _nan_case():
    g = np.random.default_rng(55)
    x = O.bf16(g.standard_normal((M_C, C_C)).astype(np.float32) * 2)
    x2 = O.bf16(g.standard_normal((M_C, C_C)).astype(np.float32))
    scale, shift = g.uniform(0.5, 1.5, C_C).astype(np.float32), g.uniform(-0.5, 0.5, C_C).astype(np.float32)
    scale2, shift2 = g.uniform(0.5, 1.5, C_C).astype(np.float32), g.uniform(-0.5, 0.5, C_C).astype(np.float32)
    scale[[3, 40]] = np.nan       # a NaN coefficient on two channels (both halves of a 64-channel group's lanes)
    shift[17] = np.nan
    scale2[50] = np.nan
    scale[9] = -scale[9]          # -inf * negative scale = +inf below
    x[0, 0] = x[39, 63] = x[20, 21] = np.nan
    x[5, 8] = np.inf              # relu(+inf) = +inf
    x[6, 8] = -np.inf             # relu(-inf) = 0
    x[7, 9] = -np.inf             # negative scale: +inf
    x2[1, 1] = x2[38, 62] = np.nan
    x2[5, 8] = -np.inf            # modes 2 / 3: inf - inf = NaN
    x2[11, 12] = np.inf
    return x, x2, scale, shift, scale2, shift2


def _z(x, scale, shift):
    """x * scale + shift in float64 and the bound on the fp32 value the kernel holds for it (two fp32 roundings of
    magnitudes at most |x * scale| + |shift|; 4 U covers them with or without the fused multiply-add)."""
    with np.errstate(invalid="ignore"):
        x, scale, shift = (np.asarray(v, np.float64) for v in (x, scale, shift))
        z = x * scale + shift
        return z, 4 * U * (np.abs(x * scale) + np.abs(shift))


def _nan_refs():
    x, x2, scale, shift, scale2, shift2 = _nan_case()
    with np.errstate(invalid="ignore"):
        z1, d1 = _z(x, scale, shift)
        z2, d2 = _z(x2, scale2, shift2)
        r1 = B.bn_apply_ref_tol(z1, d1)
        r2 = (O.relu(O.bf16(z1).astype(np.float64) + x2), B.bn_apply_ref_tol(z1, d1, res=x2)[1])
        r3 = (O.relu(O.bf16(z1).astype(np.float64) + O.bf16(z2)), B.bn_apply_ref_tol(z1, d1, z2=z2, dz2=d2)[1])
    return r1, r2, r3


def test_apply_relu_keeps_nan(dtc, cuda):
    """dtc_bn_apply_relu / _add_relu / _dual_relu (bn_apply_kernel) with NaN coefficients on some channels and NaN,
    +inf and -inf in x, res and x2: NaN exactly where the float64 oracle (np.maximum, as torch.relu) has NaN, +inf
    where it has +inf, 0 for -inf, and the usual bn_apply bound everywhere else."""
    x, x2, scale, shift, scale2, shift2 = _nan_case()
    xd, x2d = _bf(x, cuda), _bf(x2, cuda)
    s, h, s2, h2 = (_f(a, cuda) for a in (scale, shift, scale2, shift2))
    got = (dtc.ops.bn_apply_relu(xd, s, h), dtc.ops.bn_apply_add_relu(xd, s, h, x2d),
           dtc.ops.bn_apply_dual_relu(xd, s, h, x2d, s2, h2))
    torch.cuda.synchronize()
    for name, y, (ref, tol) in zip(("relu", "add_relu", "dual_relu"), got, _nan_refs()):
        assert np.isnan(ref).sum() >= 2 * M_C and np.isinf(ref).any() and (ref[~np.isnan(ref)] == 0).any()
        ratio = _assert_nan_aware(y.float().cpu().numpy(), ref, tol, f"bn_apply_{name}")
        print(f"bn_apply_{name}: {int(np.isnan(ref).sum())} NaN, worst |err|/tol elsewhere {ratio:.3f}")


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_fin_apply_relu_keeps_nan_data(dtc, cuda, mode):
    """dtc_bn_fin_apply (bn_fin_apply_kernel) with a clean accumulator and NaN / +-inf in x and x2: the statistics
    are what the words say (finite), the outputs NaN where the oracle's are."""
    c1, c2 = _fwd_case(0), _fwd_case(1)
    x, x2 = c1["x"].copy(), (c2["x"] if mode == 3 else O.bf16(np.random.default_rng(9).standard_normal((M_B, C_B)).astype(np.float32))).copy()
    x[0, 0] = x[31, 63] = x[13, 30] = np.nan
    x[4, 20] = np.inf
    x[5, 20] = -np.inf
    x2[2, 2] = np.nan
    x2[4, 20] = -np.inf
    gamma = np.abs(c1["gamma"]) + 0.25  # positive scale everywhere: +inf stays +inf, -inf becomes 0
    st1, _ = _device_words(dtc, cuda, "lo_slot_max", c1["s"], c1["q"])
    st2, _ = _device_words(dtc, cuda, "hi_negative", c2["s"], c2["q"])
    bn2 = dict(stats=st2, gamma=_f(c2["gamma"], cuda), beta=_f(c2["beta"], cuda)) if mode == 3 else None
    y, _, _, _ = dtc.ops.bn_fin_apply(mode, _bf(x, cuda), st1, W.COUNT, _f(gamma, cuda), _f(c1["beta"], cuda),
                                      x2=None if mode == 1 else _bf(x2, cuda), bn2=bn2)
    torch.cuda.synchronize()
    with np.errstate(invalid="ignore"):
        z1, dz1 = B.bn_z(x, gamma, c1["beta"], c1["ref"]["mean"], c1["ref"]["invstd"])
        if mode == 1:
            ref, tol = B.bn_apply_ref_tol(z1, dz1)
        elif mode == 2:
            ref, tol = O.relu(O.bf16(z1).astype(np.float64) + x2), B.bn_apply_ref_tol(z1, dz1, res=x2)[1]
        else:
            z2, dz2 = B.bn_z(x2, c2["gamma"], c2["beta"], c2["ref"]["mean"], c2["ref"]["invstd"])
            ref, tol = O.relu(O.bf16(z1).astype(np.float64) + O.bf16(z2)), B.bn_apply_ref_tol(z1, dz1, z2=z2, dz2=dz2)[1]
    assert np.isnan(ref).sum() >= 3 and (mode == 1) == bool(np.isposinf(ref).any())
    _assert_nan_aware(y.float().cpu().numpy(), ref, tol, f"bn_fin_apply mode {mode} with NaN data")
