"""BN statistic accumulator words (csrc/common.h) built by hand, and their exact value.

An accumulator is [header, word 0 = flag][slot k][statistic j][hi, lo][channel c] int64 words and stands for the
per-channel totals sum_k hi[k] * 2^-8 + sum_k lo[k] * 2^-52. The producers only ever write what stat_add1 forms
(one slot per workgroup, 0 <= lo < 2^44 per add); the consumers must fold ANY words inside the documented range:
at most 2^15 adds per slot (lo up to 2^15 * (2^44 - 1)), totals below 2^55, no int64 wrap. `encodings` writes the
same targets in five such ways; tests/test_native_abi.py (host decoder) and tests/test_gpu_bn_stat_edges.py (the
device consumers) hold every one of them to the same exact reference.
"""
from fractions import Fraction

import numpy as np

LO_BITS = 44
LO_ONE = 1 << LO_BITS          # one unit of hi, in units of lo
LO_MAX_ADD = LO_ONE - 1        # the largest lo word of one add
LO_MAX_SLOT = (1 << 15) * LO_MAX_ADD  # the documented per-slot maximum (2^15 adds)
UNIT = Fraction(1, 1 << 52)    # value of one lo unit
COUNT = 512
ENCODINGS = ("slot0", "lo_add_max", "lo_slot_max", "hi_negative", "hi_cancel")


def layout(lib):
    """(header words, slots) of the accumulator format, from the size query alone."""
    hdr = 2 * int(lib.dtc_bn_stat_words(1)) - int(lib.dtc_bn_stat_words(2))
    return hdr, (int(lib.dtc_bn_stat_words(1)) - hdr) // 4


def build(lib, hi, lo, flag=0):
    """The accumulator words (numpy int64) of explicit per-slot words: hi, lo are [slots][2 statistics][C] arrays
    of Python ints (or int64); flag goes into header word 0."""
    hdr, slots = layout(lib)
    hi = np.array(hi, dtype=object)
    lo = np.array(lo, dtype=object)
    assert hi.shape == lo.shape and hi.shape[:2] == (slots, 2), hi.shape
    c = hi.shape[2]
    words = np.zeros(int(lib.dtc_bn_stat_words(c)), np.int64)
    body = words[hdr:].reshape(slots, 2, 2, c)
    for v in list(hi.ravel()) + list(lo.ravel()):
        assert -(1 << 63) <= int(v) < (1 << 63)
    body[:, :, 0, :] = hi.astype(np.int64)
    body[:, :, 1, :] = lo.astype(np.int64)
    words[0] = flag
    return words


def exact_totals(lib, words, c):
    """[2][c] Fractions: the value the words stand for (flag ignored)."""
    hdr, slots = layout(lib)
    body = np.asarray(words)[hdr:].reshape(slots, 2, 2, c)
    return [[sum(Fraction(int(body[k, j, 0, ch]), 256) + int(body[k, j, 1, ch]) * UNIT for k in range(slots))
             for ch in range(c)] for j in range(2)]


def encode(name, units, slots=8):
    """One total of `units` * 2^-52 (a Python int, either sign) as per-slot (hi[slots], lo[slots]) in the named
    way. Every form satisfies sum(hi) * 2^44 + sum(lo) == units exactly."""
    h0, l0 = units >> LO_BITS, units & (LO_ONE - 1)  # the producers' own split (floor)
    hi, lo = [0] * slots, [0] * slots
    if name == "slot0":
        hi[0], lo[0] = h0, l0
    elif name == "lo_add_max":
        # 2^44 - 1, the largest word of one add, in all eight slots where the total's low bits allow it (units = -8
        # mod 2^44: TARGETS has such channels); otherwise in seven, and slot 0 takes the remainder. The low words
        # sum to 7 * 2^44 and more: the carry out of lo is what the fold has to move into hi.
        for k in range(1, slots):
            lo[k] = LO_MAX_ADD
        lo[0] = (units - (slots - 1) * LO_MAX_ADD) & (LO_ONE - 1)
        hi[slots - 1] = (units - sum(lo)) >> LO_BITS
    elif name == "lo_slot_max":
        # every slot's lo at the documented per-slot maximum 2^15 * (2^44 - 1) (slot 0 short of it by what the
        # total's low bits ask for); hi compensates and comes out negative
        for k in range(slots):
            lo[k] = LO_MAX_SLOT
        lo[0] -= (sum(lo) - units) & (LO_ONE - 1)
        hi[3] = (units - sum(lo)) >> LO_BITS
    elif name == "hi_negative":
        # hi < 0 with lo > 0: 2^10 units of hi moved into the low words (2^7 * 2^44 per slot)
        for k in range(slots):
            lo[k] = 1 << (LO_BITS + 7)
        lo[5] += l0
        hi[2] = h0 - (1 << 10)
    else:
        assert name == "hi_cancel"
        # +-2^62 in different slots (one in each half of the slots: the finalize kernels sum the halves apart)
        hi[1], hi[6], lo[7] = 1 << 62, h0 - (1 << 62), l0
    assert sum(hi) * LO_ONE + sum(lo) == units and all(v >= 0 for v in lo)
    assert all(v <= LO_MAX_SLOT for v in lo) and all(abs(v) < (1 << 63) for v in hi)
    return hi, lo


def encoded(lib, name, s, q, flag=0):
    """The accumulator holding per-channel totals s, q (lists of Fractions, multiples of 2^-52) in encoding `name`."""
    _, slots = layout(lib)
    c = len(s)
    hi = np.zeros((slots, 2, c), dtype=object)
    lo = np.zeros((slots, 2, c), dtype=object)
    for j, tot in enumerate((s, q)):
        for ch, t in enumerate(tot):
            u = t / UNIT
            assert u.denominator == 1 and abs(t) < (1 << 55)
            h, l = encode(name, int(u), slots)
            hi[:, j, ch], lo[:, j, ch] = h, l
    return build(lib, hi, lo, flag)


def forward_targets(c=64, seed=11, count=COUNT):
    """(s, q): per-channel totals of sum x, sum x^2 over `count` elements as Fractions, multiples of 2^-52, with
    q / count >= (s / count)^2. Channel 0: constant a = 8 (variance exactly 0); 1: constant a = 2^-10; 2: mean / std
    = 2^10 (the variance is what is left of a 2^20-fold cancellation); 3: a large total (q ~ 2^53.1); 4-7: low bits
    2^44 - 8, so that `lo_add_max` is 2^44 - 1 in all eight slots; the rest random, means of either sign with bits
    far below 2^-8 (negative hi with positive lo in the plain form)."""
    g = np.random.default_rng(seed)
    mean, var = [], []
    for ch in range(c):
        m = Fraction(int(g.integers(-(1 << 34), 1 << 34)), 1 << 30)
        v = Fraction(int(g.integers(1, 1 << 28)), 1 << 24)
        if ch == 0:
            m, v = Fraction(8), Fraction(0)
        elif ch == 1:
            m, v = Fraction(1, 1 << 10), Fraction(0)
        elif ch == 2:
            m, v = Fraction(1 << 10) + Fraction(1, 1 << 12), Fraction(1) + Fraction(1, 1 << 20)
        elif ch == 3:
            m, v = Fraction(1 << 22) + Fraction(1, 1 << 8), Fraction(1 << 40)
        mean.append(m)
        var.append(v)
    s = [count * m for m in mean]
    q = [count * (v + m * m) for m, v in zip(mean, var)]
    for ch in range(4, min(8, c)):  # low bits 2^44 - 8; s moves by < 2^-8, so s^2 / count by < 1 (|s| < 2^14): q + 1
        s[ch] = _with_low_bits(s[ch], LO_ONE - 8)
        q[ch] = _with_low_bits(q[ch] + 1, LO_ONE - 8) + Fraction(1, 256)
    assert all(qq * count >= ss * ss for ss, qq in zip(s, q))
    return s, q


def backward_targets(c=64, seed=12):
    """(sum dz, sum dz * xhat): any in-range values of either sign, low bits everywhere."""
    g = np.random.default_rng(seed)
    sd = [Fraction(int(g.integers(-(1 << 40), 1 << 40)), 1 << 30) for _ in range(c)]
    sx = [Fraction(int(g.integers(-(1 << 44), 1 << 44)), 1 << 36) for _ in range(c)]
    sd[0], sx[1] = Fraction(0), Fraction(0)
    sd[2], sx[2] = _with_low_bits(sd[2], LO_ONE - 8), _with_low_bits(sx[2], LO_ONE - 8)
    return sd, sx


def _with_low_bits(t, low):
    u = int(t / UNIT)
    return ((u >> LO_BITS << LO_BITS) + low) * UNIT


def f64(fr):
    return np.array([float(v) for v in fr], np.float64)


def forward_reference(s, q, count, gamma, beta, rm0, rv0, momentum=0.1, eps=1e-5):
    """float64 reference of what a forward consumer forms from the exact totals (bn.hip: bn_fwd_finalize_kernel,
    bn_coef.h: fa_fwd_coef_from): dict of float64 arrays. eps and momentum are the fp32 values the kernel is
    handed."""
    s, q = f64(s), f64(q)  # correctly rounded from the exact totals
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    mean = s / count
    var = np.maximum(q / count - mean * mean, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    unbiased = var * count / (count - 1.0) if count > 1 else var
    return dict(mean=mean, var=var, invstd=invstd, scale=gamma * invstd, shift=beta - mean * gamma * invstd,
                running_mean=(1.0 - momentum) * np.asarray(rm0, np.float64) + momentum * mean,
                running_var=(1.0 - momentum) * np.asarray(rv0, np.float64) + momentum * unbiased)


def backward_reference(sd, sx, count, gamma, mean, invstd, gscale):
    """float64 reference of bn_bwd_finalize_kernel / fa_bwd_coef_from from the exact totals and the fp32 inputs."""
    sd, sx = f64(sd), f64(sx)
    gamma, mean, invstd = (np.asarray(v, np.float64) for v in (gamma, mean, invstd))
    gscale = float(np.float32(gscale))
    A = gamma * invstd
    Bc = -A * invstd * sx / count
    Cc = -A * sd / count - Bc * mean
    return dict(dgamma=sx * gscale, dbeta=sd * gscale, coef=np.stack([A, Bc, Cc]))


def ulps32(got, ref64, at=None):
    """|got - float32(ref64)| in units of the fp32 spacing at max(|ref64|, |at|) (at: a larger magnitude the value
    was formed from, for results of a cancelling fp32 subtraction). NaN / inf where either side is non-finite."""
    got = np.asarray(got, np.float32).astype(np.float64)
    ref = np.asarray(ref64, np.float64).astype(np.float32)
    mag = np.abs(ref) if at is None else np.maximum(np.abs(ref), np.asarray(at, np.float64).astype(np.float32))
    sp = np.spacing(np.maximum(mag, np.float32(2.0 ** -126)).astype(np.float32)).astype(np.float64)
    return np.abs(got - ref.astype(np.float64)) / sp
