"""Element-wise error bounds for the bf16-output kernels, a reporting assert, and guard-band arenas.

A Frobenius-norm criterion (tests/conftest.py rel_err < 1e-2) absorbs bf16 rounding but also lets 1e-4 of a
tensor's energy be arbitrarily wrong: a few zeroed pixels, a tap dropped at a border, one workgroup's channels
in a few rows. The bounds here hold every element to what the arithmetic of a correct kernel allows. They are
derived from the number formats and from how the kernels accumulate, never fitted to an observed error.

    U = 2**-24   fp32 unit roundoff
    HB = 2**-8   largest relative half-ulp of bf16 (8 significand bits)

An fp32 value within `d` of the exact `ref`, rounded to bf16, lies within

    tol(ref, d) = HB * (|ref| + d) + d

of `ref`. Everything is numpy float64.

Conv FWD / DGRAD (exact bf16 operands, fp32 accumulation, bf16 store): with S the same convolution of the
absolute operands (plus |res| where a residual is added before the rounding, plus the absolute shortcut
dgrad where a fused shortcut shares the accumulator) and L the reduction length (R*S*C for FWD, R*S*K for
DGRAD, + K for a fused shortcut), d = CONV_FACTOR * L * U * S: the classic bound L * U * S of a length-L fp32
dot product in any order, times 2 (see CONV_FACTOR).

BN forward applies: z = x*a + b with a = gamma*invstd, b = beta - mean*a, unrounded in float64. The kernel's
coefficients come from a mean and invstd held to rtol 1e-5 (mean atol 1e-6) by the same tests, so
dz = 3e-5 * (|x*a| + |mean*a| + |beta|) + 1e-6 * |a| (1e-5 each for invstd and mean plus the fp32 roundings,
all well under the third 1e-5). Modes 2 / 3 round each BN output to bf16 before the add: e = tol(z, dz) per
branch, then tol(ref, e1 [+ e2]); the reference itself holds no intermediate rounding.

BN backward dx: mean / invstd are inputs; the kernels evaluate A*dz + B*x + C, which cancels when |mean| >> std,
so the bound is in |x| and |mean| separately:
T = |a| * (|dz| + |mean(dz)| + invstd * (|x| + |mean|) * mean(|dz * xhat|)), d = 16 * U * T (at most 8 fp32
roundings in the chain, doubled).

Head dact: d = 2 * ncls * U * (|dlogits| @ |W|) / HW.

Head pool: feat = bf16(mean_p act). HW - 1 fp32 adds in any order plus the divide: d = (HW + 1) * U * mean_p |act|
against the float64 mean; bound tol(ref, d) (fp32 executor: no rounding of the result, bound d).

Head Linear: logits = bf16(feat . W[j] + bf16(b[j])) from the kernel's own feat (exact bf16 values), the products
and the bias summed in fp32 in any order: S = |feat| @ |W|.T + |bf16(b)|, d = 2 * (C + 1) * U * S (the dot-product
bound of C + 1 terms, doubled as CONV_FACTOR is); bound tol(ref, d). fp32 executor: b unrounded, bound d.

Head dW / db (fp32 outputs, no bf16 term): scale * sum_n dl[n][j] * feat[n][c] over N images in any order, then
the multiply by scale: 2 * (N + 1) * U * scale * (|dl|.T @ |feat|), and 2 * (N + 1) * U * scale * sum_n |dl|.

Conv WGRAD (exact bf16 operands, fp32 accumulation, fp32 output, no bf16 term): dw[k,r,s,c] = scale * sum over
the M = N*P*Q output pixels of dy[n,p,q,k] * x[n, p*st-pad+r, q*st-pad+s, c] (padding taps contribute exact zeros),
the products exact in fp32, summed in any order (MFMA k-steps, split-K slabs, the reduce launch), then the multiply
by scale: the length-M dot-product bound plus one rounding, (M + 1) * U * |scale| * S with S the same weight
gradient of the absolute operands, doubled for the reasons CONV_FACTOR gives: 2 * (M + 1) * U * |scale| * S. The
bound grows with M and has no teeth at large batches; it is meant for the small shapes that use it.

SGD (Nesterov), all fp32: m' = mu*m + (g*is + wd*p), p' = p - lr*((g*is + wd*p) + mu*m'). With
Tm = mu|m| + |g|*is + wd|p| every intermediate of the first chain is at most Tm in magnitude and the chain holds at
most four roundings (g*is, wd*p, their sum, mu*m + that; fewer with FMA contraction): tol_m = 4 * U * Tm. With
Tp = |p| + lr*((|g|*is + wd|p|) + mu*Tm) the second chain adds at most four more (mu*m', the sum, the product with
lr, the subtraction) on values bounded by Tp: tol_p = 8 * U * Tp. The reference is float64 arithmetic on the fp32
inputs with the scalars at their fp32 values.
"""
import numpy as np

from oracle import ops as O

U = 2.0 ** -24
HB = 2.0 ** -8
# 2 = the plain dot-product bound L*U*S doubled. The doubling covers (a) an accumulator that truncates where
# round-to-nearest was assumed (error per add up to 2U), (b) the split-K partial adds (at most num_kt <= L/16
# of them, igemm_plan) and (c) the residual add. Raise it only with a derivation from how the accumulation is
# performed, written here; never to fit an observed ratio.
CONV_FACTOR = 2.0


def _f64(a):
    return np.asarray(a, np.float64)


def tol(ref, d):
    """Bound on |bf16(v) - ref| for any fp32 v with |v - ref| <= d."""
    ref, d = _f64(ref), _f64(d)
    return HB * (np.abs(ref) + d) + d


def assert_within(got, ref, tol, name):
    """Fail if any |got - ref| > tol, or got is non-finite where ref is finite; the message counts the offending
    elements and gives the worst |err| / tol with the multi-index of the worst and of the first offender, so a
    failure points at a tile edge. Returns the worst ratio (callers print it)."""
    got, ref = _f64(got), _f64(ref)
    bound = np.broadcast_to(_f64(tol), ref.shape)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} vs reference {ref.shape}"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = err / bound  # a non-finite got gives inf or NaN here; so does any error under a zero bound
    nan = np.isnan(ratio)
    if nan.any():  # 0 / 0 is an exact match under a zero bound; every other NaN (NaN got, inf / inf) offends
        ratio[nan] = np.where(err[nan] == 0, 0.0, np.inf)
    worst = float(ratio.max()) if ratio.size else 0.0
    bad = ratio > 1.0
    if bad.any():
        iw = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        i0 = np.unravel_index(int(np.flatnonzero(bad.ravel())[0]), ratio.shape)
        t = lambda i: tuple(int(v) for v in i)
        raise AssertionError(
            f"{name}: {int(bad.sum())} of {bad.size} elements outside the bound; worst |err|/tol {worst:.3g} at "
            f"{t(iw)} (got {got[iw]!r}, ref {ref[iw]!r}, tol {bound[iw]:.3g}); first at {t(i0)} "
            f"(got {got[i0]!r}, ref {ref[i0]!r}, tol {bound[i0]:.3g})")
    return worst


# ----------------------------------------------------------------------------- convolution
def conv_tol(ref, S, L):
    """ref: the float64 oracle output; S: the oracle on absolute operands (+ |res| ...); L: reduction length."""
    return tol(ref, CONV_FACTOR * L * U * _f64(S))


def fwd_tol(ref, x, w, stride, pad):
    K, R, S_, C = np.shape(w)
    return conv_tol(ref, O.conv2d_fwd(np.abs(x), np.abs(w), stride, pad), R * S_ * C)


def dgrad_tol(ref, dy, w, in_hw, stride, pad, res=None, dsc=None, wsc=None):
    """DGRAD (+ residual added before the rounding) (+ the fused 1x1 stride-`stride` shortcut dgrad of dsc, wsc
    [K,1,1,C], sharing the accumulator)."""
    K, R, S_, C = np.shape(w)
    S = O.conv2d_dgrad(np.abs(dy), np.abs(w), in_hw, stride, pad)
    L = R * S_ * K
    if res is not None:
        S = S + np.abs(res)
    if dsc is not None:
        S = S + O.conv2d_dgrad(np.abs(dsc), np.abs(wsc), in_hw, stride, 0)
        L += K
    return conv_tol(ref, S, L)


def wgrad_tol(x, dy, R, S, stride, pad, scale=1.0):
    """Bound on |dw - scale * O.conv2d_wgrad(x, dy, ...)| for the fp32 weight gradient [K,R,S,C]; M = N*P*Q."""
    M = int(np.prod(np.shape(dy)[:3]))
    return 2 * (M + 1) * U * abs(scale) * O.conv2d_wgrad(np.abs(x), np.abs(dy), R, S, stride, pad)


# ----------------------------------------------------------------------------- batch norm
def bn_z(x, gamma, beta, mean, invstd):
    """The unrounded BN output z = x*a + b (float64) and the bound dz on the fp32 value a kernel holds for it."""
    x, gamma, beta, mean, invstd = (_f64(v) for v in (x, gamma, beta, mean, invstd))
    a = gamma * invstd
    z = x * a + (beta - mean * a)
    dz = 3e-5 * (np.abs(x * a) + np.abs(mean * a) + np.abs(beta)) + 1e-6 * np.abs(a)
    return z, dz


def bn_apply_ref_tol(z1, dz1, res=None, z2=None, dz2=None):
    """(ref, tol) of the forward applies: relu(z1) (mode 1), relu(z1 + res) (mode 2, res exact bf16),
    relu(z1 + z2) (mode 3); in modes 2 / 3 each BN output is rounded to bf16 before the add."""
    if res is None and z2 is None:
        ref = O.relu(z1)
        return ref, tol(ref, dz1)
    e = tol(z1, dz1)
    if z2 is not None:
        ref = O.relu(z1 + z2)
        e = e + tol(z2, dz2)
    else:
        ref = O.relu(z1 + _f64(res))
    return ref, tol(ref, e)


def bn_bwd_tol(ref, dz, x, gamma, mean, invstd):
    """Bound on the bf16 dx of the BN backward applies; dz, x [M, C] (or NHWC), the rest per channel."""
    dz, x, gamma, mean, invstd = (_f64(v) for v in (dz, x, gamma, mean, invstd))
    C = x.shape[-1]
    dz2, x2 = dz.reshape(-1, C), x.reshape(-1, C)
    a = np.abs(gamma * invstd)
    xhat = (x2 - mean) * invstd
    T = a * (np.abs(dz2) + np.abs(dz2.mean(0)) + invstd * (np.abs(x2) + np.abs(mean)) * np.abs(dz2 * xhat).mean(0))
    return tol(ref, (16 * U * T).reshape(x.shape))


def head_dact_tol(ref, dlogits, w, hw, bf=True):
    """dact [N,h,w,C] = (dlogits @ W) / (h*w) broadcast over the pixels (bf=False: the fp32 executor, d alone)."""
    ncls = np.shape(w)[0]
    d = 2 * ncls * U * (np.abs(_f64(dlogits)) @ np.abs(_f64(w))) / (hw[0] * hw[1])
    d = d[:, None, None, :]
    return tol(ref, d) if bf else np.broadcast_to(d, np.shape(ref))


def head_feat_tol(ref, act, bf=True):
    """feat [N,C] = mean over the pixels of act [N,h,w,C]; ref: that mean in float64."""
    a = np.abs(_f64(act)).reshape(np.shape(act)[0], -1, np.shape(act)[-1])
    d = (a.shape[1] + 1) * U * a.mean(axis=1)
    return tol(ref, d) if bf else d


def head_logits_ref_tol(feat, w, b, bf=True):
    """(ref, bound) of the Linear on the kernel's own feat: ref = feat @ W.T + bf16(b) in float64 (fp32 executor:
    b unrounded)."""
    feat, w = _f64(feat), _f64(w)
    bb = _f64(O.bf16(b)) if bf else _f64(b)
    ref = feat @ w.T + bb
    return ref, head_logits_tol(ref, feat, w, b, bf)


def head_logits_tol(ref, feat, w, b, bf=True):
    feat, w = _f64(feat), _f64(w)
    bb = _f64(O.bf16(b)) if bf else _f64(b)
    S = np.abs(feat) @ np.abs(w).T + np.abs(bb)
    d = 2 * (feat.shape[1] + 1) * U * S
    return tol(ref, d) if bf else d


def head_dw_tol(dl, feat, scale):
    """dW [ncls,C] = scale * dl.T @ feat, fp32."""
    dl, feat = _f64(dl), _f64(feat)
    return 2 * (dl.shape[0] + 1) * U * abs(scale) * (np.abs(dl).T @ np.abs(feat))


def head_db_tol(dl, scale):
    dl = _f64(dl)
    return 2 * (dl.shape[0] + 1) * U * abs(scale) * np.abs(dl).sum(axis=0)


# ----------------------------------------------------------------------------- SGD (Nesterov)
def sgd_ref(p, g, m, lr, wd, mu, inv_scale=1.0):
    """(p', m') of one step in float64 on the fp32 inputs, the scalars at their fp32 values."""
    p, g, m = _f64(p), _f64(g), _f64(m)
    lr, wd, mu, is_ = (float(np.float32(v)) for v in (lr, wd, mu, inv_scale))
    d = g * is_ + wd * p
    m2 = mu * m + d
    return p - lr * (d + mu * m2), m2


def sgd_tol(p, g, m, lr, wd, mu, inv_scale=1.0):
    """(tol_p, tol_m) for sgd_ref's outputs."""
    p, g, m = (np.abs(_f64(v)) for v in (p, g, m))
    lr, wd, mu, is_ = (abs(float(np.float32(v))) for v in (lr, wd, mu, inv_scale))
    Tm = mu * m + g * is_ + wd * p
    Tp = p + lr * ((g * is_ + wd * p) + mu * Tm)
    return 8 * U * Tp, 4 * U * Tm


# ----------------------------------------------------------------------------- guard-band arenas
GUARD_BYTES = 1 << 20  # > the largest single tile footprint these kernels address (256 px x 512 ch x 2 B = 256 KiB)
_PAT = {2: 0x7FD5, 4: 0x7FD5AAAA, 8: 0x7FD5AAAA7FD5AAAA}  # quiet-NaN bit patterns (int64 words: two 32-bit ones)


class Arena:
    """One flat device tensor filled with a quiet-NaN bit pattern, with `view` (the tensor under test) in its
    middle and at least GUARD_BYTES of pattern on each side: an over-read stays inside mapped memory and shows
    as NaN in an accumulator, a stray store shows in `dirty()`."""

    def __init__(self, shape, dtype, device, like=None, zero=False):
        import torch

        self.isz = torch.empty((), dtype=dtype).element_size()
        self.idt = {2: torch.int16, 4: torch.int32, 8: torch.int64}[self.isz]
        pat = _PAT[self.isz]
        self.pat = pat - (1 << (8 * self.isz)) if pat >= 1 << (8 * self.isz - 1) else pat
        n = 1
        for s in shape:
            n *= int(s)
        self.n = n
        g = GUARD_BYTES // self.isz
        self.bits = torch.full((2 * g + n + 256 // self.isz,), self.pat, dtype=self.idt, device=device)
        self.g = g + (-(self.bits.data_ptr() + GUARD_BYTES) % 256) // self.isz  # the view starts 256-byte aligned
        tail = self.bits.numel() - self.g - n
        self.flat = self.bits.view(dtype)
        self.view = self.flat[self.g:self.g + n].view(*shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 256 == 0
        assert self.g * self.isz >= GUARD_BYTES and tail * self.isz >= GUARD_BYTES
        if like is not None:
            self.view.copy_(like)
        elif zero:
            self.view.zero_()

    def dirty(self):
        """Number of guard words that no longer hold the pattern."""
        lo, hi = self.bits[:self.g], self.bits[self.g + self.n:]
        return int((lo != self.pat).sum().item()) + int((hi != self.pat).sum().item())


def arena(shape, dtype, device, like=None, zero=False):
    """(Arena, embedded tensor): `like` is copied into the view, `zero` zeroes it (statistics slots); otherwise
    the view keeps the NaN pattern (outputs, workspaces)."""
    a = Arena(shape, dtype, device, like=like, zero=zero)
    return a, a.view
