"""The element-wise comparator (tests/bounds.py) can fail: on the CPU, float32 emulations of the kernels'
formulas stay inside every derived bound, and localized faults that the global-norm criterion
(rel_err < 1e-2) accepts are rejected.

Each `got` is the bf16 rounding of a float32 numpy emulation whose accumulation is chunked (16 reduction
elements at a time, as an MFMA k-step) so that its order differs from the float64 oracle's. Mutations:

* conv FWD and DGRAD + residual at (16,32,32,64,64) (16 384 output pixels: one zeroed pixel moves the norm by
  7.8e-3): one pixel zeroed; one border pixel with its centre tap dropped; one corner pixel whose padding tap
  reads the neighbouring image's last row; two channels of one pixel swapped.
* bn_fin_apply mode 2 at M=4100 C=512 and the BN backward at M=4096 C=512: one 8-channel group of one row
  computed with the neighbouring channels' coefficients; two channels of one row swapped; one 64-channel group
  of one row zeroed (a whole zeroed row is 1/sqrt(M) = 1.6e-2 of the norm, which rel_err already rejects; the
  64-channel group is the largest zeroed piece it accepts). The tap mutations have no BN counterpart.
"""
import numpy as np
import pytest

from oracle import ops as O
from tests import bounds as B
from tests.conftest import rel_err

N, H, W, C, K = 16, 32, 32, 64, 64


def _rand_bf16(shape, gen, scale=1.0, shift=0.0):
    return O.bf16(gen.standard_normal(shape).astype(np.float32) * scale + shift)


def _check(name, clean, ref, tol, mutants):
    r = B.assert_within(clean, ref, tol, name)
    print(f"{name}: clean emulation worst |err|/tol {r:.3f}, rel_err {rel_err(clean, ref):.2e}")
    assert r < 1.0 and rel_err(clean, ref) < 1e-2
    for what, got in mutants.items():
        assert not np.array_equal(got, clean), what
        e = rel_err(got, ref)
        assert e < 1e-2, f"{name} / {what}: the norm criterion is meant to accept this ({e:.2e})"
        with pytest.raises(AssertionError, match="outside the bound") as ei:
            B.assert_within(got, ref, tol, f"{name} / {what}")
        print(f"{name} / {what}: rel_err {e:.2e} accepted; element-wise: {str(ei.value).split(':', 1)[1][:110]}")


class _ConvEmu:
    """3x3 stride-1 pad-1 convolution of `inp` [N,H,W,Ci] with `w` [Co,3,3,Ci] in float32, the reduction in
    16-element chunks, + res, rounded to bf16."""

    def __init__(self, inp, w, res=None):
        self.inp, self.res = inp, res
        self.cols = O._im2col(inp, 3, 3, 1, 1).astype(np.float32)  # [N,H,W,3,3,Ci]
        self.wt = np.ascontiguousarray(w.reshape(w.shape[0], -1).astype(np.float32).T)

    def _acc(self, rows):
        acc = np.zeros((rows.shape[0], self.wt.shape[1]), np.float32)
        for k0 in range(0, rows.shape[1], 16):
            acc += rows[:, k0:k0 + 16] @ self.wt[k0:k0 + 16]
        return acc

    def full(self):
        acc = self._acc(self.cols.reshape(-1, self.wt.shape[0])).reshape(self.inp.shape[:3] + (-1,))
        if self.res is not None:
            acc = acc + self.res.astype(np.float32)
        return O.bf16(acc)

    def pixel(self, n, h, w, taps):
        """The pixel's output with its gathered taps [3,3,Ci] replaced by `taps`."""
        acc = self._acc(taps.reshape(1, -1).astype(np.float32))[0]
        if self.res is not None:
            acc = acc + self.res[n, h, w].astype(np.float32)
        return O.bf16(acc)

    def mutants(self, clean):
        out = {}
        m = clean.copy()
        m[7, 13, 21, :] = 0
        out["one pixel zeroed"] = m
        m = clean.copy()
        taps = self.cols[3, 0, 5].copy()
        taps[1, 1, :] = 0
        m[3, 0, 5] = self.pixel(3, 0, 5, taps)
        out["border pixel, centre tap dropped"] = m
        m = clean.copy()
        taps = self.cols[2, 0, 0].copy()
        assert not taps[0, 1].any()  # the padding tap above the corner
        taps[0, 1, :] = self.inp[1, H - 1, 0, :]  # what lies there in memory: the previous image's last row
        m[2, 0, 0] = self.pixel(2, 0, 0, taps)
        out["corner pixel, padding tap from the neighbouring image"] = m
        m = clean.copy()
        m[9, 31, 31, [4, 5]] = m[9, 31, 31, [5, 4]]
        out["two channels of one pixel swapped"] = m
        return out


def test_conv_fwd_bound_rejects_localized_faults():
    g = np.random.default_rng(1)
    x = _rand_bf16((N, H, W, C), g)
    w = _rand_bf16((K, 3, 3, C), g, 0.05)
    ref = O.conv2d_fwd(x, w, 1, 1)
    emu = _ConvEmu(x, w)
    clean = emu.full()
    _check("conv FWD (16,32,32,64,64)", clean, ref, B.fwd_tol(ref, x, w, 1, 1), emu.mutants(clean))


def test_conv_dgrad_res_bound_rejects_localized_faults():
    g = np.random.default_rng(2)
    dy = _rand_bf16((N, H, W, K), g)
    w = _rand_bf16((K, 3, 3, C), g, 0.05)
    res = _rand_bf16((N, H, W, C), g)
    ref = O.conv2d_dgrad(dy, w, (H, W), 1, 1) + res
    # stride 1: dx = the forward conv of dy with the taps mirrored and K, C exchanged
    wflip = np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))
    emu = _ConvEmu(dy, wflip, res)
    clean = emu.full()
    _check("conv DGRAD + res (16,32,32,64,64)", clean, ref, B.dgrad_tol(ref, dy, w, (H, W), 1, 1, res=res),
           emu.mutants(clean))


def _affine(Cn, gen):
    return gen.uniform(0.5, 1.5, Cn).astype(np.float32), gen.uniform(-0.5, 0.5, Cn).astype(np.float32)


def _bn_mutants(clean, row_fn):
    """row_fn(row, channel permutation) -> that row computed with coefficient channel perm[c] for channel c."""
    Cn = clean.shape[1]
    out = {}
    perm = np.arange(Cn)
    perm[72:80] = np.arange(73, 81)
    m = clean.copy()
    m[2049] = row_fn(2049, perm)
    out["8-channel group of one row with the neighbouring channels' coefficients"] = m
    m = clean.copy()
    m[4095, [130, 131]] = m[4095, [131, 130]]
    out["two channels of one row swapped"] = m
    m = clean.copy()
    m[100, 448:512] = 0
    out["64-channel group of one row zeroed"] = m
    return out


def test_bn_fin_apply_mode2_bound_rejects_localized_faults():
    M, Cn = 4100, 512
    g = np.random.default_rng(3)
    x = _rand_bf16((M, Cn), g, 2.0, 0.5)
    res = _rand_bf16((M, Cn), g, 0.7, -0.3)
    gamma, beta = _affine(Cn, g)
    _, mean, invstd, _, _ = O.bn_train_fwd(x, gamma, beta)
    z, dz = B.bn_z(x, gamma, beta, mean, invstd)
    ref, tol = B.bn_apply_ref_tol(z, dz, res=res)
    f = np.float32
    scale = gamma * invstd.astype(f)                      # fp32 coefficients, as bn_coef.h forms them
    shift = beta - mean.astype(f) * scale

    def row(r, perm=slice(None)):
        zb = O.bf16(x[r] * scale[perm] + shift[perm])      # the BN output is rounded before the add
        return O.bf16(np.maximum(zb + res[r], f(0)))

    clean = row(slice(None))
    assert clean.dtype == np.float32
    _check("bn_fin_apply mode 2 M=4100 C=512", clean, ref, tol, _bn_mutants(clean, row))


def test_bn_bwd_bound_rejects_localized_faults():
    M, Cn = 4096, 512
    g = np.random.default_rng(4)
    x = _rand_bf16((M, Cn), g, 1.5, 0.2)
    dy = _rand_bf16((M, Cn), g)
    dz = np.where(g.random((M, Cn)) < 0.6, dy, 0).astype(np.float32)
    gamma, _ = _affine(Cn, g)
    f = np.float32
    _, mean, invstd, _, _ = O.bn_train_fwd(x, gamma, np.zeros(Cn))
    mean, invstd = mean.astype(f), invstd.astype(f)       # as the forward saves them
    ref, _, _ = O.bn_train_bwd(dz, x, gamma.astype(np.float64), mean.astype(np.float64), invstd.astype(np.float64))
    tol = B.bn_bwd_tol(ref, dz, x, gamma, mean, invstd)
    # exact sums (the kernels' fixed-point slots), then fp32 coefficients of A*dz + B*x + C
    s1 = dz.astype(np.float64).sum(0)
    s2 = (dz.astype(np.float64) * ((x - mean) * invstd).astype(np.float64)).sum(0)
    A = gamma * invstd
    Bc = -A * invstd * (s2 / M).astype(f)
    Cc = -A * (s1 / M).astype(f) - Bc * mean

    def row(r, perm=slice(None)):
        return O.bf16(A[perm] * dz[r] + Bc[perm] * x[r] + Cc[perm])

    clean = row(slice(None))
    assert clean.dtype == np.float32
    _check("bn_bwd M=4096 C=512", clean, ref, tol, _bn_mutants(clean, row))


def test_arena_layout_and_stray_store_detection():
    """The guard-band arena (host tensors here; tests/test_gpu_guard_bands.py uses it on the device): the view is
    256-byte aligned with at least 1 MiB of the quiet-NaN pattern on each side, and one changed guard word on
    either side is counted."""
    import torch

    for dtype, bits, shape in ((torch.bfloat16, 0x7FD5, (3, 5, 7, 64)), (torch.float32, 0x7FD5AAAA, (64, 27)),
                               (torch.int64, 0x7FD5AAAA7FD5AAAA, (131,))):
        src = torch.arange(int(np.prod(shape))).reshape(shape).to(dtype)
        a, v = B.arena(shape, dtype, "cpu", like=src)
        isz = v.element_size()
        assert v.data_ptr() % 256 == 0 and v.is_contiguous() and torch.equal(v, src)
        assert v.data_ptr() - a.flat.data_ptr() >= 1 << 20
        assert a.flat.data_ptr() + a.flat.numel() * isz - (v.data_ptr() + v.numel() * isz) >= 1 << 20
        guards = torch.cat([a.bits[:a.g], a.bits[a.g + a.n:]])
        assert (guards == bits).all() and a.dirty() == 0
        if dtype != torch.int64:
            assert torch.isnan(a.flat[:a.g]).all() and torch.isnan(a.flat[a.g + a.n:]).all()
            assert torch.isnan(B.arena(shape, dtype, "cpu")[1]).all()  # an output starts as the pattern
        else:
            assert not B.arena(shape, dtype, "cpu", zero=True)[1].any()
        v.flatten()[-1] = 0  # stores inside the view are not the guards' business
        assert a.dirty() == 0
        a.flat[a.g + a.n] = 0  # one word past the tensor
        a.flat[a.g - 1] = 0    # one word before it
        assert a.dirty() == 2


def test_assert_within_reports_and_flags_non_finite():
    ref = np.zeros((2, 3, 4))
    got = ref.copy()
    assert B.assert_within(got, ref, 0.0, "exact zero") == 0.0
    got[1, 2, 3] = 3e-3
    got[0, 1, 2] = 2e-3
    assert B.assert_within(got, ref, 4e-3, "inside") == pytest.approx(0.75)
    with pytest.raises(AssertionError, match=r"2 of 24 .* worst \|err\|/tol 3 at \(1, 2, 3\).* first at \(0, 1, 2\)"):
        B.assert_within(got, ref, 1e-3, "x")
    got[:] = 0
    got[1, 0, 0] = np.nan
    with pytest.raises(AssertionError, match=r"1 of 24 .* at \(1, 0, 0\)"):
        B.assert_within(got, ref, 1.0, "nan")
    got[1, 0, 0] = np.inf
    with pytest.raises(AssertionError, match="outside the bound"):
        B.assert_within(got, ref, np.inf, "inf under an infinite bound")
    with pytest.raises(AssertionError, match="outside the bound"):
        B.assert_within(np.full(3, 1e-30), np.zeros(3), 0.0, "zero bound")
    # tol(): an fp32 value within d of ref, rounded to bf16
    g = np.random.default_rng(0)
    v = g.standard_normal(100000).astype(np.float32) * np.float32(10.0) ** g.integers(-3, 3, 100000).astype(np.float32)
    d = np.abs(v) * 1e-3
    r = v.astype(np.float64) + d * g.uniform(-1, 1, v.shape)
    assert B.assert_within(O.bf16(v), r, B.tol(r, d), "tol") <= 1.0
