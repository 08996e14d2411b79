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


# ----------------------------------------------------------------------------- head and SGD bounds
# (N, HW, C, ncls): the prefetch path's limits, groups > HW, tpr not dividing 256, two 64-chunk rounds, largest /
# smallest C -- the shapes tests/test_gpu_head.py runs on the device
HEAD_SHAPES = [(3, 49, 512, 128), (2, 1, 512, 10), (3, 15, 96, 129), (2, 16, 1024, 1000), (2, 4, 2048, 33),
               (5, 64, 32, 7)]


def _head_data(shape, seed):
    """Seeded head operands. The bias is of the logits' own size (scale 2): an unrounded bias differs from the
    rounded one by at most 2^-9 |b|, which can only show beside the output's own half-ulp when |b| ~ |logit|."""
    Nn, HW, Cn, ncls = shape
    g = np.random.default_rng(seed)
    act = O.relu(_rand_bf16((Nn, HW, 1, Cn), g))
    w = _rand_bf16((ncls, Cn), g, 0.05)
    b = (g.standard_normal(ncls) * 2).astype(np.float32)
    dl = (g.standard_normal((Nn, ncls)) * 0.25).astype(np.float32)
    return act, w, b, dl


def _pool_emu(act, skip=None):
    """fp32 pool, pixels summed last to first (the kernels: strided groups, first to last); skip = (n, p) drops
    that pixel from image n's sum."""
    Nn, HW = act.shape[0], act.shape[1] * act.shape[2]
    a = act.reshape(Nn, HW, -1).astype(np.float32)
    s = np.zeros((Nn, a.shape[2]), np.float32)
    for p in range(HW - 1, -1, -1):
        v = a[:, p].copy()
        if skip is not None and skip[1] == p:
            v[skip[0]] = 0
        s = s + v
    return O.bf16(s / np.float32(HW))


def _linear_emu(feat, w, b, round_bias=True):
    """fp32 Linear in 16-channel chunks, last chunk first, + the bias, rounded to bf16."""
    f, wt = feat.astype(np.float32), np.ascontiguousarray(w.astype(np.float32).T)
    acc = np.zeros((f.shape[0], wt.shape[1]), np.float32)
    for k0 in range(f.shape[1] - 16, -1, -16):
        acc = acc + f[:, k0:k0 + 16] @ wt[k0:k0 + 16]
    return O.bf16(acc + (O.bf16(b) if round_bias else b.astype(np.float32)))


def _dact_emu(dl, w, HW, skip=None):
    """fp32 dact row per image (the same at every pixel): classes summed last to first; skip = (n, j)."""
    acc = np.zeros((dl.shape[0], w.shape[1]), np.float32)
    for j in range(w.shape[0] - 1, -1, -1):
        d = dl[:, j].astype(np.float32).copy()
        if skip is not None and skip[1] == j:
            d[skip[0]] = 0
        acc = acc + d[:, None] * w[j].astype(np.float32)[None, :]
    return O.bf16(acc * (np.float32(1) / np.float32(HW)))


def _dw_emu(dl, feat, scale, skip=None):
    """fp32 dW / db, images summed last to first; skip = (n, j) drops image n from row j and from db[j]."""
    dw = np.zeros((dl.shape[1], feat.shape[1]), np.float32)
    db = np.zeros(dl.shape[1], np.float32)
    for n in range(dl.shape[0] - 1, -1, -1):
        d = dl[n].astype(np.float32).copy()
        if skip is not None and skip[0] == n:
            d[skip[1]] = 0
        dw = dw + d[:, None] * feat[n].astype(np.float32)[None, :]
        db = db + d
    return dw * np.float32(scale), db * np.float32(scale)


def _outside(got, ref, tol, name):
    with pytest.raises(AssertionError, match="outside the bound") as ei:
        B.assert_within(got, ref, tol, name)
    print(f"{name}: {str(ei.value).split(':', 1)[1][:110]}")


def test_head_bounds_hold_for_fp32_emulation_and_reject_planted_defects():
    worst = {"feat": 0.0, "logits": 0.0, "dact": 0.0, "dW": 0.0, "db": 0.0}
    scale = 0.25
    for i, shape in enumerate(HEAD_SHAPES):
        Nn, HW, Cn, ncls = shape
        act, w, b, dl = _head_data(shape, 100 + i)
        f_ref = act.astype(np.float64).reshape(Nn, HW, Cn).mean(axis=1)
        f_tol = B.head_feat_tol(f_ref, act)
        feat = _pool_emu(act)
        l_ref, l_tol = B.head_logits_ref_tol(feat, w, b)
        logits = _linear_emu(feat, w, b)
        dw_ref, db_ref, dact_ref = O.head_bwd(dl, feat.astype(np.float64), w, (HW, 1))
        dw_ref, db_ref = scale * dw_ref, scale * db_ref
        dact_tol = B.head_dact_tol(dact_ref, dl, w, (HW, 1))
        dw_tol, db_tol = B.head_dw_tol(dl, feat, scale), B.head_db_tol(dl, scale)
        dact = np.broadcast_to(_dact_emu(dl, w, HW)[:, None, None, :], dact_ref.shape)
        dw, db = _dw_emu(dl, feat, scale)
        r = {"feat": B.assert_within(feat, f_ref, f_tol, f"feat {shape}"),
             "logits": B.assert_within(logits, l_ref, l_tol, f"logits {shape}"),
             "dact": B.assert_within(dact, dact_ref, dact_tol, f"dact {shape}"),
             "dW": B.assert_within(dw, dw_ref, dw_tol, f"dW {shape}"),
             "db": B.assert_within(db, db_ref, db_tol, f"db {shape}")}
        print(f"head {shape}: clean emulation |err|/tol " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
        worst = {k: max(v, r[k]) for k, v in worst.items()}
        # fp32 executor: the same sums without the bf16 rounding are inside the d-only bounds
        a32 = act.reshape(Nn, HW, Cn).astype(np.float32)
        f32 = a32[:, ::-1].sum(axis=1, dtype=np.float32) / np.float32(HW)
        assert B.assert_within(f32, f_ref, B.head_feat_tol(f_ref, act, bf=False), "feat fp32") <= 1.0
        l32_ref, l32_tol = B.head_logits_ref_tol(f32, w, b, bf=False)
        l32 = (f32 @ w.astype(np.float32).T + b).astype(np.float32)
        assert B.assert_within(l32, l32_ref, l32_tol, "logits fp32") <= 1.0
        # planted defects
        n = Nn - 1
        if HW > 1:
            _outside(_pool_emu(act, skip=(n, HW // 2)), f_ref, f_tol, f"feat {shape} / one pixel dropped")
        m = np.array(dact)
        m[n] = _dact_emu(dl, w, HW, skip=(n, ncls // 2))[n][None, None, :]
        _outside(m, dact_ref, dact_tol, f"dact {shape} / one class dropped from one image")
        dw_m, db_m = _dw_emu(dl, feat, scale, skip=(n, ncls - 1))
        assert np.array_equal(dw_m[:-1], dw[:-1]) and np.array_equal(db_m[:-1], db[:-1])
        _outside(dw_m, dw_ref, dw_tol, f"dW {shape} / one image dropped from one row")
        _outside(db_m, db_ref, db_tol, f"db {shape} / one image dropped")
        if Nn * ncls >= 256:  # (an element must sit at a half-ulp edge: enough elements)
            _outside(_linear_emu(feat, w, b, round_bias=False), l_ref, l_tol, f"logits {shape} / bias unrounded")
    print("head bounds, worst clean |err|/tol: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _wgrad_emu(x, dy, R, stride, pad, scale, order, drop=None):
    """fp32 weight gradient, the output pixels summed one at a time in `order` (a permutation of the N*P*Q
    pixels), then the multiply by scale; drop = (pixel, r, s): that pixel contributes nothing to tap (r, s)."""
    cols = O._im2col(x, R, R, stride, pad).astype(np.float32)
    Kn, Cn = dy.shape[3], x.shape[3]
    cols = cols.reshape(-1, R, R, Cn)
    d = dy.reshape(-1, Kn).astype(np.float32)
    dw = np.zeros((Kn, R, R, Cn), np.float32)
    for m in order:
        t = cols[m].copy()
        if drop is not None and drop[0] == m:
            t[drop[1], drop[2]] = 0
        dw = dw + d[m][:, None, None, None] * t[None]  # exact fp32 products (bf16 operands), one rounded add each
    return dw * np.float32(scale)


@pytest.mark.parametrize("R", [3, 1])
def test_wgrad_bound_holds_for_shuffled_fp32_sum_and_rejects_a_dropped_tap(R):
    """wgrad_tol at (3,7,7,64,64) stride 2 (an odd map: M = 3*4*4 = 48 output pixels, the last row's and column's
    r = 2 / s = 2 taps are padding): the float64 reference re-summed in fp32 in a shuffled pixel order stays inside
    the bound; one pixel's contribution dropped from one tap lands outside it."""
    Nn, Hh, Ww, Cn, Kn = 3, 7, 7, 64, 64
    pad, scale = (1 if R == 3 else 0), 0.5
    g = np.random.default_rng(17)
    x, dy = _rand_bf16((Nn, Hh, Ww, Cn), g), _rand_bf16((Nn, 4, 4, Kn), g)
    ref = scale * O.conv2d_wgrad(x, dy, R, R, 2, pad)
    tl = B.wgrad_tol(x, dy, R, R, 2, pad, scale)
    assert tl.shape == ref.shape == (Kn, R, R, Cn) and (tl > 0).all()
    order = g.permutation(Nn * 16)
    clean = _wgrad_emu(x, dy, R, 2, pad, scale, order)
    assert clean.dtype == np.float32
    r = B.assert_within(clean, ref, tl, f"wgrad {R}x{R}")
    print(f"wgrad {R}x{R} (3,7,7,64,64) stride 2: shuffled fp32 sum worst |err|/tol {r:.3f}, rel_err {rel_err(clean, ref):.2e}")
    assert r < 1.0 and rel_err(clean, ref) < 1e-5
    # an interior pixel of the middle image, its centre tap (in range for both filter sizes)
    tap = (R // 2, R // 2)
    m = _wgrad_emu(x, dy, R, 2, pad, scale, order, drop=(16 + 1 * 4 + 2,) + tap)
    other = np.ones((R, R), bool)
    other[tap] = False
    assert np.array_equal(m[:, other], clean[:, other]) and not np.array_equal(m, clean)
    _outside(m, ref, tl, f"wgrad {R}x{R} / one pixel dropped from one tap")
    # the bound scales with |scale| and is symmetric in its sign
    np.testing.assert_array_equal(B.wgrad_tol(x, dy, R, R, 2, pad, -2.0), 4 * tl)


def _sgd_emu(p, g, m, lr, wd, mu, is_, once=False):
    """Unfused fp32 step (every product and sum rounded; the kernel may contract to FMAs), the decay term first.
    once: the look-ahead adds m' instead of mu * m' (momentum applied once)."""
    f = np.float32
    d = f(wd) * p + g * f(is_)
    m2 = d + f(mu) * m
    d2 = (m2 if once else f(mu) * m2) + d
    return p - f(lr) * d2, m2


def test_sgd_bound_holds_for_fp32_emulation_and_rejects_planted_defects():
    n = 4096
    g_ = np.random.default_rng(9)
    worst = [0.0, 0.0]
    for lr, wd, mu, is_ in ((0.1, 5e-4, 0.9, 1.0), (3.2, 5e-4, 0.9, 1.0 / 65536), (0.1, 0.0, 0.0, 1.0)):
        p = g_.standard_normal(n).astype(np.float32)
        m = np.zeros(n, np.float32)
        for step in range(3):
            g = (g_.standard_normal(n) / is_).astype(np.float32)
            (p_ref, m_ref), (tp, tm) = B.sgd_ref(p, g, m, lr, wd, mu, is_), B.sgd_tol(p, g, m, lr, wd, mu, is_)
            p2, m2 = _sgd_emu(p, g, m, lr, wd, mu, is_)
            assert p2.dtype == np.float32 and m2.dtype == np.float32
            worst[0] = max(worst[0], B.assert_within(p2, p_ref, tp, "sgd p"))
            worst[1] = max(worst[1], B.assert_within(m2, m_ref, tm, "sgd m"))
            if mu > 0:
                _outside(_sgd_emu(p, g, m, lr, wd, mu, is_, once=True)[0], p_ref, tp, "sgd p / momentum applied once")
            p, m = p2, m2
    print(f"sgd n={n}: clean emulation worst |err|/tol p {worst[0]:.3f}, m {worst[1]:.3f}")
    assert worst[0] < 1.0 and worst[1] < 1.0


def test_bf16_shadow_truncation_differs_from_rounding_on_ties_and_random_data():
    """The shadow's criterion is bit equality with O.bf16_bits: a truncating conversion differs on the exact ties
    with an odd upper half, one ulp above any tie, and on about half of random data."""
    u = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x00000000, 0x80000000,
                  0x00800000, 0x7F7FFFFF], np.uint32)
    want = np.array([0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x0000, 0x8000, 0x0080, 0x7F80], np.uint16)
    np.testing.assert_array_equal(O.bf16_bits(u.view(np.float32)), want)
    trunc = (u >> 16).astype(np.uint16)
    assert (trunc != want).sum() == 4  # the odd ties, the value above the tie, the largest finite
    r = np.random.default_rng(5).standard_normal(4096).astype(np.float32)
    assert 0.4 < np.mean((r.view(np.uint32) >> 16).astype(np.uint16) != O.bf16_bits(r)) < 0.6
