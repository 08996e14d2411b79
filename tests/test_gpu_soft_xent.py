"""Soft-target cross-entropy kernels (label smoothing, Mixup, CutMix as one target distribution
q = (1 - eps) * (lam * onehot(ya) + (1 - lam) * onehot(yb)) + eps / ncls): dtc_xent_soft_fwd_ex / dtc_xent_soft_bwd
against torch's float64 ``F.cross_entropy`` on the two-hot mixture, their bit-identity reductions to the
index-label kernels, edge cases and determinism."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# both kernel branches (ncls <= 128 in registers, above it re-read), row counts off the 64 / 256 / 1024 multiples,
# the row cap
SHAPES = [(1, 100), (7, 10), (65, 129), (300, 100), (33, 1000), (4096, 100)]
GSCALE = 4.0


def _case(n, ncls, seed=0):
    g = np.random.default_rng(seed + 1000 * n + ncls)
    z = (g.standard_normal((n, ncls)) * 3).astype(np.float32)
    ya = g.integers(0, ncls, n)
    yb = g.integers(0, ncls, n)
    lam = g.random(n).astype(np.float32)
    lam[0] = 1.0  # exact end points ...
    lam[n // 2] = 0.0 if n > 1 else 1.0
    yb[n - 1] = ya[n - 1]  # ... and a row whose two labels coincide
    return z, ya, yb, lam


_REF = {}


def _reference(n, ncls, eps, mixed):
    """loss and dloss/dz * GSCALE of F.cross_entropy(z.double(), q, label_smoothing=eps) on the CPU (computed once
    per case and shared)."""
    key = (n, ncls, eps, mixed)
    if key not in _REF:
        z, ya, yb, lam = _case(n, ncls)
        zt = torch.from_numpy(z).double().requires_grad_(True)
        q = F.one_hot(torch.from_numpy(ya), ncls).double()
        if mixed:
            lt = torch.from_numpy(lam).double()[:, None]
            q = lt * q + (1 - lt) * F.one_hot(torch.from_numpy(yb), ncls).double()
        loss = F.cross_entropy(zt, q, label_smoothing=eps)
        (loss * GSCALE).backward()
        _REF[key] = (float(loss.detach()), zt.grad.numpy().copy())
    return _REF[key]


def _dev(cuda, z, ya, yb, lam, mixed):
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)  # noqa: E731
    return D(z), D(ya), (D(yb) if mixed else None), (D(lam) if mixed else None)


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("eps", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("n,ncls", SHAPES)
def test_soft_xent_matches_float64_reference(dtc, cuda, n, ncls, eps, mixed):
    z, ya, yb, lam = _case(n, ncls)
    ref_loss, ref_dz = _reference(n, ncls, eps, mixed)
    zd, yad, ybd, lamd = _dev(cuda, z, ya, yb, lam, mixed)
    loss, lse, _ = dtc.ops.xent_soft_fwd(zd, yad, ybd, lamd, eps)
    gs = torch.tensor([GSCALE], device=cuda)
    dl = dtc.ops.xent_soft_bwd(zd, yad, ybd, lamd, eps, lse, gs)
    torch.cuda.synchronize()
    got = float(loss)
    dz = dl.cpu().numpy()
    print(f"n={n} ncls={ncls} eps={eps} mixed={mixed}: loss err {abs(got - ref_loss):.3e} "
          f"(bound {1e-5 * max(1, abs(ref_loss)):.1e}), dlogits max err {np.abs(dz - ref_dz).max():.3e}, "
          f"max |row sum| {np.abs(dz.astype(np.float64).sum(1)).max():.3e} (bound {1e-6 * GSCALE / n:.1e})")
    assert abs(got - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    np.testing.assert_allclose(dz, ref_dz, rtol=1e-4, atol=1e-6)
    assert np.abs(dz.astype(np.float64).sum(1)).max() <= 1e-6 * GSCALE / n
    np.testing.assert_allclose(lse.cpu().numpy(), torch.logsumexp(torch.from_numpy(z).double(), 1).numpy(), rtol=1e-6)


def _hard_fwd_ex(dtc, cuda, zd, yd, scale):
    """dtc_xent_fwd_ex with every output: (loss, lse, scaled, host word)."""
    n, ncls = zd.shape
    loss = torch.empty((), dtype=torch.float32, device=cuda)
    lse = torch.empty(n, dtype=torch.float32, device=cuda)
    scaled = torch.empty((), dtype=torch.float32, device=cuda)
    host = torch.zeros(1, dtype=torch.float32).pin_memory()
    dtc._native.call("dtc_xent_fwd_ex", zd.data_ptr(), yd.data_ptr(), n, ncls, loss.data_ptr(), lse.data_ptr(),
                     scale.data_ptr(), scaled.data_ptr(), host.data_ptr(), dtc._native.stream_ptr())
    torch.cuda.synchronize()
    return loss, lse, scaled, host.clone()


@pytest.mark.parametrize("n,ncls", SHAPES)
def test_soft_xent_reduces_to_the_hard_kernels_bit_for_bit(dtc, cuda, n, ncls):
    z, ya, yb, lam = _case(n, ncls)
    zd, yad, ybd, lamd = _dev(cuda, z, ya, yb, lam, True)
    scale = torch.tensor([1024.0], device=cuda)
    h_loss, h_lse, h_scaled, h_host = _hard_fwd_ex(dtc, cuda, zd, yad, scale)
    host = torch.zeros(1, dtype=torch.float32).pin_memory()
    loss, lse, scaled = dtc.ops.xent_soft_fwd(zd, yad, None, None, 0.0, scale, host)
    torch.cuda.synchronize()
    assert torch.equal(loss, h_loss) and torch.equal(lse, h_lse) and torch.equal(scaled, h_scaled)
    assert torch.equal(host, h_host) and float(host) == float(loss)
    gs = torch.tensor([GSCALE], device=cuda)
    assert torch.equal(dtc.ops.xent_soft_bwd(zd, yad, None, None, 0.0, lse, gs), dtc.ops.xent_bwd(zd, yad, h_lse, gs))
    assert torch.equal(dtc.ops.xent_soft_bwd(zd, yad, None, None, 0.0, lse), dtc.ops.xent_bwd(zd, yad, h_lse))
    # eps > 0 or lam < 1: another loss, the same lse bits
    for lb, lm, eps in ((None, None, 0.1), (ybd, lamd, 0.0), (ybd, lamd, 0.3)):
        loss2, lse2, _ = dtc.ops.xent_soft_fwd(zd, yad, lb, lm, eps)
        assert torch.equal(lse2, h_lse)
        if n > 1:
            assert not torch.equal(loss2, h_loss)
    # lam = 1 everywhere with a second label array is the hard loss too (the second term is an exact zero)
    ones = torch.ones(n, device=cuda)
    loss3, _, _ = dtc.ops.xent_soft_fwd(zd, yad, ybd, ones, 0.0)
    assert torch.equal(loss3, h_loss)
    assert torch.equal(dtc.ops.xent_soft_bwd(zd, yad, ybd, ones, 0.0, lse, gs), dtc.ops.xent_bwd(zd, yad, h_lse, gs))


@pytest.mark.parametrize("n,ncls", [(7, 10), (65, 129)])
def test_soft_xent_edge_cases(dtc, cuda, n, ncls):
    z, ya, yb, lam = _case(n, ncls)
    zd, yad, ybd, lamd = _dev(cuda, z, ya, yb, lam, True)
    for which, bad in (("a", ncls), ("a", -1), ("b", ncls), ("b", -3)):
        a2, b2 = yad.clone(), ybd.clone()
        (a2 if which == "a" else b2)[3] = bad
        loss, lse, _ = dtc.ops.xent_soft_fwd(zd, a2, b2, lamd, 0.1)
        assert torch.isnan(loss).item() and torch.isfinite(lse).all().item()
        dl = dtc.ops.xent_soft_bwd(zd, a2, b2, lamd, 0.1, lse)  # the bad label hits no class: finite everywhere
        assert torch.isfinite(dl).all().item()
    loss, _, _ = dtc.ops.xent_soft_fwd(zd, yad, None, None, 0.1)
    assert torch.isfinite(loss).item()
    for bad_lam in (1.5, -0.25, float("nan")):  # a lam outside [0, 1] makes that row's term NaN
        l2 = lamd.clone()
        l2[2] = bad_lam
        assert torch.isnan(dtc.ops.xent_soft_fwd(zd, yad, ybd, l2, 0.0)[0]).item()
    # smoothing outside [0, 1]: an error and no launch (the outputs keep their sentinel)
    loss = torch.full((), -7.0, device=cuda)
    lse = torch.full((n,), -7.0, device=cuda)
    rc = dtc._native.lib.dtc_xent_soft_fwd_ex(zd.data_ptr(), yad.data_ptr(), None, None, 1.5, n, ncls, loss.data_ptr(),
                                              lse.data_ptr(), None, None, None, dtc._native.stream_ptr())
    torch.cuda.synchronize()
    assert rc < 0 and "smoothing" in dtc._native.last_error()
    assert float(loss) == -7.0 and (lse == -7.0).all().item()
    dl = torch.full((n, ncls), -7.0, device=cuda)
    with pytest.raises(dtc.NativeError, match="smoothing"):
        dtc.ops.xent_soft_bwd(zd, yad, None, None, 1.5, lse, out=dl)
    torch.cuda.synchronize()
    assert (dl == -7.0).all().item()
    with pytest.raises(ValueError):
        dtc.ops.xent_soft_fwd(zd, yad, ybd, None, 0.1)  # labels_b without lam


@pytest.mark.parametrize("n,ncls", [(300, 100), (33, 1000)])
def test_soft_xent_two_calls_give_equal_bits(dtc, cuda, n, ncls):
    z, ya, yb, lam = _case(n, ncls)
    zd, yad, ybd, lamd = _dev(cuda, z, ya, yb, lam, True)
    a = dtc.ops.xent_soft_fwd(zd, yad, ybd, lamd, 0.1)
    b = dtc.ops.xent_soft_fwd(zd, yad, ybd, lamd, 0.1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(dtc.ops.xent_soft_bwd(zd, yad, ybd, lamd, 0.1, a[1]),
                       dtc.ops.xent_soft_bwd(zd, yad, ybd, lamd, 0.1, b[1]))


def test_soft_xent_beyond_the_row_cap(dtc, cuda):
    """n > 4096 takes the two-launch form (dtc_xent_soft_fwd): same lse bits as dtc_xent_fwd, the loss inside the
    one-launch kernel's tolerance."""
    n, ncls = 4100, 100
    z, ya, yb, lam = _case(n, ncls)
    zd, yad, ybd, lamd = _dev(cuda, z, ya, yb, lam, True)
    loss, lse, scaled = dtc.ops.xent_soft_fwd(zd, yad, ybd, lamd, 0.1)
    h_loss, h_lse = dtc.ops.xent_fwd(zd, yad)
    assert scaled is None and torch.equal(lse, h_lse)
    ref_loss, _ = _reference(n, ncls, 0.1, True)
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    assert torch.equal(dtc.ops.xent_soft_fwd(zd, yad, None, None, 0.0)[0], h_loss)
