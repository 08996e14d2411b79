"""BatchNorm away from its initial state: gamma != 1 (with a negative and a zero channel), beta != 0, running
statistics that start off (0, 1) and num_batches_tracked > 0.

Every other GPU test that compares the executor's default BN path with the oracle builds a freshly
initialised ResNet18 (gamma = 1, beta = 0, running statistics (0, 1)). There, a dual-BN forward that reads
the first BN's gamma / beta for the projection branch is invisible to every oracle comparison, and a dx
without gamma or a biased running variance shows only indirectly (a fused-vs-separate difference after a
few SGD steps, an fp32 end-to-end norm). Two layers of checks here:

* the whole network, teacher-forced (tests/test_gpu_resnet.py::_teacher_forced with bn_state_seed), in both
  precisions, at a ragged size, with each BN-path option switched off, as SyncBatchNorm, and in eval mode;
* the fused kernels themselves through their C ABI entries (dtc_bn_fin_apply, dtc_bn_bwd_mask) against the
  float64 oracle at shapes from one row to several pixel blocks, on both sides of the one-launch limits.

Inputs of the op-level tests are bf16-representable, so kernel and oracle see identical operands.
"""
import contextlib

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import bounds as B
from tests.conftest import rel_err
from tests.test_gpu_resnet import _teacher_forced

pytestmark = pytest.mark.gpu

# The BN state draw (tests/test_gpu_resnet.py::_bn_state_draw). Chosen on the CPU with the oracle alone
# (oracle.resnet.forward_backward on the drawn state, every case below): no relu1 / out activation is all
# zero and no compared tensor has a zero norm; the tests assert both again on the executor's tensors.
BN_STATE_SEED = 7


@contextlib.contextmanager
def _precision(dtc, precision):
    """bf16: under autocast, as tests/test_gpu_resnet.py runs; fp32: outside it, as tests/test_gpu_fp32.py."""
    prev = dtc.nn.is_autocast_enabled()
    dtc.nn.set_autocast_enabled(precision == "bf16")
    try:
        yield
    finally:
        dtc.nn.set_autocast_enabled(prev)


# --------------------------------------------------------------------------- whole network, teacher-forced
@pytest.mark.parametrize("precision,batch", [("bf16", 2), ("bf16", 8), ("fp32", 2), ("fp32", 8)])
def test_teacher_forced_with_bn_state(dtc, cuda, precision, batch):
    """Default options. At batch 8 layer1 (M = 8192) takes the two-pass mask-bit backward and layers 2-4 the
    one-launch form, layer2.0 its dual form at its limit M = 2048."""
    with _precision(dtc, precision):
        errs = _teacher_forced(dtc, cuda, batch, precision=precision, bn_state_seed=BN_STATE_SEED)
    assert len(errs) > 130  # the 129 usual checks + the 12 bias gradients of bn1 / shortcut.1 / the stem


def test_teacher_forced_with_bn_state_ragged_b5_8x8(dtc, cuda):
    """Batch 5 at 8x8: ragged pixel counts everywhere, down to M = 5 at layer4 (unbiased factor 5/4)."""
    with _precision(dtc, "bf16"):
        errs = _teacher_forced(dtc, cuda, 5, hw=8, seed=3, bn_state_seed=BN_STATE_SEED)
    assert len(errs) > 130


@pytest.mark.parametrize("option", ["bn_fused_fin", "bn_mask", "bn_cg", "stem_bn_fuse", "sc_fuse"])
def test_teacher_forced_with_bn_state_option_off(dtc, cuda, option):
    """Each alternative BN path (separate finalize, bf16-output mask, two-pass backward on the small layers,
    unfused stem BN backward, unfused projection shortcut) on the same drawn state."""
    lib = dtc._native.lib
    prev = lib.dtc_get_option(option.encode())
    assert prev == 1
    try:
        lib.dtc_set_option(option.encode(), 0)
        with _precision(dtc, "bf16"):
            errs = _teacher_forced(dtc, cuda, 8, bn_state_seed=BN_STATE_SEED)
    finally:
        lib.dtc_set_option(option.encode(), prev)
    assert len(errs) > 130


def test_teacher_forced_with_bn_state_sync_bn_one_rank(dtc, cuda):
    """SyncBatchNorm over a one-rank loopback communicator (factor 1: the all-reduce is the identity): every
    BN's slots are compacted (bn_fold_slots) and go through the in-stream collective before the apply kernels
    fold them -- 20 forward + 20 backward collectives, logged."""
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 1.0, world=1)
    try:
        with _precision(dtc, "bf16"):
            errs = _teacher_forced(dtc, cuda, 8, bn_state_seed=BN_STATE_SEED, sync_comm=comm)
        assert len(comm.log()) == 40
    finally:
        comm.close()
    assert len(errs) > 130


def test_eval_after_training_forward_with_bn_state(dtc, cuda):
    """model.eval() on the model that just trained one step from the drawn state: the eval coefficients
    (bn_eval_coef_all) come from the running statistics that forward wrote."""
    with _precision(dtc, "bf16"):
        _teacher_forced(dtc, cuda, 8, bn_state_seed=BN_STATE_SEED, eval_after=True)


# --------------------------------------------------------------------------- op level
def _rand_bf16(shape, gen, scale=1.0, shift=0.0):
    return O.bf16(gen.standard_normal(shape).astype(np.float32) * scale + shift)


def _bf(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).to(torch.bfloat16)


def _f(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _affine(C, gen):
    """gamma in [0.5, 1.5] with one negative and one zero channel (in different 64-channel groups when there
    are several), beta in [-0.5, 0.5]."""
    gamma = gen.uniform(0.5, 1.5, C).astype(np.float32)
    neg, zero = 5, C - 3
    gamma[neg] = -gamma[neg]
    gamma[zero] = 0.0
    return gamma, gen.uniform(-0.5, 0.5, C).astype(np.float32)


def _unpack_bits(mask, M, C):
    return np.unpackbits(mask.cpu().numpy(), bitorder="little").reshape(M, C).astype(bool)


class _FwdBN:
    """One BatchNorm's operands on the device and its float64 reference."""

    def __init__(self, dtc, dev, x, gen, nbt0):
        M, C = x.shape
        self.gamma, self.beta = _affine(C, gen)
        self.rm0 = (gen.standard_normal(C) * 0.1).astype(np.float32)
        self.rv0 = gen.uniform(0.5, 2.0, C).astype(np.float32)
        self.nbt0 = nbt0
        xs = x.astype(np.float64)
        self.stats = dtc.ops.stat_from_totals(xs.sum(0), (xs * xs).sum(0), dev)
        self.rm, self.rv = _f(self.rm0, dev), _f(self.rv0, dev)
        self.nbt = torch.full((1,), nbt0, dtype=torch.int64, device=dev)
        self.y, self.mean_ref, self.invstd_ref, self.rm_ref, self.rv_ref = O.bn_train_fwd(
            x, self.gamma, self.beta, self.rm0.astype(np.float64), self.rv0.astype(np.float64))
        self.g_d, self.b_d = _f(self.gamma, dev), _f(self.beta, dev)

    def as_second(self):
        return dict(stats=self.stats, gamma=self.g_d, beta=self.b_d, running_mean=self.rm, running_var=self.rv,
                    nbt=self.nbt)

    def check_side_outputs(self, mean, invstd, what):
        """test_bn_forward's tolerances, every channel (so every 64-channel group's first pixel block wrote)."""
        np.testing.assert_allclose(mean.cpu().numpy(), self.mean_ref, rtol=1e-5, atol=1e-6, err_msg=what)
        np.testing.assert_allclose(invstd.cpu().numpy(), self.invstd_ref, rtol=1e-5, err_msg=what)
        np.testing.assert_allclose(self.rm.cpu().numpy(), self.rm_ref, rtol=1e-5, atol=1e-7, err_msg=what)
        np.testing.assert_allclose(self.rv.cpu().numpy(), self.rv_ref, rtol=1e-5, err_msg=what)
        assert int(self.nbt.item()) == self.nbt0 + 1, what


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 31, 129, 300, 4100])
@pytest.mark.parametrize("C", [64, 128, 512])
def test_bn_fin_apply(dtc, cuda, C, M, mode):
    """dtc_bn_fin_apply (bn_fin_apply_kernel, modes relu / add + relu / dual + relu) against the oracle: M = 1
    (a single row, variance 0), 31 (less than one 32-row stripe), 129 (a ragged last block: blocks are 128
    rows), 300 and 4100 (several pixel blocks). In mode 3 the two BNs differ in every operand."""
    g = np.random.default_rng(1000 * mode + M + C)
    x = _rand_bf16((M, C), g, 2.0, 0.5)
    x2 = _rand_bf16((M, C), g, 0.7, -0.3)
    b1 = _FwdBN(dtc, cuda, x, g, nbt0=7)
    b2 = _FwdBN(dtc, cuda, x2, g, nbt0=3) if mode == 3 else None
    y, mask, (mean, invstd), second = dtc.ops.bn_fin_apply(
        mode, _bf(x, cuda), b1.stats, M, b1.g_d, b1.b_d, b1.rm, b1.rv, b1.nbt,
        x2=None if mode == 1 else _bf(x2, cuda), bn2=b2.as_second() if b2 else None)
    torch.cuda.synchronize()
    if mode == 1:
        ref = O.relu(b1.y)
    elif mode == 2:
        ref = O.relu(O.bf16(b1.y) + x2)
    else:
        ref = O.relu(O.bf16(b1.y).astype(np.float64) + O.bf16(b2.y))
    assert np.linalg.norm(ref) > 0
    yh = y.float().cpu().numpy()
    e = rel_err(yh, ref)
    print(f"bn_fin_apply mode {mode} M={M} C={C}: y rel err {e:.2e}")
    assert e < 1e-2
    # element-wise (tests/bounds.py), against the unrounded z = x*a + b of each branch
    z1, dz1 = B.bn_z(x, b1.gamma, b1.beta, b1.mean_ref, b1.invstd_ref)
    if mode == 1:
        ref_b, tol_b = B.bn_apply_ref_tol(z1, dz1)
    elif mode == 2:
        ref_b, tol_b = B.bn_apply_ref_tol(z1, dz1, res=x2)
    else:
        z2, dz2 = B.bn_z(x2, b2.gamma, b2.beta, b2.mean_ref, b2.invstd_ref)
        ref_b, tol_b = B.bn_apply_ref_tol(z1, dz1, z2=z2, dz2=dz2)
    ratio = B.assert_within(yh, ref_b, tol_b, f"bn_fin_apply mode {mode} M={M} C={C}")
    print(f"bn_fin_apply mode {mode} M={M} C={C}: worst |err|/tol {ratio:.3f}")
    # the zero-gamma channel is relu(beta [+ the other branch]) whatever x holds; per channel, so that a wrong
    # shift in one channel cannot hide in the norm
    zc = C - 3
    if np.linalg.norm(ref[:, zc]) > 0:
        assert rel_err(yh[:, zc], ref[:, zc]) < 1e-2
    else:
        assert not yh[:, zc].any()
    assert torch.equal(mask, dtc.ops.bn_mask_bits(y).reshape(-1))
    frac = _unpack_bits(mask, M, C).mean()
    assert 0.0 < frac < 1.0 or M == 1  # both bit values occur
    b1.check_side_outputs(mean, invstd, "first BN")
    if mode == 3:
        b2.check_side_outputs(*second, "second BN")
    assert float(b1.stats.abs().sum()) > 0  # the fused kernel reads the slots and leaves them (bn.hip)


# (dual, M, one_launch forms that must run, one_launch must be refused)
_BWD_CASES = [(False, 1, (0, 1), False), (False, 31, (0, 1), False), (False, 129, (0, 1), False),
              (False, 300, (0, 1), False), (False, 4096, (0, 1), False), (False, 4097, (0,), True),
              (True, 129, (0, 1), False), (True, 2048, (0, 1), False), (True, 2049, (0,), True)]


@pytest.mark.parametrize("dual,M,forms,refused", _BWD_CASES)
@pytest.mark.parametrize("C", [64, 128, 512])
def test_bn_bwd_mask(dtc, cuda, C, dual, M, forms, refused):
    """dtc_bn_bwd_mask against the oracle, as two launches (bn_bwd_reduce_mask + bn_bwd_fin_apply_mask) and as
    one (bn_bwd_cg) up to its limits M = 4096 / 2048 (dual), past which the one-launch form is refused with
    the argument error. gscale = 0.5. dz = dy * bit exactly; dgamma / dbeta at test_bn_backward's rtol = atol
    = 1e-4; dx at 1e-2; a dz output aliasing dy changes nothing. Accumulator contract (bn.hip, the fused
    kernels: "the slots are zeroed by a memset node at the start of the executor's forward" -- the apply folds
    them and does not re-zero): after the two-pass call the caller's accumulator holds the sums, from which
    dbeta was formed; the one-launch form leaves it untouched."""
    g = np.random.default_rng(17 * M + C + dual)
    dev = cuda
    x1, x2 = _rand_bf16((M, C), g, 1.5, 0.2), _rand_bf16((M, C), g, 0.7, -0.1)
    dy = _rand_bf16((M, C), g)
    bits = g.random((M, C)) < 0.6
    gamma1, _ = _affine(C, g)
    gamma2, _ = _affine(C, g)
    f32 = lambda a: np.asarray(a, np.float32)
    # the statistics as the forward saves them (fp32); the oracle uses the same rounded values
    _, m1, i1, _, _ = O.bn_train_fwd(x1, gamma1, np.zeros(C))
    _, m2, i2, _, _ = O.bn_train_fwd(x2, gamma2, np.zeros(C))
    m1, i1, m2, i2 = f32(m1), f32(i1), f32(m2), f32(i2)
    dz_ref = np.where(bits, dy, 0).astype(np.float32)
    dx1_ref, dg1_ref, db1_ref = O.bn_train_bwd(dz_ref, x1, gamma1.astype(np.float64), m1.astype(np.float64),
                                               i1.astype(np.float64))
    dx2_ref, dg2_ref, db2_ref = O.bn_train_bwd(dz_ref, x2, gamma2.astype(np.float64), m2.astype(np.float64),
                                               i2.astype(np.float64))
    tol1 = B.bn_bwd_tol(dx1_ref, dz_ref, x1, gamma1, m1, i1)  # element-wise bounds (tests/bounds.py)
    tol2 = B.bn_bwd_tol(dx2_ref, dz_ref, x2, gamma2, m2, i2)
    mask = torch.from_numpy(np.packbits(bits, axis=-1, bitorder="little").reshape(-1)).to(dev)
    dy_d, x1_d, x2_d = _bf(dy, dev), _bf(x1, dev), _bf(x2, dev)
    second = dict(x2=x2_d, gamma2=_f(gamma2, dev), mean2=_f(m2, dev), invstd2=_f(i2, dev)) if dual else {}
    words = int(dtc._native.lib.dtc_bn_stat_words(C))

    def run(one_launch, dy_in, dz_out):
        acc = torch.zeros((2 if dual else 1) * words, dtype=torch.int64, device=dev)
        r = dtc.ops.bn_bwd_mask(dy_in, mask, x1_d, _f(gamma1, dev), _f(m1, dev), _f(i1, dev), count=M, gscale=0.5,
                                one_launch=one_launch, dz_out=dz_out, acc=acc, **second)
        torch.cuda.synchronize()
        return {k: v.float().cpu().numpy() if v.dtype != torch.int64 else v for k, v in r.items()}

    for one_launch in forms:
        dz = torch.empty_like(dy_d)
        r = run(one_launch, dy_d, dz)
        np.testing.assert_array_equal(dz.float().cpu().numpy(), dz_ref)
        np.testing.assert_allclose(r["dgamma1"], 0.5 * dg1_ref, rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(r["dbeta1"], 0.5 * db1_ref, rtol=1e-4, atol=1e-4)
        if M > 1:
            assert np.linalg.norm(dx1_ref) > 0
        else:
            # one pixel: dz is its own mean and xhat = 0, so dx = 0 exactly. The kernels form A * dz + C with
            # A = fp32(gamma * invstd) and C = fp32(-A * dz) rounded on their own: at most three fp32 roundings
            # of |A * dz| (and the bf16 rounding of the result) remain
            for dx, gm, iv in ((r["dx1"], gamma1, i1),) + (((r["dx2"], gamma2, i2),) if dual else ()):
                assert np.max(np.abs(dx)) <= 4 * 2.0 ** -24 * np.max(np.abs(gm * iv * dy))
        e1 = rel_err(r["dx1"], dx1_ref)
        e2 = 0.0
        assert not r["dx1"][:, C - 3].any()  # gamma = 0: no gradient reaches x in that channel
        if dual:
            np.testing.assert_allclose(r["dgamma2"], 0.5 * dg2_ref, rtol=1e-4, atol=1e-4)
            np.testing.assert_allclose(r["dbeta2"], 0.5 * db2_ref, rtol=1e-4, atol=1e-4)
            e2 = rel_err(r["dx2"], dx2_ref)
        print(f"bn_bwd_mask C={C} M={M} dual={dual} one_launch={one_launch}: dx1 rel err {e1:.2e}, dx2 {e2:.2e}")
        assert e1 < 1e-2 and e2 < 1e-2
        ratio = B.assert_within(r["dx1"], dx1_ref, tol1, f"bn_bwd_mask C={C} M={M} one_launch={one_launch} dx1")
        if dual:
            ratio = max(ratio, B.assert_within(r["dx2"], dx2_ref, tol2,
                                               f"bn_bwd_mask C={C} M={M} one_launch={one_launch} dx2"))
        print(f"bn_bwd_mask C={C} M={M} dual={dual} one_launch={one_launch}: worst |err|/tol {ratio:.3f}")
        if one_launch:
            assert float(r["acc"].abs().sum()) == 0.0
        else:
            for j, db in enumerate(("dbeta1", "dbeta2") if dual else ("dbeta1",)):
                tot = dtc.ops.stat_totals(r["acc"][j * words:(j + 1) * words], C).numpy()
                np.testing.assert_array_equal((tot[0] * 0.5).astype(np.float32), r[db])
                np.testing.assert_allclose(tot[0], db1_ref, rtol=1e-4, atol=1e-4)
        # dz written over dy
        dy_alias = dy_d.clone()
        ra = run(one_launch, dy_alias, dy_alias)
        np.testing.assert_array_equal(dy_alias.float().cpu().numpy(), dz_ref)
        for k in r:
            if k != "acc":
                np.testing.assert_array_equal(ra[k], r[k], err_msg=k)
    if refused:
        with pytest.raises(dtc._native.NativeError, match="one-launch limit"):
            dtc.ops.bn_bwd_mask(dy_d, mask, x1_d, _f(gamma1, dev), _f(m1, dev), _f(i1, dev), count=M, gscale=0.5,
                                one_launch=True, **second)
        assert dtc._native.lib.dtc_bn_bwd_mask(*([None] * 17), M, 0.5, 1, None, 0, M, C, None) == -1  # null operands
