"""The general-geometry (row-segment tile) instances of the split-bf16 fp32 convolution (csrc/conv_f32x.hip, GEN = 1;
option f32x_gen), forward and data gradient, against the fp64 oracle on the kernel's own fp32 inputs. Inputs, the
element-wise bound 2^-22 (|x| conv |w|) and the norm-wise 1e-5 are test_gpu_conv_f32_split.py's, derived there."""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests.test_gpu_conv_f32_split import KINDS, _check, _inputs
from tests.test_gpu_resnet import _teacher_forced

pytestmark = pytest.mark.gpu

SHAPES = [  # (N, H, W, C, K)
    (1, 4, 28, 64, 64),    # one tile, seg 28 in 32 slots, rs 4: padded slots at every row end
    (2, 6, 56, 128, 64),   # seg 56, rs 2: top, interior and bottom tiles, two images, two reduction chunks
    (1, 2, 112, 64, 128),  # two segments per row (q0 != 0): real pixels in the side halo columns; two channel tiles
    (1, 4, 64, 64, 64),    # seg 64: all 128 slots valid, halo 264 rows of 288
    (1, 3, 56, 64, 64),    # rs falls to 1
    (2, 7, 7, 64, 64),     # 49 of 128 slots: the statistics must ignore 79 padded ones
]


@pytest.fixture
def gen(dtc):
    try:
        dtc._native.lib.dtc_set_option(b"f32x_gen", 2)
        yield dtc._native.lib
    finally:
        dtc._native.lib.dtc_set_option(b"f32x_gen", 0)


def _routes(dtc, lib, shape, mode):
    """"split" under the option and "exact" with it at 0"""
    d = dtc.ops.conv_desc(*shape, 3, 3, 1, 1)
    lib.dtc_set_option(b"f32x_gen", 0)
    exact = dtc.ops.conv2d_f32_route(d, mode, 1)
    lib.dtc_set_option(b"f32x_gen", 2)
    assert (exact, dtc.ops.conv2d_f32_route(d, mode, 1)) == ("exact", "split")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gen_forward_and_statistics(dtc, cuda, gen, shape, kind):
    _routes(dtc, gen, shape, 0)
    x, w = _inputs(shape, kind, False)
    stats = dtc.ops.new_stats(shape[4], cuda)
    y = dtc.ops.conv2d_f32(torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda), 1, 1, algo=1, stats=stats)
    y = y.cpu().numpy()
    _check(f"gen fwd {shape} {kind}", y, O.conv2d_fwd(x, w, 1, 1), O.conv2d_fwd(np.abs(x), np.abs(w), 1, 1))
    if kind == "randn":  # the statistics of the kernel's own output, tests/test_gpu_ops.py's tolerance for them
        s = dtc.ops.stat_totals(stats, shape[4]).numpy()
        yb = y.reshape(-1, shape[4]).astype(np.float64)
        np.testing.assert_allclose(s[0], yb.sum(0), rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose(s[1], (yb * yb).sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gen_dgrad(dtc, cuda, gen, shape, kind, with_res):
    N, H, W, C, K = shape
    _routes(dtc, gen, shape, 1)
    dy, w = _inputs(shape, kind, True)
    res = np.random.default_rng(5).standard_normal((N, H, W, C)).astype(np.float32) if with_res else None
    dx = dtc.ops.conv2d_dgrad_f32(torch.from_numpy(dy).to(cuda), torch.from_numpy(w).to(cuda), (H, W), 1, 1, algo=1,
                                  res=torch.from_numpy(res).to(cuda) if with_res else None).cpu().numpy()
    ref = O.conv2d_dgrad(dy, w, (H, W), 1, 1)
    mag = O.conv2d_dgrad(np.abs(dy), np.abs(w), (H, W), 1, 1)
    if with_res:  # one more fp32 rounding, of dx + res: 2^-23 |dx + res| is granted, as in the classic test
        ref = ref + res
        mag = mag + np.abs(ref) * 0.5
    _check(f"gen dgrad {shape} {kind} res={with_res}", dx, ref, mag)


def test_gen_past_2gib(dtc, cuda, gen):
    """A 2,147,532,800-byte activation tensor (just over 2^31): the per-image descriptor and the 64-bit output offsets.
    The first and the last image against the oracle on those two images."""
    N, H, W, C = 10700, 28, 28, 64
    _routes(dtc, gen, (N, H, W, C, C), 0)
    a, w = torch.randn(N, H, W, C, device=cuda), torch.randn(C, 3, 3, C, device=cuda) * 0.05
    ends, wn = a[[0, N - 1]].cpu().numpy(), w.cpu().numpy()
    y = dtc.ops.conv2d_f32(a, w, 1, 1, algo=1)[[0, N - 1]].cpu().numpy()
    _check("gen fwd past 2 GiB", y, O.conv2d_fwd(ends, wn, 1, 1), O.conv2d_fwd(np.abs(ends), np.abs(wn), 1, 1))
    dx = dtc.ops.conv2d_dgrad_f32(a, w, (H, W), 1, 1, algo=1)[[0, N - 1]].cpu().numpy()
    _check("gen dgrad past 2 GiB", dx, O.conv2d_dgrad(ends, wn, (H, W), 1, 1),
           O.conv2d_dgrad(np.abs(ends), np.abs(wn), (H, W), 1, 1))


def test_gen_runs_are_bit_identical(dtc, cuda, gen):
    x, w = (torch.from_numpy(v).to(cuda) for v in _inputs((2, 6, 56, 64, 64), "randn", False))
    runs = [(dtc.ops.conv2d_f32(x, w, 1, 1, algo=1), dtc.ops.conv2d_dgrad_f32(x, w, (6, 56), 1, 1, algo=1))
            for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_gen_executor_56_per_layer(dtc, cuda, gen):
    """The fp32 executor at 56x56 (rows of 56 / 28 / 14 / 7) with f32_split = 1 and the general tiles: every layer
    within the fp32 tolerance (1e-5) of the oracle on that layer's inputs, as the classic executor test."""
    for hw, c, mode in ((56, 64, 0), (56, 64, 1), (28, 128, 0), (28, 128, 1)):
        assert dtc.ops.conv2d_f32_route(dtc.ops.conv_desc(2, hw, hw, c, c, 3, 3, 1, 1), mode, 1) == "split"
    try:
        gen.dtc_set_option(b"f32_split", 1)
        errs = _teacher_forced(dtc, cuda, 2, hw=56, precision="fp32")
    finally:
        gen.dtc_set_option(b"f32_split", 0)
    assert len(errs) > 90
