"""The general-geometry (row-segment step) split-bf16 fp32 weight gradient (csrc/conv_f32x_wgrad.hip, GEN = 1; option
f32x_gen) against the fp64 oracle on its own inputs; inputs and bounds are test_gpu_conv_f32_split_wgrad.py's.
Measured worst element-wise error over these shapes: 1.1e-7 of the magnitude (the 8 x 8 blocks), 5.3e-8 past 2 GiB."""
import pytest
import torch

from tests.test_gpu_conv_f32_split_gen import gen  # noqa: F401  (the fixture: f32x_gen = 2, restored to 0)
from tests.test_gpu_conv_f32_split_wgrad import KINDS, _check, _inputs, _wgrad
from tests.test_gpu_resnet import _teacher_forced

pytestmark = pytest.mark.gpu

SHAPES = [  # (N, H, W, C, K)
    (1, 4, 224, 64, 64),    # 32 x 2 steps, seven segments per row, two row steps: real pixels in every side halo column
    (2, 8, 112, 128, 64),   # 16 x 4: two c-slices, two images, 28 steps: several splits and the reduce
    (1, 8, 56, 64, 128),    # 8 x 8 blocks, two k-slices
    (3, 28, 28, 64, 64),    # 28 x 2: 56 of 64 slots, the padded slots must add nothing
    (2, 14, 14, 64, 64),    # 7 x 7: 49-pixel steps, four per image
    (2, 7, 7, 64, 64),      # 7 x 7: one step per image
    (1, 3, 56, 64, 64),     # rs falls short of its target (14 x 3)
]


def _routes(dtc, lib, shape):
    d, got = dtc.ops.conv_desc(*shape, 3, 3, 1, 1), []
    for v in (0, 2):
        lib.dtc_set_option(b"f32x_gen", v)
        got.append(dtc.ops.conv2d_f32_wgrad_route(d, 1))
    assert got == ["exact", "split"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gen_wgrad(dtc, cuda, gen, shape, kind):
    _routes(dtc, gen, shape)
    x, dy = _inputs(shape, kind)
    scale = 0.25 if shape == SHAPES[1] else 1.0  # a power of two: the bound is unchanged
    _check(f"gen wgrad {shape} {kind}", _wgrad(dtc, cuda, x, dy, algo=1, scale=scale).cpu().numpy(), x, dy, scale)


def test_gen_workspace_tiers_and_determinism(dtc, cuda, gen):
    """Several splits plus the reduce, and one split writing dw itself: both within the bound, each bit-identical."""
    x, dy = _inputs(SHAPES[1], "randn")
    assert gen.dtc_conv2d_f32_wgrad_workspace_size(dtc.ops.conv_desc(*SHAPES[1], 3, 3, 1, 1), 1) > 0
    for what, kw in (("default workspace", {}), ("no workspace", {"workspace": torch.empty(0, device=cuda)})):
        runs = [_wgrad(dtc, cuda, x, dy, algo=1, **kw) for _ in range(2)]
        assert torch.equal(runs[0], runs[1]), what
        _check("gen " + what, runs[0].cpu().numpy(), x, dy)


def test_gen_past_2gib(dtc, cuda, gen):
    """2,147,532,800-byte x and dy (per-image descriptors, 64-bit bases); dy is zero but in the first and last image."""
    N, H, W, C = 10700, 28, 28, 64
    _routes(dtc, gen, (N, H, W, C, C))
    x, dy = torch.randn(N, H, W, C, device=cuda), torch.zeros(N, H, W, C, device=cuda)
    dy[[0, N - 1]] = torch.randn(2, H, W, C, device=cuda) * 0.05
    dw = dtc.ops.conv2d_wgrad_f32(x, dy, 3, 3, 1, 1, algo=1).cpu().numpy()
    _check("gen wgrad past 2 GiB", dw, x[[0, N - 1]].cpu().numpy(), dy[[0, N - 1]].cpu().numpy())


def test_gen_executor_56_with_f32_split_2_per_layer(dtc, cuda, gen):
    """The fp32 executor at 56x56 (rows of 56 / 28 / 14 / 7): every layer, weight gradients included, within 1e-5."""
    try:
        gen.dtc_set_option(b"f32_split", 2)
        assert len(_teacher_forced(dtc, cuda, 2, hw=56, precision="fp32")) > 90
    finally:
        gen.dtc_set_option(b"f32_split", 0)
