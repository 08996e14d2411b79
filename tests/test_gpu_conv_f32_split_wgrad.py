"""The split-bf16 fp32 weight gradient (csrc/conv_f32x_wgrad.hip; ops.conv2d_wgrad_f32 with algo=1, the executor
with option f32_split = 2) and the exact fp32 weight gradient's entry point (algo=0), against the fp64 oracle on the
kernel's own fp32 inputs.

Element-wise bound: |dw - ref| <= 2^-22 * conv2d_wgrad(|x|, |dy|), norm-wise rel_err < 1e-5: the bounds of
tests/test_gpu_conv_f32_split.py. A CPU emulation of the six-product scheme gives 5e-8 or better at reductions of 64
to 16,384 pixels, a two-plane look-alike 3.8e-6 at 64 pixels and 1.6e-6 at 256: the short reductions are the sharp
cases. Only one operand carries wide exponents: with both, the exact f32-MFMA kernel itself leaves 2^-22."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests.conftest import rel_err
from tests.test_gpu_resnet import _teacher_forced

pytestmark = pytest.mark.gpu

SHAPES = [  # (N, H, W, C, K)
    (1, 4, 4, 64, 64),     # one ragged 16-pixel step
    (2, 8, 8, 128, 64),    # two c-slices, C != K
    (1, 16, 16, 64, 128),  # two k-slices
    (3, 32, 32, 64, 64),   # 48 steps: several splits plus the reduce
    (9, 4, 4, 64, 64),     # the last step ragged across images
    (2, 4, 4, 512, 512),   # 64 tiles
]
KINDS = ["randn", "delta_interior", "delta_corner"]
BOUND = 2.0 ** -22


def _inputs(shape, kind):
    """fp32 x [N,H,W,C] and dy [N,H,W,K]. delta_*: x with wide exponents, dy one 1.0 per output channel k (image
    k % N, the centre pixel or the corner (0, W - 1)): dw[k] is a shifted copy of that image, zeros from the padding."""
    N, H, W, C, K = shape
    g = np.random.default_rng(1000 * sum(shape) + KINDS.index(kind))
    if kind == "randn":
        x = g.standard_normal((N, H, W, C))
        dy = g.standard_normal((N, H, W, K)) * 0.05
    else:
        x = g.standard_normal((N, H, W, C)) * np.exp(3 * g.standard_normal((N, H, W, C)))
        dy = np.zeros((N, H, W, K))
        y, xx = (H // 2, W // 2) if kind == "delta_interior" else (0, W - 1)
        dy[np.arange(K) % N, y, xx, np.arange(K)] = 1.0
    return x.astype(np.float32), dy.astype(np.float32)


def _check(what, got, x, dy, scale=1.0):
    ref = scale * O.conv2d_wgrad(x, dy, 3, 3, 1, 1)
    mag = scale * O.conv2d_wgrad(np.abs(x), np.abs(dy), 3, 3, 1, 1)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(mag, 1e-300)).max())
    print(f"{what}: worst |err| / (|x| wgrad |dy|) = {worst:.3e} (bound {BOUND:.3e}), rel_err {rel_err(got, ref):.3e}")
    assert (err <= BOUND * mag).all(), (what, worst)
    assert rel_err(got, ref) < 1e-5, what


def _wgrad(dtc, cuda, x, dy, r=3, stride=1, pad=1, **kw):
    return dtc.ops.conv2d_wgrad_f32(torch.from_numpy(x).to(cuda), torch.from_numpy(dy).to(cuda), r, r, stride, pad, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_split_wgrad(dtc, cuda, shape, kind):
    N, H, W, C, K = shape
    assert dtc.ops.conv2d_f32_wgrad_route(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 1, 1), 1) == "split"
    x, dy = _inputs(shape, kind)
    scale = 0.25 if shape == SHAPES[1] else 1.0  # a power of two: the bound is unchanged
    dw = _wgrad(dtc, cuda, x, dy, algo=1, scale=scale)
    assert dw.shape == (K, 3, 3, C) and dw.dtype == torch.float32
    _check(f"wgrad {shape} {kind}", dw.cpu().numpy(), x, dy, scale)


def test_workspace_tiers_and_determinism(dtc, cuda):
    """The default workspace (several splits and the reduce) and a zero-length one (one split writes dw itself) are both
    within the bound; two runs of either give equal bits."""
    shape = SHAPES[3]
    x, dy = _inputs(shape, "randn")
    none = torch.empty(0, dtype=torch.uint8, device=cuda)
    assert dtc._native.lib.dtc_conv2d_f32_wgrad_workspace_size(dtc.ops.conv_desc(*shape, 3, 3, 1, 1), 1) > 0
    for what, kw in (("default workspace", {}), ("no workspace", {"workspace": none})):
        runs = [_wgrad(dtc, cuda, x, dy, algo=1, **kw) for _ in range(2)]
        assert torch.equal(runs[0], runs[1]), what
        _check(what, runs[0].cpu().numpy(), x, dy)


def test_slab_on_hand_bounds_the_splits(dtc, cuda):
    """(8, 16, 16, 64, 64): 32 steps of four rows, one tile, so the kernel wants 8 splits. A workspace of three slabs
    runs three (11 + 11 + 10 steps) and the reduce, none runs one split that writes dw itself: both within the bound."""
    shape = (8, 16, 16, 64, 64)
    x, dy = _inputs(shape, "randn")
    one = 64 * 9 * 64 * 4
    assert dtc._native.lib.dtc_conv2d_f32_wgrad_workspace_size(dtc.ops.conv_desc(*shape, 3, 3, 1, 1), 1) == 8 * one
    for what, nbytes in (("three slabs", 3 * one), ("no workspace", 0)):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
        _check(f"wgrad {shape} {what}", _wgrad(dtc, cuda, x, dy, algo=1, workspace=ws).cpu().numpy(), x, dy)


def test_refused_shape_runs_the_exact_kernel(dtc, cuda):
    """algo=1 at a shape the split kernel refuses (7-wide rows) is conv_f32's weight gradient, bit for bit."""
    shape = (1, 5, 7, 64, 64)
    x, dy = _inputs(shape, "randn")
    assert dtc.ops.conv2d_f32_wgrad_route(dtc.ops.conv_desc(*shape, 3, 3, 1, 1), 1) == "exact"
    assert torch.equal(_wgrad(dtc, cuda, x, dy, algo=1), _wgrad(dtc, cuda, x, dy, algo=0))


@pytest.mark.parametrize("r,stride,pad", [(3, 2, 1), (1, 1, 0)])
def test_exact_entry_point(dtc, cuda, r, stride, pad):
    g = np.random.default_rng(r)
    x = g.standard_normal((2, 8, 8, 64)).astype(np.float32)
    p = (8 + 2 * pad - r) // stride + 1
    dy = (g.standard_normal((2, p, p, 128)) * 0.05).astype(np.float32)
    dw = _wgrad(dtc, cuda, x, dy, r, stride, pad, algo=0).cpu().numpy()
    assert rel_err(dw, O.conv2d_wgrad(x, dy, r, r, stride, pad)) < 1e-5
    with pytest.raises(dtc._native.NativeError):  # the exact kernel needs one slab
        _wgrad(dtc, cuda, x, dy, r, stride, pad, algo=0, workspace=torch.empty(0, dtype=torch.uint8, device=cuda))


def test_executor_with_f32_split_2_per_layer(dtc, cuda):
    """The fp32 executor with option f32_split = 2: every layer, weight gradients included, within the fp32 tolerance
    (1e-5) of the oracle on that layer's inputs."""
    lib = dtc._native.lib
    try:
        lib.dtc_set_option(b"f32_split", 2)
        errs = _teacher_forced(dtc, cuda, 2, precision="fp32")
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    assert len(errs) > 90


def test_trainer_fp32_conv_split_all_trains(dtc, cuda, tmp_path):
    """`train.py single --fp32-conv split-all`: two epochs of the same three batches; the loss is finite and falls."""
    lib = dtc._native.lib
    try:
        t = dtc.trainer.main(["--epoch", "2", "--batch-size", "32", "--max-steps", "3", "--workers", "0", "--lr", "0.02",
                              "--synthetic-train", "120", "--synthetic-test", "32", "--eval-step", "1",
                              "--fp32-conv", "split-all", "--ckpt-path", str(tmp_path)], "single")
        assert lib.dtc_get_option(b"f32_split") == 2
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    rows = [json.loads(line) for line in open(os.path.join(t.save_path, "scalars.jsonl"))]
    losses = [r["train"] for r in rows if r["tag"] == "loss/epoch"]
    print("train loss per epoch:", losses)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and losses[1] < losses[0]
