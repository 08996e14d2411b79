"""The split-bf16 fused weight gradient of the transition blocks (csrc/conv_f32x_s2_wgrad.hip;
ops.conv2d_wgrad_sc_f32 with algo=1, the executor with option f32_split = 4) against the fp64 oracle on the kernel's
own fp32 inputs, with the bound of tests/test_gpu_conv_f32_split_wgrad.py for both outputs:
|err| <= 2^-22 * conv2d_wgrad(|x|, |dy|) element-wise and rel_err < 1e-5. As there, only x carries wide exponents.

Measured worst |err| / conv2d_wgrad(|x|, |dy|) over these cases (MI355X): 1.25e-7 (dw), 9.6e-8 (dwsc)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests.test_gpu_conv_f32_split import _check
from tests.test_gpu_resnet import _teacher_forced

pytestmark = pytest.mark.gpu

SHAPES = [  # (N, H, W, C, K)
    (1, 8, 8, 64, 64),      # 16 positions: one ragged step, 4-wide output rows
    (3, 8, 8, 128, 64),     # whole-image steps, the last ragged across images, two c-slices
    (2, 16, 16, 64, 128),   # 8-wide rows, several steps per image, two k-slices
    (1, 32, 32, 64, 64),    # 16-wide rows, enough steps for several splits plus the reduce
    (2, 8, 8, 256, 512),    # 32 tiles
]
KINDS = ["randn", "delta_interior", "delta_origin", "delta_last"]


def _inputs(shape, kind):
    """fp32 x [N,H,W,C], dy and dsc [N,H/2,W/2,K]. delta_*: x with wide exponents, dy and dsc one 1.0 per output channel
    k (image k % N; an interior position, (0, 0) -- taps r = 0 / s = 0 are padding: zeros -- or (Ho - 1, Wo - 1) --
    taps r = 2 / s = 2 read row H - 1 / column W - 1): dw[k] is a strided copy of that image, dwsc[k] one pixel of it."""
    N, H, W, C, K = shape
    Ho, Wo = H // 2, W // 2
    g = np.random.default_rng(1000 * sum(shape) + KINDS.index(kind))
    if kind == "randn":
        x = g.standard_normal((N, H, W, C))
        dy, dsc = (g.standard_normal((N, Ho, Wo, K)) * 0.05 for _ in range(2))
    else:
        x = g.standard_normal((N, H, W, C)) * np.exp(3 * g.standard_normal((N, H, W, C)))
        y, xx = {"delta_interior": (Ho // 2, Wo // 2 - 1), "delta_origin": (0, 0), "delta_last": (Ho - 1, Wo - 1)}[kind]
        dy = np.zeros((N, Ho, Wo, K))
        dy[np.arange(K) % N, y, xx, np.arange(K)] = 1.0
        dsc = dy.copy()
    return x.astype(np.float32), dy.astype(np.float32), dsc.astype(np.float32)


@pytest.fixture
def every_geometry(dtc):
    """The kernel's whole geometry family: by default small problems with 16-wide output rows (SHAPES[3]) take the exact
    pair, because the fused launch measured no faster there; option f32x_s2_wgrad = 2 opens the predicate."""
    dtc._native.lib.dtc_set_option(b"f32x_s2_wgrad", 2)
    yield
    dtc._native.lib.dtc_set_option(b"f32x_s2_wgrad", 1)


def _run_and_check(dtc, cuda, what, x, dy, dsc, scale=1.0, **kw):
    dw, dwsc = dtc.ops.conv2d_wgrad_sc_f32(*(torch.from_numpy(a).to(cuda) for a in (x, dy, dsc)), scale=scale, **kw)
    K, C = dy.shape[3], x.shape[3]
    assert dw.shape == (K, 3, 3, C) and dwsc.shape == (K, C) and dw.dtype == dwsc.dtype == torch.float32
    for name, got, g, r, pad in (("dw", dw, dy, 3, 1), ("dwsc", dwsc, dsc, 1, 0)):
        ref = scale * O.conv2d_wgrad(x, g, r, r, 2, pad)
        mag = scale * O.conv2d_wgrad(np.abs(x), np.abs(g), r, r, 2, pad)
        _check(f"{what} {name}", got.cpu().numpy().reshape(ref.shape), ref, mag)
    return dw, dwsc


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_split_wgrad_pair(dtc, cuda, every_geometry, shape, kind):
    N, H, W, C, K = shape
    assert dtc.ops.conv2d_f32_wgrad_sc_route(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 2, 1), 1) == "split"
    scale = 0.25 if shape == SHAPES[1] else 1.0  # a power of two: the bound is unchanged
    _run_and_check(dtc, cuda, f"wgrad_sc {shape} {kind}", *_inputs(shape, kind), scale=scale, algo=1)


def test_workspace_tiers_and_determinism(dtc, cuda, every_geometry):
    """The default workspace (several splits and the two reduces) and a zero-length one (one split writes dw and dwsc
    itself) are both within the bound; two runs of either give equal bits."""
    shape = SHAPES[3]
    ins = _inputs(shape, "randn")
    none = torch.empty(0, dtype=torch.uint8, device=cuda)
    assert dtc._native.lib.dtc_conv2d_f32_wgrad_sc_workspace_size(dtc.ops.conv_desc(*shape, 3, 3, 2, 1), 1) > 0
    for what, kw in (("default workspace", {}), ("no workspace", {"workspace": none})):
        a, b = (_run_and_check(dtc, cuda, what, *ins, algo=1, **kw) for _ in range(2))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what


def test_slab_on_hand_bounds_the_splits(dtc, cuda, every_geometry):
    """(8, 16, 16, 64 -> 128): 16 steps of four output rows, four tiles, so the kernel wants 4 splits. A workspace of two
    slabs runs two and the reduces, none runs one split that writes dw and dwsc itself: both within the bound."""
    shape = (8, 16, 16, 64, 128)
    ins = _inputs(shape, "randn")
    one = 128 * 10 * 64 * 4
    assert dtc._native.lib.dtc_conv2d_f32_wgrad_sc_workspace_size(dtc.ops.conv_desc(*shape, 3, 3, 2, 1), 1) == 4 * one
    for what, nbytes in (("two slabs", 2 * one), ("no workspace", 0)):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
        _run_and_check(dtc, cuda, f"wgrad_sc {shape} {what}", *ins, algo=1, workspace=ws)


def test_exact_pair_is_the_separate_calls_and_serves_refused_shapes(dtc, cuda):
    """algo=0 equals the two conv2d_wgrad_f32(algo=0) calls bit for bit; algo=1 at a refused shape (6-wide output rows)
    equals algo=0."""
    shape = (2, 12, 12, 64, 128)
    assert dtc.ops.conv2d_f32_wgrad_sc_route(dtc.ops.conv_desc(*shape, 3, 3, 2, 1), 1) == "exact"
    xd, dyd, dscd = (torch.from_numpy(a).to(cuda) for a in _inputs(shape, "randn"))
    dw, dwsc = dtc.ops.conv2d_wgrad_sc_f32(xd, dyd, dscd, algo=0)
    assert torch.equal(dw, dtc.ops.conv2d_wgrad_f32(xd, dyd, 3, 3, 2, 1, algo=0))
    assert torch.equal(dwsc, dtc.ops.conv2d_wgrad_f32(xd, dscd, 1, 1, 2, 0, algo=0).reshape(dwsc.shape))
    for got, want in zip(dtc.ops.conv2d_wgrad_sc_f32(xd, dyd, dscd, algo=1), (dw, dwsc)):
        assert torch.equal(got, want)


def test_executor_with_f32_split_4_per_layer(dtc, cuda):
    """The fp32 executor with option f32_split = 4: every layer, the transition blocks' fused weight gradients included,
    within the fp32 tolerance (1e-5) of the oracle on that layer's inputs (at batch 2 layers 3 and 4 take the fused
    kernel, layer 2 the exact pair)."""
    lib = dtc._native.lib
    try:
        lib.dtc_set_option(b"f32_split", 4)
        errs = _teacher_forced(dtc, cuda, 2, precision="fp32")
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    assert len(errs) > 90


def test_trainer_fp32_conv_split_full_trains(dtc, cuda, tmp_path):
    """`train.py single --fp32-conv split-full`: two epochs of the same three batches; the loss is finite and falls."""
    lib = dtc._native.lib
    try:
        t = dtc.trainer.main(["--epoch", "2", "--batch-size", "32", "--max-steps", "3", "--workers", "0", "--lr", "0.02",
                              "--synthetic-train", "120", "--synthetic-test", "32", "--eval-step", "1",
                              "--fp32-conv", "split-full", "--ckpt-path", str(tmp_path)], "single")
        assert lib.dtc_get_option(b"f32_split") == 4
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    rows = [json.loads(line) for line in open(os.path.join(t.save_path, "scalars.jsonl"))]
    losses = [r["train"] for r in rows if r["tag"] == "loss/epoch"]
    print("train loss per epoch:", losses)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and losses[1] < losses[0]
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--amp", "--fp32-conv", "split-full"], "single")
