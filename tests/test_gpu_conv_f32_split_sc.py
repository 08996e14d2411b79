"""The split-bf16 transition-block pair (csrc/conv_f32x_s2.hip; ops.conv2d_f32_fwd_sc / conv2d_dgrad_sc_f32 with algo=1,
the executor with option f32_split = 3) against the fp64 oracle on the kernel's own fp32 inputs, with the bound of
tests/test_gpu_conv_f32_split.py: |err| <= 2^-22 (|x| conv |w|) element-wise and rel_err < 1e-5."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests.test_gpu_conv_f32_split import KINDS, _check, _inputs
from tests.test_gpu_resnet import _teacher_forced

pytestmark = pytest.mark.gpu

SHAPES = [  # (N, H, W, C, K)
    (1, 8, 8, 64, 128),     # one ragged tile (1 of 2 image slots), 4-wide output rows
    (5, 8, 8, 256, 512),    # whole-image tiles, the last one ragged; the deepest reduction
    (2, 16, 16, 128, 256),  # 8-wide rows, several chunks
    (1, 32, 32, 64, 128),   # 16-wide rows, several row tiles, two output-channel tiles
    (3, 16, 16, 64, 64),    # C = K
]


def _sc_filter(shape, kind):
    """The shortcut's [K, C] filter: random, or one-hot like the 3x3 one."""
    _, _, _, C, K = shape
    if kind == "randn":
        return (np.random.default_rng(sum(shape)).standard_normal((K, C)) * 0.1).astype(np.float32)
    wsc = np.zeros((K, C), np.float32)
    wsc[np.arange(K), (np.arange(K) + 3) % C] = 1.0
    return wsc


def _dev(cuda, *arrays):
    return [torch.from_numpy(a).to(cuda) for a in arrays]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_split_forward_pair_and_statistics(dtc, cuda, shape, kind):
    N, H, W, C, K = shape
    assert dtc.ops.conv2d_f32_sc_route(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 2, 1), 0, 1) == "split"
    x, w = _inputs(shape, kind, False)
    wsc = _sc_filter(shape, kind)
    st, st_sc = dtc.ops.new_stats(K, cuda), dtc.ops.new_stats(K, cuda)
    y, ysc = dtc.ops.conv2d_f32_fwd_sc(*_dev(cuda, x, w, wsc), algo=1, stats=st, stats_sc=st_sc)
    w1 = wsc[:, None, None, :]
    for what, got, s, ww, pad in (("y", y, st, w, 1), ("ysc", ysc, st_sc, w1, 0)):
        got = got.cpu().numpy()
        _check(f"fwd_sc {what} {shape} {kind}", got, O.conv2d_fwd(x, ww, 2, pad), O.conv2d_fwd(np.abs(x), np.abs(ww), 2, pad))
        if kind == "randn":  # the statistics of the kernel's own output
            tot = dtc.ops.stat_totals(s, K).numpy()
            yb = got.reshape(-1, K).astype(np.float64)
            np.testing.assert_allclose(tot[0], yb.sum(0), rtol=1e-5, atol=1e-3)
            np.testing.assert_allclose(tot[1], (yb * yb).sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_split_dgrad_pair(dtc, cuda, shape, kind):
    N, H, W, C, K = shape
    assert dtc.ops.conv2d_f32_sc_route(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 2, 1), 1, 1) == "split"
    full, w = _inputs((N, H, W, C, K), kind, True)  # [N, H, W, K]: dy and dsc are two of its stride-2 sub-grids
    dy, dsc = np.ascontiguousarray(full[:, ::2, ::2]), np.ascontiguousarray(full[:, 1::2, 1::2])
    wsc = _sc_filter(shape, kind)
    dyd, wd, dscd, wscd = _dev(cuda, dy, w, dsc, wsc)
    dx = dtc.ops.conv2d_dgrad_sc_f32(dyd, wd, dscd, wscd, (H, W), algo=1).cpu().numpy()
    w1 = wsc[:, None, None, :]
    ref = O.conv2d_dgrad(dy, w, (H, W), 2, 1) + O.conv2d_dgrad(dsc, w1, (H, W), 2, 0)
    mag = (O.conv2d_dgrad(np.abs(dy), np.abs(w), (H, W), 2, 1) + O.conv2d_dgrad(np.abs(dsc), np.abs(w1), (H, W), 2, 0)
           + 0.5 * np.abs(ref))  # the one extra fp32 rounding of a sum of two terms
    _check(f"dgrad_sc {shape} {kind}", dx, ref, mag)


def _pair(dtc, cuda, shape, algo):
    N, H, W, C, K = shape
    x, w = _inputs(shape, "randn", False)
    dy = np.ascontiguousarray(_inputs(shape, "randn", True)[0][:, ::2, ::2])
    xd, wd, wscd, dyd = _dev(cuda, x, w, _sc_filter(shape, "randn"), dy)
    y, ysc = dtc.ops.conv2d_f32_fwd_sc(xd, wd, wscd, algo=algo)
    return (xd, wd, wscd, dyd), (y, ysc, dtc.ops.conv2d_dgrad_sc_f32(dyd, wd, y, wscd, (H, W), algo=algo))


def test_exact_pair_is_the_separate_calls_and_serves_refused_shapes(dtc, cuda):
    """algo=0 equals the two existing calls bit for bit; algo=1 at a refused shape (6-wide output rows) equals algo=0."""
    shape = (2, 12, 12, 64, 128)
    assert dtc.ops.conv2d_f32_sc_route(dtc.ops.conv_desc(2, 12, 12, 64, 128, 3, 3, 2, 1), 0, 1) == "exact"
    (xd, wd, wscd, dyd), exact = _pair(dtc, cuda, shape, 0)
    w1 = wscd[:, None, None, :].contiguous()
    y = dtc.ops.conv2d_f32(xd, wd, 2, 1)
    ysc = dtc.ops.conv2d_f32(xd, w1, 2, 0)
    dxs = dtc.ops.conv2d_dgrad_f32(y, w1, (12, 12), 2, 0)  # (_pair feeds y back as dsc)
    dx = dtc.ops.conv2d_dgrad_f32(dyd, wd, (12, 12), 2, 1, res=dxs)
    for got, want in zip(exact, (y, ysc, dx)):
        assert torch.equal(got, want)
    for got, want in zip(_pair(dtc, cuda, shape, 1)[1], exact):
        assert torch.equal(got, want)


def test_split_pair_runs_are_bit_identical(dtc, cuda):
    a, b = (_pair(dtc, cuda, (2, 16, 16, 128, 256), 1)[1] for _ in range(2))
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_executor_with_f32_split_3_per_layer(dtc, cuda):
    """The fp32 executor with option f32_split = 3: every layer within the fp32 tolerance (1e-5) of the oracle on that
    layer's inputs. The transition blocks' `.dx` is the fused kernel's; the capture-enabled executor of this check
    also runs the shortcut's own data gradient, only to store `.dxs`."""
    lib = dtc._native.lib
    try:
        lib.dtc_set_option(b"f32_split", 3)
        errs = _teacher_forced(dtc, cuda, 2, precision="fp32")
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    assert len(errs) > 90


def test_trainer_fp32_conv_split_s2_trains(dtc, cuda, tmp_path):
    """`train.py single --fp32-conv split-s2`: two epochs of the same three batches; the loss is finite and falls."""
    lib = dtc._native.lib
    try:
        t = dtc.trainer.main(["--epoch", "2", "--batch-size", "32", "--max-steps", "3", "--workers", "0", "--lr", "0.02",
                              "--synthetic-train", "120", "--synthetic-test", "32", "--eval-step", "1",
                              "--fp32-conv", "split-s2", "--ckpt-path", str(tmp_path)], "single")
        assert lib.dtc_get_option(b"f32_split") == 3
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    rows = [json.loads(line) for line in open(os.path.join(t.save_path, "scalars.jsonl"))]
    losses = [r["train"] for r in rows if r["tag"] == "loss/epoch"]
    print("train loss per epoch:", losses)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and losses[1] < losses[0]
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--amp", "--fp32-conv", "split-s2"], "single")
