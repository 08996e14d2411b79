"""The split-bf16 fp32 convolution (csrc/conv_f32x.hip; ops.conv2d_f32 / conv2d_dgrad_f32 with algo=1, the executor
with option f32_split) against the fp64 oracle on the kernel's own fp32 inputs.

Element-wise bound: |y - ref| <= 2^-22 (|x| conv |w|). 2^-22 = 2.4e-7 is 8x the CPU-emulated worst case of the
six-product three-plane scheme (3.0e-8 of sum |x||w| on 576-long dot products) and 4x below what a two-plane or
dropped-term kernel gives (1.06e-6): it admits the design and rejects its cheaper look-alikes. Norm-wise the
project's fp32 tolerance, 1e-5."""
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
    (1, 4, 4, 64, 64),     # one ragged tile (1 of 8 image slots), the 4-wide pixel permutation
    (2, 8, 8, 128, 64),    # two reduction chunks, C != K, the 8-wide permutation
    (1, 16, 16, 64, 128),  # two output-channel tiles
    (3, 32, 32, 64, 64),   # several tiles, whole rows per tile
    (2, 4, 4, 512, 512),   # deepest reduction
    (9, 4, 4, 64, 64),     # two tiles of whole images, the second ragged
]
KINDS = ["randn", "onehot_centre", "onehot_corner"]
BOUND = 2.0 ** -22


def _inputs(shape, kind, rows_k):
    """fp32 activations [N,H,W,c_act] and a KRSC filter [K,3,3,C]; rows_k: the activations carry K channels (dy)."""
    N, H, W, C, K = shape
    g = np.random.default_rng(1000 * sum(shape) + 10 * KINDS.index(kind) + rows_k)
    ca = K if rows_k else C
    if kind == "randn":
        a = g.standard_normal((N, H, W, ca))
        w = g.standard_normal((K, 3, 3, C)) * 0.05
    else:  # wide-exponent activations, one 1.0 per filter: at the centre tap or at a corner (the padded border)
        a = g.standard_normal((N, H, W, ca)) * np.exp(3 * g.standard_normal((N, H, W, ca)))
        w = np.zeros((K, 3, 3, C))
        r, s = (1, 1) if kind == "onehot_centre" else (0, 2)
        w[np.arange(K), r, s, np.arange(K) % C] = 1.0
    return a.astype(np.float32), w.astype(np.float32)


def _check(what, got, ref, mag):
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / np.maximum(mag, 1e-300)).max())
    print(f"{what}: worst |err| / (|x| conv |w|) = {worst:.3e} (bound {BOUND:.3e}), rel_err {rel_err(got, ref):.3e}")
    assert (err <= BOUND * mag).all(), (what, worst)
    assert rel_err(got, ref) < 1e-5, what


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_split_forward_and_statistics(dtc, cuda, shape, kind):
    N, H, W, C, K = shape
    assert dtc.ops.conv2d_f32_route(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 1, 1), 0, 1) == "split"
    x, w = _inputs(shape, kind, False)
    stats = dtc.ops.new_stats(K, cuda)
    y = dtc.ops.conv2d_f32(torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda), 1, 1, algo=1, stats=stats)
    y = y.cpu().numpy()
    _check(f"fwd {shape} {kind}", y, O.conv2d_fwd(x, w, 1, 1), O.conv2d_fwd(np.abs(x), np.abs(w), 1, 1))
    if kind == "randn":  # the statistics of the kernel's own output, tests/test_gpu_ops.py's tolerance for them
        s = dtc.ops.stat_totals(stats, K).numpy()
        yb = y.reshape(-1, K).astype(np.float64)
        np.testing.assert_allclose(s[0], yb.sum(0), rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose(s[1], (yb * yb).sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_split_dgrad(dtc, cuda, shape, kind, with_res):
    N, H, W, C, K = shape
    assert dtc.ops.conv2d_f32_route(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 1, 1), 1, 1) == "split"
    dy, w = _inputs(shape, kind, True)
    res = np.random.default_rng(5).standard_normal((N, H, W, C)).astype(np.float32) if with_res else None
    dx = dtc.ops.conv2d_dgrad_f32(torch.from_numpy(dy).to(cuda), torch.from_numpy(w).to(cuda), (H, W), 1, 1, algo=1,
                                  res=torch.from_numpy(res).to(cuda) if with_res else None).cpu().numpy()
    ref = O.conv2d_dgrad(dy, w, (H, W), 1, 1)
    mag = O.conv2d_dgrad(np.abs(dy), np.abs(w), (H, W), 1, 1)
    if with_res:  # one more fp32 rounding, of dx + res: at most half an ulp of the sum, 2^-24 |dx|; 2^-23 |dx| is granted
        ref = ref + res
        mag = mag + np.abs(ref) * 0.5
    _check(f"dgrad {shape} {kind} res={with_res}", dx, ref, mag)


SPECIALS = np.array([0.0, -0.0, 3 * 2.0 ** -128, np.finfo(np.float32).max, -np.finfo(np.float32).max, np.nan],
                    np.float32)  # +-0, a subnormal (on the bf16 subnormal grid of 2^-133), the largest finite, NaN


@pytest.mark.parametrize("n", [1, 7, 8193])
def test_f32_split3_reconstructs_every_finite_input(dtc, cuda, n):
    g = np.random.default_rng(n)
    body = (g.standard_normal(n) * np.exp(3 * g.standard_normal(n))).astype(np.float32)
    cases = [SPECIALS[i:i + 1] for i in range(len(SPECIALS))] if n == 1 else [np.concatenate([SPECIALS, body])[:n]]
    for a in cases:
        pl = dtc.ops.f32_split3(torch.from_numpy(a.copy()).to(cuda))
        assert pl.shape == (3, n) and pl.dtype == torch.bfloat16
        p = (pl.view(torch.int16).cpu().numpy().astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            back = (p[2] + p[1]) + p[0]
        fin = np.isfinite(a)
        np.testing.assert_array_equal(back[fin].view(np.uint32), a[fin].view(np.uint32))
        assert np.isnan(back[~fin]).all() and np.isnan(p[0][~fin]).all()


def test_refused_shape_runs_the_exact_kernel(dtc, cuda):
    """algo=1 at a shape the split kernel refuses (7-wide rows) is conv_f32, bit for bit."""
    shape = (1, 5, 7, 64, 64)
    x, w = _inputs(shape, "randn", False)
    xd, wd = torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda)
    assert dtc.ops.conv2d_f32_route(dtc.ops.conv_desc(1, 5, 7, 64, 64, 3, 3, 1, 1), 0, 1) == "exact"
    assert torch.equal(dtc.ops.conv2d_f32(xd, wd, 1, 1, algo=1), dtc.ops.conv2d_f32(xd, wd, 1, 1, algo=0))
    assert torch.equal(dtc.ops.conv2d_dgrad_f32(xd, wd, (5, 7), 1, 1, algo=1),
                       dtc.ops.conv2d_dgrad_f32(xd, wd, (5, 7), 1, 1, algo=0))
    assert rel_err(dtc.ops.conv2d_f32(xd, wd, 1, 1, algo=0).cpu().numpy(), O.conv2d_fwd(x, w, 1, 1)) < 1e-5


def test_split_runs_are_bit_identical(dtc, cuda):
    shape = (3, 32, 32, 64, 64)
    x, w = _inputs(shape, "randn", False)
    xd, wd = torch.from_numpy(x).to(cuda), torch.from_numpy(w).to(cuda)
    runs = [(dtc.ops.conv2d_f32(xd, wd, 1, 1, algo=1), dtc.ops.conv2d_dgrad_f32(xd, wd, (32, 32), 1, 1, algo=1))
            for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_executor_with_f32_split_per_layer(dtc, cuda):
    """The fp32 executor with option f32_split: every layer within the fp32 tolerance (1e-5) of the oracle on that
    layer's inputs, as with the exact convs."""
    lib = dtc._native.lib
    try:
        lib.dtc_set_option(b"f32_split", 1)
        errs = _teacher_forced(dtc, cuda, 2, precision="fp32")
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    assert len(errs) > 90


def test_trainer_fp32_conv_split_trains(dtc, cuda, tmp_path):
    """`train.py single --fp32-conv split`: two epochs of the same three batches on the fp32 executor with the
    split convs; the loss is finite and falls."""
    lib = dtc._native.lib
    try:
        t = dtc.trainer.main(["--epoch", "2", "--batch-size", "32", "--max-steps", "3", "--workers", "0", "--lr", "0.02",
                              "--synthetic-train", "120", "--synthetic-test", "32", "--eval-step", "1",
                              "--fp32-conv", "split", "--ckpt-path", str(tmp_path)], "single")
        assert lib.dtc_get_option(b"f32_split") == 1
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    assert {k[3] for k in t.model._executors} == {"fp32"}
    rows = [json.loads(line) for line in open(os.path.join(t.save_path, "scalars.jsonl"))]
    losses = [r["train"] for r in rows if r["tag"] == "loss/epoch"]
    print("train loss per epoch:", losses)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses) and losses[1] < losses[0]
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--amp", "--fp32-conv", "split"], "single")
