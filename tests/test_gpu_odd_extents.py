"""Stride-2 convolutions of odd-extent maps, and the stride-1 3x3 convs at the odd maps behind them, per kernel.

Every other stride-2 case of the suite has an even input height and width, which is what the stride-2 tiled
kernels require (the parity-class dgrad, the column-split halo forward, the stride-2 halo wgrad with and without
its fused shortcut, the sub-pixel halo dgrad, the compact shortcut residual: each guards itself with H % 2 == 0 &&
W % 2 == 0). A 28x28, 36x36 or 18x21 image sends its stride-2 layers down the generic code instead, with
P = (H + 1) / 2 output rows, where tap r = 2 of the last output row reads input row H: padding for odd H, data for
even H. The shapes here are those layers (and the stride-1 convs of the odd maps they produce), each against
oracle/ops.py: the norm criteria of tests/test_gpu_ops.py with the element-wise bounds of tests/bounds.py beside
them, the weight gradients' included (wgrad_tol). Inputs are bf16-representable.

Paths at the default options: conv_route in distributed-training-comparison_amd/csrc/conv_route.cpp is the one
function that picks the kernel of a (shape, pass), from each kernel's own predicate (DESIGN.md §7m has the order);
tools/conv_digest.py prints the kernels every shape here launches, under the forced options below too. Listed, not
asserted:

Stride 2, 3x3 / pad 1 and 1x1 / pad 0 alike -- every case is refused by every stride-2 tiled plan (odd H or W; the
1x1 has none) and runs the implicit GEMM: forward at P x Q = ceil(H / 2) x ceil(W / 2), the masked (non-class)
dgrad whatever dgrad_classes says, the generic wgrad. igemm_plan's tiles and split-K factors (fwd | dgrad | wgrad;
64 / 128: 64x64 / 128x128 tiles, xS: S splits, every wgrad one split of ceil(N P Q / 64) pixel steps) and the wgrad
loader (fast: a 64-pixel step is whole output images; slow: per-pixel decode):

    (3, 7, 7, 256, 512)   3x3: 64 x4 | 64 x9 | 128, fast (16-pixel outputs)   1x1: 64 x1 | 64 x1 | 64, fast
    (2, 9, 11, 128, 256)  3x3: 64 x2 | 64 x4 | 64, slow (30-pixel outputs)    1x1: 64 x1 | 64 x1 | 64, slow
    (2, 5, 6, 256, 512)   3x3: 64 x4 | 64 x9 | 128, slow (9-pixel outputs)    1x1: 64 x1 | 64 x1 | 64, slow
    (3, 18, 21, 64, 128)  3x3: 64 x1 | 64 x2 | 64, slow (99-pixel outputs)    1x1: 64 x1 | 64 x1 | 64, slow
    (3, 15, 17, 64, 128)  3x3: 64 x1 | 64 x2 | 64, slow (72-pixel outputs)    1x1: 64 x1 | 64 x1 | 64, slow
    (2, 3, 3, 256, 512)   3x3: 64 x4 | 64 x9 | 128, fast (4-pixel outputs)    1x1: 64 x1 | 64 x1 | 64, fast
    (4, 1, 1, 256, 512)   3x3: 64 x4 | 64 x9 | 128, fast (1-pixel outputs)    1x1: 64 x1 | 64 x1 | 64, fast
    (9, 13, 15, 64, 128)  3x3: 64 x1 | 64 x2 | 64, slow (56-pixel outputs)    1x1: 64 x1 | 64 x1 | 64, slow

The fused forward (conv2d_fwd_sc, implicit GEMM with the shortcut on the centre-tap tiles) takes the three C = 64
cases (one split, at most 512 workgroups); the C = 128 / 256 cases plan split-K and are refused. The fused dgrad
and the fused wgrad have no plan at any of them.

Stride 1, 3x3 / pad 1 (fwd and dgrad | wgrad):

    (3, 7, 7, 256, 256)    implicit GEMM, 64x64 tiles, 4 splits: no whole-row / whole-image halo tile of 49 pixels,
                           and the general geometry would fill 49 of 128 slots (under half) | implicit GEMM, slow loader
    (3, 9, 11, 128, 128)   conv_halo general geometry, configuration 2: one 9 x 11 tile per image, 99 of 128 slots
                           real | implicit GEMM, slow loader (64 / 11 = 5 rows per step do not divide 9)
    (3, 5, 6, 256, 256)    implicit GEMM, 4 splits (30 of 128 slots) | implicit GEMM, slow loader
    (3, 3, 3, 512, 512)    implicit GEMM, 9 splits (9 of 128 slots) | implicit GEMM, 128x128 tiles, slow loader
    (3, 2, 3, 512, 512)    implicit GEMM, 9 splits (6 of 128 slots) | implicit GEMM, 128x128 tiles, slow loader
    (2, 15, 17, 64, 64)    conv_c64 refuses (17 divides neither 256 nor by 32) also when forced; conv_halo general
                           geometry, configuration 2: 5 x 17 tiles, 85 of 128 slots real | wgrad_halo general geometry:
                           3 x 17 steps, 51 of 64 slots real, one split (writes dw itself); the only case with a
                           batched plan
    (2, 14, 14, 128, 128)  conv_halo general geometry, configuration 2: 7 x 14 tiles, 98 of 128 slots real | implicit
                           GEMM, slow loader (64 / 14 = 4 rows per step do not divide 14)

Forced classic halo configurations (halo_conv >= 2) fit none of these maps and fall back to the implicit GEMM, as
halo_gen = 0 does; wgrad_halo = 0 and wgrad_gen = 0 move 15 x 17 to the implicit GEMM.
"""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import bounds as B
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

# (N, H, W, C, K), each as 3x3 / pad 1 and as 1x1 / pad 0, stride 2
S2_ODD = [
    (3, 7, 7, 256, 512),    # layer4.0 of a 28x28 net: ragged pixel count, split-K
    (2, 9, 11, 128, 256),   # odd / odd
    (2, 5, 6, 256, 512),    # odd / even
    (3, 18, 21, 64, 128),   # even / odd, C = 64
    (3, 15, 17, 64, 128),   # odd / odd, C = 64
    (2, 3, 3, 256, 512),
    (4, 1, 1, 256, 512),    # a 1x1 map: P = Q = 1
    (9, 13, 15, 64, 128),   # M = 504: several pixel tiles, a ragged last one
]
# (N, H, W, C, K), 3x3 / pad 1, stride 1: the odd maps those networks produce
S1_ODD = [
    (3, 7, 7, 256, 256),
    (3, 9, 11, 128, 128),
    (3, 5, 6, 256, 256),
    (3, 3, 3, 512, 512),
    (3, 2, 3, 512, 512),
    (2, 15, 17, 64, 64),
    (2, 14, 14, 128, 128),
]
SC_MUST_FUSE = [(3, 18, 21, 64, 128), (3, 15, 17, 64, 128)]  # conv_fwd_sc_ok: 64x64 plan, one split, <= 512 workgroups

# forced options that must not get past the parity guards (stride-2 3x3): each alone, then all together
_S2_ALONE = [{"halo_s2": 2}, {"halo_s2": 3}, {"halo_s2": 4}, {"dgrad_s2h": 2}, {"wgrad_s2": 1}, {"dgrad_scf": 1}]
S2_FORCED = _S2_ALONE + [{"halo_s2": k, "dgrad_s2h": 2, "wgrad_s2": 1, "dgrad_scf": 1} for k in (2, 3, 4)]
# forced settings of test_conv_halo_configs, test_conv_c64, test_conv_wgrad_halo (+ the general geometries off)
S1_FORCED = [{"halo_conv": 2 + cfg, "halo_split": split} for cfg in range(8) for split in (0, 2)] + \
            [{"conv_c64": 2}, {"wgrad_halo": 0}, {"wgrad_gen": 0}, {"halo_small": 0}, {"halo_gen": 0}]

FILL16, FILL32 = 0x7FD5, 0x7FD5AAAA  # quiet-NaN bit patterns (tests/bounds.py's): an untouched output


def _opt_id(o):
    return ",".join(f"{k}={v}" for k, v in o.items())


def _rand_bf16(shape, gen, scale=1.0):
    return O.bf16(gen.standard_normal(shape).astype(np.float32) * scale)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(torch.bfloat16)


def _np(t):
    return t.float().cpu().numpy()


class _Opts:
    """Set the given options, restore the previous values on exit."""

    def __init__(self, dtc, opts):
        self.lib, self.opts = dtc._native.lib, opts

    def __enter__(self):
        self.prev = {k: self.lib.dtc_get_option(k.encode()) for k in self.opts}
        try:
            for k, v in self.opts.items():
                assert self.lib.dtc_set_option(k.encode(), v) == 0, k
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            self.lib.dtc_set_option(k.encode(), v)


def _filled(shape, dtype, dev):
    """A tensor holding the NaN bit pattern in every word (an output no kernel may touch)."""
    if dtype == torch.bfloat16:
        return torch.full(shape, FILL16, dtype=torch.int16, device=dev).view(torch.bfloat16)
    return torch.full(shape, FILL32, dtype=torch.int32, device=dev).view(torch.float32)


def _untouched(t):
    bits, pat = (torch.int16, FILL16) if t.dtype == torch.bfloat16 else (torch.int32, FILL32)
    return bool((t.view(bits) == pat).all())


def _same_bits(a, b):
    bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return a.shape == b.shape and torch.equal(a.view(bits), b.view(bits))


_PROBLEMS = {}


def _problem(case, R, stride):
    """The operands, oracle results and bounds of one geometry, computed once and shared; no test modifies the
    dictionary or its arrays (_sc_problem keeps the shortcut's operands in a dictionary of its own)."""
    key = (case, R, stride)
    if key not in _PROBLEMS:
        N, H, W, C, K = case
        pad = 1 if R == 3 else 0
        P, Q = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
        g = np.random.default_rng(1000 * R + 10 * H + W + stride)
        x, w = _rand_bf16((N, H, W, C), g), _rand_bf16((K, R, R, C), g, 0.05)
        dy, res = _rand_bf16((N, P, Q, K), g), _rand_bf16((N, H, W, C), g)
        y = O.conv2d_fwd(x, w, stride, pad)
        dx = O.conv2d_dgrad(dy, w, (H, W), stride, pad)
        pr = dict(case=case, R=R, st=stride, pad=pad, P=P, Q=Q, x=x, w=w, dy=dy, res=res, y=y,
                  y_tol=B.fwd_tol(y, x, w, stride, pad), dx=dx, dx_tol=B.dgrad_tol(dx, dy, w, (H, W), stride, pad),
                  dxr=dx + res, dxr_tol=B.dgrad_tol(dx + res, dy, w, (H, W), stride, pad, res=res),
                  dw=0.5 * O.conv2d_wgrad(x, dy, R, R, stride, pad), dw_tol=B.wgrad_tol(x, dy, R, R, stride, pad, 0.5))
        assert y.shape == (N, P, Q, K) and all(np.linalg.norm(pr[k]) > 0 for k in ("y", "dx", "dw"))
        _PROBLEMS[key] = pr
    return _PROBLEMS[key]


def _run(dtc, cuda, pr):
    """fwd (+ statistics), dgrad with and without the residual, wgrad (scale 0.5) under the options in force."""
    N, H, W, C, K = pr["case"]
    R, st, pad = pr["R"], pr["st"], pr["pad"]
    xd, wd, dyd, rd = (_dev(pr[k], cuda) for k in ("x", "w", "dy", "res"))
    stats = dtc.ops.new_stats(K, cuda)
    out = {"y": dtc.ops.conv2d_fwd(xd, wd, st, pad, stats=stats),
           "dx": dtc.ops.conv2d_dgrad(dyd, wd, (H, W), st, pad),
           "dxr": dtc.ops.conv2d_dgrad(dyd, wd, (H, W), st, pad, res=rd),
           "dw": dtc.ops.conv2d_wgrad(xd, dyd, R, R, st, pad, scale=0.5)}
    torch.cuda.synchronize()
    out["stats"] = dtc.ops.stat_totals(stats, K)
    return out


def _check_stats(totals, yk, K):
    """BN statistics of the bf16 output as test_conv_fwd checks them."""
    s = totals.numpy()
    yb = yk.reshape(-1, K).astype(np.float64)
    np.testing.assert_allclose(s[0], yb.sum(0), rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(s[1], (yb * yb).sum(0), rtol=1e-5, atol=1e-3)


def _check(name, pr, out):
    """The norm criteria and the element-wise bounds of one _run; prints the worst |err| / tol per pass."""
    K = pr["case"][4]
    yk, dx, dxr, dw = _np(out["y"]), _np(out["dx"]), _np(out["dxr"]), out["dw"].cpu().numpy()
    assert yk.shape == pr["y"].shape and dw.shape == pr["dw"].shape
    assert rel_err(yk, pr["y"]) < 1e-2, name
    _check_stats(out["stats"], yk, K)
    assert rel_err(dx, pr["dx"]) < 1e-2 and rel_err(dxr, pr["dxr"]) < 1e-2, name
    assert rel_err(dw, pr["dw"]) < 1e-5, name
    r = (B.assert_within(yk, pr["y"], pr["y_tol"], f"{name} y"),
         max(B.assert_within(dx, pr["dx"], pr["dx_tol"], f"{name} dx"),
             B.assert_within(dxr, pr["dxr"], pr["dxr_tol"], f"{name} dx + res")),
         B.assert_within(dw, pr["dw"], pr["dw_tol"], f"{name} dw"))
    print(f"{name}: worst |err|/tol fwd {r[0]:.3f} dgrad {r[1]:.3f} wgrad {r[2]:.3f}")


_DEFAULT_RUNS = {}
# csrc/kernels.h DTC_OPTION_LIST: the defaults of every option this module forces and of those that choose the plan
# of the launches it compares bit for bit
DEFAULTS = {"dgrad_classes": 1, "halo_s2": 1, "dgrad_s2h": 1, "wgrad_s2": 1, "dgrad_scf": 1, "halo_conv": 1,
            "halo_split": 0, "conv_c64": 1, "wgrad_halo": 224, "wgrad_gen": 1, "halo_small": 1, "halo_gen": 1,
            "igemm_tile": 0, "igemm_split": 0, "sc_fuse": 1, "wgrad_fast": 1, "wgrad_direct": 1, "splitk_ink": 1,
            "xcd_remap": 1}


def _assert_defaults(dtc):
    """Every option in DEFAULTS reads back its default: an option another test leaked would otherwise become the
    'default' that the bit comparisons are made against."""
    now = {k: dtc._native.lib.dtc_get_option(k.encode()) for k in DEFAULTS}
    assert now == DEFAULTS, {k: (v, DEFAULTS[k]) for k, v in now.items() if v != DEFAULTS[k]}


def _default_run(dtc, cuda, pr):
    """The default-option run of a geometry, kept for the bit comparisons; the options are checked to be at their
    defaults before it is made."""
    key = (pr["case"], pr["R"], pr["st"])
    if key not in _DEFAULT_RUNS:
        _assert_defaults(dtc)
        _DEFAULT_RUNS[key] = _run(dtc, cuda, pr)
    return _DEFAULT_RUNS[key]


def _assert_same_run(name, a, b):
    for k in ("y", "dx", "dxr", "dw"):
        assert _same_bits(a[k], b[k]), f"{name}: {k} differs bit-wise from the default-option run"
    assert torch.equal(a["stats"], b["stats"]), f"{name}: BN statistics differ from the default-option run"


# ----------------------------------------------------------------------------- stride 2
@pytest.mark.parametrize("R", [3, 1])
@pytest.mark.parametrize("case", S2_ODD, ids=str)
def test_stride2_odd_fwd_dgrad_wgrad(dtc, cuda, case, R):
    """conv2d_fwd (+ statistics), conv2d_dgrad (with and without res) and conv2d_wgrad at an odd stride-2 map against
    the oracle; the parity-class path cannot apply, so dgrad_classes 0 and 1 must give bit-identical results."""
    pr = _problem(case, R, 2)
    name = f"s2 {case} {R}x{R}"
    out = _default_run(dtc, cuda, pr)
    _check(name, pr, out)
    runs = {}
    for classes in (0, 1):
        with _Opts(dtc, {"dgrad_classes": classes}):
            runs[classes] = _run(dtc, cuda, pr)
        _check(f"{name} dgrad_classes={classes}", pr, runs[classes])
    _assert_same_run(f"{name} dgrad_classes 0 vs 1", runs[0], runs[1])
    _assert_same_run(f"{name} dgrad_classes=1", runs[1], out)


@pytest.mark.parametrize("opts", S2_FORCED, ids=_opt_id)
@pytest.mark.parametrize("case", S2_ODD, ids=str)
def test_stride2_odd_forced_options_fall_back(dtc, cuda, case, opts):
    """Forced stride-2 tiled kernels (column-split halo forward, sub-pixel halo dgrad, stride-2 halo wgrad, fused
    shortcut dgrad) must be refused by their parity guards: correct against the oracle and bit-identical to the
    default-option run of the same shape."""
    pr = _problem(case, 3, 2)
    name = f"s2 {case} 3x3 {_opt_id(opts)}"
    base = _default_run(dtc, cuda, pr)
    with _Opts(dtc, opts):
        out = _run(dtc, cuda, pr)
    _check(name, pr, out)
    _assert_same_run(name, out, base)


# ----------------------------------------------------------------------------- stride 1
@pytest.mark.parametrize("case", S1_ODD, ids=str)
def test_stride1_odd_maps(dtc, cuda, case):
    """The stride-1 3x3 convs at the odd maps: fwd (+ statistics), dgrad, wgrad against the oracle; where a batched
    halo plan exists (a non-zero workspace query), conv2d_wgrad_batch of two problems against the oracle, bit-identical
    when repeated, and bit-identical to the one-by-one conv2d_wgrad launches test_conv_wgrad_batch compares against
    (that test allows 1e-6 for split counts that differ between the two; at the one shape with a batched plan here,
    15x17, both plans are a single split of the same 10 steps whose kernel writes dw itself, in the same order)."""
    N, H, W, C, K = case
    pr = _problem(case, 3, 1)
    _check(f"s1 {case}", pr, _default_run(dtc, cuda, pr))
    nb = dtc._native.lib.dtc_conv2d_wgrad_batch_workspace_size(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 1, 1), 2)
    print(f"s1 {case}: batched wgrad workspace for 2 problems {nb} bytes")
    if nb == 0:
        with pytest.raises(ValueError, match="no batched halo plan"):
            dtc.ops.conv2d_wgrad_batch([_dev(pr["x"], cuda)] * 2, [_dev(pr["dy"], cuda)] * 2)
        return
    g = np.random.default_rng(11)
    xs = [pr["x"], _rand_bf16((N, H, W, C), g)]
    dys = [pr["dy"], _rand_bf16((N, H, W, K), g)]
    xd, dyd = [_dev(a, cuda) for a in xs], [_dev(a, cuda) for a in dys]
    got = dtc.ops.conv2d_wgrad_batch(xd, dyd, scale=0.25)
    again = dtc.ops.conv2d_wgrad_batch(xd, dyd, scale=0.25)
    ones = [dtc.ops.conv2d_wgrad(xd[i], dyd[i], 3, 3, 1, 1, scale=0.25) for i in range(2)]
    torch.cuda.synchronize()
    assert len(got) == 2
    worst = 0.0
    for i in range(2):
        assert torch.equal(got[i], again[i]), i
        ref = 0.25 * O.conv2d_wgrad(xs[i], dys[i], 3, 3, 1, 1)
        gi = got[i].cpu().numpy()
        assert rel_err(gi, ref) < 1e-5, i
        assert torch.equal(got[i], ones[i]), f"s1 {case} batch dw {i}: differs bit-wise from the one-by-one conv2d_wgrad"
        worst = max(worst, B.assert_within(gi, ref, B.wgrad_tol(xs[i], dys[i], 3, 3, 1, 1, 0.25), f"s1 {case} batch dw {i}"))
    print(f"s1 {case} wgrad_batch: worst |err|/tol {worst:.3f}")


@pytest.mark.parametrize("opts", S1_FORCED, ids=_opt_id)
@pytest.mark.parametrize("case", S1_ODD, ids=str)
def test_stride1_odd_maps_forced_settings(dtc, cuda, case, opts):
    """Every forced setting the halo / conv_c64 / wgrad_halo tests use, at the odd maps: the result is correct
    whether the forced kernel accepts the shape or falls back."""
    pr = _problem(case, 3, 1)
    with _Opts(dtc, opts):
        out = _run(dtc, cuda, pr)
    _check(f"s1 {case} {_opt_id(opts)}", pr, out)


# ----------------------------------------------------------------------------- fused entry points
_SC_PROBLEMS = {}


def _sc_problem(case):
    """_problem(case, 3, 2) plus the projection shortcut's operands and oracle results (a dictionary of its own,
    computed once, never modified)."""
    if case not in _SC_PROBLEMS:
        pr = dict(_problem(case, 3, 2))
        N, H, W, C, K = case
        g = np.random.default_rng(77 + H * W)
        wsc = _rand_bf16((K, 1, 1, C), g, 0.1)
        ysc = O.conv2d_fwd(pr["x"], wsc, 2, 0)
        pr.update(wsc=wsc, dsc=_rand_bf16((N, pr["P"], pr["Q"], K), g), ysc=ysc,
                  ysc_tol=B.fwd_tol(ysc, pr["x"], wsc, 2, 0))
        assert ysc.shape == pr["y"].shape
        _SC_PROBLEMS[case] = pr
    return _SC_PROBLEMS[case]


def _fwd_sc_attempt(dtc, cuda, pr, name):
    """conv2d_fwd_sc into pre-filled outputs under the options in force: (y, ysc, totals, totals_sc), or None after a
    refusal (NativeError), which must have left every output and statistics word as it was."""
    N, H, W, C, K = pr["case"]
    xd, wd = _dev(pr["x"], cuda), _dev(pr["w"], cuda)
    wscd = _dev(pr["wsc"].reshape(K, C), cuda)
    y, ysc = (_filled((N, pr["P"], pr["Q"], K), torch.bfloat16, cuda) for _ in range(2))
    st1, st2 = dtc.ops.new_stats(K, cuda), dtc.ops.new_stats(K, cuda)
    try:
        dtc.ops.conv2d_fwd_sc(xd, wd, wscd, stats=st1, stats_sc=st2, out=(y, ysc))
    except dtc._native.NativeError as e:
        torch.cuda.synchronize()
        assert _untouched(y) and _untouched(ysc), f"{name}: a refusal wrote its outputs"
        assert int(st1.abs().sum()) == 0 and int(st2.abs().sum()) == 0, f"{name}: a refusal wrote its statistics"
        print(f"{name}: refused ({e})")
        return None
    torch.cuda.synchronize()
    return y, ysc, dtc.ops.stat_totals(st1, K), dtc.ops.stat_totals(st2, K)


@pytest.mark.parametrize("case", S2_ODD, ids=str)
def test_stride2_odd_fused_forward(dtc, cuda, case):
    """conv2d_fwd_sc at the odd maps: it must run at the two C = 64 network shapes (conv_fwd_sc_ok admits odd extents:
    a 64x64 plan, one split, at most 512 workgroups), elsewhere it runs or refuses. Where it runs: y and ysc against
    the oracle (norm and fwd_tol), both statistics, and y bit-identical to the unfused conv2d_fwd (neither splits K;
    the same MFMA sequence per element). A refusal raises NativeError and launches nothing. Then once more under each
    forced column-split halo forward (halo_s2 in {2, 3, 4}), whose parity guard must refuse the odd map through this
    entry point too: the same outcome (fused or refused), every output and statistic bit-identical to the default
    run's."""
    K = case[4]
    pr = _sc_problem(case)
    name = f"fwd_sc {case}"
    unfused = _default_run(dtc, cuda, pr)  # (also checks that the options are at their defaults)
    base = _fwd_sc_attempt(dtc, cuda, pr, name)
    assert base is not None or case not in SC_MUST_FUSE, f"{name}: the fused plan must exist here"
    if base is not None:
        y, ysc, tot, tot_sc = base
        yk, ysck = _np(y), _np(ysc)
        assert rel_err(yk, pr["y"]) < 1e-2 and rel_err(ysck, pr["ysc"]) < 1e-2
        r = max(B.assert_within(yk, pr["y"], pr["y_tol"], f"{name} y"),
                B.assert_within(ysck, pr["ysc"], pr["ysc_tol"], f"{name} ysc"))
        print(f"{name}: fused; worst |err|/tol {r:.3f}")
        _check_stats(tot, yk, K)
        _check_stats(tot_sc, ysck, K)
        assert _same_bits(y, unfused["y"]), f"{name}: y differs from the unfused conv2d_fwd"
    for cfg in (2, 3, 4):
        what = f"{name} halo_s2={cfg}"
        with _Opts(dtc, {"halo_s2": cfg}):
            forced = _fwd_sc_attempt(dtc, cuda, pr, what)
        assert (forced is None) == (base is None), f"{what}: fused / refused differs from the default options"
        if forced is not None:
            assert _same_bits(forced[0], base[0]) and _same_bits(forced[1], base[1]), f"{what}: outputs differ"
            assert torch.equal(forced[2], base[2]) and torch.equal(forced[3], base[3]), f"{what}: statistics differ"


@pytest.mark.parametrize("opts", [{}, {"dgrad_scf": 1, "dgrad_s2h": 2, "wgrad_s2": 1}], ids=["default", "forced"])
@pytest.mark.parametrize("case", S2_ODD, ids=str)
def test_stride2_odd_fused_backward_is_refused(dtc, cuda, case, opts):
    """No fused shortcut dgrad and no fused shortcut wgrad at an odd map: conv2d_dgrad_sc raises NativeError,
    dtc_conv2d_wgrad_sc_workspace_size is 0 (the wrapper raises ValueError; the entry point itself NativeError),
    and no output word changes."""
    N, H, W, C, K = case
    pr = _sc_problem(case)
    lib = dtc._native.lib
    dyd, dscd, xd, wd = (_dev(pr[k], cuda) for k in ("dy", "dsc", "x", "w"))
    wscd = _dev(pr["wsc"].reshape(K, C), cuda)
    dx = _filled((N, H, W, C), torch.bfloat16, cuda)
    dw, dwsc = _filled((K, 3, 3, C), torch.float32, cuda), _filled((K, C), torch.float32, cuda)
    ws = torch.empty(1 << 20, dtype=torch.float32, device=cuda)
    with _Opts(dtc, opts):
        with pytest.raises(dtc._native.NativeError):
            dtc.ops.conv2d_dgrad_sc(dyd, wd, dscd, wscd, (H, W), out=dx)
        d = dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 2, 1)
        assert lib.dtc_conv2d_wgrad_sc_workspace_size(d) == 0
        with pytest.raises(ValueError, match="no fused plan"):
            dtc.ops.conv2d_wgrad_sc(xd, dyd, dscd, scale=0.5, out=(dw, dwsc))
        with pytest.raises(dtc._native.NativeError):
            dtc._native.call("dtc_conv2d_wgrad_sc", d, dtc._native.ptr(xd), dtc._native.ptr(dyd), dtc._native.ptr(dscd),
                             dtc._native.ptr(dw), dtc._native.ptr(dwsc), 0.5, dtc._native.ptr(ws), ws.numel() * 4,
                             dtc._native.stream_ptr())
    torch.cuda.synchronize()
    assert _untouched(dx) and _untouched(dw) and _untouched(dwsc)
