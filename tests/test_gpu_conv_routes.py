"""Every route and short-workspace fallback of the conv router against the oracle, route asserted first.

tests/test_gpu_ops.py's conv cases run whatever kernel the router picks for their shape under the default options and
with the workspace the size query returns. Here each case names the route it means to cover and
dtc_conv2d_route_query must confirm it before anything is launched (a case whose shape the router has since sent
elsewhere fails instead of passing on another kernel). The C entry points are called directly (the ops wrappers
refuse a short workspace, rightly) with every operand, output, statistics block and the workspace -- exactly the
stated bytes, 0 meaning NULL -- embedded in a tests/bounds.py arena. Outputs are compared with oracle/ops.py under
test_gpu_ops.py's criteria (rel_err < 1e-2 for bf16, < 1e-5 for dw; every element within B.fwd_tol / B.dgrad_tol /
B.wgrad_tol; BN totals against the bf16 output, rtol 1e-5, atol 1e-3), every guard word must be unchanged and no
output may hold a NaN.

    A  the implicit GEMM's three tiles x split-K 1 / planned / forced, 297 pixels (ragged last tile at 64, 128, 256)
    B  stride 2 on the GEMM: odd extents (generic DGRAD, split-K), parity classes at both tiles and class orders,
       1x1 stride 2, the shortcut-fused class DGRAD
    C  the shortcut-fused forward on the GEMM at 64x64 and 128x128 tiles (sc_fuse=3)
    D  the GEMM weight gradient: tiles, uneven split shares, the fast row / image loaders on and off, xcd_remap=0
    E  short workspaces under the defaults: every tier tests/test_conv_route.py pins, and the queried size
    F  refusals: an error code and a message, outputs and workspace untouched
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import bounds as B
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
SCALE = 0.5
G, GC, NA = "GEMM", "GEMM_CLASSES", None


def conv3(n, h, w, c, k, stride=1):
    return (n, h, w, c, k, 3, 3, stride, 1)


def conv1(n, h, w, c, k, stride=2):
    return (n, h, w, c, k, 1, 1, stride, 0)


def _rand_bf16(shape, gen, scale=1.0):
    return O.bf16(gen.standard_normal(shape).astype(np.float32) * scale)


def _out_hw(shape):
    n, h, w, c, k, r, s, st, pad = shape
    return (h + 2 * pad - r) // st + 1, (w + 2 * pad - s) // st + 1


@functools.lru_cache(maxsize=None)
def _data(shape):
    """The operands of every entry point for one descriptor, drawn once (read-only afterwards)."""
    n, h, w, c, k, r, s, st, pad = shape
    p, q = _out_hw(shape)
    g = np.random.default_rng(zlib.crc32(repr(shape).encode()))
    d = {"x": _rand_bf16((n, h, w, c), g), "w": _rand_bf16((k, r, s, c), g, 0.05), "dy": _rand_bf16((n, p, q, k), g),
         "res": _rand_bf16((n, h, w, c), g), "wsc": _rand_bf16((k, 1, 1, c), g, 0.1), "dsc": _rand_bf16((n, p, q, k), g)}
    for v in d.values():
        v.setflags(write=False)
    return d


def _batch_operands(shape, nprob):
    D = _data(shape)
    return [np.roll(D["x"], i, axis=2) for i in range(nprob)], [np.roll(D["dy"], i, axis=2) for i in range(nprob)]


@functools.lru_cache(maxsize=None)
def _refs(shape, entry):
    """[(output name, float64 oracle, element-wise bound)] of one entry point, computed once per (shape, entry)."""
    n, h, w, c, k, r, s, st, pad = shape
    D = _data(shape)
    x, wt, dy, res, wsc, dsc = (D[v] for v in ("x", "w", "dy", "res", "wsc", "dsc"))
    if entry in ("fwd", "fwd_sc"):
        ref = O.conv2d_fwd(x, wt, st, pad)
        out = [("y", ref, B.fwd_tol(ref, x, wt, st, pad))]
        if entry == "fwd_sc":
            ref_sc = O.conv2d_fwd(x, wsc, 2, 0)
            out.append(("ysc", ref_sc, B.fwd_tol(ref_sc, x, wsc, 2, 0)))
        return out
    if entry in ("dgrad", "dgrad_res", "dgrad_sc"):
        ref = O.conv2d_dgrad(dy, wt, (h, w), st, pad)
        if entry == "dgrad_res":
            return [("dx", ref + res, B.dgrad_tol(ref + res, dy, wt, (h, w), st, pad, res=res))]
        if entry == "dgrad_sc":
            ref = ref + O.conv2d_dgrad(dsc, wsc, (h, w), 2, 0)
            return [("dx", ref, B.dgrad_tol(ref, dy, wt, (h, w), st, pad, dsc=dsc, wsc=wsc))]
        return [("dx", ref, B.dgrad_tol(ref, dy, wt, (h, w), st, pad))]
    if entry in ("wgrad", "wgrad_sc"):
        out = [("dw", SCALE * O.conv2d_wgrad(x, dy, r, s, st, pad), B.wgrad_tol(x, dy, r, s, st, pad, SCALE))]
        if entry == "wgrad_sc":
            out.append(("dw_sc", SCALE * O.conv2d_wgrad(x, dsc, 1, 1, 2, 0).reshape(k, c),
                        B.wgrad_tol(x, dsc, 1, 1, 2, 0, SCALE).reshape(k, c)))
        return out
    assert entry.startswith("wgrad_batch")
    xs, dys = _batch_operands(shape, int(entry[-1]))
    return [(f"dw{i}", SCALE * O.conv2d_wgrad(xi, dyi, 3, 3, 1, 1), B.wgrad_tol(xi, dyi, 3, 3, 1, 1, SCALE))
            for i, (xi, dyi) in enumerate(zip(xs, dys))]


def _request(entry):
    """(pass, res, sc, nprob) of dtc_conv2d_route_query for an entry point."""
    return {"fwd": (0, False, False, 1), "fwd_sc": (0, False, True, 1), "dgrad": (1, False, False, 1),
            "dgrad_res": (1, True, False, 1), "dgrad_sc": (1, False, True, 1), "wgrad": (2, False, False, 1),
            "wgrad_sc": (2, False, True, 1)}.get(entry) or (2, False, False, int(entry[-1]))


def _queried_size(dtc, shape, entry):
    lib, d = dtc._native.lib, dtc.ops.conv_desc(*shape)
    mode, _, sc, nprob = _request(entry)
    if entry in ("fwd_sc", "dgrad_sc"):
        return 0
    if sc:
        return lib.dtc_conv2d_wgrad_sc_workspace_size(d)
    return lib.dtc_conv2d_wgrad_batch_workspace_size(d, nprob) if nprob > 1 else lib.dtc_conv2d_workspace_size(d, mode)


class _Moat:
    """Arena allocation: inputs, outputs (left at the NaN pattern), zeroed statistics, the workspace."""

    def __init__(self, dtc, dev):
        self.dtc, self.dev, self.arenas, self.written = dtc, dev, [], []

    def _new(self, *a, written=False, **k):
        ar, view = B.arena(*a, **k)
        self.arenas.append(ar)
        if written:
            self.written.append(ar)
        return view

    def inp(self, a, dtype=BF):
        t = torch.from_numpy(np.array(a)).to(self.dev).to(dtype)  # (a copy: the cached operands are read-only)
        return self._new(t.shape, dtype, self.dev, like=t)

    def out(self, shape, dtype=BF):
        return self._new(shape, dtype, self.dev, written=True)

    def stats(self, c):
        return self._new((int(self.dtc._native.lib.dtc_bn_stat_words(c)),), torch.int64, self.dev, zero=True)

    def ws(self, nbytes):
        if nbytes == 0:
            return None
        assert nbytes % 4 == 0
        return self._new((nbytes // 4,), F32, self.dev, written=True)

    def check(self):
        torch.cuda.synchronize()
        dirty = {i: a.dirty() for i, a in enumerate(self.arenas)}
        assert not any(dirty.values()), f"guard words overwritten (arena index: count): " \
                                        f"{ {i: n for i, n in dirty.items() if n} }"

    def untouched(self):
        """No word of any output or workspace arena, interior included, has changed."""
        torch.cuda.synchronize()
        return all(int((a.bits != a.pat).sum().item()) == 0 for a in self.written)


def _launch(dtc, dev, shape, entry, nbytes):
    """Call the entry point's C function on arenas with a workspace of exactly `nbytes` (a multiple of 4; a size with
    a ragged byte is rounded up for the allocation and passed as stated). Returns (rc, {name: tensor},
    {name: (statistics, channels)}, moat)."""
    N, lib = dtc._native, dtc._native.lib
    n, h, w, c, k, r, s, st, pad = shape
    p, q = _out_hw(shape)
    D, m = _data(shape), _Moat(dtc, dev)
    d, ptr, sp = dtc.ops.conv_desc(*shape), N.ptr, N.stream_ptr()
    ws = m.ws((nbytes + 3) // 4 * 4)
    outs, stats = {}, {}
    if entry == "fwd":
        outs["y"], stats["y"] = m.out((n, p, q, k)), (m.stats(k), k)
        rc = lib.dtc_conv2d_fwd(d, ptr(m.inp(D["x"])), ptr(m.inp(D["w"])), ptr(outs["y"]), ptr(stats["y"][0]), ptr(ws),
                                nbytes, sp)
    elif entry == "fwd_sc":
        outs["y"], outs["ysc"] = m.out((n, p, q, k)), m.out((n, p, q, k))
        stats["y"], stats["ysc"] = (m.stats(k), k), (m.stats(k), k)
        rc = lib.dtc_conv2d_fwd_sc(d, ptr(m.inp(D["x"])), ptr(m.inp(D["w"])), ptr(outs["y"]), ptr(stats["y"][0]),
                                   ptr(m.inp(D["wsc"].reshape(k, c))), ptr(outs["ysc"]), ptr(stats["ysc"][0]), sp)
    elif entry in ("dgrad", "dgrad_res"):
        outs["dx"] = m.out((n, h, w, c))
        res = m.inp(D["res"]) if entry == "dgrad_res" else None
        rc = lib.dtc_conv2d_dgrad(d, ptr(m.inp(D["dy"])), ptr(m.inp(D["w"])), ptr(outs["dx"]), ptr(res), ptr(ws), nbytes, sp)
    elif entry == "dgrad_sc":
        outs["dx"] = m.out((n, h, w, c))
        rc = lib.dtc_conv2d_dgrad_sc(d, ptr(m.inp(D["dy"])), ptr(m.inp(D["w"])), ptr(outs["dx"]), ptr(m.inp(D["dsc"])),
                                     ptr(m.inp(D["wsc"].reshape(k, c))), sp)
    elif entry == "wgrad":
        outs["dw"] = m.out((k, r, s, c), F32)
        rc = lib.dtc_conv2d_wgrad(d, ptr(m.inp(D["x"])), ptr(m.inp(D["dy"])), ptr(outs["dw"]), SCALE, ptr(ws), nbytes, sp)
    elif entry == "wgrad_sc":
        outs["dw"], outs["dw_sc"] = m.out((k, 3, 3, c), F32), m.out((k, c), F32)
        rc = lib.dtc_conv2d_wgrad_sc(d, ptr(m.inp(D["x"])), ptr(m.inp(D["dy"])), ptr(m.inp(D["dsc"])), ptr(outs["dw"]),
                                     ptr(outs["dw_sc"]), SCALE, ptr(ws), nbytes, sp)
    else:
        nprob = int(entry[-1])
        xs, dys = _batch_operands(shape, nprob)
        for i in range(nprob):
            outs[f"dw{i}"] = m.out((k, 3, 3, c), F32)
        arr = C.c_void_p * nprob
        rc = lib.dtc_conv2d_wgrad_batch(d, nprob, arr(*[ptr(m.inp(v)) for v in xs]), arr(*[ptr(m.inp(v)) for v in dys]),
                                        arr(*[ptr(outs[f"dw{i}"]) for i in range(nprob)]), SCALE, ptr(ws), nbytes, sp)
    return rc, outs, stats, m


class _Options:
    def __init__(self, lib, opts):
        self.lib, self.opts, self.saved = lib, opts, {}

    def __enter__(self):
        for k_, v in self.opts.items():
            self.saved[k_] = self.lib.dtc_get_option(k_.encode())
            assert self.lib.dtc_set_option(k_.encode(), int(v)) == 0, k_

    def __exit__(self, *exc):
        for k_, v in self.saved.items():
            self.lib.dtc_set_option(k_.encode(), v)


def _route(dtc, shape, entry, nbytes, ws_ptr=1 << 20):
    mode, res, sc, nprob = _request(entry)
    return dtc.ops.conv_route_info(dtc.ops.conv_desc(*shape), mode, res=res, sc=sc, nprob=nprob,
                                   ws=ws_ptr if nbytes else None, ws_bytes=nbytes)


def _assert_route(route, expect, what):
    kernel, tile, splits = expect[:3]
    got = (route["kernel"], (route["gemm_bm"], route["gemm_bn"]) if tile is not None else None, route["splits"])
    assert got == (kernel, tile, splits), f"{what}: the router plans {route}"
    for key, v in (expect[3] if len(expect) > 3 else {}).items():
        assert route[key] == v, f"{what}: {key} {route[key]} (expected {v}): {route}"


def _compare(dtc, name, shape, entry, outs, stats):
    worst = 0.0
    for what, ref, tol in _refs(shape, entry):
        got = outs[what].float().cpu().numpy()
        assert not np.isnan(got).any(), f"{name} {what}: NaN"
        assert rel_err(got, ref) < (1e-5 if what.startswith("dw") else 1e-2), f"{name} {what}"
        worst = max(worst, B.assert_within(got, ref, tol, f"{name} {what}"))
        if what in stats:  # BN statistics of the bf16 output
            st, ch = stats[what]
            tot = dtc.ops.stat_totals(st, ch).numpy()
            yb = got.reshape(-1, ch).astype(np.float64)
            np.testing.assert_allclose(tot[0], yb.sum(0), rtol=1e-5, atol=1e-3)
            np.testing.assert_allclose(tot[1], (yb * yb).sum(0), rtol=1e-5, atol=1e-3)
    print(f"conv-route {name}: worst |err|/tol {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------ cases
# (group, options, shape, entry, workspace bytes (None: the entry point's size query), (kernel, tile, splits[, more]))
GEMM_ONLY = {"halo_conv": 0, "conv_c64": 0}
SA, SA64 = conv3(3, 9, 11, 128, 128), conv3(3, 9, 11, 128, 64)
TILES = {1: (64, 64), 2: (128, 128), 3: (64, 256)}
CASES = []
for tile in (1, 2, 3):
    for split, planned in ((1, 1), (0, 2), (3, 3)):
        for entry in ("fwd", "dgrad", "dgrad_res"):
            CASES.append(("A", dict(GEMM_ONLY, igemm_tile=tile, igemm_split=split), SA, entry, None,
                          (G, TILES[tile], planned)))
CASES.append(("A", dict(GEMM_ONLY, igemm_tile=3), SA64, "fwd", None, (G, (64, 256), 2)))

S2_GEMM = dict(GEMM_ONLY, halo_s2=0, dgrad_s2h=0)
SB_ODD, SB_EVEN, SB_1X1 = conv3(3, 9, 11, 128, 256, 2), conv3(2, 8, 12, 128, 256, 2), conv1(2, 8, 12, 128, 256)
CASES += [("B", S2_GEMM, SB_ODD, "fwd", None, (G, (64, 64), 2)),
          ("B", S2_GEMM, SB_ODD, "dgrad", None, (G, (64, 64), 4)),  # odd extents: the generic stride-2 DGRAD
          ("B", S2_GEMM, SB_ODD, "dgrad_res", None, (G, (64, 64), 4)),
          ("B", S2_GEMM, SB_EVEN, "fwd", None, (G, (64, 64), 2)),
          ("B", S2_GEMM, SB_1X1, "fwd", None, (G, (64, 64), 1)),
          ("B", S2_GEMM, SB_1X1, "dgrad", None, (GC, (64, 64), 1))]
for tile in (0, 2):
    for order in (0, 1):
        for entry in ("dgrad", "dgrad_res"):
            CASES.append(("B", dict(S2_GEMM, igemm_tile=tile, dgrad_class_order=order), SB_EVEN, entry, None,
                          (GC, TILES[tile or 1], 1)))
    CASES.append(("B", dict(S2_GEMM, igemm_tile=tile), SB_EVEN, "dgrad_sc", None, (GC, TILES[tile or 1], 1, {"sc_ok": 1})))

for tile in (0, 2):
    for shape in (SB_EVEN, SB_ODD):
        CASES.append(("C", {"halo_s2": 0, "sc_fuse": 3, "igemm_split": 1, "igemm_tile": tile}, shape, "fwd_sc", None,
                      (G, TILES[tile or 1], 1, {"sc_ok": 1})))

WG_GEMM = {"wgrad_halo": 0, "wgrad_s2": 0}
WG_ODD = conv3(24, 9, 11, 64, 64)
for tile in (1, 2):
    for split in (1, 3):  # 297 pixels: 5 reduction steps, shared 2, 2, 1
        CASES.append(("D", dict(WG_GEMM, igemm_tile=tile, igemm_split=split), SA, "wgrad", None, (G, TILES[tile], split)))
CASES.append(("D", WG_GEMM, WG_ODD, "wgrad", None, (G, (64, 64), 4)))  # 38 steps, 4 splits planned
for shape in (conv3(4, 8, 8, 128, 128), conv3(4, 4, 4, 128, 128)):  # the wg_fast row and image loaders
    for fast in (0, 1):
        CASES.append(("D", dict(WG_GEMM, wgrad_fast=fast), shape, "wgrad", None, (G, (64, 64), None)))
CASES.append(("D", dict(WG_GEMM, xcd_remap=0), SA, "wgrad", None, (G, (64, 64), None)))

HALO_A, HALO_B, GEMM_S = conv3(5, 8, 8, 256, 256), conv3(9, 4, 4, 512, 256), conv3(3, 7, 7, 256, 256)
WG_S2, WG_L1, WG_B3 = conv3(16, 16, 16, 64, 128, 2), conv3(16, 16, 16, 64, 64), conv3(2, 14, 28, 128, 128)
for entry in ("fwd", "dgrad_res"):
    CASES += [("E", {}, HALO_A, entry, None, ("HALO", NA, 2, {"halo_cfg": 7, "reduce_in_kernel": 1, "slab_used": 655360})),
              ("E", {}, HALO_A, entry, 1310720, ("HALO", NA, 2, {"reduce_in_kernel": 0, "slab_used": 655360})),
              ("E", {}, HALO_A, entry, 655360, ("HALO", NA, 2, {"reduce_in_kernel": 0, "slab_used": 655360})),
              ("E", {}, HALO_A, entry, 655356, ("HALO", NA, 1, {"slab_used": 0})),
              ("E", {}, HALO_A, entry, 0, ("HALO", NA, 1, {"slab_used": 0})),
              ("E", {}, HALO_B, entry, None, ("HALO", NA, 4 if entry == "fwd" else 2,  # (DGRAD reduces over K = 256)
                                              {"halo_cfg": 7, "reduce_in_kernel": 1})),
              ("E", {}, HALO_B, entry, 0, ("HALO", NA, 1, {"slab_used": 0})),
              ("E", {}, GEMM_S, entry, None, (G, (64, 64), 4, {"slab_used": 602112})),
              ("E", {}, GEMM_S, entry, 602112, (G, (64, 64), 4, {"slab_used": 602112})),
              ("E", {}, GEMM_S, entry, 602108, (G, (64, 64), 1, {"slab_used": 0})),
              ("E", {}, GEMM_S, entry, 0, (G, (64, 64), 1, {"slab_used": 0}))]
CASES += [("E", {}, HALO_B, "fwd", 1327104, ("HALO", NA, 4, {"reduce_in_kernel": 0, "slab_used": 589824})),
          ("E", {}, WG_S2, "wgrad", None, ("WGRAD_S2", NA, 4, {"slab_used": 1310720})),
          ("E", {}, WG_S2, "wgrad", 1310720, ("WGRAD_S2", NA, 4, {"slab_used": 1310720})),
          ("E", {}, WG_S2, "wgrad", 1310716, (G, (64, 64), 4, {"slab_used": 1179648})),
          ("E", {}, WG_S2, "wgrad", 884740, (G, (64, 64), 3, {"slab_used": 884736})),
          ("E", {}, WG_S2, "wgrad", 589824, (G, (64, 64), 2, {"slab_used": 589824})),
          ("E", {}, WG_S2, "wgrad", 294912, (G, (64, 64), 1, {"slab_used": 294912})),
          ("E", {}, WG_S2, "wgrad_sc", None, ("WGRAD_S2", NA, 4, {"slab_used": 1310720, "sc_ok": 1})),
          ("E", {}, WG_L1, "wgrad", None, ("WGRAD_HALO", NA, 2, {"slab_used": 294912})),
          ("E", {}, WG_L1, "wgrad", 294908, (G, (64, 64), 1, {"slab_used": 147456})),
          ("E", {}, WG_L1, "wgrad", 147456, (G, (64, 64), 1, {"slab_used": 147456})),
          ("E", {}, WG_ODD, "wgrad", None, (G, (64, 64), 4, {"slab_used": 589824})),
          ("E", {}, WG_ODD, "wgrad", 589820, (G, (64, 64), 3, {"slab_used": 442368})),
          ("E", {}, WG_B3, "wgrad_batch3", 1769472, ("WGRAD_HALO", NA, 1, {"slab_used": 0}))]


def _case_id(c):
    group, opts, shape, entry, nbytes = c[:5]
    o = ",".join(f"{k}={v}" for k, v in opts.items() if k not in GEMM_ONLY) or "defaults"
    return f"{group}-{'x'.join(map(str, shape[:5]))}-r{shape[5]}s{shape[7]}-{entry}-{o}-ws{'full' if nbytes is None else nbytes}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_route_against_oracle(dtc, cuda, case):
    group, opts, shape, entry, nbytes, expect = case
    lib, name = dtc._native.lib, _case_id(case)
    with _Options(lib, opts):
        if nbytes is None:
            nbytes = _queried_size(dtc, shape, entry)
        if expect[2] is None:  # split count left to the planner (the case is about the loader / tile order)
            expect = expect[:2] + (_route(dtc, shape, entry, nbytes)["splits"],) + expect[3:]
        route = _route(dtc, shape, entry, nbytes)
        _assert_route(route, expect, name)
        assert route["refused"] == 0 and route["slab_used"] <= nbytes, route
        rc, outs, stats, moat = _launch(dtc, cuda, shape, entry, nbytes)
        assert rc == 0, f"{name}: {dtc._native.last_error()}"
        moat.check()
    _compare(dtc, name, shape, entry, outs, stats)


@pytest.mark.parametrize("shape", [HALO_A, HALO_B], ids=["5x8x8x256x256", "9x4x4x512x256"])
@pytest.mark.parametrize("entry", ["fwd", "dgrad_res"])
def test_halo_split_k_tiers_are_bit_identical(dtc, cuda, shape, entry):
    """The same split-K plan reduced three ways gives the same bits: by a separate splitk_reduce launch because only
    the slab is on hand, in the kernel with the queried size, and by the reduce launch because splitk_ink is off
    (test_conv_halo_splitk_in_kernel_matches_reduce_launch states this for full workspaces only). Bit-identical are the
    bf16 outputs; the BN statistics are held as that test holds them."""
    lib = dtc._native.lib
    full = _queried_size(dtc, shape, entry)
    want = _route(dtc, shape, entry, full)["slab_wanted"]
    runs = {}
    for tier, nbytes, opts, ink in (("slab only", want, {}, 0), ("queried size", full, {}, 1),
                                    ("splitk_ink=0", full, {"splitk_ink": 0}, 0)):
        with _Options(lib, opts):
            route = _route(dtc, shape, entry, nbytes)
            assert route["kernel"] == "HALO" and route["splits"] > 1 and route["reduce_in_kernel"] == ink, (tier, route)
            rc, outs, stats, moat = _launch(dtc, cuda, shape, entry, nbytes)
            assert rc == 0, dtc._native.last_error()
            moat.check()
        runs[tier] = (outs, stats)
    (o0, s0) = runs["slab only"]
    for tier in ("queried size", "splitk_ink=0"):
        o1, s1 = runs[tier]
        for what in o0:
            assert not torch.isnan(o0[what]).any()
            assert torch.equal(o0[what].view(torch.int16), o1[what].view(torch.int16)), f"{tier}: {what} differs"
        for what in s0:  # BN statistics: the same bf16 values summed; the two reduce launches group their fp32
            # partials alike (equal totals), the in-kernel reduction groups them per workgroup (the bound of
            # test_conv_halo_splitk_in_kernel_matches_reduce_launch)
            a, b = dtc.ops.stat_totals(s1[what][0], s1[what][1]), dtc.ops.stat_totals(s0[what][0], s0[what][1])
            if tier == "splitk_ink=0":
                assert torch.equal(a, b), f"{tier}: statistics of {what} differ"
            else:
                assert ((a - b).abs() <= 2e-5 * b.abs().amax(1, keepdim=True) + 1e-6).all(), (a - b).abs().max()


REFUSALS = [(WG_S2, "wgrad", 294908), (WG_L1, "wgrad", 147452), (WG_L1, "wgrad", 0), (WG_B3, "wgrad_batch3", 1769468),
            (WG_S2, "wgrad_sc", -1)]  # -1: one byte less than dtc_conv2d_wgrad_sc_workspace_size returns


@pytest.mark.parametrize("shape,entry,nbytes", REFUSALS, ids=[f"F-{'x'.join(map(str, r[0][:5]))}-{r[1]}-ws{r[2]}" for r in REFUSALS])
def test_refusals_touch_nothing(dtc, cuda, shape, entry, nbytes):
    if nbytes < 0:
        nbytes = _queried_size(dtc, shape, entry) + nbytes
        assert nbytes > 0
    assert _route(dtc, shape, entry, nbytes)["refused"] == 1
    rc, outs, stats, moat = _launch(dtc, cuda, shape, entry, nbytes)
    assert rc != 0 and len(dtc._native.last_error()) > 0
    print(f"conv-route F {entry} ws{nbytes}: refused with '{dtc._native.last_error()}'")
    moat.check()
    assert moat.untouched(), "a refused call wrote to an output or to the workspace"
