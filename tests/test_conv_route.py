"""The conv router (csrc/conv_route.cpp) through dtc_conv2d_route_query: host code only, no GPU.

The query answers from the routing and workspace code the conv entry points themselves run (capi.cpp: ws_carve, then
conv_launch), so what is pinned here is what launches. Four parts:

* the fit property over a thinned grid of shapes x option sets x bytes on hand: a launch that is not refused writes
  no more slab than is on hand, and never more than the pass wants; the size query's bytes give the unlimited route;
* the order of precedence of DESIGN.md §7m, one assertion per table cell (a partial `dw` -- the WGRAD cell "whole
  dw" -- is not expressible through the C ABI, whose dtc_conv2d_wgrad always writes whole rows, so it is left out);
* the default routes of the ten residual-layer descriptors at batch 256 on 32x32 and batch 8 on 224x224;
* the exact short-workspace tiers of seven shapes, and the shortcut-fused forward's refusal of split-K plans.
"""
import ctypes as C

import pytest

FWD, DGRAD, WGRAD = 0, 1, 2
WS = 1 << 20  # a workspace address: the query never dereferences it (nothing is mapped there)


class Options:
    def __init__(self, lib, opts):
        self.lib, self.opts, self.saved = lib, opts, {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.saved[k] = self.lib.dtc_get_option(k.encode())
            assert self.lib.dtc_set_option(k.encode(), int(v)) == 0, k

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.lib.dtc_set_option(k.encode(), v)


def conv3(n, h, w, c, k, stride=1):
    return (n, h, w, c, k, 3, 3, stride, 1)


def info(dtc, shape, mode, nbytes=None, **kw):
    """The route for `nbytes` on hand (None: the pass's size query), as ops.conv_route_info's dict."""
    d = dtc.ops.conv_desc(*shape)
    if nbytes is None:
        nbytes = dtc._native.lib.dtc_conv2d_workspace_size(d, mode)
    return dtc.ops.conv_route_info(d, mode, ws=WS if nbytes else None, ws_bytes=nbytes, **kw)


# ------------------------------------------------------------------------------------------------ the fit property
OPTION_SETS = [{}, {"halo_split": 2}, {"halo_split": 4}, {"igemm_split": 2}, {"igemm_split": 5}, {"halo_conv": 0},
               {"halo_conv": 0, "conv_c64": 0}, {"wgrad_halo": 0}, {"wgrad_s2": 0}, {"wgrad_s2": 2}, {"halo_s2": 0},
               {"dgrad_classes": 0}, {"igemm_tile": 1}, {"igemm_tile": 2}, {"igemm_tile": 3}, {"halo_small": 0},
               {"wgrad_halo": 2048}, {"wgrad_s2_wgs": 1024}, {"conv_c64": 2}, {"dgrad_s2h": 2}]
GRID = [(n, h, w, c, k) + geo
        for n in (1, 2, 3, 5, 8, 12, 32, 256) for h in (1, 3, 4, 7, 8, 16, 32) for w in sorted({h, h + 1, 2 * h})
        for c in (64, 128, 256, 512) for k in (64, 128, 512)
        for geo in ((3, 3, 1, 1), (3, 3, 2, 1), (1, 1, 2, 0), (1, 1, 1, 0))]
THIN = 29  # option set j sees the shapes i of the full grid with i % THIN == j % THIN: every shape of the grid is
# visited, each option set sees ~1/29 of them spread over every axis (29 is coprime to the axes' lengths), and the
# file stays well under a minute (the full grid was probed host-side when the router was written: 0 violations)


def _requests(shape):
    """(pass, flags, nprob) of every entry point that takes a workspace."""
    out = [(FWD, 0, 1), (DGRAD, 0, 1), (DGRAD, 1, 1)] + [(WGRAD, 0, n) for n in (1, 2, 3, 4)]
    if shape[5] == 3 and shape[7] == 2:
        out.append((WGRAD, 2, 1))
    return out


@pytest.mark.parametrize("j", range(len(OPTION_SETS)), ids=lambda j: ",".join(f"{k}={v}" for k, v in
                                                                             OPTION_SETS[j].items()) or "defaults")
def test_launches_fit_the_workspace_on_hand(dtc, j):
    lib, N = dtc._native.lib, dtc._native
    q, r, r0 = lib.dtc_conv2d_route_query, N.ConvRoute(), N.ConvRoute()
    routes = 0
    with Options(lib, OPTION_SETS[j]):
        for i in range(j % THIN, len(GRID), THIN):
            shape = GRID[i]
            d = N.ConvDesc(*shape)
            per = shape[4] * shape[5] * shape[6] * shape[3] * 4
            for mode, flags, nprob in _requests(shape):
                assert q(d, mode, flags, nprob, WS, C.c_size_t(-1).value >> 1, C.byref(r0)) == 0, N.last_error()
                want = r0.slab_wanted
                for nb in (0, per - 4, per, 2 * per, 3 * per + 4, want // 2, want - 4, want, want + 4):
                    nb = max(nb, 0)
                    assert q(d, mode, flags, nprob, WS if nb else None, nb, C.byref(r)) == 0, N.last_error()
                    routes += 1
                    what = (shape, OPTION_SETS[j], mode, flags, nprob, nb)
                    assert r.refused == 1 or r.slab_used <= nb, what
                    assert r.slab_used <= r.slab_wanted and r.slab_wanted == want, what
                # the size query's bytes (at an address that is not 256-byte aligned) give the unlimited route
                size = lib.dtc_conv2d_wgrad_sc_workspace_size(d) if flags == 2 else \
                    lib.dtc_conv2d_wgrad_batch_workspace_size(d, nprob) if nprob > 1 else \
                    lib.dtc_conv2d_workspace_size(d, mode)
                if nprob > 1 or flags == 2:
                    assert (size == 0) == bool(r0.refused), (shape, mode, flags, nprob)
                if r0.refused:
                    continue
                assert q(d, mode, flags, nprob, WS + 4 if size else None, size, C.byref(r)) == 0
                assert (r.kernel, r.splits, r.gemm_bm, r.gemm_bn, r.halo_cfg, r.refused, r.slab_used) == \
                       (r0.kernel, r0.splits, r0.gemm_bm, r0.gemm_bn, r0.halo_cfg, 0, r0.slab_used), (shape, mode, flags, nprob)
                assert r.slab_used <= size
    assert routes > 10000


# ------------------------------------------------------------------------------------------------ precedence (§7m)
L1 = conv3(256, 32, 32, 64, 64)        # layer1 at batch 256 (conv_c64=1 takes it from a tile per workgroup up)
S2 = conv3(256, 16, 16, 128, 256, 2)   # layer3.0.conv1 at batch 256: conv1 of a projection block, even extents


def test_precedence_fwd(dtc):
    lib = dtc._native.lib
    assert info(dtc, L1, FWD)["kernel"] == "C64"
    with Options(lib, {"conv_c64": 0}):
        assert info(dtc, L1, FWD)["kernel"] == "HALO"
        with Options(lib, {"halo_conv": 0}):
            assert info(dtc, L1, FWD)["kernel"] == "GEMM"
    assert info(dtc, S2, FWD)["kernel"] == "HALO"  # the stride-2 column-split kernel
    with Options(lib, {"halo_s2": 0}):
        assert info(dtc, S2, FWD)["kernel"] == "GEMM"


def test_precedence_dgrad(dtc):
    lib = dtc._native.lib
    for res in (False, True):
        assert info(dtc, L1, DGRAD, res=res)["kernel"] == "C64"
        with Options(lib, {"conv_c64": 0}):
            assert info(dtc, L1, DGRAD, res=res)["kernel"] == "HALO"
            with Options(lib, {"halo_conv": 0}):
                assert info(dtc, L1, DGRAD, res=res)["kernel"] == "GEMM"
    # stride 2, even extents: the sub-pixel halo without a residual or with the fused shortcut, else the classes
    assert info(dtc, S2, DGRAD)["kernel"] == "DGRAD_S2"
    assert info(dtc, S2, DGRAD, sc=True)["kernel"] == "DGRAD_S2"
    assert info(dtc, S2, DGRAD, res=True)["kernel"] == "GEMM_CLASSES"
    with Options(lib, {"dgrad_s2h": 0}):
        assert info(dtc, S2, DGRAD)["kernel"] == "GEMM_CLASSES"
        sc = info(dtc, S2, DGRAD, sc=True)
        assert sc["kernel"] == "GEMM_CLASSES" and sc["sc_ok"] == 1 and sc["refused"] == 0
        with Options(lib, {"dgrad_scf": 0}):
            assert info(dtc, S2, DGRAD, sc=True)["refused"] == 1
    with Options(lib, {"dgrad_classes": 0}):
        for res in (False, True):
            assert info(dtc, S2, DGRAD, res=res)["kernel"] == "GEMM"
        assert info(dtc, S2, DGRAD, sc=True)["refused"] == 1
    odd = conv3(3, 9, 11, 128, 256, 2)  # odd extents: no classes
    assert info(dtc, odd, DGRAD)["kernel"] == "GEMM" and info(dtc, odd, DGRAD, sc=True)["refused"] == 1


def test_residual_without_shortcut_never_takes_dgrad_s2(dtc):
    lib = dtc._native.lib
    for o in ({}, {"dgrad_s2h": 2}):
        with Options(lib, o):
            for shape in GRID[::7]:
                if shape[7] == 2:
                    assert info(dtc, shape, DGRAD, res=True)["kernel"] != "DGRAD_S2", (shape, o)


def test_precedence_wgrad(dtc):
    lib = dtc._native.lib
    s1 = conv3(8, 16, 16, 128, 128)
    assert info(dtc, S2, WGRAD)["kernel"] == "WGRAD_S2" and info(dtc, S2, WGRAD)["sc_ok"] == 1
    assert info(dtc, s1, WGRAD)["kernel"] == "WGRAD_HALO"
    with Options(lib, {"wgrad_s2": 0}):
        assert info(dtc, S2, WGRAD)["kernel"] == "GEMM"
        assert info(dtc, S2, WGRAD, sc=True)["refused"] == 1
    with Options(lib, {"wgrad_halo": 0}):
        assert info(dtc, s1, WGRAD)["kernel"] == "GEMM"
        assert info(dtc, s1, WGRAD, nprob=2, nbytes=1 << 30)["refused"] == 1  # wgrad_batch without a halo route
    for n in (2, 3, 4):
        for shape in GRID[::5]:  # several problems never take the stride-2 kernel, whatever the slab
            assert info(dtc, shape, WGRAD, nprob=n, nbytes=1 << 34)["kernel"] != "WGRAD_S2", (shape, n)
    # slab not on hand: 64x64 GEMM tiles (the tiers below pin the split counts)
    short = info(dtc, s1, WGRAD, nbytes=info(dtc, s1, WGRAD)["slab_wanted"] - 4)
    assert (short["kernel"], short["gemm_bm"], short["gemm_bn"]) == ("GEMM", 64, 64)


# ------------------------------------------------------------------------------------------------ default routes
# What dtc_conv2d_route_query returned, with each pass's queried workspace, when it was added on top of commit
# 3d00f71 (conv_route itself unchanged since 2b721c6, the commit that introduced it): per descriptor the routes of
# FWD, DGRAD, DGRAD + residual, WGRAD as (kernel, gemm_bm, gemm_bn, splits, halo_cfg, halo_gen). They agree with §7m's
# order: layer1 on conv_c64; the stride-1 convs of layers 2-4 on conv_halo (general geometry at 224x224); conv1 of a
# projection block forward on the column-split halo kernel where its tiles fit (32x32 layers 3-4) else the GEMM, its
# dgrad on the sub-pixel halo (K <= 256, no residual) else the parity classes; the 1x1 shortcuts on the GEMM.
G, GC, NA = "GEMM", "GEMM_CLASSES", (0, 0)
DEFAULT_ROUTES = [
    ((256, 32, 32, 64, 64, 3, 3, 1, 1), ("C64", 0, 0, 1, -1, 0), ("C64", 0, 0, 1, -1, 0), ("C64", 0, 0, 1, -1, 0), ("WGRAD_HALO", 0, 0, 170, -1, 0)),
    ((256, 32, 32, 64, 128, 3, 3, 2, 1), (G, 128, 128, 1, -1, 0), ("DGRAD_S2", 0, 0, 1, -1, 0), (GC, 64, 64, 1, -1, 0), ("WGRAD_S2", 0, 0, 64, -1, 0)),
    ((256, 32, 32, 64, 128, 1, 1, 2, 0), (G, 128, 128, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (G, 64, 64, 128, -1, 0)),
    ((256, 16, 16, 128, 128, 3, 3, 1, 1), ("HALO", 0, 0, 1, 0, 0), ("HALO", 0, 0, 1, 0, 0), ("HALO", 0, 0, 1, 0, 0), ("WGRAD_HALO", 0, 0, 42, -1, 0)),
    ((256, 16, 16, 128, 256, 3, 3, 2, 1), ("HALO", 0, 0, 1, 8, 0), ("DGRAD_S2", 0, 0, 1, -1, 0), (GC, 64, 64, 1, -1, 0), ("WGRAD_S2", 0, 0, 16, -1, 0)),
    ((256, 16, 16, 128, 256, 1, 1, 2, 0), (G, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (G, 64, 64, 32, -1, 0)),
    ((256, 8, 8, 256, 256, 3, 3, 1, 1), ("HALO", 0, 0, 1, 2, 0), ("HALO", 0, 0, 1, 2, 0), ("HALO", 0, 0, 1, 2, 0), ("WGRAD_HALO", 0, 0, 10, -1, 0)),
    ((256, 8, 8, 256, 512, 3, 3, 2, 1), ("HALO", 0, 0, 1, 8, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), ("WGRAD_S2", 0, 0, 4, -1, 0)),
    ((256, 8, 8, 256, 512, 1, 1, 2, 0), (G, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (G, 64, 64, 8, -1, 0)),
    ((256, 4, 4, 512, 512, 3, 3, 1, 1), ("HALO", 0, 0, 1, 7, 0), ("HALO", 0, 0, 1, 7, 0), ("HALO", 0, 0, 1, 7, 0), ("WGRAD_HALO", 0, 0, 2, -1, 0)),
    ((8, 224, 224, 64, 64, 3, 3, 1, 1), ("C64", 0, 0, 1, -1, 0), ("C64", 0, 0, 1, -1, 0), ("C64", 0, 0, 1, -1, 0), ("WGRAD_HALO", 0, 0, 224, -1, 0)),
    ((8, 224, 224, 64, 128, 3, 3, 2, 1), (G, 128, 128, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), ("WGRAD_S2", 0, 0, 64, -1, 0)),
    ((8, 224, 224, 64, 128, 1, 1, 2, 0), (G, 128, 128, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (G, 64, 64, 196, -1, 0)),
    ((8, 112, 112, 128, 128, 3, 3, 1, 1), ("HALO", 0, 0, 1, 0, 1), ("HALO", 0, 0, 1, 0, 1), ("HALO", 0, 0, 1, 0, 1), ("WGRAD_HALO", 0, 0, 56, -1, 0)),
    ((8, 112, 112, 128, 256, 3, 3, 2, 1), (G, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), ("WGRAD_S2", 0, 0, 16, -1, 0)),
    ((8, 112, 112, 128, 256, 1, 1, 2, 0), (G, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (G, 64, 64, 49, -1, 0)),
    ((8, 56, 56, 256, 256, 3, 3, 1, 1), ("HALO", 0, 0, 1, 2, 1), ("HALO", 0, 0, 1, 2, 1), ("HALO", 0, 0, 1, 2, 1), ("WGRAD_HALO", 0, 0, 14, -1, 0)),
    ((8, 56, 56, 256, 512, 3, 3, 2, 1), (G, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), ("WGRAD_S2", 0, 0, 4, -1, 0)),
    ((8, 56, 56, 256, 512, 1, 1, 2, 0), (G, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (GC, 64, 64, 1, -1, 0), (G, 64, 64, 11, -1, 0)),
    ((8, 28, 28, 512, 512, 3, 3, 1, 1), ("HALO", 0, 0, 1, 2, 1), ("HALO", 0, 0, 1, 2, 1), ("HALO", 0, 0, 1, 2, 1), ("WGRAD_HALO", 0, 0, 3, -1, 0)),
]


def _sig(r):
    return (r["kernel"], r["gemm_bm"], r["gemm_bn"], r["splits"], r["halo_cfg"], r["halo_gen"])


@pytest.mark.parametrize("shape,fwd,dgrad,dgrad_res,wgrad", DEFAULT_ROUTES, ids=[str(c[0]) for c in DEFAULT_ROUTES])
def test_default_routes_of_the_residual_layers(dtc, shape, fwd, dgrad, dgrad_res, wgrad):
    assert _sig(info(dtc, shape, FWD)) == fwd
    assert _sig(info(dtc, shape, DGRAD)) == dgrad
    assert _sig(info(dtc, shape, DGRAD, res=True)) == dgrad_res
    assert _sig(info(dtc, shape, WGRAD)) == wgrad


def test_default_route_table_covers_the_layer_descriptors():
    """The table's descriptors are the network's (the same construction as tools/conv_digest.py:layer_shapes)."""
    def layer_shapes(b, h):
        out, c = [(b, h, h, 64, 64, 3, 3, 1, 1)], 64
        for _ in range(3):
            out += [(b, h, h, c, 2 * c, 3, 3, 2, 1), (b, h, h, c, 2 * c, 1, 1, 2, 0),
                    (b, h // 2, h // 2, 2 * c, 2 * c, 3, 3, 1, 1)]
            c, h = 2 * c, h // 2
        return out
    assert [c[0] for c in DEFAULT_ROUTES] == layer_shapes(256, 32) + layer_shapes(8, 224)


# ------------------------------------------------------------------------------------------------ fallback tiers
# (shape, pass, request, [(bytes on hand, kernel, gemm tile, splits, slab_used, refused)]); defaults.
HALO_A, HALO_B, GEMM_S = conv3(5, 8, 8, 256, 256), conv3(9, 4, 4, 512, 256), conv3(3, 7, 7, 256, 256)
WG_S2, WG_L1, WG_ODD, WG_B3 = (conv3(16, 16, 16, 64, 128, 2), conv3(16, 16, 16, 64, 64), conv3(24, 9, 11, 64, 64),
                               conv3(2, 14, 28, 128, 128))
TIERS = [
    (HALO_A, FWD, {}, [(655360, "HALO", NA, 2, 655360, 0), (655356, "HALO", NA, 1, 0, 0), (0, "HALO", NA, 1, 0, 0)]),
    (HALO_A, DGRAD, {}, [(655360, "HALO", NA, 2, 655360, 0), (655356, "HALO", NA, 1, 0, 0), (0, "HALO", NA, 1, 0, 0)]),
    (HALO_A, DGRAD, {"res": True}, [(655360, "HALO", NA, 2, 655360, 0), (0, "HALO", NA, 1, 0, 0)]),
    (HALO_B, FWD, {}, [(1327104, "HALO", NA, 4, 589824, 0), (589824, "HALO", NA, 4, 589824, 0),
                       (589820, "HALO", NA, 1, 0, 0), (0, "HALO", NA, 1, 0, 0)]),
    (GEMM_S, FWD, {}, [(602112, G, (64, 64), 4, 602112, 0), (602108, G, (64, 64), 1, 0, 0), (0, G, (64, 64), 1, 0, 0)]),
    (GEMM_S, DGRAD, {}, [(602112, G, (64, 64), 4, 602112, 0), (602108, G, (64, 64), 1, 0, 0), (0, G, (64, 64), 1, 0, 0)]),
    (WG_S2, WGRAD, {}, [(1310720, "WGRAD_S2", NA, 4, 1310720, 0), (1310716, G, (64, 64), 4, 1179648, 0),
                        (884740, G, (64, 64), 3, 884736, 0), (589824, G, (64, 64), 2, 589824, 0),
                        (294912, G, (64, 64), 1, 294912, 0), (294908, G, (64, 64), 1, 0, 1)]),
    (WG_L1, WGRAD, {}, [(294912, "WGRAD_HALO", NA, 2, 294912, 0), (294908, G, (64, 64), 1, 147456, 0),
                        (147456, G, (64, 64), 1, 147456, 0), (147452, G, (64, 64), 1, 0, 1)]),
    (WG_ODD, WGRAD, {}, [(589824, G, (64, 64), 4, 589824, 0), (589820, G, (64, 64), 3, 442368, 0)]),
    # three problems, one split each: the halo kernel writes the dws itself (no slab), yet the entry point asks for
    # the bytes its size query returns
    (WG_B3, WGRAD, {"nprob": 3}, [(1769472, "WGRAD_HALO", NA, 1, 0, 0), (1769468, G, (64, 64), 1, 0, 1)]),
]


@pytest.mark.parametrize("shape,mode,req,tiers", TIERS, ids=[f"{t[0][:5]}-pass{t[1]}-{t[2]}" for t in TIERS])
def test_short_workspace_tiers(dtc, shape, mode, req, tiers):
    for nbytes, kernel, tile, splits, used, refused in tiers:
        r = info(dtc, shape, mode, nbytes=nbytes, **req)
        assert (r["kernel"], (r["gemm_bm"], r["gemm_bn"]), r["splits"], r["slab_used"], r["refused"]) == \
               (kernel, tile, splits, used, refused), (nbytes, r)


def test_halo_tiers_want_the_larger_slab_and_reduce_in_kernel_only_with_counters(dtc):
    lib = dtc._native.lib
    for shape, mode in ((HALO_A, FWD), (HALO_A, DGRAD), (HALO_B, FWD)):
        full = info(dtc, shape, mode)
        want = full["slab_wanted"]
        assert full["halo_cfg"] == 7 and full["reduce_in_kernel"] == 1 and full["splits"] > 1
        assert want == {HALO_A: 1310720, HALO_B: 1327104}[shape]  # max(the GEMM fallback's, the halo plan's)
        assert lib.dtc_conv2d_workspace_size(dtc.ops.conv_desc(*shape), mode) == want + 8192 * 4 + 256
        assert info(dtc, shape, mode, nbytes=want)["reduce_in_kernel"] == 0  # slab only: a separate reduce launch
        assert info(dtc, shape, mode, nbytes=want + 8192 * 4 - 4)["reduce_in_kernel"] == 0
        with Options(lib, {"splitk_ink": 0}):
            off = info(dtc, shape, mode)
            assert off["reduce_in_kernel"] == 0 and off["splits"] == full["splits"]


def test_fwd_sc_is_refused_where_the_gemm_plans_split_k(dtc):
    """Pinned as intended (conv_route.cpp: conv_launch): the fused forward has no slab, and it is offered only where
    the GEMM's PLAN is one split -- sc_ok is decided before the "no slab -> one split" demotion, so a shape whose
    plan wants split-K (a grid too small to fill the chip) is refused although one split could run; callers run the
    two convs separately there (dtc.h). Forcing one split (igemm_split=1) offers it."""
    lib = dtc._native.lib
    shape = conv3(3, 4, 4, 256, 512, 2)
    with Options(lib, {"halo_s2": 0}):
        plain = info(dtc, shape, FWD)
        assert plain["kernel"] == G and plain["splits"] > 1
        sc = info(dtc, shape, FWD, sc=True)
        assert (sc["kernel"], sc["splits"], sc["sc_ok"], sc["refused"], sc["slab_used"]) == (G, 1, 0, 1, 0)
        with Options(lib, {"igemm_split": 1}):
            sc = info(dtc, shape, FWD, sc=True)
            assert (sc["kernel"], sc["splits"], sc["sc_ok"], sc["refused"]) == (G, 1, 1, 0)
    sc = info(dtc, S2, FWD, sc=True)  # where the stride-2 halo kernel takes the shape it always fuses
    assert (sc["kernel"], sc["sc_ok"], sc["refused"]) == ("HALO", 1, 0)


def test_wgrad_sc_needs_the_bytes_its_size_query_returns(dtc):
    lib = dtc._native.lib
    d = dtc.ops.conv_desc(*WG_S2)
    size = lib.dtc_conv2d_wgrad_sc_workspace_size(d)
    assert size == 1310720 + 8192 * 4
    ok = dtc.ops.conv_route_info(d, WGRAD, sc=True, ws=WS, ws_bytes=size)
    assert (ok["kernel"], ok["splits"], ok["slab_used"], ok["refused"]) == ("WGRAD_S2", 4, 1310720, 0)
    for nbytes, ws in ((size - 1, WS), (size - 4, WS), (0, None)):
        assert dtc.ops.conv_route_info(d, WGRAD, sc=True, ws=ws, ws_bytes=nbytes)["refused"] == 1


def test_route_query_rejects_what_names_no_entry_point(dtc):
    lib, N = dtc._native.lib, dtc._native
    r = N.ConvRoute()
    d = N.ConvDesc(*L1)
    bad = N.ConvDesc(8, 32, 32, 3, 64, 3, 3, 1, 1)
    assert lib.dtc_conv2d_route_query(bad, 0, 0, 1, None, 0, C.byref(r)) != 0
    assert b"unsupported convolution descriptor" in lib.dtc_last_error()
    for mode, flags, nprob in ((3, 0, 1), (-1, 0, 1), (0, 1, 1), (2, 1, 1), (0, 0, 2), (2, 2, 2), (2, 0, 5), (2, 0, 0),
                               (1, 3, 1), (0, 4, 1)):
        assert lib.dtc_conv2d_route_query(d, mode, flags, nprob, None, 0, C.byref(r)) != 0, (mode, flags, nprob)
        assert b"name no entry point" in lib.dtc_last_error()
    assert lib.dtc_conv2d_route_query(d, 0, 0, 1, None, 0, None) != 0
    assert lib.dtc_abi_version() == 1  # a symbol was added: no caller breaks
