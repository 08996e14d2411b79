"""The fp32 convs' planner (csrc/conv_f32_route.cpp: conv_f32_plan) through the C ABI, host code only: its answers over
the grid of tools/conv_digest.py --f32-routes equal the recording made before the planner existed
(tests/golden/f32_routes.txt), and the workspace-size queries return the slab of the route the route queries name."""
import os

import pytest

from tools import conv_digest as D

EXACT = 0  # DTC_CONV_F32_EXACT
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f32_routes.txt")


def test_routes_and_slabs_equal_the_recording(dtc):
    got = []
    D.f32_routes(got.append)
    want = open(GOLDEN).read().splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


@pytest.mark.parametrize("opts", D.F32_OPTION_SETS, ids=D.oid)
def test_workspace_sizes_are_the_routes_slabs(dtc, opts):
    """exact: conv_f32's slab, what algo 0 answers (the pair: the larger of conv1's and the shortcut's, each launch
    takes the whole). split: whole slabs of the split kernel's layout ([K][9 C], the pair [K][10 C]), none (one split
    writes dw itself) or at least two, at most the 256 CUs over the kernel's (64 C x 64 K, the pair 64 C x 32 K) tiles."""
    lib, N = dtc._native.lib, dtc._native
    with D.Options(opts):
        for s in D.f32_shapes():
            n, h, w, c, k, r, _, stride, _ = s
            d = N.ConvDesc(*s)
            for sc, route, size in ((False, lib.dtc_conv2d_f32_wgrad_route_query, lib.dtc_conv2d_f32_wgrad_workspace_size),
                                    (True, lib.dtc_conv2d_f32_wgrad_sc_route_query, lib.dtc_conv2d_f32_wgrad_sc_workspace_size)):
                if route(d, 0) < 0:  # not a descriptor of this family
                    assert route(d, 1) < 0 and size(d, 0) == size(d, 1) == 0, (s, sc)
                    continue
                assert route(d, 0) == EXACT, (s, sc)
                exact = size(d, 0)
                if sc:
                    own = lib.dtc_conv2d_f32_wgrad_workspace_size
                    assert exact == max(own(d, 0), own(N.ConvDesc(n, h, w, c, k, 1, 1, stride, 0), 0)), s
                assert exact >= k * r * r * c * 4, s  # conv_f32 needs one slab
                if route(d, 1) == route(d, 0):
                    assert size(d, 1) == exact, (s, sc)
                    continue
                one = k * (10 if sc else 9) * c * 4
                slabs, rem = divmod(size(d, 1), one)
                assert rem == 0 and slabs != 1 and slabs <= max(1, 256 // ((c // 64) * (k // (32 if sc else 64)))), (s, sc)
