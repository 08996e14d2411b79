"""The fp32 weight gradient's router (conv_route.cpp: conv_f32_route for WGRAD) through
dtc_conv2d_f32_wgrad_route_query / _workspace_size, and the executor's slab with option f32_split = 2: host code only."""
import ctypes as C

import pytest

from tests.test_conv_f32_split_route import MODEL_S1, REFUSED


@pytest.mark.parametrize("batch", [2, 256])
def test_model_convs_route_to_the_split_wgrad(dtc, batch):
    for hw, c, k in MODEL_S1:
        d = dtc.ops.conv_desc(batch, hw, hw, c, k, 3, 3, 1, 1)
        assert dtc.ops.conv2d_f32_wgrad_route(d, 1) == "split", (hw, c, k)
        assert dtc.ops.conv2d_f32_wgrad_route(d, 0) == "exact", (hw, c, k)
        assert dtc._native.lib.dtc_conv2d_f32_wgrad_workspace_size(d, 0) > 0


@pytest.mark.parametrize("desc", REFUSED)
def test_refused_shapes_fall_back_to_exact(dtc, desc):
    d = dtc.ops.conv_desc(*desc)
    for algo in (0, 1):
        assert dtc.ops.conv2d_f32_wgrad_route(d, algo) == "exact"
        assert dtc._native.lib.dtc_conv2d_f32_wgrad_workspace_size(d, algo) > 0


def test_planned_workspace_grows_only_at_option_2(dtc):
    """The fp32 executor's workspace at f32_split = 1 is the default's plus the weight planes (the slab unchanged:
    tests/test_conv_f32_split_route.py bounds the difference); at 2 it is at least that."""
    lib = dtc._native.lib

    def ws_bytes(opt):
        try:
            assert lib.dtc_set_option(b"f32_split", opt) == 0
            h = C.c_void_p()
            dtc._native.call("dtc_rn18_create", C.byref(h), 8, 32, 32, 100, 25.0)
            dtc._native.call("dtc_rn18_set_precision", h, 1)
            n = lib.dtc_rn18_workspace_bytes(h)
            lib.dtc_rn18_destroy(h)
            return n
        finally:
            lib.dtc_set_option(b"f32_split", 0)

    off, one, two = ws_bytes(0), ws_bytes(1), ws_bytes(2)
    assert one - off < 3 * 2 * 11_220_132 + 4096  # the planes alone: no larger slab
    assert two >= one
