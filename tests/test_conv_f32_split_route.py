"""The fp32 convs' router (conv_route.cpp: conv_f32_route) through dtc_conv2d_f32_route_query, the f32_split option
and the executor's plan of the weight planes: host code only, no GPU."""
import ctypes as C

import pytest

# the thirteen stride-1 3x3 convs of the 32x32 model: (H = W, C, K) -- layer1's four, then conv2 of the projection
# block and both convs of the second block of layers 2-4
MODEL_S1 = [(32, 64, 64)] * 4 + [(16, 128, 128)] * 3 + [(8, 256, 256)] * 3 + [(4, 512, 512)] * 3
REFUSED = [(8, 32, 32, 64, 128, 3, 3, 2, 1),   # stride 2
           (8, 16, 16, 64, 128, 1, 1, 1, 0),   # 1x1
           (8, 16, 16, 48, 64, 3, 3, 1, 1),    # C = 48
           (1, 8, 224, 64, 64, 3, 3, 1, 1)]    # a 224-wide row


@pytest.mark.parametrize("batch", [2, 256])
def test_model_convs_route_to_the_split_kernel(dtc, batch):
    assert len(MODEL_S1) == 13
    for hw, c, k in MODEL_S1:
        d = dtc.ops.conv_desc(batch, hw, hw, c, k, 3, 3, 1, 1)
        for mode in (0, 1):
            assert dtc.ops.conv2d_f32_route(d, mode, 1) == "split", (hw, c, k, mode)
            assert dtc.ops.conv2d_f32_route(d, mode, 0) == "exact", (hw, c, k, mode)


@pytest.mark.parametrize("desc", REFUSED)
def test_refused_shapes_fall_back_to_exact(dtc, desc):
    d = dtc.ops.conv_desc(*desc)
    for mode in (0, 1):
        for algo in (0, 1):
            assert dtc.ops.conv2d_f32_route(d, mode, algo) == "exact"


def test_route_query_rejects_what_names_no_entry_point(dtc):
    lib = dtc._native.lib
    d = dtc.ops.conv_desc(2, 8, 8, 64, 64, 3, 3, 1, 1)
    assert lib.dtc_conv2d_f32_route_query(d, 2, 1) < 0  # the weight gradient has no split kernel and no fp32 entry
    assert lib.dtc_conv2d_f32_route_query(d, 0, 2) < 0
    assert lib.dtc_conv2d_f32_route_query(dtc.ops.conv_desc(2, 8, 8, 60, 64, 3, 3, 1, 1), 0, 1) < 0


def test_option_default_and_planned_weight_planes(dtc):
    """f32_split is registered with default 0; an fp32 executor created with it on plans three bf16 planes of its
    3x3 stride-1 conv weights (9,437,184 of the 11.2 M parameters; the planned range also spans what lies between
    them in the flat buffer) in its workspace, a bf16 executor plans nothing more."""
    lib = dtc._native.lib
    assert lib.dtc_get_option(b"f32_split") == 0

    def ws_bytes(fp32):
        h = C.c_void_p()
        dtc._native.call("dtc_rn18_create", C.byref(h), 8, 32, 32, 100, 25.0)
        dtc._native.call("dtc_rn18_set_precision", h, fp32)
        n = lib.dtc_rn18_workspace_bytes(h)
        lib.dtc_rn18_destroy(h)
        return n

    off = [ws_bytes(0), ws_bytes(1)]
    try:
        assert lib.dtc_set_option(b"f32_split", 1) == 0
        on = [ws_bytes(0), ws_bytes(1)]
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    assert on[0] == off[0]
    s1 = 4 * 64 * 64 + 3 * 128 * 128 + 3 * 256 * 256 + 3 * 512 * 512  # x 9 taps
    assert 3 * 2 * 9 * s1 <= on[1] - off[1] < 3 * 2 * 11_220_132 + 4096
