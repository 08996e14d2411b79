"""The fused fp32 conv1 + shortcut pair's router (conv_route.cpp: conv_f32_sc_route) through
dtc_conv2d_f32_sc_route_query, and the executor's plan at option f32_split = 3: host code only, no GPU."""
import ctypes as C

import pytest

MODEL_S2 = [(32, 64, 128), (16, 128, 256), (8, 256, 512)]  # (H = W, C, K): conv1 of layers 2-4, block 0
REFUSED = [(8, 31, 31, 64, 128, 3, 3, 2, 1),   # odd extents
           (8, 16, 16, 48, 64, 3, 3, 2, 1),    # C = 48
           (8, 16, 16, 64, 128, 3, 3, 1, 1),   # stride 1
           (1, 8, 224, 64, 64, 3, 3, 2, 1)]    # a 224-wide row


@pytest.mark.parametrize("batch", [2, 256])
def test_model_transitions_route_to_the_split_kernel(dtc, batch):
    for hw, c, k in MODEL_S2:
        d = dtc.ops.conv_desc(batch, hw, hw, c, k, 3, 3, 2, 1)
        for mode in (0, 1):
            # the forward kernel is refused where it measured no faster than the exact pair: batch 256 of
            # layers 2 and 4
            want = "exact" if mode == 0 and batch == 256 and hw != 16 else "split"
            assert dtc.ops.conv2d_f32_sc_route(d, mode, 1) == want, (hw, c, k, mode)
            assert dtc.ops.conv2d_f32_sc_route(d, mode, 0) == "exact", (hw, c, k, mode)


@pytest.mark.parametrize("desc", REFUSED)
def test_refused_shapes_run_the_exact_pair(dtc, desc):
    d = dtc.ops.conv_desc(*desc)
    for mode in (0, 1):
        for algo in (0, 1):
            assert dtc.ops.conv2d_f32_sc_route(d, mode, algo) == "exact"


def test_route_query_rejects_what_names_no_entry_point(dtc):
    lib = dtc._native.lib
    d = dtc.ops.conv_desc(2, 16, 16, 64, 128, 3, 3, 2, 1)
    assert lib.dtc_conv2d_f32_sc_route_query(d, 2, 1) < 0  # no fused weight gradient
    assert lib.dtc_conv2d_f32_sc_route_query(d, -1, 1) < 0
    assert lib.dtc_conv2d_f32_sc_route_query(d, 0, 2) < 0
    assert lib.dtc_conv2d_f32_sc_route_query(dtc.ops.conv_desc(2, 16, 16, 64, 128, 1, 1, 2, 0), 0, 1) < 0  # not a 3x3
    # the stride-1 entry points keep their answer for the transition conv: exact
    assert dtc.ops.conv2d_f32_route(d, 0, 1) == "exact"


def test_option_3_plans_the_workspace_of_option_2(dtc):
    """The transition convs' weights lie inside the plane range planned at 1 / 2, so option 3 adds nothing."""
    lib = dtc._native.lib
    sizes = {}
    try:
        for opt in (2, 3):
            assert lib.dtc_set_option(b"f32_split", opt) == 0
            h = C.c_void_p()
            dtc._native.call("dtc_rn18_create", C.byref(h), 8, 32, 32, 100, 25.0)
            dtc._native.call("dtc_rn18_set_precision", h, 1)
            sizes[opt] = lib.dtc_rn18_workspace_bytes(h)
            lib.dtc_rn18_destroy(h)
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    assert sizes[3] == sizes[2] > 0
