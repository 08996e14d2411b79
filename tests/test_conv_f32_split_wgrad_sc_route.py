"""The fused fp32 weight-gradient pair's router (conv_route.cpp: conv_f32_wgrad_sc_route) through
dtc_conv2d_f32_wgrad_sc_route_query / _workspace_size, and the executor's plan at option f32_split = 4: host code only."""
import ctypes as C

import pytest

from tests.test_conv_f32_split_sc_route import MODEL_S2, REFUSED


@pytest.mark.parametrize("batch", [2, 256])
def test_model_transitions_route_to_the_split_kernel(dtc, batch):
    """Layers 3 and 4 measured faster than the exact pair at every batch from 2 to 256. Layer 2 (16-wide output rows)
    won from batch 64 on (2048 (step, tile) units), tied or lost by up to 5% at batches 2 .. 32: 16-wide rows
    below 2048 units are refused; option f32x_s2_wgrad = 2 opens them, for measuring."""
    lib = dtc._native.lib
    for hw, c, k in MODEL_S2:
        d = dtc.ops.conv_desc(batch, hw, hw, c, k, 3, 3, 2, 1)
        want = "exact" if hw == 32 and batch == 2 else "split"
        assert dtc.ops.conv2d_f32_wgrad_sc_route(d, 1) == want, (hw, c, k)
        if want == "exact":
            try:
                assert lib.dtc_set_option(b"f32x_s2_wgrad", 2) == 0
                assert dtc.ops.conv2d_f32_wgrad_sc_route(d, 1) == "split"
            finally:
                lib.dtc_set_option(b"f32x_s2_wgrad", 1)
        assert dtc.ops.conv2d_f32_wgrad_sc_route(d, 0) == "exact", (hw, c, k)
        assert lib.dtc_conv2d_f32_wgrad_sc_workspace_size(d, 0) >= k * 9 * c * 4  # the exact pair's larger slab


@pytest.mark.parametrize("desc", REFUSED)
def test_refused_shapes_run_the_exact_pair(dtc, desc):
    d = dtc.ops.conv_desc(*desc)
    for algo in (0, 1):
        assert dtc.ops.conv2d_f32_wgrad_sc_route(d, algo) == "exact"
        assert dtc._native.lib.dtc_conv2d_f32_wgrad_sc_workspace_size(d, algo) > 0


def test_route_query_rejects_what_names_no_entry_point(dtc):
    lib = dtc._native.lib
    assert lib.dtc_conv2d_f32_wgrad_sc_route_query(dtc.ops.conv_desc(2, 16, 16, 64, 128, 3, 3, 2, 1), 2) < 0
    assert lib.dtc_conv2d_f32_wgrad_sc_route_query(dtc.ops.conv_desc(2, 16, 16, 64, 128, 1, 1, 2, 0), 1) < 0  # not a 3x3
    with pytest.raises(dtc._native.NativeError):
        dtc.ops.conv2d_f32_wgrad_sc_route(dtc.ops.conv_desc(2, 16, 16, 64, 128, 1, 1, 2, 0), 1)


def test_option_4_plans_at_least_the_workspace_of_option_3(dtc):
    """Option 4 adds only the fused weight gradient's slab [split][K][10 C], which may exceed the largest planned."""
    lib = dtc._native.lib
    sizes = {}
    try:
        for opt in (3, 4):
            assert lib.dtc_set_option(b"f32_split", opt) == 0
            h = C.c_void_p()
            dtc._native.call("dtc_rn18_create", C.byref(h), 8, 32, 32, 100, 25.0)
            dtc._native.call("dtc_rn18_set_precision", h, 1)
            sizes[opt] = lib.dtc_rn18_workspace_bytes(h)
            lib.dtc_rn18_destroy(h)
    finally:
        lib.dtc_set_option(b"f32_split", 0)
    assert sizes[4] >= sizes[3] > 0
