"""The fp32 weight gradient's router at the 224x224 model's rows under option f32x_gen (conv_f32x_wgrad.hip's general
geometry) through dtc_conv2d_f32_wgrad_route_query / _workspace_size, and the executor's planned slab: host only."""
import ctypes as C

import pytest

CONFIG5_S1 = [(224, 64), (112, 128), (56, 256), (28, 512)]  # (H = W, C = K): the stride-1 families of layers 1-4
# a 2 x 224 x 224 fp32 executor's planned bytes before the general weight gradient, by (f32_split, f32x_gen)
PLANNED_BEFORE = {(2, 0): 899_792_896, (1, 2): 966_788_608, (2, 2): 966_788_608}


@pytest.fixture
def lib(dtc):
    try:
        yield dtc._native.lib
    finally:
        dtc._native.lib.dtc_set_option(b"f32x_gen", 0)
        dtc._native.lib.dtc_set_option(b"f32_split", 0)


@pytest.mark.parametrize("batch", [2, 128])
def test_config5_convs_route_to_the_split_wgrad_under_the_option(dtc, lib, batch):
    for hw, c in CONFIG5_S1:
        d = dtc.ops.conv_desc(batch, hw, hw, c, c, 3, 3, 1, 1)
        for opt, want in ((0, "exact"), (2, "split")):
            lib.dtc_set_option(b"f32x_gen", opt)
            assert dtc.ops.conv2d_f32_wgrad_route(d, 1) == want, (hw, c, opt)
            assert lib.dtc_conv2d_f32_wgrad_workspace_size(d, 1) > 0


def test_planned_slab_grows_only_with_both_options(dtc, lib):
    for (split, gen), before in PLANNED_BEFORE.items():
        lib.dtc_set_option(b"f32_split", split)
        lib.dtc_set_option(b"f32x_gen", gen)
        h = C.c_void_p()
        dtc._native.call("dtc_rn18_create", C.byref(h), 2, 224, 224, 100, 25.0)
        dtc._native.call("dtc_rn18_set_precision", h, 1)
        n = lib.dtc_rn18_workspace_bytes(h)
        lib.dtc_rn18_destroy(h)
        assert n >= before if split == gen == 2 else n == before, (split, gen, n)
