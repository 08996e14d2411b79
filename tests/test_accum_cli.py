"""Gradient accumulation: the --accum-steps flag, the host-side argument checks of dtc_grad_accum_flat and
dtc_rn18_set_grad_accum through the raw ABI, and the module-level window state (CPU only; the kernel and the
executor hook are tested in test_gpu_grad_accum.py)."""
import ctypes as C

import pytest


@pytest.mark.parametrize("mode", ["single", "ddp"])
def test_accum_steps_flag(dtc, mode):
    assert dtc.trainer.load_config([], mode).accum_steps == 1
    assert dtc.trainer.load_config(["--accum-steps", "4"], mode).accum_steps == 4
    for bad in ("0", "-2"):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(["--accum-steps", bad], mode)
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--accum-steps", "1.5"], mode)


def test_accum_steps_under_data_parallel(dtc):
    assert dtc.trainer.load_config([], "dp").accum_steps == 1
    assert dtc.trainer.load_config(["--accum-steps", "1"], "dp").accum_steps == 1
    for bad in ("2", "0", "-1"):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(["--accum-steps", bad], "dp")


def test_new_symbols_are_bound(dtc):
    lib = dtc._native.lib
    for name in ("dtc_grad_accum_flat", "dtc_rn18_set_grad_accum"):
        assert name in dtc._native.SYMBOLS and hasattr(lib, name)
    assert (dtc.ops.ACCUM_OFF, dtc.ops.ACCUM_STORE, dtc.ops.ACCUM_ADD, dtc.ops.ACCUM_FINISH) == (0, 1, 2, 3)
    assert lib.dtc_abi_version() == 1  # no existing signature changed


def test_grad_accum_flat_rejects_bad_arguments_before_any_device_call(dtc):
    """Fake (non-null) pointers reach no GPU: every check runs on the host ahead of the launch."""
    lib, err = dtc._native.lib, dtc._native.last_error
    a, b = 4096, 1 << 20
    for args, word in (((a, b, 6, 2), "multiple of 4"), ((a, b, 0, 1), "multiple of 4"), ((a, b, -4, 1), "multiple of 4"),
                       ((a + 4, b, 8, 2), "aligned"), ((a, b + 8, 8, 3), "aligned"), ((a, a + 16, 8, 1), "overlap"),
                       ((a, a, 8, 2), "overlap"), ((a, b, 8, 0), "mode"), ((a, b, 8, 4), "mode"),
                       ((None, b, 8, 1), "null"), ((a, None, 8, 1), "null")):
        assert lib.dtc_grad_accum_flat(args[0], args[1], args[2], args[3], None) == -1, args
        assert word in err(), (args, err())


def test_set_grad_accum_host_checks(dtc):
    lib, err = dtc._native.lib, dtc._native.last_error
    assert lib.dtc_rn18_set_grad_accum(None, None, 0) == -1 and "null" in err()
    h = C.c_void_p()
    dtc._native.call("dtc_rn18_create", C.byref(h), 8, 32, 32, 100, 25.0)
    try:
        assert lib.dtc_rn18_set_grad_accum(h, None, 0) == 0  # OFF needs no buffer, bound or not
        assert lib.dtc_rn18_set_grad_accum(h, None, 1) == -1 and "NULL" in err()
        assert lib.dtc_rn18_set_grad_accum(h, 4096, 2) == -1 and "bind" in err()  # no gradients bound yet
        assert lib.dtc_rn18_set_grad_accum(h, 4100, 0) == -1 and "aligned" in err()
        assert lib.dtc_rn18_set_grad_accum(h, 4096, 5) == -1 and "mode" in err()
        assert lib.dtc_rn18_set_grad_accum(h, 4096, -1) == -1 and "mode" in err()
    finally:
        lib.dtc_rn18_destroy(h)


def test_window_state_of_the_module(dtc):
    """accumulate() nests and restores its depth on an exception; grad_accum_steps defaults to 1 and is validated
    when a backward asks for it; DistributedDataParallel.no_sync is the module's accumulate."""
    m = dtc.ResNet18()
    assert m.grad_accum_steps == 1 and m._accum_depth == 0 and not m._accum_open
    with m.accumulate() as inner:
        assert inner is m and m._accum_depth == 1
        with m.accumulate():
            assert m._accum_depth == 2
        assert m._accum_depth == 1
    with pytest.raises(RuntimeError):
        with m.accumulate():
            raise RuntimeError("boom")
    assert m._accum_depth == 0
    m._accum_open = True
    m.reset_accumulation()
    assert not m._accum_open
    for bad in (0, -1, 2.0, None):
        m.grad_accum_steps = bad
        with pytest.raises(ValueError):
            m._begin_backward(None)
    assert dtc.DistributedDataParallel.no_sync is not None and hasattr(dtc.DDP, "no_sync")
