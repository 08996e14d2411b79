"""bf16 gradient compression: the --grad-compress flag, the host-side argument checks of dtc_grad_compress_bf16,
dtc_grad_decompress_bf16 and dtc_rn18_set_grad_compress through the raw ABI, the communication-hook resolution and
the module-level setting (CPU only; the kernels, the transports and the executor are tested in
test_gpu_grad_compress.py)."""
import ctypes as C

import pytest


def test_grad_compress_flag(dtc):
    assert dtc.trainer.load_config([], "ddp").grad_compress == "none"
    assert dtc.trainer.load_config(["--grad-compress", "bf16"], "ddp").grad_compress == "bf16"
    assert dtc.trainer.load_config(["--grad-compress", "none"], "ddp").grad_compress == "none"
    for bad in ("fp16", "BF16", "1"):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(["--grad-compress", bad], "ddp")
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--grad-compress"], "ddp")


@pytest.mark.parametrize("mode", ["single", "dp"])
def test_grad_compress_flag_exists_only_under_ddp(dtc, mode):
    assert not hasattr(dtc.trainer.load_config([], mode), "grad_compress")
    for value in ("bf16", "none"):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(["--grad-compress", value], mode)


def test_new_symbols_are_bound(dtc):
    lib = dtc._native.lib
    for name in ("dtc_grad_compress_bf16", "dtc_grad_decompress_bf16", "dtc_rn18_set_grad_compress"):
        assert name in dtc._native.SYMBOLS and hasattr(lib, name)
    assert (dtc.ops.COMPRESS_OFF, dtc.ops.COMPRESS_BF16) == (0, 1)
    assert lib.dtc_abi_version() == 1  # no existing signature changed


def test_flat_entry_points_reject_bad_arguments_before_any_device_call(dtc):
    """Fake (non-null) pointers reach no GPU: every check runs on the host ahead of the launch."""
    lib, err = dtc._native.lib, dtc._native.last_error
    g, a, c = 1 << 20, 2 << 20, 4096  # fp32 g, fp32 acc, bf16 c
    for args, word in (((g, None, c, 6), "multiple of 4"), ((g, None, c, 0), "multiple of 4"),
                       ((g, a, c, -4), "multiple of 4"), ((g + 8, None, c, 8), "16-byte"), ((g, a + 4, c, 8), "16-byte"),
                       ((g, None, c + 4, 8), "8-byte"), ((g, None, c + 2, 8), "8-byte"), ((None, None, c, 8), "null"),
                       ((g, a, None, 8), "null"), ((g, None, g, 8), "overlap"), ((g, None, g + 24, 8), "overlap"),
                       ((g, None, g - 8, 8), "overlap"), ((g, a, a + 16, 8), "overlap"), ((g, a, a - 8, 8), "overlap")):
        assert lib.dtc_grad_compress_bf16(args[0], args[1], args[2], args[3], None) == -1, args
        assert word in err(), (args, err())
    for args, word in (((c, g, 6), "multiple of 4"), ((c, g, 0), "multiple of 4"), ((c, g + 8, 8), "16-byte"),
                       ((c + 4, g, 8), "8-byte"), ((None, g, 8), "null"), ((c, None, 8), "null"),
                       ((g + 16, g, 8), "overlap"), ((g - 8, g, 8), "overlap")):
        assert lib.dtc_grad_decompress_bf16(args[0], args[1], args[2], None) == -1, args
        assert word in err(), (args, err())


def test_set_grad_compress_host_checks(dtc):
    lib, err = dtc._native.lib, dtc._native.last_error
    assert lib.dtc_rn18_set_grad_compress(None, None, 0) == -1 and "null" in err()
    h = C.c_void_p()
    dtc._native.call("dtc_rn18_create", C.byref(h), 8, 32, 32, 100, 25.0)
    try:
        assert lib.dtc_rn18_set_grad_compress(h, None, 0) == 0  # OFF needs no buffer, bound or not
        assert lib.dtc_rn18_set_grad_compress(h, None, 1) == -1 and "NULL" in err()
        assert lib.dtc_rn18_set_grad_compress(h, 4096, 1) == -1 and "bind" in err()  # no gradients bound yet
        assert lib.dtc_rn18_set_grad_compress(h, 4104, 0) == -1 and "aligned" in err()
        assert lib.dtc_rn18_set_grad_compress(h, 4096, 2) == -1 and "mode" in err()
        assert lib.dtc_rn18_set_grad_compress(h, 4096, -1) == -1 and "mode" in err()
    finally:
        lib.dtc_rn18_destroy(h)


def test_resolve_comm_hook(dtc):
    from torch.distributed.algorithms.ddp_comm_hooks import default_hooks

    par = dtc.parallel
    assert par.resolve_comm_hook(par.bf16_compress_hook) == "bf16"
    assert par.resolve_comm_hook(par.allreduce_hook) is None
    assert par.resolve_comm_hook(default_hooks.bf16_compress_hook) == "bf16"
    assert par.resolve_comm_hook(default_hooks.allreduce_hook) is None
    for other in (lambda state, bucket: None, default_hooks.fp16_compress_hook, None, "bf16"):
        with pytest.raises(NotImplementedError, match="bf16_compress_hook.*allreduce_hook"):
            par.resolve_comm_hook(other)
    assert hasattr(dtc.DistributedDataParallel, "register_comm_hook")


def test_module_setting_is_validated(dtc):
    m = dtc.ResNet18()
    assert m.grad_compression is None
    for bad in ("fp16", "BF16", 1, True):
        m.grad_compression = bad
        with pytest.raises(ValueError, match="grad_compression"):
            m._begin_backward(None)
    with pytest.raises(ValueError, match="gradient_compression"):
        dtc.DistributedDataParallel(m, gradient_compression="fp16")
