"""PowerSGD gradient compression: the trainer flags, PowerSGDState and the hook resolution, the host-side argument
checks of the dtc_psgd_* entry points through the raw ABI and the plan sizes of the real layout (CPU only; the
kernels, the collectives and the model path are tested in test_gpu_powersgd.py)."""
import ctypes as C

import pytest


def test_powersgd_flags(dtc):
    cfg = dtc.trainer.load_config
    h = cfg([], "ddp")
    assert (h.grad_compress, h.powersgd_rank, h.powersgd_start_iter) == ("none", 2, 1000)
    h = cfg(["--grad-compress", "powersgd", "--powersgd-rank", "4", "--powersgd-start-iter", "2"], "ddp")
    assert (h.grad_compress, h.powersgd_rank, h.powersgd_start_iter) == ("powersgd", 4, 2)
    for r in ("1", "2", "3", "4"):
        assert cfg(["--powersgd-rank", r], "ddp").powersgd_rank == int(r)
    for bad in (["--powersgd-rank", "0"], ["--powersgd-rank", "5"], ["--powersgd-rank", "x"],
                ["--powersgd-start-iter", "1"], ["--powersgd-start-iter", "0"], ["--grad-compress", "PowerSGD"]):
        with pytest.raises(SystemExit):
            cfg(bad, "ddp")


@pytest.mark.parametrize("mode", ["single", "dp"])
def test_powersgd_flags_exist_only_under_ddp(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert not hasattr(h, "powersgd_rank") and not hasattr(h, "powersgd_start_iter")
    for args in (["--grad-compress", "powersgd"], ["--powersgd-rank", "2"], ["--powersgd-start-iter", "5"]):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(args, mode)


def test_state_validation_mirrors_torch(dtc):
    S = dtc.parallel.PowerSGDState
    s = S()
    assert (s.matrix_approximation_rank, s.start_powerSGD_iter, s.min_compression_rate, s.use_error_feedback,
            s.warm_start, s.orthogonalization_epsilon, s.random_seed, s.iter) == (1, 1000, 2, True, True, 0, 0, 0)
    for start in (1, 0):
        with pytest.raises(ValueError, match="start_powerSGD_iter"):
            S(start_powerSGD_iter=start)
    with pytest.raises(NotImplementedError, match="warm_start"):
        S(warm_start=False)
    with pytest.raises(ValueError, match="matrix_approximation_rank"):
        S(matrix_approximation_rank=5)
    assert S(use_error_feedback=False, start_powerSGD_iter=2).use_error_feedback is False


def test_hook_resolution_and_registration(dtc):
    from torch.distributed.algorithms.ddp_comm_hooks import powerSGD_hook as tp

    par = dtc.parallel
    assert par.resolve_comm_hook(par.powerSGD_hook) == "powersgd"
    assert par.resolve_comm_hook(tp.powerSGD_hook) == "powersgd"
    with pytest.raises(NotImplementedError, match="bf16_compress_hook.*allreduce_hook"):
        par.resolve_comm_hook(tp.batched_powerSGD_hook)
    assert "powersgd" in dtc.nn.GRAD_COMPRESSIONS
    # register_comm_hook touches only the module: a stand-in wrapper is enough on the CPU
    m = dtc.ResNet18()
    ddp = dtc.DistributedDataParallel.__new__(dtc.DistributedDataParallel)
    object.__setattr__(ddp, "_modules", {"module": m})
    reg = dtc.DistributedDataParallel.register_comm_hook
    for state in (par.PowerSGDState(matrix_approximation_rank=2, start_powerSGD_iter=3, random_seed=7),
                  tp.PowerSGDState(None, matrix_approximation_rank=2, start_powerSGD_iter=3)):
        reg(ddp, state, par.powerSGD_hook)
        assert m.grad_compression == "powersgd" and m._powersgd.rank == 2 and m._powersgd.start == 3
        assert m._powersgd.state is state and state.iter == 0
    assert m._powersgd.take() is False and m._powersgd.take() is False and m._powersgd.take() is False
    assert m._powersgd.take() is True and state.iter == 4  # torch's counter: `start` plain steps first
    with pytest.raises(TypeError, match="PowerSGDState"):
        reg(ddp, None, par.powerSGD_hook)
    with pytest.raises(ValueError, match="matrix_approximation_rank"):
        reg(ddp, tp.PowerSGDState(None, matrix_approximation_rank=8, start_powerSGD_iter=3), tp.powerSGD_hook)
    with pytest.raises(NotImplementedError, match="bf16_compress_hook.*allreduce_hook"):
        reg(ddp, par.PowerSGDState(), tp.batched_powerSGD_hook)
    reg(ddp, None, par.allreduce_hook)
    assert m.grad_compression is None and m._powersgd is None
    # the constructor argument keeps its two values; the bare setting needs a state
    with pytest.raises(ValueError, match="gradient_compression"):
        dtc.DistributedDataParallel(m, gradient_compression="powersgd")
    m.grad_compression = "powersgd"
    with pytest.raises(dtc.NativeError, match="register_comm_hook"):
        m._begin_backward(None)


def test_new_symbols_are_bound(dtc):
    lib = dtc._native.lib
    for name in ("dtc_psgd_plan_create", "dtc_psgd_plan_destroy", "dtc_psgd_plan_numel", "dtc_psgd_plan_device_bytes",
                 "dtc_psgd_plan_bind", "dtc_psgd_orthonormalize", "dtc_psgd_project", "dtc_psgd_backproject",
                 "dtc_psgd_reconstruct"):
        assert name in dtc._native.SYMBOLS and hasattr(lib, name)
    assert lib.dtc_abi_version() == 1  # additive: no existing signature changed


def _create(dtc, rows):
    T = dtc._native.PsgdTensor
    table = (T * max(1, len(rows)))(*[T(*r) for r in rows])
    h = C.c_void_p(123)
    rc = dtc._native.lib.dtc_psgd_plan_create(C.byref(h), table, len(rows))
    return rc, h


def test_plan_argument_checks(dtc):
    lib, err = dtc._native.lib, dtc._native.last_error
    good = [(0, 4, 12, 1, 0), (64, 10, 1, 0, 0)]
    for rows, word in (([(0, 4, 12, 1, 0), (40, 10, 1, 0, 0)], "overlaps"),
                       ([(64, 10, 1, 0, 0), (0, 4, 12, 1, 0)], "sorted"),
                       ([(2, 4, 12, 1, 0)], "multiple of 4"), ([(-4, 4, 12, 1, 0)], "multiple of 4"),
                       ([(0, 0, 12, 1, 0)], "positive"), ([(0, 4, -1, 0, 0)], "positive"),
                       ([(0, 1 << 40, 1 << 40, 0, 0)], "overflows"),
                       ([((1 << 62), (1 << 31), (1 << 31), 0, 0)], "overflows"),
                       ([(0, 4, 12, 5, 0)], "rank"), ([(0, 4, 12, -1, 0)], "rank"), ([(0, 3, 12, 4, 0)], "rank"),
                       ([(0, 12, 2, 3, 0)], "rank"), ([(0, 4, 12, 1, 1)], "reserved"),
                       ([(0, 1 << 31, 8, 2, 0)], "2^31")):
        rc, h = _create(dtc, rows)
        assert rc == -1 and h.value is None, rows
        assert word in err(), (rows, err())
    assert lib.dtc_psgd_plan_create(None, None, 1) == -1 and "null" in err()
    h = C.c_void_p()
    assert lib.dtc_psgd_plan_create(C.byref(h), None, 1) == -1 and "null" in err()
    T = dtc._native.PsgdTensor
    assert lib.dtc_psgd_plan_create(C.byref(h), (T * 1)(T(0, 4, 12, 1, 0)), 0) == -1 and "[1, 4096]" in err()
    rc, h = _create(dtc, good)
    assert rc == 0 and h.value
    try:
        assert [lib.dtc_psgd_plan_numel(h, w) for w in range(5)] == [4, 12, 10, 14, 12]
        assert lib.dtc_psgd_plan_numel(h, 5) == -1
        assert lib.dtc_psgd_plan_device_bytes(h) % 16 == 0 and lib.dtc_psgd_plan_device_bytes(h) > 0
        g = 1 << 20  # a fake pointer: no check reaches a GPU
        assert lib.dtc_psgd_plan_bind(h, None, 1 << 20, None) == -1 and "null" in err()
        assert lib.dtc_psgd_plan_bind(h, g + 8, 1 << 20, None) == -1 and "16-byte" in err()
        assert lib.dtc_psgd_plan_bind(h, g, 16, None) == -1 and "needs" in err()
    finally:
        assert lib.dtc_psgd_plan_destroy(h) == 0


def test_phase_argument_checks_run_before_any_device_call(dtc):
    """Fake (non-null) pointers reach no GPU: the pointer checks come first, then the plan must be bound."""
    lib, err = dtc._native.lib, dtc._native.last_error
    rc, h = _create(dtc, [(0, 4, 12, 1, 0)])
    assert rc == 0
    try:
        g, e, q, st, state = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20
        orth, proj, back, rec = (lib.dtc_psgd_orthonormalize, lib.dtc_psgd_project, lib.dtc_psgd_backproject,
                                 lib.dtc_psgd_reconstruct)
        for args, word in (((None, 1, q, st, state, 0.0), "null"), ((h, 2, q, st, state, 0.0), "what"),
                           ((h, -1, q, st, state, 0.0), "what"), ((h, 1, q, st, state, -1.0), "epsilon"),
                           ((h, 1, None, st, state, 0.0), "null"), ((h, 1, q, st, None, 0.0), "null"),
                           ((h, 1, q + 4, st, state, 0.0), "16-byte"), ((h, 1, q, st, state + 8, 0.0), "16-byte"),
                           ((h, 0, q, None, state, 0.0), "null"), ((h, 0, q, st + 4, state, 0.0), "16-byte"),
                           ((h, 1, q, st, state, 0.0), "bound"), ((h, 0, q, st, state, 0.0), "bound")):
            assert orth(*args, None) == -1, args
            assert word in err(), (args, err())
        for fn, order in ((proj, lambda g_, e_, q_, s_: (g_, e_, q_, s_)), (back, lambda g_, e_, q_, s_: (g_, e_, s_, q_))):
            for ptrs, word in (((None, e, q, st), "null"), ((g, e, None, st), "null"), ((g, e, q, None), "null"),
                               ((g + 4, e, q, st), "16-byte"), ((g, e + 8, q, st), "16-byte"),
                               ((g, e, q + 4, st), "16-byte"), ((g, e, q, st + 12), "16-byte"),
                               ((g, None, q, st), "bound"), ((g, e, q, st), "bound")):
                assert fn(h, *order(*ptrs), None) == -1, ptrs
                assert word in err(), (ptrs, err())
        for args, word in (((None, g, e, st, q, state, 1.0), "null"), ((h, None, e, st, q, state, 1.0), "null"),
                           ((h, g, e, None, q, state, 1.0), "null"), ((h, g, e, st, None, state, 1.0), "null"),
                           ((h, g, e, st, q, None, 1.0), "null"), ((h, g + 4, e, st, q, state, 1.0), "16-byte"),
                           ((h, g, e + 4, st, q, state, 1.0), "16-byte"), ((h, g, e, st, q, state + 4, 1.0), "16-byte"),
                           ((h, g, e, st, q, state, 0.0), "(0, 1]"), ((h, g, e, st, q, state, 1.5), "(0, 1]"),
                           ((h, g, None, st, q, state, 0.5), "bound"), ((h, g, e, st, q, state, 1.0), "bound")):
            assert rec(*args, None) == -1, args
            assert word in err(), (args, err())
    finally:
        lib.dtc_psgd_plan_destroy(h)


@pytest.mark.parametrize("rank", [1, 2, 4])
def test_plan_sizes_of_the_real_layout(dtc, rank):
    """ResNet-18 with 100 classes under torch's _should_compress rule (min_compression_rate 2): all 21 tensors with
    two or more dimensions are compressed, P = 4,900 r, Q = 31,515 r, 9,700 one-dimensional elements are not."""
    lay = dtc.nn.Layout()
    plan = dtc.ops.psgd_plan(lay, rank)
    comp = [t for t in plan.tensors if t[3]]
    assert len(comp) == 21 and all(t[3] == rank for t in comp)
    assert (plan.n_p, plan.n_q, plan.n_unc) == (4900 * rank, 31515 * rank, 9700)
    assert plan.n_staging == 9700 + 4900 * rank and plan.q_stride == (31515 * rank + 3) // 4 * 4
    assert sum(r * c for _, r, c, _ in plan.tensors) == 11_220_132
    by_name = dict(zip(plan.names, plan.tensors))
    assert by_name["conv1.weight"][1:3] == (64, 27) and by_name["linear.weight"][1:3] == (100, 512)
    assert by_name["layer4.1.conv2.weight"][1:3] == (512, 4608)
    assert dtc.ops.psgd_should_compress(4, 12, 1) and not dtc.ops.psgd_should_compress(4, 12, 2)
    with pytest.raises(ValueError, match="rank"):
        dtc.ops.psgd_plan(lay, 5)
