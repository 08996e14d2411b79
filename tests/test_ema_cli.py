"""Weight EMA: CLI flags, the host-side contract of ema.ModelEma and GradScaler.found_inf, and the argument checks
of dtc_ema_update / dtc_rn18_eval_batch_weights through the raw ABI (CPU only; the kernels are tested in
test_gpu_ema.py)."""
import ctypes as C

import pytest


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
def test_model_ema_flags(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert h.model_ema is False and h.model_ema_decay == 0.9998 and h.model_ema_warmup is False
    assert h.model_ema_steps == 1
    h = dtc.trainer.load_config(["--model-ema", "--model-ema-decay", "0.5", "--model-ema-warmup",
                                 "--model-ema-steps", "4"], mode)
    assert h.model_ema is True and h.model_ema_decay == 0.5 and h.model_ema_warmup is True and h.model_ema_steps == 4
    assert dtc.trainer.load_config(["--model-ema-decay", "0"], mode).model_ema_decay == 0.0
    for bad in (["--model-ema-decay", "1.0"], ["--model-ema-decay", "-0.1"], ["--model-ema-steps", "0"]):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(bad, mode)


def test_model_ema_refuses_what_is_not_on_the_gpu(dtc):
    import torch

    assert dtc.ModelEma is dtc.ema.ModelEma
    with pytest.raises(dtc.NativeError):  # not moved to a GPU: no flat buffers to average
        dtc.ModelEma(dtc.ResNet18(num_classes=10))
    with pytest.raises(dtc.NativeError):
        dtc.ModelEma(torch.nn.Linear(4, 4))
    assert dtc.GradScaler().found_inf is None  # the device word exists from the first step on
    with pytest.raises(AttributeError):
        dtc.GradScaler().found_inf = None  # read-only


def test_ema_update_rejects_bad_arguments_before_any_device_call(dtc):
    """Argument checks run on the host ahead of the launches: fabricated (aligned, non-null) addresses reach no
    GPU. Every item of the list in include/dtc.h."""
    lib, err, Range = dtc._native.lib, dtc._native.last_error, dtc._native.EmaRange
    assert lib.dtc_ema_state_words() == 4
    E, S, B, E2, S2, ST = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20  # 1 MiB apart: n <= 1024 fits

    def upd(ranges=((E, S, B, 1024),), nranges=None, state=ST, decay=0.9, null_table=False):
        table = (Range * max(1, len(ranges)))(*[Range(*r) for r in ranges])
        return lib.dtc_ema_update(None if null_table else table, len(ranges) if nranges is None else nranges,
                                  C.c_void_p(state) if state else None, decay, 0, None, None)

    two = ((E, S, B, 1024), (E2, S2, None, 8))
    cases = [
        (dict(null_table=True), "null"),
        (dict(state=None), "null"),
        (dict(ranges=((None, S, B, 1024),)), "null"),
        (dict(ranges=((E, None, B, 1024),)), "null"),
        (dict(nranges=0), "nranges"),
        (dict(ranges=two + two + two[:1]), "nranges"),                # five
        (dict(ranges=((E, S, B, 0),)), "multiple of 4"),
        (dict(ranges=((E, S, B, -4),)), "multiple of 4"),
        (dict(ranges=((E, S, B, 1022),)), "multiple of 4"),
        (dict(ranges=((E + 4, S, B, 1024),)), "aligned"),
        (dict(ranges=((E, S + 8, B, 1024),)), "aligned"),
        (dict(ranges=((E, S, B + 2, 1024),)), "aligned"),             # bf16 copy: 8 bytes
        (dict(state=ST + 8), "aligned"),
        (dict(ranges=((E, E + 4096 - 16, B, 1024),)), "overlap"),     # src starts inside [ema, ema + n)
        (dict(ranges=((E, E, B, 1024),)), "overlap"),                 # in place
        (dict(ranges=((E, S, B, 1024), (E + 2048, S2, None, 1024))), "overlap"),  # two ema ranges
        (dict(ranges=(two[1], two[0], (E2 + 16, S2 + 4096, None, 4))), "overlap"),  # ... found in any position
        (dict(decay=1.0), "decay"),
        (dict(decay=-0.1), "decay"),
        (dict(decay=float("nan")), "decay"),
    ]
    for kwargs, word in cases:
        assert upd(**kwargs) == -1, kwargs  # DTC_EINVAL
        assert word in err(), (kwargs, err())


def test_eval_batch_weights_rejects_null_and_misaligned_weights(dtc):
    lib, err = dtc._native.lib, dtc._native.last_error
    a = C.c_void_p(4096)
    h = C.c_void_p()
    assert lib.dtc_rn18_create(C.byref(h), 2, 32, 32, 10, 25.0) == 0
    try:
        def ev(net=h, p=a, pb=a, bufs=a, n_valid=2, topk=1):
            return lib.dtc_rn18_eval_batch_weights(net, p, pb, bufs, a, a, n_valid, topk, None, a, None)

        for kwargs, word in ((dict(net=None), "null"), (dict(p=None), "null weight"), (dict(pb=None), "null weight"),
                             (dict(bufs=None), "null weight"), (dict(p=C.c_void_p(4100)), "aligned"),
                             (dict(pb=C.c_void_p(4104)), "aligned"), (dict(n_valid=3), "n_valid"),
                             (dict(topk=11), "topk"), (dict(), "unbound")):  # never bound: no device call either
            assert ev(**kwargs) == -1, kwargs
            assert word in err(), (kwargs, err())
    finally:
        lib.dtc_rn18_destroy(h)
