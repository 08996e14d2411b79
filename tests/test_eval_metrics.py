"""On-device evaluation, host side (no GPU): the two C entries exist and refuse bad arguments before any
device call, --fused-eval parses in every mode, and EvalResult.reference_meters() reproduces the meters of the
trainer's default validate / test loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rank_rule(z, y):
    """The project's rank of the label's logit (include/dtc.h, dtc_eval_metrics), row by row in numpy:
    rank = #{j != y : !(z[j] <= z[y])} + #{j < y : z[j] == z[y]}; a label out of range never counts as a hit
    (rank = number of classes)."""
    z = np.asarray(z, dtype=np.float32)
    n, c = z.shape
    j = np.arange(c)
    out = np.empty(n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            if not 0 <= y[i] < c:
                out[i] = c
                continue
            zy = z[i, y[i]]
            out[i] = int((~(z[i] <= zy) & (j != y[i])).sum() + ((z[i] == zy) & (j < y[i])).sum())
    return out


def test_header_declares_and_library_exports_the_entries(dtc):
    text = open(os.path.join(ROOT, "include", "dtc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("dtc_eval_metrics", "dtc_rn18_eval_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(dtc._native.lib, name) and name in dtc._native.SYMBOLS
    assert re.search(r"\}\s*dtc_eval_record\s*;", text)
    assert C.sizeof(dtc._native.EvalRecord) == 16
    assert [f[0] for f in dtc._native.EvalRecord._fields_] == ["loss", "n", "top1", "topk"]
    assert dtc._native.lib.dtc_abi_version() == 1


def _refused(dtc, rc):
    """An argument error: a negative code with a message. (A device call would have returned a positive HIP
    error code on a host without a GPU, or run.)"""
    assert rc < 0, rc
    assert dtc._native.last_error()


def test_eval_metrics_refuses_bad_arguments(dtc):
    lib = dtc._native.lib
    p = C.c_void_p(256)  # never dereferenced: every case below is refused on the host
    ncls = 10
    _refused(dtc, lib.dtc_eval_metrics(p, p, 4, ncls, 1, None, None))  # null rec
    _refused(dtc, lib.dtc_eval_metrics(None, p, 4, ncls, 1, p, None))
    _refused(dtc, lib.dtc_eval_metrics(p, None, 4, ncls, 1, p, None))
    for n in (0, 4097):
        _refused(dtc, lib.dtc_eval_metrics(p, p, n, ncls, 1, p, None))
        assert "n = %d" % n in dtc._native.last_error()
    for k in (0, ncls + 1):
        _refused(dtc, lib.dtc_eval_metrics(p, p, 4, ncls, k, p, None))
        assert "topk = %d" % k in dtc._native.last_error()
    _refused(dtc, lib.dtc_eval_metrics(p, p, 4, 0, 1, p, None))


def test_eval_batch_refuses_bad_arguments_on_an_unbound_net(dtc):
    lib = dtc._native.lib
    h = C.c_void_p()
    batch = 8
    dtc._native.call("dtc_rn18_create", C.byref(h), batch, 32, 32, 100, 25.0)
    try:
        p = C.c_void_p(256)
        for nv in (0, batch + 1):
            _refused(dtc, lib.dtc_rn18_eval_batch(h, p, p, nv, 5, None, p, None))
            assert "n_valid = %d" % nv in dtc._native.last_error()
        for k in (0, 101):
            _refused(dtc, lib.dtc_rn18_eval_batch(h, p, p, batch, k, None, p, None))
            assert "topk = %d" % k in dtc._native.last_error()
        _refused(dtc, lib.dtc_rn18_eval_batch(h, p, p, batch, 5, None, None, None))  # null rec
        _refused(dtc, lib.dtc_rn18_eval_batch(h, p, p, batch, 5, None, p, None))  # in range, but never bound
        assert "unbound" in dtc._native.last_error()
        _refused(dtc, lib.dtc_rn18_eval_batch(None, p, p, batch, 5, None, p, None))
    finally:
        lib.dtc_rn18_destroy(h)


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
def test_fused_eval_flag(dtc, mode):
    assert dtc.trainer.load_config([], mode).fused_eval is False
    assert dtc.trainer.load_config(["--fused-eval"], mode).fused_eval is True


def test_reference_meters_reproduce_the_default_loop(dtc):
    """Three batches of 64 and a tail of 8: the meters built from per-batch records (loss, n, hit counts) are
    the very floats the default validate / test loop gets from criterion(...).item(), trainer.accuracy and
    AverageMeter -- every batch weighted 1, the tail included, as in the reference."""
    import torch

    g = torch.Generator().manual_seed(7)
    ncls = 100
    meters = [dtc.trainer.AverageMeter() for _ in range(3)]
    loss, n, top1, top5, per_batch_top1 = [], [], [], [], []
    for b in (64, 64, 64, 8):
        z = torch.randn(b, ncls, generator=g)
        y = torch.randint(0, ncls, (b,), generator=g)
        z[torch.arange(0, b, 2), y[::2]] += 2.5  # a useful share of hits
        lv = torch.nn.functional.cross_entropy(z, y)
        p1, p5 = dtc.trainer.accuracy(z, y, topk=(1, 5))
        meters[0].update(lv.item())
        meters[1].update(p1.item())
        meters[2].update(p5.item())
        per_batch_top1.append(p1.item())
        r = rank_rule(z.numpy(), y.numpy())
        loss.append(lv.numpy())
        n.append(b)
        top1.append(int((r < 1).sum()))
        top5.append(int((r < 5).sum()))
    res = dtc.EvalResult(loss, n, top1, top5, 5)
    assert len(res) == 4 and res.k == 5
    m = res.reference_meters()
    assert m == {"loss": meters[0].avg, "top1": meters[1].avg, "topk": meters[2].avg}
    # the tail carries weight 1: the plain mean of the four per-batch values, not the sample-weighted one
    assert m["top1"] == sum(per_batch_top1) / 4
    tot = res.totals()
    assert tot["n"] == 200 and tot["top1"] == 100.0 * sum(top1) / 200 and tot["topk"] == 100.0 * sum(top5) / 200
    assert tot["top1"] != m["top1"]
    assert abs(tot["loss"] - float(np.dot(np.asarray(loss, np.float64), n)) / 200) < 1e-12
    # records as they come back from the device: int32 words, word 0 = the loss bits
    words = np.stack([np.asarray(loss, np.float32).view(np.int32), np.asarray(n, np.int32), np.asarray(top1, np.int32),
                      np.asarray(top5, np.int32)], axis=1)
    again = dtc.EvalResult.from_records(torch.from_numpy(words.copy()), 5)
    assert again.reference_meters() == m
    empty = dtc.EvalResult.from_records(torch.empty(0, 4, dtype=torch.int32), 5)
    assert len(empty) == 0 and empty.reference_meters() == {"loss": 0.0, "top1": 0.0, "topk": 0.0}
