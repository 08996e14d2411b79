"""LARS and learning-rate warm-up: CLI flags, the host-side contract of optim.LARS, segment-plan validation and
the argument checks of dtc_lars_flat through the raw ABI (CPU only; the kernels are tested in test_gpu_lars.py)."""
import ctypes as C

import pytest
import torch


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
def test_lars_and_warmup_flags(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert h.optimizer == "sgd" and h.lars_trust_coef == 1e-3 and h.lars_clip is False and h.warmup_epochs == 0
    assert h.lr == 0.1 and h.weight_decay == 0.0001 and h.clip_grad_norm == 0.0
    h = dtc.trainer.load_config(["--optimizer", "lars", "--lars-trust-coef", "0.02", "--lars-clip",
                                 "--warmup-epochs", "5"], mode)
    assert h.optimizer == "lars" and h.lars_trust_coef == 0.02 and h.lars_clip is True and h.warmup_epochs == 5
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--optimizer", "lamb"], mode)
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--warmup-epochs", "-1"], mode)
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--lars-trust-coef", "0"], mode)


def test_lars_is_a_torch_optimizer(dtc):
    p = [torch.nn.Parameter(torch.zeros(4))]
    opt = dtc.optim.LARS(p, lr=0.5)
    assert isinstance(opt, torch.optim.Optimizer) and dtc.LARS is dtc.optim.LARS
    assert opt.defaults == dict(lr=0.5, momentum=0.9, weight_decay=0.0, nesterov=False, trust_coef=1e-3, eps=1e-8,
                                trust_clip=False)
    assert opt._flat is None  # GradScaler reaches for this attribute
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)
    assert opt.param_groups[0]["lr"] == 0.5
    opt.zero_grad()
    sched.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(0.05, rel=1e-12)
    with pytest.raises(NotImplementedError):
        dtc.optim.LARS([{"params": p}], lr=0.1)
    with pytest.raises(NotImplementedError):
        opt.step(closure=lambda: 0.0)
    with pytest.raises(dtc.NativeError):  # not the parameters of a native model on the GPU
        opt.step()
    with pytest.raises(dtc.NativeError):
        opt.layer_norms()
    for bad in (dict(lr=-1.0), dict(lr=0.1, momentum=1.0), dict(lr=0.1, trust_coef=0.0), dict(lr=0.1, eps=-1.0),
                dict(lr=0.1, weight_decay=-1.0)):
        with pytest.raises(ValueError):
            dtc.optim.LARS(p, **bad)


def _create(dtc, segs, nseg=None):
    Seg, lib = dtc._native.Seg, dtc._native.lib
    table = (Seg * max(1, len(segs)))(*[Seg(*s) for s in segs])
    h = C.c_void_p()
    rc = lib.dtc_segplan_create(C.byref(h), table, len(segs) if nseg is None else nseg)
    return rc, h


def test_segplan_create_validates_on_the_host(dtc):
    lib, err = dtc._native.lib, dtc._native.last_error
    good = [(0, 10, 0, 0), (64, 100, 1, 0), (192, 8192 * 3 - 6, 1, 0)]
    rc, h = _create(dtc, good)
    assert rc == 0 and h.value
    assert lib.dtc_segplan_num_segments(h) == 3
    nbytes = lib.dtc_segplan_device_bytes(h)
    assert nbytes > 0 and nbytes % 16 == 0
    assert lib.dtc_segplan_destroy(h) == 0
    many = [(64 * i, 1, 0, 0) for i in range(4097)]
    cases = [
        ([(64, 4, 0, 0), (0, 4, 0, 0)], None, "sorted"),            # unsorted
        ([(0, 100, 0, 0), (64, 4, 0, 0)], None, "overlaps"),        # overlapping
        ([(0, 4, 0, 0), (0, 4, 0, 0)], None, "overlaps"),           # not strictly increasing
        ([(2, 4, 0, 0)], None, "multiple of 4"),                     # offset % 4
        ([(-4, 4, 0, 0)], None, "multiple of 4"),
        ([(0, 0, 0, 0)], None, "numel"),
        ([(0, 4, 0, 0)], 0, "nseg"),
        (many, None, "nseg"),
        ([(0, 4, 0, 7)], None, "reserved"),
        ([(0, 4, 2, 0)], None, "flag"),
    ]
    for segs, nseg, word in cases:
        rc, h = _create(dtc, segs, nseg)
        assert rc < 0 and not h.value, (segs[:2], nseg)
        assert word in err(), (word, err())
    rc, h = _create(dtc, many[:4096])  # the largest table
    assert rc == 0 and lib.dtc_segplan_num_segments(h) == 4096
    lib.dtc_segplan_destroy(h)
    assert lib.dtc_segplan_num_segments(None) == 0 and lib.dtc_segplan_device_bytes(None) == 0
    assert lib.dtc_segplan_destroy(None) == 0


def test_segplan_of_the_model_layout(dtc):
    lib = dtc._native.lib
    layout = dtc.nn.Layout()
    plan = dtc.ops.seg_plan(layout)  # no device: created, not bound
    assert plan.nseg == 62 and lib.dtc_segplan_num_segments(plan.handle) == 62 and plan.mem is None
    nbytes = lib.dtc_segplan_device_bytes(plan.handle)
    assert nbytes > 0 and nbytes % 16 == 0
    chunk = lib.dtc_segplan_chunk_elems()
    assert chunk > 0 and chunk % 4 == 0
    nchunks = sum(-(-n // chunk) for _, n, _ in plan.segments)
    assert nbytes >= 62 * 16 + nchunks * 16  # at least the results and one slot of two doubles per chunk
    assert [o for o, _, _ in plan.segments] == sorted(o for o, _, _ in plan.segments)
    assert sum(n for _, n, _ in plan.segments) == 11_220_132 and plan.end <= layout.flat_numel
    by_name = dict(zip(plan.names, plan.segments))
    assert set(plan.names) == {q.name for q in layout.params}
    for q in layout.params:
        assert by_name[q.name] == (q.offset, q.numel, len(q.shape) > 1)
    adapt = {k for k, (_, _, a) in by_name.items() if a}
    assert "linear.weight" in adapt and "conv1.weight" in adapt and "linear.bias" not in adapt
    assert len(adapt) == 21 and not any("bn" in k or k.endswith(".bias") for k in adapt)  # 20 convs + linear.weight


def test_lars_flat_rejects_bad_arguments_before_any_device_call(dtc):
    """Argument checks run on the host ahead of the launches: fake (aligned, non-null) pointers and a plan that was
    never bound reach no GPU."""
    lib, err = dtc._native.lib, dtc._native.last_error
    rc, plan = _create(dtc, [(0, 8, 1, 0)])
    assert rc == 0
    a, off = C.c_void_p(4096), C.c_void_p(4100)

    def lars(plan=plan, p=a, pb=a, lr=0.1, wd=1e-4, mu=0.9, tc=1e-3, eps=1e-8, clip=0):
        return lib.dtc_lars_flat(plan, p, a, a, pb, lr, wd, mu, 1, tc, eps, clip, None, None, None, None)

    for kwargs, word in ((dict(), "not bound"), (dict(plan=None), "null"), (dict(p=None), "null"),
                         (dict(p=off), "aligned"), (dict(pb=C.c_void_p(4098)), "aligned"),
                         (dict(tc=0.0), "trust_coef"), (dict(mu=1.0), "momentum"), (dict(mu=-0.1), "momentum"),
                         (dict(lr=0.0, clip=1), "trust_clip"), (dict(lr=-1.0), "lr"), (dict(wd=-1.0), "weight_decay"),
                         (dict(eps=-1.0), "eps"), (dict(tc=float("nan")), "trust_coef")):
        assert lars(**kwargs) < 0, kwargs
        assert word in err(), (kwargs, err())
    assert lib.dtc_seg_norms(plan, a, a, None, None, None) < 0 and "not bound" in err()
    assert lib.dtc_seg_norms(plan, off, a, None, None, None) < 0 and "aligned" in err()
    assert lib.dtc_segplan_bind(plan, None, 1 << 20, None) < 0 and "null" in err()
    assert lib.dtc_segplan_bind(plan, off, 1 << 20, None) < 0 and "aligned" in err()
    assert lib.dtc_segplan_bind(plan, a, 8, None) < 0 and "bytes" in err()
    lib.dtc_segplan_destroy(plan)


def _lrs(dtc, extra, epochs, lr=0.1):
    p = [torch.nn.Parameter(torch.zeros(4))]
    h = dtc.trainer.load_config(["--lr", str(lr)] + extra, "single")
    opt = dtc.optim.LARS(p, lr=h.lr)
    sched = dtc.trainer.make_scheduler(opt, h)
    out = []
    for _ in range(epochs):  # Trainer.fit: the epoch runs at the current lr, then lr_scheduler.step()
        out.append(opt.param_groups[0]["lr"])
        sched.step()
    return out, sched


def test_warmup_learning_rates(dtc):
    args = ["--lr-decay-step-size", "2", "--lr-decay-gamma", "0.1"]
    got, sched = _lrs(dtc, args + ["--warmup-epochs", "3"], 8)
    want = [0.1 * (e + 1) / 3 if e < 3 else 0.1 * 0.1 ** ((e - 3) // 2) for e in range(8)]
    assert got == pytest.approx(want, rel=1e-12, abs=0.0)
    assert got[2] == 0.1 and got[3] == 0.1  # the full lr is reached at the last warm-up epoch, decay counts from N
    # N = 0: the StepLR object the trainer always built, and its learning rates element for element
    got0, sched0 = _lrs(dtc, args, 8)
    assert type(sched0) is torch.optim.lr_scheduler.StepLR and sched0.step_size == 2 and sched0.gamma == 0.1
    ref_opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(4))], lr=0.1)
    ref = torch.optim.lr_scheduler.StepLR(ref_opt, step_size=2, gamma=0.1)
    plain = []
    for _ in range(8):
        plain.append(ref_opt.param_groups[0]["lr"])
        ref.step()
    assert got0 == plain
