"""LAMB: CLI flags, the host-side contract of optim.LAMB and the argument checks of dtc_lamb_flat through the raw ABI
(CPU only; the kernels are tested in test_gpu_lamb.py)."""
import ctypes as C

import pytest
import torch


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
def test_lamb_flags(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert h.lamb is False and h.lamb_max_trust == 0.0
    h = dtc.trainer.load_config(["--optimizer", "adamw", "--lamb", "--lamb-max-trust", "10", "--lr", "0.002"], mode)
    assert h.optimizer == "adamw" and h.lamb is True and h.lamb_max_trust == 10.0 and h.lr == 0.002
    for bad in (["--lamb"], ["--lamb", "--optimizer", "adam"], ["--lamb", "--optimizer", "lars"],
                ["--optimizer", "adamw", "--lamb", "--lamb-max-trust", "-1"]):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(bad, mode)
    assert "lamb" in dtc.trainer.RESUME_KEYS and "lamb_max_trust" in dtc.trainer.RESUME_KEYS


def test_lamb_is_a_torch_optimizer(dtc):
    p = [torch.nn.Parameter(torch.zeros(4))]
    opt = dtc.optim.LAMB(p)
    assert isinstance(opt, torch.optim.Optimizer) and dtc.LAMB is dtc.optim.LAMB
    assert opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, bias_correction=True,
                                max_trust=0.0)
    assert opt._flat is None and opt._get_step() == 0  # GradScaler reaches for _flat
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)
    opt.zero_grad()
    sched.step()
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-4, rel=1e-12)
    sam = dtc.optim.SAM(dtc.optim.LAMB(p, lr=0.5), rho=0.1)
    assert sam.param_groups is sam.base.param_groups and sam.param_groups[0]["lr"] == 0.5
    for call in (opt.step, opt.layer_norms):  # not the parameters of a native model on the GPU / no step yet
        with pytest.raises(dtc.NativeError):
            call()
    for bad in (dict(lr=-1.0), dict(eps=0.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)),
                dict(weight_decay=-1.0), dict(max_trust=-1.0)):
        with pytest.raises(ValueError):
            dtc.optim.LAMB(p, **bad)


def test_lamb_flat_rejects_bad_arguments_before_any_device_call(dtc):
    """Host-side checks ahead of the launches: fake (aligned, non-null) pointers and an unbound plan reach no GPU."""
    lib, err = dtc._native.lib, dtc._native.last_error
    assert lib.dtc_lamb_state_words() == 4
    plan = C.c_void_p()
    assert lib.dtc_segplan_create(C.byref(plan), (dtc._native.Seg * 1)(dtc._native.Seg(0, 8, 1, 0)), 1) == 0
    a, off = C.c_void_p(4096), C.c_void_p(4100)

    def lamb(plan=plan, p=a, v=a, pb=a, state=a, lr=0.1, b1=0.9, b2=0.999, eps=1e-6, wd=0.01, mt=0.0):
        return lib.dtc_lamb_flat(plan, p, a, a, v, pb, state, lr, b1, b2, eps, wd, 1, mt, None, None, None, None)

    for kwargs, word in ((dict(), "not bound"), (dict(plan=None), "null"), (dict(v=None), "null"),
                         (dict(state=None), "null"), (dict(p=off), "aligned"), (dict(state=off), "aligned"),
                         (dict(pb=C.c_void_p(4098)), "aligned"), (dict(b1=1.0), "betas"), (dict(b2=-0.1), "betas"),
                         (dict(eps=0.0), "eps"), (dict(lr=-1.0), "lr"), (dict(wd=-1.0), "weight_decay"),
                         (dict(mt=-1.0), "max_trust"), (dict(mt=float("nan")), "max_trust")):
        assert lamb(**kwargs) < 0, kwargs
        assert word in err(), (kwargs, err())
    lib.dtc_segplan_destroy(plan)
