"""Optimizer choice and gradient clipping: CLI flags and the host-side contract of optim.Adam / AdamW /
clip_grad_norm_ (CPU only; the kernels are tested in test_gpu_optim.py)."""
import pytest
import torch


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
def test_optimizer_and_clip_flags(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert h.optimizer == "sgd" and h.clip_grad_norm == 0.0
    h = dtc.trainer.load_config(["--optimizer", "adamw", "--clip-grad-norm", "1.5"], mode)
    assert h.optimizer == "adamw" and h.clip_grad_norm == 1.5
    assert dtc.trainer.load_config(["--optimizer=adam"], mode).optimizer == "adam"
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--optimizer", "lamb"], mode)


def test_adam_defaults_match_torch(dtc):
    p = [torch.nn.Parameter(torch.zeros(4))]
    for ours, theirs in ((dtc.optim.Adam, torch.optim.Adam), (dtc.optim.AdamW, torch.optim.AdamW)):
        d, ref = ours(p).defaults, theirs(p).defaults
        for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize"):
            assert d[k] == ref[k], (ours.__name__, k)
        assert isinstance(ours(p), torch.optim.Optimizer)
    assert dtc.optim.Adam(p).defaults["weight_decay"] == 0 and dtc.optim.AdamW(p).defaults["weight_decay"] == 1e-2
    assert dtc.Adam is dtc.optim.Adam and dtc.AdamW is dtc.optim.AdamW
    assert dtc.clip_grad_norm_ is dtc.optim.clip_grad_norm_
    opt = dtc.optim.AdamW(p, lr=0.5)
    torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)  # drives param_groups[0]['lr']
    assert opt.param_groups[0]["lr"] == 0.5


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_adam_unimplemented_variants_raise(dtc, name):
    cls = getattr(dtc.optim, name)
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(NotImplementedError):
        cls(p, amsgrad=True)
    with pytest.raises(NotImplementedError):
        cls(p, maximize=True)
    with pytest.raises(NotImplementedError):
        cls([{"params": p}])
    with pytest.raises(NotImplementedError):
        cls(p).step(closure=lambda: 0.0)
    assert cls(p).zero_grad() is None


def test_sgd_keeps_its_contract(dtc):
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(NotImplementedError):
        dtc.optim.SGD(p, lr=0.1)  # no momentum / nesterov
    with pytest.raises(NotImplementedError):
        dtc.optim.SGD([{"params": p}], lr=0.1, momentum=0.9, nesterov=True)
    opt = dtc.optim.SGD(p, lr=0.1, momentum=0.9, nesterov=True)
    assert opt._flat is None  # GradScaler reaches for this attribute
    with pytest.raises(NotImplementedError):
        opt.step(closure=lambda: 0.0)


def test_clip_grad_norm_rejects_other_norms_and_foreign_parameters(dtc):
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(NotImplementedError):
        dtc.optim.clip_grad_norm_(p, 1.0, norm_type=1)
    with pytest.raises(NotImplementedError):
        dtc.optim.clip_grad_norm_(p, 1.0, norm_type=float("inf"))
    with pytest.raises(dtc.NativeError):  # not the parameters of a native model on the GPU
        dtc.optim.clip_grad_norm_(p, 1.0)


def test_new_abi_host_queries(dtc):
    lib = dtc._native.lib
    assert lib.dtc_adam_state_words() == 4
    assert lib.dtc_grad_norm_workspace_bytes(0) == 0 and lib.dtc_grad_norm_workspace_bytes(-4) == 0
    assert lib.dtc_grad_norm_workspace_bytes(4) == 8  # one workgroup, one double
    big = lib.dtc_grad_norm_workspace_bytes(11_220_132 + 60)
    assert big % 8 == 0 and 8 < big <= 8 * 1024
    assert lib.dtc_grad_norm_workspace_bytes(1 << 33) == big  # capped grid


def test_abi_rejects_bad_arguments_before_any_device_call(dtc):
    """Argument checks run on the host ahead of the launches: fake (aligned, non-null) pointers never reach a GPU."""
    import ctypes as C
    lib = dtc._native.lib
    a, off = C.c_void_p(4096), C.c_void_p(4100)

    def adam(p=a, n=8, state=a, eps=1e-8, b1=0.9, b2=0.999):
        return lib.dtc_adam_flat(p, a, a, a, a, n, state, 1e-3, b1, b2, eps, 0.0, 0, None, None, None)

    for kwargs, word in ((dict(n=6), "multiple of 4"), (dict(n=0), "multiple of 4"), (dict(p=off), "aligned"),
                         (dict(p=None), "null"), (dict(state=None), "null"), (dict(eps=0.0), "eps"),
                         (dict(b2=1.0), "betas"), (dict(b1=-0.1), "betas")):
        assert adam(**kwargs) < 0, kwargs
        assert word in dtc._native.last_error(), (kwargs, dtc._native.last_error())

    def norm(g=a, n=8, max_norm=1.0, ws=a, out=a):
        return lib.dtc_grad_norm_clip(g, n, None, max_norm, ws, out, out, None)

    for kwargs, word in ((dict(n=6), "multiple of 4"), (dict(g=off), "aligned"), (dict(g=None), "null"),
                         (dict(ws=None), "null"), (dict(out=None), "null"), (dict(max_norm=0.0), "max_norm"),
                         (dict(max_norm=float("nan")), "max_norm")):
        assert norm(**kwargs) < 0, kwargs
        assert word in dtc._native.last_error(), (kwargs, dtc._native.last_error())
