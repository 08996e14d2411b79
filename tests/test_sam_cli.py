"""SAM / ASAM: the --sam-rho / --sam-adaptive flags, the optimizer wrapper's host-side behaviour, and the argument
checks of dtc_sam_perturb / dtc_sam_restore through the raw ABI (CPU only; the kernels, the two-pass step and the
model's local_grads() are tested in test_gpu_sam.py)."""
import ctypes as C

import pytest
import torch


@pytest.mark.parametrize("mode", ["single", "ddp"])
def test_sam_flags(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert h.sam_rho == 0.0 and h.sam_adaptive is False
    h = dtc.trainer.load_config(["--sam-rho", "0.05"], mode)
    assert h.sam_rho == 0.05 and h.sam_adaptive is False
    h = dtc.trainer.load_config(["--sam-rho", "2.0", "--sam-adaptive", "--optimizer", "lars", "--amp",
                                 "--clip-grad-norm", "1.0", "--model-ema", "--label-smoothing", "0.1"], mode)
    assert h.sam_rho == 2.0 and h.sam_adaptive is True
    assert dtc.trainer.load_config(["--sam-rho", "0.05", "--accum-steps", "1"], mode).sam_rho == 0.05
    for bad in (["--sam-rho", "-0.1"], ["--sam-rho", "nan"], ["--sam-rho", "0.05", "--accum-steps", "2"]):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(bad, mode)


def test_sam_flags_with_the_ddp_only_options(dtc):
    h = dtc.trainer.load_config(["--sam-rho", "0.05", "--sync-bn", "--grad-compress", "bf16"], "ddp")
    assert h.sam_rho == 0.05 and h.sync_bn and h.grad_compress == "bf16"


def test_sam_is_refused_under_data_parallel(dtc):
    assert dtc.trainer.load_config([], "dp").sam_rho == 0.0
    assert dtc.trainer.load_config(["--sam-rho", "0"], "dp").sam_rho == 0.0
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--sam-rho", "0.05"], "dp")


def _base(dtc, kind, params):
    if kind == "sgd":
        return dtc.SGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    if kind == "lars":
        return dtc.LARS(params, lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    return {"adam": dtc.Adam, "adamw": dtc.AdamW}[kind](params, lr=0.1)


@pytest.mark.filterwarnings("ignore:Detected call of")
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw", "lars"])
def test_wrapper_shares_param_groups_with_the_base(dtc, kind):
    base = _base(dtc, kind, dtc.ResNet18().parameters())
    sam = dtc.SAM(base, rho=0.1, adaptive=True)
    assert isinstance(sam, torch.optim.Optimizer)
    assert sam.param_groups is base.param_groups
    assert (sam.rho, sam.adaptive, sam.eps) == (0.1, True, 1e-12)
    assert sam._flat is None and sam.zero_grad() is None
    sched = torch.optim.lr_scheduler.StepLR(sam, step_size=1, gamma=0.1)
    sched.step()
    assert base.param_groups[0]["lr"] == pytest.approx(0.01)
    sched.step()
    assert base.param_groups[0]["lr"] == pytest.approx(0.001) and sam.param_groups[0]["lr"] == pytest.approx(0.001)


def test_wrapper_validates_its_arguments(dtc):
    params = list(dtc.ResNet18().parameters())
    base = _base(dtc, "sgd", params)
    assert dtc.SAM(base, rho=0.0).rho == 0.0  # legal: the perturbation is zero
    assert dtc.optim.SAM is dtc.SAM
    for kw in ({"rho": -0.1}, {"rho": float("nan")}, {"eps": 0.0}, {"eps": -1e-12}):
        with pytest.raises(ValueError):
            dtc.SAM(base, **kw)
    with pytest.raises(TypeError):
        dtc.SAM(torch.optim.SGD(params, lr=0.1))
    sam = dtc.SAM(base)
    with pytest.raises(dtc.NativeError, match="first_step"):
        sam.step()
    with pytest.raises(dtc.NativeError, match="first_step"):
        sam.grad_norm
    with pytest.raises(dtc.NativeError):  # the model is not on a GPU: nothing to bind to
        sam.first_step()


def test_local_grads_state_of_the_module(dtc):
    m = dtc.ResNet18()
    assert m._local_depth == 0
    with m.local_grads() as inner:
        assert inner is m and m._local_depth == 1
    with pytest.raises(RuntimeError, match="boom"):
        with m.local_grads():
            raise RuntimeError("boom")
    assert m._local_depth == 0
    with m.accumulate():
        with pytest.raises(dtc.NativeError, match="accumulation window"):
            with m.local_grads():
                pass
    m._accum_open = True
    with pytest.raises(dtc.NativeError, match="accumulation window"):
        with m.local_grads():
            pass
    m.reset_accumulation()
    m.grad_accum_steps = 2
    with pytest.raises(dtc.NativeError, match="grad_accum_steps"):
        with m.local_grads():
            pass
    assert m._local_depth == 0
    assert not hasattr(dtc.DistributedDataParallel, "local_grads")  # no new public method on the wrapper


def test_new_symbols_are_bound(dtc):
    lib = dtc._native.lib
    for name in ("dtc_sam_state_words", "dtc_sam_workspace_bytes", "dtc_sam_perturb", "dtc_sam_restore"):
        assert name in dtc._native.SYMBOLS and hasattr(lib, name)
    assert lib.dtc_sam_state_words() == 4
    assert lib.dtc_sam_workspace_bytes(4) == 8  # one workgroup, one double
    assert lib.dtc_sam_workspace_bytes(0) == 0
    assert lib.dtc_sam_workspace_bytes(1 << 24) == 256 * 8  # the norm pass's grid cap
    assert C.sizeof(dtc._native.SamKeep) == 24 and dtc._native.SAM_MAX_KEEP == 4
    assert lib.dtc_abi_version() == 1  # no existing signature changed
    for f in ("sam_state", "sam_workspace", "sam_perturb", "sam_restore"):
        assert callable(getattr(dtc.ops, f))


# fake (non-null) addresses, far apart: p, g, p_saved, p_bf16, state, workspace
P, G, SV, PB, ST, WS = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20


def _keep(dtc, *recs):
    return (dtc._native.SamKeep * max(1, len(recs)))(*[dtc._native.SamKeep(*r) for r in recs])


def _perturb(dtc, p=P, g=G, sv=SV, pb=PB, n=8, rho=0.05, eps=1e-12, adaptive=0, gmul=None, keep=None, nkeep=0,
             state=ST, ws=WS):
    return dtc._native.lib.dtc_sam_perturb(p, g, sv, pb, n, rho, eps, adaptive, gmul, keep, nkeep, state, ws, None)


def _restore(dtc, p=P, sv=SV, pb=PB, n=8, keep=None, nkeep=0, state=ST, found=None):
    return dtc._native.lib.dtc_sam_restore(p, sv, pb, n, keep, nkeep, state, found, None)


def test_perturb_rejects_bad_arguments_before_any_device_call(dtc):
    """Fake pointers reach no GPU: every check runs on the host ahead of the first launch, and the message names
    the argument at fault."""
    err = dtc._native.last_error
    live, saved = 7 << 20, 8 << 20
    cases = [
        (dict(p=None), "null pointer (p)"), (dict(g=None), "null pointer (g)"),
        (dict(sv=None), "null pointer (p_saved)"), (dict(pb=None), "null pointer (p_bf16)"),
        (dict(state=None), "null pointer (state)"), (dict(ws=None), "null pointer (workspace)"),
        (dict(n=0), "n = 0"), (dict(n=-4), "n = -4"), (dict(n=6), "n = 6"),
        (dict(p=P + 4), "p and p_saved"), (dict(sv=SV + 8), "p and p_saved"), (dict(g=G + 4), "g must"),
        (dict(pb=PB + 4), "p_bf16"), (dict(state=ST + 8), "state"), (dict(ws=WS + 4), "workspace"),
        (dict(sv=P + 16), "p_saved overlaps p"), (dict(sv=P - 16), "p_saved overlaps p"),
        (dict(sv=G + 16), "p_saved overlaps g"),
        (dict(rho=-0.05), "rho"), (dict(rho=float("nan")), "rho"), (dict(eps=0.0), "eps"), (dict(eps=-1.0), "eps"),
        (dict(eps=float("nan")), "eps"),
        (dict(nkeep=-1), "nkeep"), (dict(nkeep=5, keep=_keep(dtc, (live, saved, 8))), "nkeep"),
        (dict(nkeep=1, keep=None), "keep"),
        (dict(nkeep=1, keep=_keep(dtc, (None, saved, 8))), "keep 0: null"),
        (dict(nkeep=1, keep=_keep(dtc, (live, None, 8))), "keep 0: null"),
        (dict(nkeep=1, keep=_keep(dtc, (live + 4, saved, 8))), "keep 0: live and saved"),
        (dict(nkeep=1, keep=_keep(dtc, (live, saved + 4, 8))), "keep 0: live and saved"),
        (dict(nkeep=1, keep=_keep(dtc, (live, saved, 12))), "keep 0: bytes = 12"),
        (dict(nkeep=1, keep=_keep(dtc, (live, saved, 0))), "keep 0: bytes = 0"),
        (dict(nkeep=1, keep=_keep(dtc, (live, live + 8, 16))), "keep 0: live and saved overlap"),
        (dict(nkeep=2, keep=_keep(dtc, (live, saved, 64), (9 << 20, saved + 56, 64))), "keep 0 and keep 1 overlap"),
        (dict(nkeep=2, keep=_keep(dtc, (live, saved, 64), (live + 8, 9 << 20, 64))), "keep 0 and keep 1 overlap"),
    ]
    for kw, word in cases:
        assert _perturb(dtc, **kw) == -1, kw
        assert "sam_perturb" in err() and word in err(), (kw, err())


def test_restore_rejects_bad_arguments_before_any_device_call(dtc):
    err = dtc._native.last_error
    live, saved = 7 << 20, 8 << 20
    cases = [
        (dict(p=None), "null pointer (p)"), (dict(sv=None), "null pointer (p_saved)"),
        (dict(pb=None), "null pointer (p_bf16)"), (dict(state=None), "null pointer (state)"),
        (dict(n=0), "n = 0"), (dict(n=10), "n = 10"),
        (dict(p=P + 8), "p and p_saved"), (dict(sv=SV + 4), "p and p_saved"), (dict(pb=PB + 2), "p_bf16"),
        (dict(state=ST + 4), "state"), (dict(sv=P), "p_saved overlaps p"),
        (dict(nkeep=5, keep=_keep(dtc, (live, saved, 8))), "nkeep"), (dict(nkeep=2, keep=None), "keep"),
        (dict(nkeep=1, keep=_keep(dtc, (live, saved, 4))), "keep 0: bytes = 4"),
        (dict(nkeep=1, keep=_keep(dtc, (live, live, 8))), "keep 0: live and saved overlap"),
    ]
    for kw, word in cases:
        assert _restore(dtc, **kw) == -1, kw
        assert "sam_restore" in err() and word in err(), (kw, err())
