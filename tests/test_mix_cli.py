"""Label smoothing / Mixup / CutMix: the trainer flags and the host-side contract of CrossEntropyLoss and
MixedTarget (CPU only; the kernels are tested in test_gpu_soft_xent*.py and test_gpu_mix_augment.py)."""
import pytest
import torch


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
def test_flags_parse_with_their_defaults(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert (h.label_smoothing, h.mixup_alpha, h.cutmix_alpha, h.mix_prob) == (0.0, 0.0, 0.0, 1.0)
    h = dtc.trainer.load_config(["--device-data", "--label-smoothing", "0.1", "--mixup-alpha", "0.8",
                                 "--cutmix-alpha", "1.0", "--mix-prob", "0.5"], mode)
    assert (h.label_smoothing, h.mixup_alpha, h.cutmix_alpha, h.mix_prob) == (0.1, 0.8, 1.0, 0.5)
    assert dtc.trainer.load_config(["--label-smoothing", "0.1"], mode).label_smoothing == 0.1  # no loader needed


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
@pytest.mark.parametrize("argv", [["--mixup-alpha", "1"], ["--cutmix-alpha", "0.5"], ["--label-smoothing", "1.5"],
                                  ["--device-data", "--mixup-alpha", "-1"], ["--device-data", "--mix-prob", "2"]])
def test_bad_flag_combinations_are_argument_errors(dtc, mode, argv):
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(argv, mode)


def test_defaults_carry_no_soft_or_mix_state(dtc):
    h = dtc.trainer.load_config(["--device-data"], "single")
    crit, eval_crit = dtc.trainer.make_criteria(h)
    assert crit is eval_crit and crit.label_smoothing == 0.0
    assert dtc.trainer.mix_kwargs(h) == {}
    assert dtc.CrossEntropyLoss().label_smoothing == 0.0
    h = dtc.trainer.load_config(["--device-data", "--label-smoothing", "0.1", "--cutmix-alpha", "1"], "single")
    crit, eval_crit = dtc.trainer.make_criteria(h)
    assert crit.label_smoothing == 0.1 and eval_crit.label_smoothing == 0.0  # evaluation stays plain
    assert dtc.trainer.mix_kwargs(h) == {"mixup_alpha": 0.0, "cutmix_alpha": 1.0, "mix_prob": 1.0}


def test_cross_entropy_unbuilt_variants_raise(dtc):
    for kw in (dict(weight=torch.ones(3)), dict(ignore_index=0), dict(reduction="sum"), dict(reduction="none")):
        with pytest.raises(NotImplementedError):
            dtc.CrossEntropyLoss(**kw)
    with pytest.raises(ValueError):
        dtc.CrossEntropyLoss(label_smoothing=1.5)
    for eps in (0.0, 0.1):  # probability-tensor targets, with and without smoothing
        with pytest.raises(NotImplementedError):
            dtc.CrossEntropyLoss(label_smoothing=eps)(torch.zeros(2, 3), torch.full((2, 3), 1 / 3))
    with pytest.raises(dtc.NativeError):  # no CPU fallback for the soft routes either
        dtc.CrossEntropyLoss(label_smoothing=0.1)(torch.zeros(2, 3), torch.zeros(2, dtype=torch.long))


def test_mixed_target_to_returns_itself(dtc):
    t = dtc.MixedTarget(torch.zeros(2, dtype=torch.long), torch.ones(2, dtype=torch.long), torch.full((2,), 0.5))
    assert t.to("cpu") is t and t.to(torch.device("cpu"), non_blocking=True) is t
    assert dtc.MixedTarget is dtc.nn.MixedTarget


def test_eval_loader_refuses_mixing(dtc):
    import inspect

    import numpy as np

    sig = inspect.signature(dtc.data.DeviceLoader.__init__)
    assert [sig.parameters[k].default for k in ("mixup_alpha", "cutmix_alpha", "mix_prob")] == [0.0, 0.0, 1.0]
    imgs, tg = np.zeros((4, 32, 32, 3), np.uint8), np.zeros(4, np.int64)
    for kw in (dict(mixup_alpha=1.0), dict(cutmix_alpha=0.5)):  # refused before anything touches a device
        with pytest.raises(ValueError, match="training"):
            dtc.data.DeviceLoader(imgs, tg, 2, train=False, device="cpu", **kw)
    with pytest.raises(ValueError, match="mix_prob"):
        dtc.data.DeviceLoader(imgs, tg, 2, device="cpu", mixup_alpha=1.0, mix_prob=2.0)


def test_soft_abi_rejects_bad_arguments_before_any_device_call(dtc):
    """Argument checks run on the host ahead of the launches: fake (aligned, non-null) pointers never reach a GPU."""
    import ctypes as C
    lib = dtc._native.lib
    a = C.c_void_p(4096)

    def fwd(lb=None, lam=None, eps=0.1, n=8):
        return lib.dtc_xent_soft_fwd_ex(a, a, lb, lam, eps, n, 100, a, a, None, None, None, None)

    def bwd(lb=None, lam=None, eps=0.1):
        return lib.dtc_xent_soft_bwd(a, a, lb, lam, eps, a, None, 8, 100, a, None)

    for f in (fwd, bwd):
        for kw in (dict(eps=1.5), dict(eps=-0.1), dict(eps=float("nan")), dict(lb=a), dict(lam=a)):
            assert f(**kw) < 0, kw
            assert "smoothing" in dtc._native.last_error()
    assert fwd(n=4097) < 0 and fwd(n=0) < 0
    assert lib.dtc_rn18_xent_soft_backward(None, a, a, None, None, 0.0, a, None, 1.0, None, None) < 0
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    s = (C.c_float * 3)(0.2, 0.2, 0.2)

    def mix(mode=1, lam=a, box=None, w=32):
        return lib.dtc_cifar_augment_mix(a, a, 10, None, None, None, 4, 32, w, 4, m, s, None, mode, lam, box, a, a, a,
                                         None, None)

    for kw in (dict(mode=0), dict(mode=3), dict(mode=1, lam=None), dict(mode=2, box=None), dict(w=30)):
        assert mix(**kw) < 0, kw
