"""Augmentation policies and RandomErasing: the trainer flags, the DeviceLoader keywords and the host-side argument
checks of dtc_cifar_augment_policy (CPU only; the kernel is tested in test_gpu_augment_policy.py)."""
import numpy as np
import pytest


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
def test_flags_parse_with_their_defaults(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert (h.auto_augment, h.ra_num_ops, h.ra_magnitude, h.random_erasing) == ("none", 2, 9, 0.0)
    h = dtc.trainer.load_config(["--device-data", "--auto-augment", "randaugment", "--ra-num-ops", "3",
                                 "--ra-magnitude", "14", "--random-erasing", "0.25"], mode)
    assert (h.auto_augment, h.ra_num_ops, h.ra_magnitude, h.random_erasing) == ("randaugment", 3, 14, 0.25)
    h = dtc.trainer.load_config(["--device-data", "--auto-augment", "trivialwide", "--cutmix-alpha", "1"], mode)
    assert h.auto_augment == "trivialwide" and h.cutmix_alpha == 1.0  # a policy does combine with Mixup / CutMix


@pytest.mark.parametrize("mode", ["single", "dp", "ddp"])
@pytest.mark.parametrize("argv", [
    ["--auto-augment", "randaugment"], ["--random-erasing", "0.25"],  # no --device-data
    ["--device-data", "--auto-augment", "autoaugment"],
    ["--device-data", "--ra-num-ops", "0"], ["--device-data", "--ra-num-ops", "5"],
    ["--device-data", "--ra-magnitude", "31"], ["--device-data", "--ra-magnitude", "-1"],
    ["--device-data", "--random-erasing", "1.5"], ["--device-data", "--random-erasing", "-0.1"],
    ["--device-data", "--random-erasing", "0.25", "--mixup-alpha", "1"],
    ["--device-data", "--random-erasing", "0.25", "--cutmix-alpha", "1"]])
def test_bad_flag_combinations_are_argument_errors(dtc, mode, argv):
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(argv, mode)


def test_policy_kwargs(dtc):
    T = dtc.trainer
    assert T.policy_kwargs(T.load_config(["--device-data"], "single")) == {}
    assert T.policy_kwargs(T.load_config([], "ddp")) == {}
    h = T.load_config(["--device-data", "--auto-augment", "randaugment", "--random-erasing", "0.25"], "single")
    assert T.policy_kwargs(h) == {"policy": "randaugment", "policy_num_ops": 2, "policy_magnitude": 9,
                                  "erase_prob": 0.25}
    h = T.load_config(["--device-data", "--random-erasing", "0.1"], "single")
    assert T.policy_kwargs(h)["policy"] == "none" and T.policy_kwargs(h)["erase_prob"] == 0.1
    assert T.mix_kwargs(h) == {}


def test_device_loader_keywords(dtc):
    import inspect

    sig = inspect.signature(dtc.data.DeviceLoader.__init__)
    assert [sig.parameters[k].default for k in ("policy", "policy_num_ops", "policy_magnitude", "erase_prob")] == \
        ["none", 2, 9, 0.0]
    imgs, tg = np.zeros((4, 32, 32, 3), np.uint8), np.zeros(4, np.int64)
    mk = lambda **kw: dtc.data.DeviceLoader(imgs, tg, 2, device="cpu", **kw)  # refused before any device call
    for kw in (dict(policy="randaugment"), dict(policy="trivialwide"), dict(erase_prob=0.25)):
        with pytest.raises(ValueError, match="training"):
            mk(train=False, **kw)
    with pytest.raises(ValueError, match="Mixup"):
        mk(erase_prob=0.25, cutmix_alpha=1.0)
    for kw in (dict(policy="autoaugment"), dict(policy_num_ops=5), dict(policy_num_ops=0), dict(policy_magnitude=31),
               dict(erase_prob=1.5)):
        with pytest.raises(ValueError):
            mk(**kw)
    plain = mk()
    assert not plain.policing and plain.last_policy is None
    assert mk(policy="randaugment", mixup_alpha=1.0).policing and mk(erase_prob=0.1).policing


def test_policy_abi_rejects_bad_arguments_before_any_device_call(dtc):
    """Argument checks run on the host ahead of the launch: fake (aligned, non-null) pointers never reach a GPU."""
    import ctypes as C

    lib = dtc._native.lib
    a = C.c_void_p(4096)
    m = (C.c_float * 3)(0.5, 0.5, 0.5)
    s = (C.c_float * 3)(0.2, 0.2, 0.2)

    def pol(out=a, out_u8=None, erase=None, n_ops=2, w=32, ops=a, args=a):
        return lib.dtc_cifar_augment_policy(a, a, 10, None, None, None, 4, 32, w, 4, m, s, ops, args, n_ops, erase,
                                            out, out_u8, a, None, None)

    for kw in (dict(out=a, out_u8=a), dict(out=None, out_u8=None), dict(out=None, out_u8=a, erase=a),
               dict(n_ops=5), dict(n_ops=-1), dict(w=30), dict(ops=None), dict(args=None)):
        assert pol(**kw) < 0, kw
        assert "cifar_augment_policy" in dtc._native.last_error()
    with pytest.raises(dtc.NativeError):  # and no host fallback behind the wrapper
        import torch

        dtc.ops.cifar_augment_policy(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), None, None, None, (0.5,) * 3,
                                     (0.2,) * 3)
