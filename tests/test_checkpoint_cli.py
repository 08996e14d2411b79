"""Training checkpoints, the host side: the --checkpoint-every / --resume flags, dtc.checkpoint's file format,
GradScaler.load_state_dict before the device words exist, the optimizers' refusal of foreign parameters and the
flag comparison of --resume (CPU only; the bit-exact continuation is tested in test_gpu_checkpoint.py)."""
import argparse
import os
import random

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("mode", ["single", "ddp"])
def test_flags_parse(dtc, mode):
    h = dtc.trainer.load_config([], mode)
    assert h.checkpoint_every == 0 and h.resume is None
    h = dtc.trainer.load_config(["--checkpoint-every", "5", "--resume", "runs/version-3"], mode)
    assert h.checkpoint_every == 5 and h.resume == "runs/version-3"
    assert dtc.trainer.load_config(["--checkpoint-every", "0"], mode).checkpoint_every == 0
    with pytest.raises(SystemExit):
        dtc.trainer.load_config(["--checkpoint-every", "-1"], mode)


def test_flags_are_refused_under_data_parallel(dtc, capsys):
    h = dtc.trainer.load_config([], "dp")
    assert h.checkpoint_every == 0 and h.resume is None
    for argv in (["--checkpoint-every", "1"], ["--resume", "x"]):
        with pytest.raises(SystemExit):
            dtc.trainer.load_config(argv, "dp")
        assert "single and ddp only" in capsys.readouterr().err


def test_save_load_round_trip_and_rng(dtc, tmp_path):
    ck = dtc.checkpoint
    for seed_fn in (torch.manual_seed, np.random.seed, random.seed):
        seed_fn(1234)
    np.random.standard_normal()  # leaves a cached gaussian in numpy's state
    random.gauss(0.0, 1.0)       # and one in random's
    strided = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4).permute(2, 0, 1)
    state = {ck.FORMAT_KEY: ck.FORMAT, "rng": ck.get_rng_state(),
             "nested": ck.to_plain({"t": strided, "n": 3, "x": 0.25, "s": "name", "b": b"\x00\x01", "none": None,
                                    "list": [1, (2.0, "three")], 7: torch.tensor(5, dtype=torch.int32),
                                    "np": np.float32(1.5)})}
    want = (torch.rand(3), np.random.rand(3), np.random.standard_normal(2), [random.random() for _ in range(3)],
            random.gauss(0.0, 1.0))
    path = str(tmp_path / "last.ckpt")
    ck.save(path, state)
    assert sorted(os.listdir(tmp_path)) == ["last.ckpt"]  # written through last.ckpt.tmp, which is gone
    got = ck.load(path)
    n = got["nested"]
    assert torch.equal(n["t"], strided) and n["t"].is_contiguous() and n["t"].untyped_storage().nbytes() == 24 * 4
    assert (n["n"], n["x"], n["s"], n["b"], n["none"], n["np"]) == (3, 0.25, "name", b"\x00\x01", None, 1.5)
    assert n["list"] == [1, (2.0, "three")] and n[7].dtype == torch.int32 and int(n[7]) == 5
    for seed_fn in (torch.manual_seed, np.random.seed, random.seed):
        seed_fn(99)  # somewhere else entirely
    ck.set_rng_state(got["rng"])
    again = (torch.rand(3), np.random.rand(3), np.random.standard_normal(2), [random.random() for _ in range(3)],
             random.gauss(0.0, 1.0))
    assert torch.equal(again[0], want[0]) and np.array_equal(again[1], want[1]) and np.array_equal(again[2], want[2])
    assert again[3] == want[3] and again[4] == want[4]


def test_capturing_the_rng_draws_nothing(dtc):
    torch.manual_seed(5)
    np.random.seed(5)
    random.seed(5)
    before = dtc.checkpoint.get_rng_state()
    after = dtc.checkpoint.get_rng_state()
    assert torch.equal(before["torch"], after["torch"]) and torch.equal(before["numpy"]["keys"], after["numpy"]["keys"])
    assert before["numpy"]["pos"] == after["numpy"]["pos"] and before["random"] == after["random"]


def test_to_plain_refuses_objects(dtc):
    with pytest.raises(TypeError, match=r"state\['a'\]\[1\]"):
        dtc.checkpoint.to_plain({"a": [1, object()]})
    with pytest.raises(TypeError, match="key"):
        dtc.checkpoint.to_plain({(1, 2): 3})


def test_load_refuses_unknown_tags_and_pickled_objects(dtc, tmp_path):
    ck = dtc.checkpoint
    for k, state in enumerate(({ck.FORMAT_KEY: ck.FORMAT + 1, "x": 1}, {"x": torch.zeros(2)}, [1, 2])):
        path = str(tmp_path / f"tag{k}.ckpt")
        torch.save(state, path)
        with pytest.raises(ck.CheckpointError, match="format tag"):
            ck.load(path)
    path = str(tmp_path / "object.ckpt")
    torch.save({ck.FORMAT_KEY: ck.FORMAT, "hparams": argparse.Namespace(lr=0.1)}, path)
    with pytest.raises(ck.CheckpointError, match="plain values"):
        ck.load(path)
    with pytest.raises(ck.CheckpointError, match="format tag"):
        ck.restore({"model": {}}, None, None)


def test_grad_scaler_load_before_lazy_init(dtc):
    sd = {"scale": 1024.0, "growth_factor": 3.0, "backoff_factor": 0.25, "growth_interval": 17, "_growth_tracker": 11}
    sc = dtc.GradScaler()
    version = sc._version
    sc.load_state_dict(sd)
    assert sc.state_dict() == sd and sc.get_scale() == 1024.0 and sc._version > version
    assert sc._scale is None  # still lazy: the device words are created with these values
    with pytest.raises(KeyError, match="_growth_tracker"):
        sc.load_state_dict({k: v for k, v in sd.items() if k != "_growth_tracker"})
    with pytest.raises(ValueError):
        sc.load_state_dict({**sd, "scale": 0.0})
    assert dtc.GradScaler().state_dict()["_growth_tracker"] == 0  # untouched default


def _stepped(opt, params):
    g = torch.Generator().manual_seed(0)
    for _ in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt.state_dict()


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_optimizer_load_on_foreign_parameters_is_refused(dtc, kind):
    """Before load_state_dict was implemented the call returned silently and loaded nothing."""
    params = [torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(5))]
    if kind == "sgd":
        ref = torch.optim.SGD(params, lr=0.1, momentum=0.9, nesterov=True)
        opt = dtc.optim.SGD(params, lr=0.1, momentum=0.9, nesterov=True)
    else:
        ref = torch.optim.Adam(params, lr=0.1)
        opt = dtc.optim.Adam(params, lr=0.1)
    sd = _stepped(ref, params)
    assert len(sd["state"]) == 2
    with pytest.raises(dtc.NativeError, match="do not belong to a native ResNet"):
        opt.load_state_dict(sd)
    with pytest.raises(dtc.NativeError):  # a native model that was never moved to the GPU: nothing to bind to
        dtc.optim.SGD(dtc.ResNet18().parameters(), lr=0.1, momentum=0.9, nesterov=True).load_state_dict(sd)
    # not attached: torch's shell with an empty state, as ever
    shell = opt.state_dict()
    assert shell["state"] == {} and shell["param_groups"][0]["params"] == [0, 1]


def test_hparam_mismatch_names_the_state_shaping_keys(dtc):
    tr = dtc.trainer
    base = ["--amp", "--optimizer", "adamw", "--model-ema", "--batch-size", "8"]
    saved = vars(tr.load_config(base + ["--epoch", "1", "--checkpoint-every", "1", "--workers", "0"], "single"))
    same = vars(tr.load_config(base + ["--epoch", "3", "--resume", "somewhere", "--eval-step", "7", "--contain-test",
                                       "--workers", "2"], "single"))
    assert tr.hparam_mismatch(saved, same) == []
    other = vars(tr.load_config(["--optimizer", "lars", "--model-ema", "--batch-size", "16", "--seed", "7",
                                 "--epoch", "3", "--lr-decay-step-size", "2"], "single"))
    diff = tr.hparam_mismatch(saved, other)
    assert [k for k, _, _ in diff] == ["seed", "batch_size", "amp", "optimizer", "lr_decay_step_size"]
    assert ("optimizer", "adamw", "lars") in diff and ("batch_size", 8, 16) in diff
    assert "epoch" not in tr.RESUME_KEYS and "checkpoint_every" not in tr.RESUME_KEYS
    # the ddp-only flags count as soon as either side has them
    ddp = vars(tr.load_config(base + ["--grad-compress", "powersgd"], "ddp"))
    ddp2 = vars(tr.load_config(base + ["--grad-compress", "powersgd", "--powersgd-rank", "4"], "ddp"))
    assert tr.hparam_mismatch(ddp, ddp2) == [("powersgd_rank", 2, 4)]
    assert {k for k, _, _ in tr.hparam_mismatch(saved, ddp)} == {"world_size", "sync_bn", "grad_compress",
                                                                 "powersgd_rank", "powersgd_start_iter"}


def test_resume_path_resolution(dtc, tmp_path):
    tr = dtc.trainer
    with pytest.raises(dtc.checkpoint.CheckpointError, match="no last.ckpt"):
        tr.resolve_resume(str(tmp_path))
    with pytest.raises(dtc.checkpoint.CheckpointError, match="no last.ckpt"):
        tr.resolve_resume(str(tmp_path / "missing" / "last.ckpt"))
    file = tmp_path / "last.ckpt"
    file.write_bytes(b"")
    assert tr.resolve_resume(str(tmp_path)) == (str(tmp_path), str(file))
    assert tr.resolve_resume(str(file)) == (str(tmp_path), str(file))
