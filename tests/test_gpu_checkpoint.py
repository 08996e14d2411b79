"""Training checkpoints on the GPU: a run interrupted at an epoch boundary and resumed ends in the same bits as the
uninterrupted run. Every comparison is bit equality (torch.equal on integer views); each round trip has a control
that loads less and must differ, so no test passes vacuously. The host side is in test_checkpoint_cli.py."""
import glob
import json
import os
import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ["sgd", "adam", "adamw", "lars"]
STATE_ATTRS = {"sgd": ("_mom",), "lars": ("_mom",), "adam": ("_exp_avg", "_exp_avg_sq"),
               "adamw": ("_exp_avg", "_exp_avg_sq")}


def _bits(t):
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _model(dtc, cuda, seed=42):
    torch.manual_seed(seed)
    return dtc.ResNet18().to(cuda)


def _batches(cuda, n, batch=8, seed=23):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(batch, 3, 32, 32, generator=g).to(cuda) for _ in range(n)]
    ys = [torch.randint(0, 100, (batch,), generator=g).to(cuda) for _ in range(n)]
    return xs, ys


def _optimizer(dtc, kind, params, lr=0.05):
    if kind == "sgd":
        return dtc.SGD(params, lr=lr, momentum=0.9, weight_decay=1e-4, nesterov=True)
    if kind == "lars":
        return dtc.LARS(params, lr=lr, momentum=0.9, weight_decay=1e-4, nesterov=True, trust_coef=0.02)
    return {"adam": dtc.Adam, "adamw": dtc.AdamW}[kind](params, lr=lr * 0.02, weight_decay=1e-2)


def _real_mask(flat):
    """True where the flat buffer holds a parameter element, False on the alignment padding."""
    mask = torch.zeros(flat.params.numel(), dtype=torch.bool, device=flat.device)
    for q in flat.layout.params:
        torch.as_strided(mask, q.shape, q.stride, q.offset).fill_(True)
    return mask


# ----------------------------------------------------------------------------- 1. optimizer round trip
@pytest.mark.parametrize("kind", KINDS)
def test_optimizer_round_trip(dtc, cuda, kind):
    ck = dtc.checkpoint
    xs, ys = _batches(cuda, 4)
    crit = dtc.CrossEntropyLoss()

    def step(m, opt, sc, k, skip=False):
        with dtc.autocast():
            loss = crit(m(xs[k]), ys[k])
        sc.scale(loss).backward()
        if skip:  # what the finiteness check leaves behind on an overflow
            sc.unscale_(opt)
            sc._found_inf.fill_(1)
        sc.step(opt)
        sc.update()

    a = _model(dtc, cuda, 1)
    opt_a, sc_a = _optimizer(dtc, kind, a.parameters()), dtc.GradScaler(init_scale=256.0, growth_interval=2)
    assert opt_a.state_dict()["state"] == {}  # not attached yet: torch's empty shell
    for k in range(3):
        step(a, opt_a, sc_a, k, skip=(k == 1))
    sd = opt_a.state_dict()
    assert sorted(sd["state"]) == list(range(62)) and sd["param_groups"][0]["params"] == list(range(62))
    if kind in ("adam", "adamw"):
        st = sd["state"][61]["step"]
        assert st.dtype == torch.float32 and st.dim() == 0 and st.device.type == "cpu" and float(st) == 2.0
        assert int(opt_a._step_state[0]) == 2
    names = [n for n, _ in a.named_parameters()]
    for i, p in enumerate(a.parameters()):
        for t in sd["state"][i].values():
            assert t.dim() == 0 or t.shape == p.shape, names[i]
    saved = ck.to_plain({"model": dict(a.state_dict()), "optimizer": sd, "scaler": sc_a.state_dict()})
    assert saved["scaler"]["scale"] == 128.0 and saved["scaler"]["_growth_tracker"] == 1  # one back-off, one clean step
    assert all(t.is_contiguous() and t.device.type == "cpu" for e in saved["optimizer"]["state"].values()
               for t in e.values())

    b = _model(dtc, cuda, 2)
    opt_b, sc_b = _optimizer(dtc, kind, b.parameters(), lr=0.5), dtc.GradScaler()
    if kind in ("adam", "lars"):
        sc_b._lazy_init(cuda)  # the load then fills existing device words; otherwise it is kept for _lazy_init
    b.load_state_dict(saved["model"])
    opt_b.load_state_dict(saved["optimizer"])
    sc_b.load_state_dict(saved["scaler"])
    assert opt_b.param_groups[0]["lr"] == opt_a.param_groups[0]["lr"]
    c = _model(dtc, cuda, 3)  # the control: the weights alone
    opt_c, sc_c = _optimizer(dtc, kind, c.parameters()), dtc.GradScaler()
    c.load_state_dict(saved["model"])
    sc_c.load_state_dict(saved["scaler"])
    for attr in ("params", "params_bf16", "bufs", "nbt"):
        assert _same_bits(getattr(b.flat, attr), getattr(a.flat, attr)), attr
        assert _same_bits(getattr(c.flat, attr), getattr(a.flat, attr)), attr

    for m, opt, sc in ((a, opt_a, sc_a), (b, opt_b, sc_b), (c, opt_c, sc_c)):
        step(m, opt, sc, 3)
    torch.cuda.synchronize()
    for attr in ("params", "params_bf16", "bufs", "nbt"):
        assert _same_bits(getattr(b.flat, attr), getattr(a.flat, attr)), attr
    assert not _same_bits(c.flat.params, a.flat.params) and not _same_bits(c.flat.params_bf16, a.flat.params_bf16)
    pad = ~_real_mask(a.flat)
    for attr in STATE_ATTRS[kind]:
        assert _same_bits(getattr(opt_b, attr), getattr(opt_a, attr)), attr
        assert not _same_bits(getattr(opt_c, attr), getattr(opt_a, attr)), attr
        assert not getattr(opt_b, attr)[pad].any(), attr  # the alignment padding is still zero
    if kind in ("adam", "adamw"):
        assert int(opt_b._step_state[0]) == int(opt_a._step_state[0]) == 3 and int(opt_c._step_state[0]) == 1
    # growth_interval 2: the fourth step grows the scale again
    assert _same_bits(sc_b._scale, sc_a._scale) and _same_bits(sc_b._inv_scale, sc_a._inv_scale)
    assert _same_bits(sc_b._tracker, sc_a._tracker) and float(sc_a._scale) == 256.0 and int(sc_a._tracker) == 0


def test_optimizer_load_refusals(dtc, cuda):
    m = _model(dtc, cuda)
    opt = _optimizer(dtc, "adam", m.parameters())
    opt.attach(m)
    sd = dtc.checkpoint.to_plain(opt.state_dict())
    before = opt._exp_avg.clone()

    def broken(fn):
        out = {"state": {i: dict(e) for i, e in sd["state"].items()}, "param_groups": [dict(sd["param_groups"][0])]}
        fn(out)
        return out

    with pytest.raises(ValueError, match="61 parameters"):
        opt.load_state_dict(broken(lambda d: d["param_groups"][0].update(params=list(range(61)))))
    with pytest.raises(ValueError, match=r"conv1\.weight"):
        opt.load_state_dict(broken(lambda d: d["state"][0].update(exp_avg=torch.zeros(64, 3, 3))))
    with pytest.raises(KeyError, match=r"linear\.bias.*exp_avg_sq"):
        opt.load_state_dict(broken(lambda d: d["state"][61].pop("exp_avg_sq")))
    with pytest.raises(KeyError, match="parameter 5"):
        opt.load_state_dict(broken(lambda d: d["state"].pop(5)))
    with pytest.raises(ValueError, match="step"):
        opt.load_state_dict(broken(lambda d: d["state"][3].update(step=2.0)))
    with pytest.raises(NotImplementedError):
        opt.load_state_dict(broken(lambda d: d["param_groups"][0].update(amsgrad=True)))
    assert _same_bits(opt._exp_avg, before) and opt.param_groups[0]["amsgrad"] is False  # nothing half-loaded
    opt.load_state_dict(broken(lambda d: [e.update(step=7) for e in d["state"].values()]))  # a number will do
    assert int(opt._step_state[0]) == 7


# ----------------------------------------------------------------------------- 2. torch interop
@pytest.mark.filterwarnings("ignore:Detected call of")
@pytest.mark.parametrize("kind", ["sgd", "adam", "adamw"])
def test_torch_interop(dtc, cuda, kind):
    m = _model(dtc, cuda)
    flat = m.flat

    def torch_side():
        params = [torch.nn.Parameter(p.detach().cpu().contiguous().clone()) for p in m.parameters()]
        if kind == "sgd":
            return params, torch.optim.SGD(params, lr=0.03, momentum=0.8, weight_decay=2e-4, nesterov=True)
        cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[kind]
        return params, cls(params, lr=0.03, betas=(0.8, 0.95), weight_decay=2e-3)

    def torch_step(params, opt, g):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()

    params, ref = torch_side()
    g = torch.Generator().manual_seed(7)
    for _ in range(2):
        torch_step(params, ref, g)
    opt = _optimizer(dtc, kind, m.parameters(), lr=0.1)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)  # built BEFORE the load
    group = opt.param_groups[0]
    opt.load_state_dict(ref.state_dict())
    assert opt.param_groups[0] is group and group["lr"] == 0.03
    assert group["weight_decay"] == ref.defaults["weight_decay"]
    if kind == "sgd":
        assert group["momentum"] == 0.8
    else:
        assert tuple(group["betas"]) == (0.8, 0.95) and int(opt._step_state[0]) == 2

    def check_against(ref_opt, ref_params):
        for q, p in zip(flat.layout.params, ref_params):
            for key, attr in opt._STATE_BUFFERS:
                want, buf = ref_opt.state[p][key], getattr(opt, attr)
                assert _same_bits(torch.as_strided(buf, q.shape, q.stride, q.offset), want), (q.name, key)
                if want.dim() == 4:  # KRSC storage, spelled out without the layout's strides
                    assert _same_bits(buf[q.offset:q.offset + q.numel], want.permute(0, 2, 3, 1).reshape(-1)), q.name

    check_against(ref, params)
    # back into a fresh torch optimizer: the same state bit for bit, and a group torch can step with (the loaded
    # tensors keep the views' strides, which torch's CPU kernels may round differently: the step is only close)
    params2, ref2 = torch_side()
    ref2.load_state_dict(opt.state_dict())
    for p, p2 in zip(params, params2):
        assert sorted(ref.state[p]) == sorted(ref2.state[p2])
        for key, want in ref.state[p].items():
            assert _same_bits(ref2.state[p2][key], want), key
    with torch.no_grad():
        for p, p2 in zip(params, params2):
            p2.copy_(p)
    g1, g2 = torch.Generator().manual_seed(8), torch.Generator().manual_seed(8)
    torch_step(params, ref, g1)
    torch_step(params2, ref2, g2)
    assert all(torch.allclose(p, p2, rtol=1e-5, atol=1e-7) for p, p2 in zip(params, params2))
    # the package's own round trip: clear, load its own dict back
    sd = dtc.checkpoint.to_plain(opt.state_dict())
    for _, attr in opt._STATE_BUFFERS:
        getattr(opt, attr).zero_()
    opt.load_state_dict(sd)
    got = opt.state_dict()
    assert got["param_groups"] == sd["param_groups"]
    for i, entry in sd["state"].items():
        assert all(_same_bits(got["state"][i][key], t) for key, t in entry.items()), i
    # the scheduler built before the load still drives the lr the kernel reads
    sched.step()
    assert opt.param_groups[0] is group and group["lr"] == pytest.approx(0.015)


# ----------------------------------------------------------------------------- 3. SAM
def test_sam_state_dict(dtc, cuda):
    m = _model(dtc, cuda)
    (x,), (y,) = _batches(cuda, 1)
    crit = dtc.CrossEntropyLoss()
    sam = dtc.SAM(_optimizer(dtc, "sgd", m.parameters()), rho=0.05)
    with dtc.autocast():
        loss = crit(m(x), y)
    with m.local_grads():
        loss.backward()
    sam.first_step()
    with pytest.raises(dtc.NativeError, match="perturbed"):
        sam.state_dict()
    with pytest.raises(dtc.NativeError, match="perturbed"):
        sam.load_state_dict({})
    with dtc.autocast():
        crit(m(x), y).backward()
    sam.step()
    sd, base = sam.state_dict(), sam.base.state_dict()
    assert sd["param_groups"] == base["param_groups"] and sorted(sd["state"]) == list(range(62))
    assert all(_same_bits(sd["state"][i]["momentum_buffer"], base["state"][i]["momentum_buffer"]) for i in range(62))
    assert sam.base._mom.abs().max() > 0
    saved = dtc.checkpoint.to_plain(sd)
    saved["param_groups"][0]["lr"] = 0.0125
    sam.base._mom.zero_()
    sam.load_state_dict(saved)
    assert sam.param_groups is sam.base.param_groups and sam.base.param_groups[0]["lr"] == 0.0125
    assert all(_same_bits(sam.state_dict()["state"][i]["momentum_buffer"], saved["state"][i]["momentum_buffer"])
               for i in range(62))


# ----------------------------------------------------------------------------- 4. EMA with warm-up
def test_ema_train_state(dtc, cuda):
    m = _model(dtc, cuda)

    def move(k):  # new weights and statistics for the next update; the padding (zeros) stays zero
        m.flat.params.mul_(1.0 + 0.01 * (k + 1))
        m.flat.bufs.mul_(1.0 - 0.02 * (k + 1))
        m.sync_weights()

    a = dtc.ModelEma(m, decay=0.999, warmup=True)
    for k in range(3):
        move(k)
        a.update()
    ts = dtc.checkpoint.to_plain(a.train_state())
    assert ts["num_updates"] == 3 and set(ts) == {"weights", "num_updates"}
    b = dtc.ModelEma(m, decay=0.999, warmup=True)
    assert not _same_bits(b.params, a.params)
    b.load_train_state(ts)
    c = dtc.ModelEma(m, decay=0.999, warmup=True)  # the control: the weights without the count
    c.load_state_dict(ts["weights"])
    for e in (b, c):
        assert _same_bits(e.params, a.params) and _same_bits(e.bufs, a.bufs)
        assert _same_bits(e.params_bf16, a.params_bf16)  # re-rounding the fp32 EMA reproduces the bf16 copy
    assert (a.num_updates, b.num_updates, c.num_updates) == (3, 3, 0)
    move(3)
    for e in (a, b, c):
        e.update()
    torch.cuda.synchronize()
    for attr in ("params", "params_bf16", "bufs"):
        assert _same_bits(getattr(b, attr), getattr(a, attr)), attr
    assert (a.num_updates, b.num_updates, c.num_updates) == (4, 4, 1)
    assert not _same_bits(c.params, a.params) and not _same_bits(c.bufs, a.bufs)


# ----------------------------------------------------------------------------- 5. PowerSGD, two ranks on one GPU
def _run_ranks(fn, world):
    """fn(rank) in `world` threads, each on its own stream; re-raise the first failure (test_gpu_ddp_group)."""
    out, errs = [None] * world, [None] * world
    streams = [torch.cuda.Stream() for _ in range(world)]

    def body(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(streams[r]):
                out[r] = fn(r)
                torch.cuda.current_stream().synchronize()
        except BaseException as e:  # noqa: BLE001 - re-raised in the caller
            errs[r] = e

    ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    for e in errs:
        if e is not None:
            raise e
    assert not any(t.is_alive() for t in ts), "a rank thread hung"
    return out


def test_powersgd_hook_state_two_ranks(dtc, cuda):
    """No optimizer step is taken, so every backward sees the same local gradients; what changes from one to the
    next is the hook's state: the warm-start Q and each rank's error-feedback buffer."""
    world, par = 2, dtc.parallel
    xs, ys = _batches(cuda, world)
    comms = par.Comm.thread_group(cuda.index or 0, world)
    models = [[_model(dtc, cuda) for _ in range(world)] for _ in range(3)]
    torch.cuda.synchronize()
    crit = dtc.CrossEntropyLoss()

    def rank(r):
        def wrapped(m):
            ddp = dtc.DistributedDataParallel(m, device_ids=[0], comm=comms[r])
            ddp.register_comm_hook(par.PowerSGDState(matrix_approximation_rank=2, start_powerSGD_iter=2,
                                                     random_seed=5), par.powerSGD_hook)
            return ddp

        def backward(ddp):
            with dtc.autocast():
                crit(ddp(xs[r]), ys[r]).backward()
            torch.cuda.current_stream().synchronize()
            return ddp.module.flat.grads.cpu(), ddp.module.flat.grad_err.cpu()

        run = wrapped(models[0][r])  # the uninterrupted run
        assert run.comm_hook_state_dict() == {"iter": 0}
        for _ in range(4):
            fourth = backward(run)
        live = run.comm_hook_state_dict()
        assert live["iter"] == 4 and live["matrix_approximation_rank"] == 2 and live["random_seed"] == 5
        assert live["q"] is run.module._powersgd.q and live["grad_err"] is run.module.flat.grad_err
        saved = dtc.checkpoint.to_plain(live)
        fifth = backward(run)
        resumed = wrapped(models[1][r])  # fresh model and wrapper, the captured state
        resumed.load_comm_hook_state_dict(saved)
        assert resumed.module._powersgd.state.iter == 4 and resumed.module._powersgd.plan is not None
        got = backward(resumed)
        control = wrapped(models[2][r])  # the count alone: a compressed step from a fresh Q and no error
        control.load_comm_hook_state_dict({"iter": 4})
        ctl = backward(control)
        return saved, fourth, fifth, got, ctl, resumed.module._powersgd.state.iter

    try:
        res = _run_ranks(rank, world)
    finally:
        for cm in comms:
            cm.close()
    for r in range(world):
        saved, fourth, fifth, got, ctl, it = res[r]
        assert it == 5
        assert _same_bits(got[0], fifth[0]) and _same_bits(got[1], fifth[1]), r
        assert not _same_bits(fifth[0], fourth[0]) and not _same_bits(fifth[1], fourth[1])  # the state matters
        assert not _same_bits(ctl[0], fifth[0]) and not _same_bits(ctl[1], fifth[1]), r
    assert _same_bits(res[0][3][0], res[1][3][0])  # both ranks hold the same gradients ...
    assert not _same_bits(res[0][0]["grad_err"], res[1][0]["grad_err"])  # ... and their own error buffers
    assert _same_bits(res[0][0]["q"], res[1][0]["q"])
    other = dtc.nn.PowerSGD(par.PowerSGDState(matrix_approximation_rank=1, start_powerSGD_iter=2, random_seed=5),
                            models[2][0].flat)
    with pytest.raises(ValueError, match="matrix_approximation_rank = 2"):
        other.load_state_dict(res[0][0])
    assert other.plan is None and other.state.iter == 0
    with pytest.raises(dtc.NativeError, match="flat buffers"):
        dtc.nn.PowerSGD(par.PowerSGDState(matrix_approximation_rank=2, start_powerSGD_iter=2,
                                          random_seed=5)).load_state_dict(res[0][0])


# ----------------------------------------------------------------------------- 6. / 7. the trainer
BASE = ["--synthetic-train", "64", "--synthetic-test", "16", "--batch-size", "8", "--workers", "0", "--max-steps", "3"]


def _trainer(dtc, argv, mode="single", **kw):
    dtc.data.fix_seed(42)
    h = dtc.trainer.load_config(BASE + argv, mode)
    return dtc.trainer.Trainer(h, dtc.ResNet18(), dtc.GradScaler() if h.amp else None, **kw)


def _rows(trainer):
    """The per-epoch scalar rows of epochs 1 and 2."""
    rows = [json.loads(line) for line in open(os.path.join(trainer.save_path, "scalars.jsonl"))]
    rows = [r for r in rows if r["tag"] in ("lr", "loss/epoch", "acc/epoch") and r["step"] in (1, 2)]
    assert len(rows) == 6
    return rows


def _module(trainer):
    return getattr(trainer.model, "module", trainer.model)


def _compare_runs(s, r, opt_attrs):
    ms, mr = _module(s), _module(r)
    for attr in ("params", "params_bf16", "bufs", "nbt"):
        assert _same_bits(getattr(mr.flat, attr), getattr(ms.flat, attr)), attr
    bs, br = getattr(s.optimizer, "base", s.optimizer), getattr(r.optimizer, "base", r.optimizer)
    for attr in opt_attrs:
        assert getattr(bs, attr).abs().max() > 0 and _same_bits(getattr(br, attr), getattr(bs, attr)), attr
    if "_exp_avg" in opt_attrs:
        assert int(br._step_state[0]) == int(bs._step_state[0]) > 0
    if s.scaler is not None:
        assert _same_bits(r.scaler._scale, s.scaler._scale) and _same_bits(r.scaler._tracker, s.scaler._tracker)
        assert _same_bits(r.scaler._inv_scale, s.scaler._inv_scale)
    if s.ema is not None:
        for attr in ("params", "params_bf16", "bufs"):
            assert _same_bits(getattr(r.ema, attr), getattr(s.ema, attr)), attr
        assert r.ema.num_updates == s.ema.num_updates > 0
    assert (r.global_step, r.optimizer_step) == (s.global_step, s.optimizer_step) and s.global_step == 9
    assert r.global_top1_acc == s.global_top1_acc
    assert r.optimizer.param_groups[0]["lr"] == s.optimizer.param_groups[0]["lr"]
    assert r.lr_scheduler.last_epoch == s.lr_scheduler.last_epoch == 3
    assert _rows(r) == _rows(s)
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(r.save_path, "*.pt"))) == \
        sorted(os.path.basename(f) for f in glob.glob(os.path.join(s.save_path, "*.pt")))


CASES = {
    "sgd_host_loader": ([], ("_mom",)),
    "adamw_ema_mixup": (["--amp", "--device-data", "--optimizer", "adamw", "--model-ema", "--model-ema-warmup",
                         "--label-smoothing", "0.1", "--mixup-alpha", "1", "--lr-decay-step-size", "1"],
                        ("_exp_avg", "_exp_avg_sq")),
    "lars_warmup_accum_clip": (["--amp", "--optimizer", "lars", "--warmup-epochs", "2", "--accum-steps", "2",
                                "--clip-grad-norm", "1"], ("_mom",)),
    "sam": (["--amp", "--sam-rho", "0.05"], ("_mom",)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_trainer_resume_single(dtc, cuda, tmp_path, case):
    flags, opt_attrs = CASES[case]
    s = _trainer(dtc, flags + ["--epoch", "3", "--ckpt-path", str(tmp_path / "s")])
    s.fit()
    assert glob.glob(os.path.join(s.save_path, "*.ckpt*")) == []  # no flag, no checkpoint file
    r1 = _trainer(dtc, flags + ["--epoch", "1", "--checkpoint-every", "1", "--ckpt-path", str(tmp_path / "r")])
    r1.fit()
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(r1.save_path, "*.ckpt*"))) == ["last.ckpt"]
    hparams_json = open(os.path.join(r1.save_path, "hparams.json")).read()
    r = _trainer(dtc, flags + ["--epoch", "3", "--resume", r1.save_path, "--ckpt-path", str(tmp_path / "elsewhere")])
    assert r.save_path == os.path.abspath(r1.save_path) and r.version == r1.version == 0 and r.start_epoch == 1
    assert (r.global_step, r.optimizer_step) == (r1.global_step, r1.optimizer_step)
    r.fit()
    assert not os.path.exists(tmp_path / "elsewhere") and os.listdir(tmp_path / "r") == ["version-0"]
    assert open(os.path.join(r.save_path, "hparams.json")).read() == hparams_json
    _compare_runs(s, r, opt_attrs)
    assert not _same_bits(_module(r1).flat.params, _module(s).flat.params)  # epochs 1 and 2 did train


def test_trainer_resume_ddp_powersgd(dtc, cuda, tmp_path):
    import torch.distributed as dist

    par = dtc.parallel
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rendezvous", rank=0, world_size=1)
    made = []
    try:
        flags = ["--world-size", "1", "--grad-compress", "powersgd", "--powersgd-rank", "2",
                 "--powersgd-start-iter", "2"]
        kw = dict(mode="ddp", rank=cuda.index or 0, ngpus_per_node=1, distributed=True)

        def run(argv):
            t = _trainer(dtc, flags + argv, **kw)
            made.append(t)
            t.fit()
            return t

        s = run(["--epoch", "3", "--ckpt-path", str(tmp_path / "s")])
        assert glob.glob(os.path.join(s.save_path, "*.ckpt*")) == []
        r1 = run(["--epoch", "1", "--checkpoint-every", "1", "--ckpt-path", str(tmp_path / "r")])
        assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(r1.save_path, "*.ckpt*"))) == \
            ["last.ckpt", "last.rank0.ckpt"]
        r = run(["--epoch", "3", "--resume", os.path.join(r1.save_path, "last.ckpt"), "--ckpt-path",
                 str(tmp_path / "r")])
        assert r.save_path == os.path.abspath(r1.save_path)
        _compare_runs(s, r, ("_mom",))
        ps, pr = _module(s)._powersgd, _module(r)._powersgd
        assert pr.state.iter == ps.state.iter == 9
        assert _same_bits(_module(r).flat.grad_err, _module(s).flat.grad_err)
        assert _module(s).flat.grad_err.abs().max() > 0
        assert _same_bits(pr.q, ps.q) and _same_bits(pr.dev_state, ps.dev_state)
        os.remove(os.path.join(r1.save_path, "last.rank0.ckpt"))
        with pytest.raises(dtc.checkpoint.CheckpointError, match="last.rank0.ckpt is missing"):
            made.append(_trainer(dtc, flags + ["--epoch", "3", "--resume", r1.save_path], **kw))
    finally:
        for t in made:
            if getattr(t.model, "comm", None) is not None:
                if par._WORLD_COMM[0] is t.model.comm:
                    par._WORLD_COMM[0] = None
                t.model.comm.close()
        dist.destroy_process_group()


# ----------------------------------------------------------------------------- 8. refusals
def test_resume_refusals(dtc, cuda, tmp_path):
    r1 = _trainer(dtc, ["--epoch", "1", "--checkpoint-every", "1", "--ckpt-path", str(tmp_path / "r")])
    r1.fit()
    scalars = open(os.path.join(r1.save_path, "scalars.jsonl")).read()
    with pytest.raises(dtc.checkpoint.CheckpointError, match="optimizer: saved 'sgd', now 'adam'"):
        _trainer(dtc, ["--epoch", "3", "--optimizer", "adam", "--resume", r1.save_path])
    with pytest.raises(dtc.checkpoint.CheckpointError, match="amp: saved False, now True.*accum_steps: saved 1, now 2"):
        _trainer(dtc, ["--epoch", "3", "--amp", "--accum-steps", "2", "--resume", r1.save_path])
    assert open(os.path.join(r1.save_path, "scalars.jsonl")).read() == scalars  # no step was taken, nothing logged
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(dtc.checkpoint.CheckpointError, match="no last.ckpt"):
        _trainer(dtc, ["--epoch", "3", "--resume", str(empty)])
    # --epoch below the saved epoch: nothing left to train, nothing breaks
    done = _trainer(dtc, ["--epoch", "1", "--resume", r1.save_path])
    done.fit()
    assert done.global_step == r1.global_step == 3 and _same_bits(done.model.flat.params, r1.model.flat.params)
