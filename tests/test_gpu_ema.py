"""Weight EMA on the flat buffers (dtc_ema_update, ema.ModelEma) and evaluation from weights other than the bound
ones (dtc_rn18_eval_batch_weights).

Numeric reference: the formula of include/dtc.h, `ema += (src - ema) * w`, written with torch on the CPU (`_ref`)
and run in float64; the same code run in float32 gives the error a correct fp32 implementation makes. Both use the
w the interface specifies: 1 - decay (or the warm-up value) formed in double and rounded once to fp32. Bound, the
one of test_gpu_optim.py / test_gpu_lars.py, over all elements of a range:

    max|e_gpu - e64| <= 2 * max|e32 - e64|

(the factor 2 allows for FMA contraction: the kernel's update is one fused multiply-add, torch's CPU run rounds
the product and the sum separately). The three trajectories (GPU, float32, float64) start from the same fp32
values and run independently, so the bound is asserted on the accumulated error after every update.

Everything else is exact: the bf16 copy against dtc_cast_f32_bf16, the skip, the device-side count and weight,
one three-range launch against three one-range launches, guard bands, and every eval_batch_weights comparison.
"""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 64  # sentinel elements in front of and behind every buffer the kernel writes
E_SENTINEL, BF_SENTINEL = 1234.5, -7.0
TWO_TRIPS = 2048 * 256 * 4 + 4  # the grid is capped at 2048 blocks of 256 float4: one block takes a second trip


def _w32(decay, t=None):
    """The fp32 weight of update t (None: no warm-up), formed in Python doubles and rounded once."""
    d = decay if t is None else min(decay, (1 + t) / (10 + t))
    return np.float32(1 - d)


def _ref(e, p, w):
    """One update in place on e, in e's dtype; w is the fp32 weight (exact in either dtype)."""
    e.add_((p.to(e.dtype) - e) * float(w))


def _bound(name, e_gpu, e32, e64):
    err = float((e_gpu.detach().cpu().double() - e64).abs().max())
    ref = float((e32.double() - e64).abs().max())
    print(f"{name}: max|gpu - f64| = {err:.3e}, max|f32 - f64| = {ref:.3e}, ratio {err / ref if ref else float('inf'):.3f}")
    assert err <= 2 * ref, (name, err, ref)


def _guarded(n, dtype, fill, cuda):
    """(whole buffer, its [PAD, PAD + n) view) with `fill` everywhere."""
    whole = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=cuda)
    return whole, whole[PAD:PAD + n]


def _guards_intact(whole, fill):
    return bool((whole[:PAD] == fill).all()) and bool((whole[-PAD:] == fill).all())


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def _cast(dtc, e):
    out = torch.empty(e.numel(), dtype=torch.bfloat16, device=e.device)
    dtc.ops.cast_f32_bf16(e.contiguous(), out)
    return out


# ----------------------------------------------------------------------------- 1, 2: update and bf16 copy
@pytest.mark.parametrize("n", [4, 1028, TWO_TRIPS])
def test_update_matches_reference_and_bf16_copy(dtc, cuda, n):
    """Five updates at decay 0.9 with the source changed in between: the bound after every update, and the bf16
    copy bit-equal to dtc_cast_f32_bf16 of the fp32 EMA after every update.
    Measured on an MI355X, the worst ratio max|gpu - f64| / max|f32 - f64| over the five updates: n = 4: 1.000,
    n = 1028: 0.960, n = 2 097 156: 1.001 (bound: 2)."""
    g = torch.Generator().manual_seed(100 + n % 97)
    e0 = torch.randn(n, generator=g)
    e32, e64 = e0.clone(), e0.double()
    ew, e = _guarded(n, torch.float32, E_SENTINEL, cuda)
    bw, b = _guarded(n, torch.bfloat16, BF_SENTINEL, cuda)
    e.copy_(e0)
    state = dtc.ops.ema_state(cuda)
    w = _w32(0.9)
    for k in range(5):
        p = torch.randn(n, generator=g) * (1 + k)
        pd = p.to(cuda)
        dtc.ops.ema_update([(e, pd, b)], state, 0.9)
        _ref(e32, p, w)
        _ref(e64, p, w)
        _bound(f"n={n} update {k + 1}", e, e32, e64)
        assert torch.equal(_bits(b), _bits(_cast(dtc, e))), (n, k)
        assert torch.equal(pd.cpu(), p)  # the source is only read
    assert _guards_intact(ew, E_SENTINEL) and _guards_intact(bw, BF_SENTINEL)
    st = state.cpu()
    assert int(st[0]) == 5 and st[1:2].view(torch.float32).numpy()[0] == w and st[2:].tolist() == [0, 0]


# ----------------------------------------------------------------------------- 3: skip
def test_found_inf_skips_update_and_count(dtc, cuda):
    n = 1028
    g = torch.Generator().manual_seed(3)
    e = torch.randn(n, generator=g).to(cuda)
    b = torch.full((n,), BF_SENTINEL, dtype=torch.bfloat16, device=cuda)
    p = torch.randn(n, generator=g).to(cuda)
    state = dtc.ops.ema_state(cuda)
    found = torch.zeros(1, dtype=torch.int32, device=cuda)
    for _ in range(2):
        dtc.ops.ema_update([(e, p, b)], state, 0.9, found_inf=found)
    before = (_bits(e), _bits(b), state.cpu().clone())
    assert int(before[2][0]) == 2
    found.fill_(1)
    dtc.ops.ema_update([(e, p * 3, b)], state, 0.5, warmup=True, found_inf=found)
    assert torch.equal(_bits(e), before[0]) and torch.equal(_bits(b), before[1])
    assert torch.equal(state.cpu(), before[2])  # all four words
    found.fill_(0)
    dtc.ops.ema_update([(e, p, b)], state, 0.9, found_inf=found)
    assert int(state.cpu()[0]) == 3
    assert not torch.equal(_bits(e), before[0])


# ----------------------------------------------------------------------------- 4: warm-up
def test_warmup_count_and_weight(dtc, cuda):
    """decay 0.5 with warm-up, twelve updates: (1 + t) / (10 + t) is below 0.5 up to t = 7, so the branch of the
    min changes at t = 8. The device words after every update, and the EMA within the bound.
    Measured on an MI355X: the worst ratio over the twelve updates is 1.717 (at t = 9), the others 0.52 - 1.23."""
    n = 1028
    g = torch.Generator().manual_seed(4)
    e0 = torch.randn(n, generator=g)
    e32, e64 = e0.clone(), e0.double()
    e = e0.to(cuda)
    state = dtc.ops.ema_state(cuda)
    assert _w32(0.5, 7) > np.float32(0.5) and _w32(0.5, 8) == np.float32(0.5)
    for t in range(1, 13):
        p = torch.randn(n, generator=g)
        dtc.ops.ema_update([(e, p.to(cuda), None)], state, 0.5, warmup=True)
        w = _w32(0.5, t)
        st = state.cpu()
        assert int(st[0]) == t
        assert st[1:2].numpy().view(np.int32)[0] == np.asarray(w).view(np.int32), (t, w)
        _ref(e32, p, w)
        _ref(e64, p, w)
        _bound(f"warm-up t={t}", e, e32, e64)


# ----------------------------------------------------------------------------- 5: ranges
def test_three_ranges_in_one_launch(dtc, cuda):
    sizes = [TWO_TRIPS, 4, 1028]
    with_bf = [True, False, True]
    g = torch.Generator().manual_seed(5)
    e0 = [torch.randn(n, generator=g) for n in sizes]
    src0 = [torch.randn(n, generator=g) for n in sizes]

    def run(together):
        ews, es, bws, bs = [], [], [], []
        for n, e_init, bf in zip(sizes, e0, with_bf):
            ew, e = _guarded(n, torch.float32, E_SENTINEL, cuda)
            e.copy_(e_init)
            bw, b = _guarded(n, torch.bfloat16, BF_SENTINEL, cuda) if bf else (None, None)
            ews.append(ew), es.append(e), bws.append(bw), bs.append(b)
        src = [s.to(cuda) for s in src0]
        if together:
            dtc.ops.ema_update(list(zip(es, src, bs)), dtc.ops.ema_state(cuda), 0.9)
        else:
            for r in zip(es, src, bs):
                dtc.ops.ema_update([r], dtc.ops.ema_state(cuda), 0.9)
        torch.cuda.synchronize()
        for s, s0 in zip(src, src0):
            assert torch.equal(s.cpu(), s0)  # src bit-unchanged
        for ew, bw in zip(ews, bws):
            assert _guards_intact(ew, E_SENTINEL)
            assert bw is None or _guards_intact(bw, BF_SENTINEL)
        return [_bits(e) for e in es], [None if b is None else _bits(b) for b in bs]

    e_one, b_one = run(False)
    e_all, b_all = run(True)
    for k in range(3):
        assert torch.equal(e_all[k], e_one[k]), k
        assert not torch.equal(e_all[k], _bits(e0[k])), k  # the range was updated at all
        assert (b_all[k] is None) == (not with_bf[k])
        if with_bf[k]:
            assert torch.equal(b_all[k], b_one[k]), k


# ----------------------------------------------------------------------------- 6: eval_batch_weights
B, NCLS = 8, 10


def _ctx(dtc, prec):
    return dtc.autocast() if prec == "bf16" else dtc.autocast(enabled=False)


def _flat_state(model):
    f = model.flat
    return [t.detach().clone() for t in (f.params, f.params_bf16, f.bufs, f.nbt)]


def _restore(model, saved):
    f = model.flat
    for t, s in zip((f.params, f.params_bf16, f.bufs, f.nbt), saved):
        t.copy_(s)


def _same(a, b):
    """Two _flat_state lists agree bit for bit (num_batches_tracked is int64: compared as it is)."""
    def key(t):
        return _bits(t) if t.is_floating_point() else t.cpu()

    return all(torch.equal(key(x), key(y)) for x, y in zip(a, b))


def _eval(exe, x, y, n_valid, weights=None):
    lg = torch.full((B, NCLS), float("nan"), dtype=torch.float32, device=x.device)
    rec = torch.zeros(4, dtype=torch.int32, device=x.device)
    exe.eval_batch(x, y, n_valid, 3, rec, logits=lg, weights=weights)
    return _bits(lg[:n_valid]), rec.cpu()


def _train_step(dtc, model, prec, x, y):
    """Forward + backward of one batch in training mode (no optimizer step)."""
    model.train()
    with _ctx(dtc, prec):
        loss = dtc.CrossEntropyLoss()(model(x), y)
    loss.backward()
    model.eval()


@pytest.fixture(scope="module", params=["bf16", "fp32"])
def ema_net(request, dtc, cuda):
    """Per precision: a 10-class ResNet18 after three SGD steps at batch 8, a ModelEma (decay 0.5) updated after
    each of them -- so its parameters, bf16 copy and running statistics all differ from the model's -- and a second
    model that loaded ema.state_dict(). Built once; the tests restore whatever they change."""
    prec = request.param
    torch.manual_seed(61)
    model = dtc.ResNet18(num_classes=NCLS).to(cuda)
    g = torch.Generator().manual_seed(62)
    x = torch.randn(B, 3, 32, 32, generator=g).to(cuda)
    y = torch.randint(0, NCLS, (B,), generator=g).to(cuda)
    opt = dtc.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    ema = dtc.ModelEma(model, decay=0.5)
    for _ in range(3):
        _train_step(dtc, model, prec, x, y)
        opt.step()
        ema.update()
    assert ema.num_updates == 3
    assert not torch.equal(ema.params, model.flat.params) and not torch.equal(ema.bufs, model.flat.bufs)
    assert not torch.equal(_bits(ema.params_bf16), _bits(model.flat.params_bf16))
    torch.manual_seed(63)  # another initialisation: everything model2 evaluates with comes from the EMA
    model2 = dtc.ResNet18(num_classes=NCLS).to(cuda)
    model2.load_state_dict(ema.state_dict())
    model2.eval()
    return prec, model, ema, model2, x, y


@pytest.mark.parametrize("n_valid", [8, 5])
def test_eval_batch_weights_is_eval_batch_on_other_buffers(dtc, cuda, ema_net, n_valid):
    prec, model, ema, model2, x, y = ema_net
    exe = model.executor(B, 32, 32, prec)
    saved = _flat_state(model)
    # (a) the model's own buffers passed as weights: plain eval_batch, bit for bit
    plain = _eval(exe, x, y, n_valid)
    own = _eval(exe, x, y, n_valid, weights=model.flat)
    assert torch.equal(own[0], plain[0]) and torch.equal(own[1], plain[1])
    assert int(plain[1][1]) == n_valid and np.isfinite(plain[1][:1].numpy().view(np.float32)[0])
    # (b) the EMA's buffers: what a second model holding the EMA's state computes
    got = _eval(exe, x, y, n_valid, weights=ema)
    want = _eval(model2.executor(B, 32, 32, prec), x, y, n_valid)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], plain[0])  # and they are other weights
    # (c) the bound buffers are untouched and still the ones evaluated
    assert _same(_flat_state(model), saved)
    again = _eval(exe, x, y, n_valid)
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])
    short = types.SimpleNamespace(params=ema.params[:-64], params_bf16=ema.params_bf16, bufs=ema.bufs)
    with pytest.raises(dtc.NativeError):  # not the model's layout
        _eval(exe, x, y, n_valid, weights=short)


def test_training_step_after_ema_evaluation_is_bit_identical(dtc, cuda, ema_net):
    """One training step from a saved state, with and without an EMA evaluation ahead of it: the step is
    bit-reproducible, so every gradient, the running statistics and num_batches_tracked agree exactly."""
    prec, model, ema, _, x, y = ema_net
    saved = _flat_state(model)
    try:
        _train_step(dtc, model, prec, x, y)
        want = (_bits(model.flat.grads), _flat_state(model))
        _restore(model, saved)
        model.flat.grads.zero_()
        with _ctx(dtc, prec):
            res = ema.evaluate([(x, y), (x[:5].contiguous(), y[:5].contiguous())], topk=3)
        assert res.n.tolist() == [8, 5] and np.isfinite(res.loss).all()
        assert _same(_flat_state(model), saved)
        _train_step(dtc, model, prec, x, y)
        assert torch.equal(_bits(model.flat.grads), want[0])
        assert _same(_flat_state(model), want[1])
    finally:
        _restore(model, saved)
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 7: ModelEma in a training loop
def test_model_ema_follows_training_with_grad_scaler(dtc, cuda):
    """Four AMP steps at batch 8 with SGD and GradScaler, the EMA updated between step() and update(). Step 3 has an
    inf written into the gradients: the parameters, the EMA and its count stay as they were. The EMA of parameters
    and running statistics against the host recurrence over the snapshots taken after each applied step.
    Measured on an MI355X: ratio 1.000 for the parameters, 1.001 for the running statistics."""
    torch.manual_seed(71)
    model = dtc.ResNet18(num_classes=NCLS).to(cuda)
    g = torch.Generator().manual_seed(72)
    opt = dtc.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    scaler = dtc.GradScaler()
    crit = dtc.CrossEntropyLoss()
    ema = dtc.ModelEma(model, decay=0.9)
    flat = model.flat
    w = _w32(0.9)
    ref = {"params": [flat.params.cpu().clone(), flat.params.cpu().double()],
           "bufs": [flat.bufs.cpu().clone(), flat.bufs.cpu().double()]}
    assert ema.num_updates == 0 and scaler.found_inf is None
    applied = 0
    model.train()
    for k in range(4):
        x = torch.randn(B, 3, 32, 32, generator=g).to(cuda)
        y = torch.randint(0, NCLS, (B,), generator=g).to(cuda)
        with dtc.autocast():
            loss = crit(model(x), y)
        scaler.scale(loss).backward()
        before = (_bits(flat.params), _bits(ema.params), _bits(ema.params_bf16), _bits(ema.bufs), ema.state.cpu())
        if k == 2:
            flat.grads[flat.layout.params[0].offset + 5] = float("inf")
        scaler.step(opt)
        ema.update(found_inf=scaler.found_inf)
        skipped = bool(scaler.found_inf.item())
        scaler.update()
        assert skipped == (k == 2)
        if skipped:
            after = (_bits(flat.params), _bits(ema.params), _bits(ema.params_bf16), _bits(ema.bufs), ema.state.cpu())
            assert all(torch.equal(a, b) for a, b in zip(before, after))
        else:
            applied += 1
            for key in ("params", "bufs"):
                snap = getattr(flat, key).cpu()
                _ref(ref[key][0], snap, w)
                _ref(ref[key][1], snap, w)
        assert ema.num_updates == applied
    model.eval()
    assert applied == 3
    _bound("ModelEma params", ema.params, *ref["params"])
    _bound("ModelEma bufs", ema.bufs, *ref["bufs"])
    assert torch.equal(_bits(ema.params_bf16), _bits(_cast(dtc, ema.params)))
    # state_dict: the model's keys, order and shapes; loadable into the EMA and into a model
    sd, msd = ema.state_dict(), model.state_dict()
    assert list(sd) == list(msd)
    assert all(sd[k].shape == msd[k].shape and sd[k].dtype == msd[k].dtype for k in msd)
    assert torch.equal(sd["bn1.num_batches_tracked"].cpu(), msd["bn1.num_batches_tracked"].cpu())
    assert sd["layer1.0.conv1.weight"].stride() == msd["layer1.0.conv1.weight"].stride()  # the strided KCRS view
    other = dtc.ModelEma(model)
    other.load_state_dict({k: v.cpu() for k, v in sd.items()})
    assert torch.equal(_bits(other.params), _bits(ema.params)) and torch.equal(_bits(other.bufs), _bits(ema.bufs))
    assert torch.equal(_bits(other.params_bf16), _bits(ema.params_bf16))
    # copy_to + model.evaluate == ema.evaluate, bit for bit, in both precisions
    batches = [(x, y), (x[:3].contiguous(), y[:3].contiguous())]
    raw = model.evaluate(batches, topk=3)
    ema.copy_to(model)
    for prec in ("bf16", "fp32"):
        with _ctx(dtc, prec):
            want = ema.evaluate(batches, topk=3)
            got = model.evaluate(batches, topk=3)
        assert np.array_equal(got.loss.view(np.int32), want.loss.view(np.int32)) and np.isfinite(want.loss).all()
        assert got.n.tolist() == want.n.tolist() == [8, 3]
        assert got.top1.tolist() == want.top1.tolist() and got.topk.tolist() == want.topk.tolist()
    assert not np.array_equal(raw.loss.view(np.int32), want.loss.view(np.int32))  # (raw: fp32, as `want` now)


# ----------------------------------------------------------------------------- trainer
def test_trainer_model_ema_runs(dtc, cuda, tmp_path):
    """--model-ema through the single-process trainer: one update per step, validate() reports the EMA and logs
    the raw weights beside it, the checkpoint holds the EMA under the model's keys."""
    dtc.data.fix_seed(42)
    t = dtc.trainer.main(["--max-steps", "3", "--epoch", "1", "--synthetic-train", "64", "--synthetic-test", "16",
                          "--batch-size", "8", "--device-data", "--amp", "--model-ema", "--model-ema-decay", "0.5",
                          "--model-ema-steps", "2", "--ckpt-path", str(tmp_path)], "single")
    assert t.global_step == 3 and isinstance(t.ema, dtc.ModelEma) and t.ema.decay == 0.5
    assert t.ema.num_updates == 1  # global steps 1..3, every second one
    rows = [json.loads(line) for line in open(os.path.join(t.save_path, "scalars.jsonl"))]
    acc = [r for r in rows if r["tag"] == "acc/epoch"]
    assert len(acc) == 1 and set(acc[0]) == {"tag", "step", "val", "val_raw"}
    m = t.ema.evaluate(t.val_loader, topk=1).reference_meters()
    loss = [r for r in rows if r["tag"] == "loss/epoch"][0]
    assert loss["val"] == m["loss"] and acc[0]["val"] == m["top1"]
    t.save_checkpoint(0, 1.0, t.model)
    path = [f for f in os.listdir(t.save_path) if f.endswith(".pt")]
    assert len(path) == 1
    state = torch.load(os.path.join(t.save_path, path[0]), weights_only=True)
    sd = t.ema.state_dict()
    assert list(state) == list(t.model.state_dict())
    assert all(torch.equal(state[k].cpu(), sd[k].cpu()) for k in sd)
    assert not torch.equal(state["linear.weight"].cpu(), t.model.state_dict()["linear.weight"].cpu())
