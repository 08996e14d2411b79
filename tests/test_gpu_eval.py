"""On-device evaluation on the GPU: the metrics kernel against a numpy statement of the rank rule and against
trainer.accuracy, the executor's eval-batch call against the eval-mode forward (bit for bit, full and short
batches), the backward guard, and the trainer's --fused-eval against its default path."""
import numpy as np
import pytest

from tests.test_eval_metrics import rank_rule

pytestmark = pytest.mark.gpu

# (n, c) for i = 0..7 and the top-1 / top-5 hit counts of the seeded inputs below, computed on the CPU: the rank
# rule and trainer.accuracy agree on every row of these inputs
SHAPES = [(1, 100), (5, 100), (65, 100), (257, 100), (4096, 100), (7, 10), (33, 129), (16, 1000)]
COUNTS = [(0, 1), (1, 2), (15, 23), (56, 84), (932, 1346), (4, 5), (8, 10), (2, 5)]


def _bits(t):
    """Raw 32-bit words of an fp32 tensor (NaNs compare by payload)."""
    return t.detach().reshape(-1).cpu().contiguous().numpy().view(np.int32)


def _record(rec):
    """(loss bits, n, top1, topk) of one int32 [4] device record."""
    r = rec.cpu().numpy()
    return int(r[0]), int(r[1]), int(r[2]), int(r[3])


def _loss_of(rec):
    return float(rec.cpu().numpy()[:1].view(np.float32)[0])


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_metrics_kernel_matches_rank_rule(dtc, cuda, i):
    import torch

    n, c = SHAPES[i]
    g = torch.Generator().manual_seed(1000 + i)
    z = torch.randn(n, c, generator=g)
    y = torch.randint(0, c, (n,), generator=g)
    rows = torch.arange(0, n, 3)
    z[rows, y[rows]] += 3
    # the two references, every row
    r = rank_rule(z.numpy(), y.numpy())
    ref = (int((r < 1).sum()), int((r < 5).sum()))
    a1, a5 = dtc.trainer.accuracy(z, y, topk=(1, 5))
    acc = (int(round(float(a1) * n / 100)), int(round(float(a5) * n / 100)))
    zd, yd = z.to(cuda), y.to(cuda)
    rec = dtc.ops.eval_metrics(zd, yd, topk=5)
    loss, _ = dtc.ops.xent_fwd(zd, yd)
    torch.cuda.synchronize()
    lb, rn, t1, t5 = _record(rec)
    print(f"case {i} ({n}x{c}): rank rule {ref}, accuracy {acc}, kernel {(t1, t5)}, loss bits {lb:#x} / "
          f"{int(_bits(loss)[0]):#x}")
    assert ref == COUNTS[i] and acc == COUNTS[i]
    assert rn == n and (t1, t5) == COUNTS[i]
    assert np.array_equal(np.array([lb], np.int32), _bits(loss))


def test_metrics_special_rows(dtc, cuda):
    import torch

    nan, inf = float("nan"), float("inf")
    z = torch.tensor([[1, nan, .5], [nan, 1, 2], [1, 1, 1], [inf, -inf, 0]], dtype=torch.float32)
    y = torch.tensor([0, 0, 2, 1])
    want = [1, 2, 2, 2]
    assert rank_rule(z.numpy(), y.numpy()).tolist() == want
    zd, yd = z.to(cuda), y.to(cuda)
    _, rn, t1, t2 = _record(dtc.ops.eval_metrics(zd, yd, topk=2))
    assert (rn, t1, t2) == (4, 0, 1)
    # each row alone: rank < k is a hit, which pins the rank exactly
    for row, rk in enumerate(want):
        for k in (1, 2, 3):
            _, _, _, tk = _record(dtc.ops.eval_metrics(zd[row:row + 1].contiguous(), yd[row:row + 1].contiguous(), topk=k))
            assert tk == (1 if rk < k else 0), (row, k)
    # one label out of range: NaN loss, the same bits as xent_fwd's, and the row is a miss for both counts
    g = torch.Generator().manual_seed(5)
    z = torch.randn(6, 10, generator=g)
    y = z.argmax(1)
    yb = y.clone()
    yb[4] = 10
    zd = z.to(cuda)
    rec_ok = dtc.ops.eval_metrics(zd, y.to(cuda), topk=2)
    rec_bad = dtc.ops.eval_metrics(zd, yb.to(cuda), topk=2)
    loss_bad, _ = dtc.ops.xent_fwd(zd, yb.to(cuda))
    assert _record(rec_ok)[1:] == (6, 6, 6)
    lb, rn, t1, t2 = _record(rec_bad)
    assert np.isnan(_loss_of(rec_bad)) and np.array_equal(np.array([lb], np.int32), _bits(loss_bad))
    assert (rn, t1, t2) == (6, 5, 5)
    yb[4] = -1
    assert _record(dtc.ops.eval_metrics(zd, yb.to(cuda), topk=2))[1:] == (6, 5, 5)


def test_metrics_writes_one_slot_only(dtc, cuda):
    import torch

    sentinel = 0x5A5A5A5A
    recs = torch.full((5, 4), sentinel, dtype=torch.int32, device=cuda)
    g = torch.Generator().manual_seed(11)
    z = torch.randn(33, 100, generator=g).to(cuda)
    y = torch.randint(0, 100, (33,), generator=g).to(cuda)
    out = dtc.ops.eval_metrics(z, y, topk=5, out=recs[2])
    assert out.data_ptr() == recs[2].data_ptr()
    got = recs.cpu().numpy()
    assert (got[[0, 1, 3, 4]] == sentinel).all()
    assert tuple(got[2]) == _record(dtc.ops.eval_metrics(z, y, topk=5)) and got[2, 1] == 33


# ----------------------------------------------------------------------------- the executor's eval batch
B = 8


@pytest.fixture(scope="module")
def net(dtc, cuda):
    """Seeded ResNet18 on the GPU with non-trivial running statistics, one seeded input batch, and per
    precision the eval-mode forward's logits of the full batch (computed once, never modified)."""
    import torch

    torch.manual_seed(21)
    model = dtc.ResNet18().to(cuda)
    g = torch.Generator().manual_seed(22)
    model.flat.bufs.copy_(torch.rand(model.flat.bufs.numel(), generator=g) + 0.5)  # running mean / var in [0.5, 1.5)
    x = torch.randn(B, 3, 32, 32, generator=g).to(cuda)
    y = torch.randint(0, 100, (B,), generator=g).to(cuda)
    ref = {}
    for prec in dtc.nn.PRECISIONS:
        lg = torch.empty(B, 100, dtype=torch.float32, device=cuda)
        model.executor(B, 32, 32, prec).forward(x, lg, False)
        ref[prec] = lg
    torch.cuda.synchronize()
    return model, x, y, ref


def _state(model):
    """Parameters, their bf16 shadow (as words), running statistics and num_batches_tracked, on the host."""
    import torch

    f = model.flat
    return [t.detach().cpu().numpy().copy() for t in (f.params, f.params_bf16.view(torch.int16), f.bufs, f.nbt)]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_eval_batch_full(dtc, cuda, net, prec):
    import torch

    model, x, y, ref = net
    exe = model.executor(B, 32, 32, prec)
    before = _state(model)
    lg = torch.full((B, 100), float("nan"), dtype=torch.float32, device=cuda)
    rec = torch.zeros(4, dtype=torch.int32, device=cuda)
    exe.eval_batch(x, y, B, 5, rec, logits=lg)
    want = dtc.ops.eval_metrics(ref[prec], y, topk=5)
    torch.cuda.synchronize()
    assert np.isfinite(ref[prec].cpu().numpy()).all()
    assert np.array_equal(_bits(lg), _bits(ref[prec]))
    assert _record(rec) == _record(want) and _record(rec)[1] == B
    for a, b in zip(before, _state(model)):
        assert np.array_equal(a, b)
    # logits = None: the record alone, from the executor's own logits region
    rec2 = torch.zeros(4, dtype=torch.int32, device=cuda)
    exe.eval_batch(x, y, B, 5, rec2)
    assert _record(rec2) == _record(want)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("n_valid", [5, 1])
def test_eval_batch_partial(dtc, cuda, net, prec, n_valid):
    """A short batch on the full-batch executor: rows [0, n_valid) are bit-equal to the full-batch run, also
    when the rows >= n_valid of the tensor passed in are NaN (they are never read; the executor's padding is
    zeros), and the record is that of the valid rows alone."""
    import torch

    model, x, y, ref = net
    exe = model.executor(B, 32, 32, prec)
    want = dtc.ops.eval_metrics(ref[prec][:n_valid].contiguous(), y[:n_valid].contiguous(), topk=5)
    for poison in (False, True):
        xin = x.clone()
        if poison:
            xin[n_valid:] = float("nan")
        lg = torch.full((B, 100), float("nan"), dtype=torch.float32, device=cuda)
        rec = torch.zeros(4, dtype=torch.int32, device=cuda)
        exe.eval_batch(xin, y, n_valid, 5, rec, logits=lg)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(lg[:n_valid]), _bits(ref[prec][:n_valid])), (prec, n_valid, poison)
        assert np.isfinite(lg.cpu().numpy()).all()  # the padding rows are the zero image's, not stale or NaN
        assert np.isfinite(_loss_of(rec))
        assert _record(rec) == _record(want) and _record(rec)[1] == n_valid


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_eval_batch_odd_extents(dtc, cuda, net, prec):
    """eval_batch at 18x21 (every stride-2 block sees an odd map: even/odd, odd/odd, odd/even), batch 3, the full
    batch (n_valid 3) and a short one (2), as test_eval_batch_partial: the valid rows bit-equal to the eval-mode
    forward's, the padding rows finite, the record that of the valid rows; the weights untouched."""
    import torch

    model = net[0]
    nb, h, w = 3, 18, 21
    g = torch.Generator().manual_seed(23)
    x = torch.randn(nb, 3, h, w, generator=g).to(cuda)
    y = torch.randint(0, 100, (nb,), generator=g).to(cuda)
    exe = model.executor(nb, h, w, prec)
    ref = torch.empty(nb, 100, dtype=torch.float32, device=cuda)
    exe.forward(x, ref, False)
    torch.cuda.synchronize()
    assert np.isfinite(ref.cpu().numpy()).all()
    before = _state(model)
    for n_valid in (3, 2):
        want = dtc.ops.eval_metrics(ref[:n_valid].contiguous(), y[:n_valid].contiguous(), topk=5)
        for poison in (False, True):
            xin = x.clone()
            if poison:
                xin[n_valid:] = float("nan")
            lg = torch.full((nb, 100), float("nan"), dtype=torch.float32, device=cuda)
            rec = torch.zeros(4, dtype=torch.int32, device=cuda)
            exe.eval_batch(xin, y, n_valid, 5, rec, logits=lg)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(lg[:n_valid]), _bits(ref[:n_valid])), (prec, n_valid, poison)
            assert np.isfinite(lg.cpu().numpy()).all()
            assert np.isfinite(_loss_of(rec))
            assert _record(rec) == _record(want) and _record(rec)[1] == n_valid
    for a, b in zip(before, _state(model)):
        assert np.array_equal(a, b)


def test_backward_after_eval_batch_is_refused(dtc, cuda, net):
    import torch

    model, x, y, _ = net
    before = _state(model)
    model.train()
    try:
        loss = dtc.CrossEntropyLoss()(model(x), y)
        exe = model.executor(B, 32, 32)
        exe.eval_batch(x, y, B, 5, torch.zeros(4, dtype=torch.int32, device=cuda))
        with pytest.raises(dtc.NativeError):
            loss.backward()
    finally:
        model.eval()
        f = model.flat  # the training forward updated the running statistics: put the fixture's back
        f.bufs.copy_(torch.from_numpy(before[2]))
        f.nbt.copy_(torch.from_numpy(before[3]))
        torch.cuda.synchronize()


def test_evaluate_short_last_batch_uses_one_executor(dtc, cuda, net):
    """ResNet.evaluate over 8 + 8 + 3 images: the records equal the per-batch default computation, and the short
    batch took no executor of its own."""
    import torch

    model, x, y, ref = net
    model.precision = "fp32"
    try:
        n_exec = len(model._executors)
        batches = [(x, y), (x, y.flip(0).contiguous()), (x[:3].contiguous(), y[:3].contiguous())]
        res = model.evaluate(batches, topk=5)
        assert len(model._executors) == n_exec
        assert res.n.tolist() == [8, 8, 3]
        for i, (xb, yb) in enumerate(batches):
            want = dtc.ops.eval_metrics(ref["fp32"][:xb.shape[0]].contiguous(), yb, topk=5)
            lb, rn, t1, t5 = _record(want)
            assert (int(res.loss[i:i + 1].view(np.int32)[0]), int(res.n[i]), int(res.top1[i]), int(res.topk[i])) == \
                (lb, rn, t1, t5)
    finally:
        model.precision = None


def test_trainer_fused_eval_matches_default(dtc, cuda, tmp_path):
    """Trainer.test with --fused-eval returns exactly the default path's three numbers for the same weights
    (192 test images at batch 64: three full batches, the same executor on both paths)."""
    import torch

    base = ["--device-data", "--synthetic-train", "640", "--synthetic-test", "192", "--batch-size", "64",
            "--workers", "0", "--ckpt-path", str(tmp_path)]
    torch.manual_seed(3)
    off = dtc.trainer.Trainer(dtc.trainer.load_config(base, "single"), dtc.ResNet18(), None)
    state = {k: v.detach().clone() for k, v in off.model.state_dict().items()}
    on = dtc.trainer.Trainer(dtc.trainer.load_config(base + ["--fused-eval"], "single"), dtc.ResNet18(), None)
    want = off.test(state)
    got = on.test(state)
    print("default", want, "fused", got)
    assert set(got) == {"test_loss", "top_1_acc", "top_5_acc"}
    assert np.isfinite(want["test_loss"]) and got == want
    assert len(on._module_for_eval()._executors) == 1
