"""Gradient accumulation: the flat accumulate kernel (dtc_grad_accum_flat), the executor's bucket-point hook
(dtc_rn18_set_grad_accum), ResNet.accumulate() / grad_accum_steps and DistributedDataParallel.no_sync().

Everything here is bit-exact. The kernel does one IEEE fp32 add per element, so numpy's float32 add is its
reference; the executor's window is compared against the same kernel applied to the three gradients taken one by
one (the backward itself is bit-reproducible: DESIGN §2); a two-term fp32 sum over ranks has no order.
"""
import contextlib
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OFF, STORE, ADD, FINISH = 0, 1, 2, 3
# accum.hip / kernels.h: a workgroup of DTC_ACCUM_THREADS takes DTC_ACCUM_UNROLL float4 rows per thread and trip, the
# grid is capped at DTC_ACCUM_MAX_BLOCKS workgroups
THREADS, UNROLL, MAX_BLOCKS = 256, 4, 1024
TRIP = THREADS * UNROLL * 4  # fp32 elements of one workgroup trip
SENTINEL = np.int32(0x7FC0DEAD)  # a NaN bit pattern no add of these inputs produces
BASE = 64  # element offset of every range into its arena

# n = 4; one workgroup trip - 4, exactly one, + 4; ~1.1 M elements: 268 full chunks and a ragged one (at this
# grid cap still one grid trip); two full grid-stride trips, a third partial one and a ragged last chunk
LENGTHS = [4, TRIP - 4, TRIP, TRIP + 4, 1_100_004, (2 * MAX_BLOCKS + 3) * TRIP + 1028]


def _values(rng, n):
    """random sign, magnitude in [2^-10, 2^10]: every sum is a multiple of 2^-33, far from the denormal range"""
    mag = np.exp2(rng.uniform(-10.0, 10.0, n)).astype(np.float32)
    return np.where(rng.random(n) < 0.5, -mag, mag).astype(np.float32)


def _arena(vals):
    a = np.full(vals.size + 2 * BASE, SENTINEL, dtype=np.int32)
    a[BASE:BASE + vals.size] = vals.view(np.int32)
    return a


def _dev(a, cuda):
    return torch.from_numpy(a.copy()).to(cuda).view(torch.float32)


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("mode", [STORE, ADD, FINISH])
@pytest.mark.parametrize("n", LENGTHS)
def test_flat_kernel_bit_exact_against_numpy(dtc, cuda, mode, n):
    rng = np.random.default_rng(1000 * mode + n % 997)
    acc, g = _values(rng, n), _values(rng, n)
    acc_arena, g_arena = _arena(acc), _arena(g)
    want_acc, want_g = acc_arena.copy(), g_arena.copy()
    if mode == STORE:
        want_acc[BASE:BASE + n] = g.view(np.int32)
    elif mode == ADD:
        want_acc[BASE:BASE + n] = (acc + g).astype(np.float32).view(np.int32)
    else:
        want_g[BASE:BASE + n] = (g + acc).astype(np.float32).view(np.int32)
    d_acc, d_g = _dev(acc_arena, cuda), _dev(g_arena, cuda)
    dtc.ops.grad_accum_flat(d_acc[BASE:BASE + n], d_g[BASE:BASE + n], mode)
    torch.cuda.synchronize()
    # the destination range bit for bit, the sentinels on both sides of both ranges and the whole other operand
    assert np.array_equal(_bits(d_acc), want_acc)
    assert np.array_equal(_bits(d_g), want_g)


def test_flat_kernel_propagates_inf_and_nan(dtc, cuda):
    inf = float("inf")
    for mode in (ADD, FINISH):
        acc = torch.tensor([inf, inf, 1.0, 2.0], device=cuda)
        g = torch.tensor([1.0, -inf, inf, 3.0], device=cuda)
        dtc.ops.grad_accum_flat(acc, g, mode)
        out = (acc if mode == ADD else g).cpu().numpy()
        assert out[0] == inf and np.isnan(out[1]) and out[2] == inf and out[3] == 5.0, (mode, out)


def _model(dtc, cuda, cap_mb=1.0):
    torch.manual_seed(42)
    m = dtc.ResNet18().to(cuda)
    m.set_bucket_cap_mb(cap_mb)
    return m


def test_argument_refusals_launch_nothing(dtc, cuda):
    lib, err = dtc._native.lib, dtc._native.last_error
    st = dtc._native.stream_ptr()
    acc = torch.full((64,), 3.0, device=cuda)
    g = torch.full((64,), 5.0, device=cuda)
    pa, pg = acc.data_ptr(), g.data_ptr()
    einval = -1
    for args, word in (((pa, pg, 6, ADD), "multiple of 4"), ((pa, pg, 0, ADD), "multiple of 4"),
                       ((pa + 4, pg, 8, ADD), "aligned"), ((pa, pg + 8, 8, FINISH), "aligned"),
                       ((pa, pa + 16, 8, STORE), "overlap"), ((pa + 16, pa, 8, ADD), "overlap"),
                       ((pa, pg, 8, OFF), "mode"), ((pa, pg, 8, 4), "mode"), ((None, pg, 8, ADD), "null")):
        assert lib.dtc_grad_accum_flat(args[0], args[1], args[2], args[3], st) == einval, args
        assert word in err(), (args, err())
    model = _model(dtc, cuda)
    exe = model.executor(8, 32, 32, "bf16")
    flat = model.flat
    good = flat.grad_acc.data_ptr()
    assert lib.dtc_rn18_set_grad_accum(exe.handle, None, STORE) == einval and "NULL" in err()
    assert lib.dtc_rn18_set_grad_accum(exe.handle, flat.grads.data_ptr() + 256, ADD) == einval and "overlaps" in err()
    assert lib.dtc_rn18_set_grad_accum(exe.handle, good + 4, ADD) == einval and "aligned" in err()
    assert lib.dtc_rn18_set_grad_accum(exe.handle, good, 7) == einval and "mode" in err()
    assert lib.dtc_rn18_set_grad_accum(exe.handle, None, OFF) == 0
    # STORE / ADD with a communicator passed to a backward
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 2.0, world=2)
    try:
        flat.grads.fill_(7.0)
        flat.grad_acc.fill_(9.0)
        dl = exe.dlogits_buffer()
        for mode in (STORE, ADD):
            assert lib.dtc_rn18_set_grad_accum(exe.handle, good, mode) == 0
            assert lib.dtc_rn18_backward(exe.handle, dl.data_ptr(), 1.0, comm.handle, st) == einval
            assert "communicator" in err()
        assert lib.dtc_rn18_set_grad_accum(exe.handle, None, OFF) == 0
        assert comm.log() == []
    finally:
        comm.close()
    torch.cuda.synchronize()
    assert bool((acc == 3.0).all()) and bool((g == 5.0).all())
    assert bool((flat.grads == 7.0).all()) and bool((flat.grad_acc == 9.0).all())


# ----------------------------------------------------------------------------- executor window
def _micro_batches(cuda, n, batch=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(batch, 3, 32, 32, generator=g).to(cuda) for _ in range(n)]
    ys = [torch.randint(0, 100, (batch,), generator=g).to(cuda) for _ in range(n)]
    return xs, ys


class _Case:
    """A model with fixed parameters, three micro-batches of 8 and one way of running a backward."""

    def __init__(self, dtc, cuda, precision, fast, soft, steps=3):
        self.dtc, self.fast = dtc, fast
        self.model = _model(dtc, cuda)
        self.model.precision = precision
        self.model.grad_accum_steps = steps
        self.crit = dtc.CrossEntropyLoss(label_smoothing=0.1 if soft else 0.0)
        self.xs, self.ys = _micro_batches(cuda, 3)
        if soft:  # a Mixup target: partner labels and a per-row lam
            g = torch.Generator().manual_seed(5)
            lam = torch.rand(8, generator=g).to(cuda)
            self.ys = [dtc.nn.MixedTarget(y, y.roll(1), lam) for y in self.ys]
        self.one = torch.ones((), device=cuda)

    def backward(self, i):
        loss = self.crit(self.model(self.xs[i]), self.ys[i])
        if self.fast:
            assert isinstance(loss, self.dtc.nn.NativeLoss)
            loss.backward()
        else:
            loss.backward(gradient=self.one)

    def singles_and_expected(self):
        """the three gradients taken one by one with plain backwards, and their window sum formed on the device
        by the flat kernel on copies: STORE g0, ADD g1, FINISH onto g2"""
        singles = []
        for i in range(3):
            self.backward(i)
            singles.append(self.model.flat.grads.clone())
        acc = torch.empty_like(singles[0])
        expected = singles[2].clone()
        self.dtc.ops.grad_accum_flat(acc, singles[0].clone(), STORE)
        self.dtc.ops.grad_accum_flat(acc, singles[1].clone(), ADD)
        self.dtc.ops.grad_accum_flat(acc, expected, FINISH)
        return singles, expected

    def window(self):
        with self.model.accumulate():
            self.backward(0)
            self.backward(1)
        self.backward(2)
        return self.model.flat.grads


_SHARED = {}


def _shared_reference(dtc, cuda):
    """(singles, expected) of the bf16 / NativeLoss / hard-label case under the default options: computed once,
    read-only, shared by the window test and the graph-mode test"""
    if "ref" not in _SHARED:
        _SHARED["ref"] = _Case(dtc, cuda, "bf16", True, False).singles_and_expected()
    return _SHARED["ref"]


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("fast", [True, False], ids=["nativeloss", "autograd"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_executor_window_bit_exact(dtc, cuda, precision, fast, soft):
    """Fails on the code before this feature (no accumulate(); the window would leave the last micro-batch's
    gradient), and for anything that merely leaves the last micro-batch's gradient in place."""
    case = _Case(dtc, cuda, precision, fast, soft)
    assert len(case.model.buckets()) >= 6  # cap 1 MB: a bucket point after most blocks
    if (precision, fast, soft) == ("bf16", True, False):
        singles, expected = _shared_reference(dtc, cuda)
    else:
        singles, expected = case.singles_and_expected()
    assert not torch.equal(expected, singles[2]) and bool(torch.isfinite(expected).all())
    got = case.window()
    assert torch.equal(got, expected)
    assert not case.model._accum_open
    # OFF is restored and the stale accumulation buffer has no effect: a plain backward, bit for bit
    case.backward(1)
    assert torch.equal(case.model.flat.grads, singles[1])
    # an abandoned window is dropped by reset_accumulation()
    with case.model.accumulate():
        case.backward(0)
    assert case.model._accum_open
    case.model.reset_accumulation()
    case.backward(2)
    assert torch.equal(case.model.flat.grads, singles[2])


def test_loss_over_n_through_autograd(dtc, cuda):
    """grad_accum_steps = 1 and (loss / N).backward(): autograd scales dlogits by 1 / N where grad_accum_steps scales
    the kernels' grad_scale, so the window holds the same mean up to fp32 rounding. fp32 executor; the bound: unit
    roundoff 6e-8, fewer than 100 rounding points on any path from dlogits to a gradient, up to ~10x amplification
    by the cancellation in the BN backward sums -> 6e-5, asserted as 1e-4 (a missed micro-batch or a wrong scale
    is off by more than 0.1)."""
    _, expected = _Case(dtc, cuda, "fp32", True, False).singles_and_expected()
    case = _Case(dtc, cuda, "fp32", True, False, steps=1)
    m = case.model
    with m.accumulate():
        for i in range(2):
            (case.crit(m(case.xs[i]), case.ys[i]) / 3).backward()
    (case.crit(m(case.xs[2]), case.ys[2]) / 3).backward()
    got = m.flat.grads.double()
    rel = float((got - expected.double()).norm() / expected.double().norm())
    print(f"loss / N through autograd vs grad_accum_steps: rel err {rel:.3e}")
    assert rel < 1e-4, rel


@pytest.mark.parametrize("on_side", [0, 1])
def test_finish_precedes_the_collective(dtc, cuda, on_side):
    lib = dtc._native.lib
    prev = lib.dtc_get_option(b"comm_on_side")
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 2.0, world=2)
    try:
        lib.dtc_set_option(b"comm_on_side", on_side)
        model = _model(dtc, cuda)
        model._grad_scale = 1.0
        crit = dtc.CrossEntropyLoss()
        xs, ys = _micro_batches(cuda, 2, seed=13)

        def bwd(i):
            with dtc.autocast():
                crit(model(xs[i]), ys[i]).backward()

        plain = []
        for i in range(2):
            bwd(i)
            plain.append(model.flat.grads.clone())
        model._comm = comm
        comm.clear_log()
        with model.accumulate():
            bwd(0)
        torch.cuda.synchronize()
        assert [e for e in comm.log() if e[2]] == []  # nothing reduced inside the window
        bwd(1)
        torch.cuda.synchronize()
        buckets = model.buckets()
        base = model.flat.grads.data_ptr()
        log = [((a - base) // 4, n) for a, n, is_bucket in comm.log() if is_bucket]
        assert log == buckets  # exactly one collective per bucket
        want = plain[1].clone()
        dtc.ops.grad_accum_flat(plain[0].clone(), want, FINISH)  # g2 + g1
        want = want * 2.0  # exact; a collective ahead of the add would give 2 * g2 + g1
        assert torch.equal(model.flat.grads, want)
        assert not torch.equal(model.flat.grads, plain[1] * 2.0 + plain[0])
    finally:
        lib.dtc_set_option(b"comm_on_side", prev)
        comm.close()


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


def test_two_ranks_no_sync_distinct_data(dtc, cuda):
    world, steps, cap_mb = 2, 2, 1.0
    xs, ys = _micro_batches(cuda, world * steps, seed=17)  # micro-batch k of rank r: index r * steps + k
    # each rank's accumulated gradient, built as in the window test, with DDP's pre-scale 1 / world
    ref = _model(dtc, cuda, cap_mb)
    ref._grad_scale = 1.0 / world
    ref.grad_accum_steps = steps
    crit = dtc.CrossEntropyLoss()
    per_rank = []
    for r in range(world):
        gs = []
        for k in range(steps):
            with dtc.autocast():
                crit(ref(xs[r * steps + k]), ys[r * steps + k]).backward()
            gs.append(ref.flat.grads.clone())
        dtc.ops.grad_accum_flat(gs[0], gs[1], FINISH)  # g1 + g0
        per_rank.append(gs[1])
    torch.cuda.synchronize()
    expect = (per_rank[0] + per_rank[1]).cpu().numpy()  # a two-term fp32 sum has no order

    comms = dtc.parallel.Comm.thread_group(cuda.index or 0, world)
    models = [_model(dtc, cuda, cap_mb) for _ in range(world)]
    n_buckets = len(models[0].buckets())

    def rank(r):
        m = models[r]
        ddp = dtc.DistributedDataParallel(m, device_ids=[0], bucket_cap_mb=cap_mb, comm=comms[r])
        m.grad_accum_steps = steps
        comms[r].clear_log()
        crit_r = dtc.CrossEntropyLoss()
        for k in range(steps):
            with dtc.autocast():
                loss = crit_r(ddp(xs[r * steps + k]), ys[r * steps + k])
            with ddp.no_sync() if k < steps - 1 else contextlib.nullcontext():
                loss.backward()
        return m.flat.grads.cpu().numpy().copy(), comms[r].log()

    res = _run_ranks(rank, world)
    for r in range(world):
        g, log = res[r]
        assert np.array_equal(g, expect), r
        assert len([e for e in log if e[2]]) == n_buckets, (r, len(log), n_buckets)  # not 2 * n_buckets


def test_amp_skip_through_a_window(dtc, cuda):
    model = _model(dtc, cuda)
    model.grad_accum_steps = 2
    crit = dtc.CrossEntropyLoss()
    opt = dtc.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    opt.attach(model)
    scaler = dtc.GradScaler(init_scale=1024.0)
    xs, ys = _micro_batches(cuda, 2, seed=19)
    flat = model.flat

    def window(poison):
        with dtc.autocast():
            loss = crit(model(xs[0]), ys[0])
        with model.accumulate():
            scaler.scale(loss).backward()
        if poison:
            flat.grad_acc[123457] = float("inf")
        with dtc.autocast():
            loss = crit(model(xs[1]), ys[1])
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    before = (flat.params.clone(), opt._mom.clone(), flat.params_bf16.clone())
    window(poison=True)
    assert not bool(torch.isfinite(flat.grads).all())  # the inf came through FINISH
    assert torch.equal(flat.params, before[0]) and torch.equal(opt._mom, before[1])
    assert torch.equal(flat.params_bf16.view(torch.int16), before[2].view(torch.int16))
    assert scaler.get_scale() == 512.0
    window(poison=False)
    assert bool(torch.isfinite(flat.grads).all())
    assert not torch.equal(flat.params, before[0]) and scaler.get_scale() == 512.0


def test_graph_modes_plain_window_plain(dtc, cuda):
    lib = dtc._native.lib
    singles, expected = _shared_reference(dtc, cuda)  # under the default options
    prev = lib.dtc_get_option(b"graphs")
    try:
        lib.dtc_set_option(b"graphs", 1)
        case = _Case(dtc, cuda, "bf16", True, False)
        case.backward(1)
        plain_a = case.model.flat.grads.clone()
        got = case.window().clone()
        case.backward(1)
        plain_b = case.model.flat.grads.clone()
        assert torch.equal(plain_a, plain_b)
        assert torch.equal(got, expected)
    finally:
        lib.dtc_set_option(b"graphs", prev)


def test_data_parallel_refuses_accumulation(dtc, cuda):
    model = _model(dtc, cuda)
    dp = dtc.DataParallel(model, device_ids=[cuda.index or 0, cuda.index or 0])
    x = torch.randn(8, 3, 32, 32, device=cuda)
    model.grad_accum_steps = 2
    with pytest.raises(dtc.NativeError, match="gradient accumulation"):
        dp(x)
    model.grad_accum_steps = 1
    with model.accumulate():
        with pytest.raises(dtc.NativeError, match="gradient accumulation"):
            dp(x)
    out = dp(x)  # and the plain path still runs
    with model.accumulate():  # a window opened between the forward and the backward
        with pytest.raises(dtc.NativeError, match="gradient accumulation"):
            out.sum().backward()


@pytest.mark.parametrize("amp", [True, False], ids=["amp", "fp32"])
def test_trainer_accum_steps_counts_optimizer_steps(dtc, cuda, tmp_path, amp):
    """--accum-steps 2 over 5 loader iterations (--max-steps ends the epoch early): windows of 2, 2 and a partial 1,
    so 3 optimizer steps and 3 EMA updates against 5 global steps; no window stays open behind the epoch."""
    dtc.data.fix_seed(42)
    init = dtc.ResNet18().state_dict()["linear.weight"].clone()
    dtc.data.fix_seed(42)
    args = ["--max-steps", "5", "--epoch", "1", "--synthetic-train", "64", "--synthetic-test", "16", "--batch-size",
            "8", "--workers", "0", "--accum-steps", "2", "--model-ema", "--model-ema-decay", "0.5", "--ckpt-path",
            str(tmp_path)] + (["--amp"] if amp else [])
    t = dtc.trainer.main(args, "single")
    assert t.global_step == 5 and t.optimizer_step == 3
    assert t.model.grad_accum_steps == 2 and not t.model._accum_open and t.model._accum_depth == 0
    assert int(t.ema.state[0].item()) == 3  # one EMA update per optimizer step
    now = t.model.state_dict()["linear.weight"].cpu()
    assert bool(torch.isfinite(now).all()) and not torch.equal(now, init.cpu())
