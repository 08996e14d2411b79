"""PowerSGD on the device (csrc/powersgd.hip, nn.PowerSGD) against tests/powersgd_ref.py, the float64 torch-CPU
restatement of the algorithm. Yardstick (test_gpu_optim.py's convention): per tensor
max|gpu - f64| <= 2 * max|f32 - f64|, f32 being the same restatement run in float32; both are printed.

The kernel-level cases run over an arena of 64-element aligned segments whose padding holds a sentinel:
4 x 12 (compressed at rank 1 only), 64 x 27 (rows not 16-byte aligned; every later Q block misaligned at ranks 1
and 2), 100 x 512, 128 x 64, 600 x 16 (19 back-project row chunks), 40 x 2052 (three column blocks of two row
chunks), 36 x 301 (scalar path, two column blocks) and 1-D segments of 10, 64 and 100 elements.

Measured on an MI355X, worst ratio max|gpu - f64| / max|f32 - f64| over the tensors and steps of a case (the bound
is 2): one rank, three steps, normal and x65536 inputs 0.976 (rank 1), 0.508 (rank 2), 0.518 (rank 4); rank-1 inputs
1.000 / 0.286 / 0.182; all-zero inputs 0 = 0; thread group of 2 ranks 0.465, of 3 ranks 0.442; through the model
(two ranks, iterations 2 and 3) 0.477. The kernels sum in double and round once, so they sit below the float32
restatement everywhere; the factor was not widened."""
import threading

import numpy as np
import pytest
import torch

from tests.powersgd_ref import PowerSGDRef

pytestmark = pytest.mark.gpu

SHAPES = [(4, 12), (10,), (64, 27), (100, 512), (64,), (128, 64), (600, 16), (100,), (40, 2052), (36, 301)]
SENT = float(np.float32(-12345.678))
SEED = 5


def _tensors(dtc, rank):
    out, off = [], 64
    for shp in SHAPES:
        if len(shp) == 1:
            out.append((off, shp[0], 1, 0))
        else:
            r, c = shp
            out.append((off, r, c, min(r, c, rank) if dtc.ops.psgd_should_compress(r, c, rank) else 0))
        off = (off + out[-1][1] * out[-1][2] + 63) // 64 * 64
        if len(shp) == 1 and shp[0] % 64 == 0:
            off += 64
    return out, off + 64


def _mask(tensors, total):
    m = torch.zeros(total, dtype=torch.bool)
    for o, r, c, _ in tensors:
        m[o:o + r * c] = True
    return m


def _inputs(tensors, total, kind, world, steps, seed=11):
    """grads[step][rank]: flat float32 CPU tensors, the sentinel between the tensors. "rank1": every 2-D tensor is
    (step + 1) * u w^T with small-integer u and w that stay the same over the steps (exact in fp32, and the warm
    start stays aligned with w: a new direction at every step would make w . Qh small against |w| and amplify the
    rounding noise the error buffer carries -- a property of the method, not of the kernels)."""
    gen = torch.Generator().manual_seed(seed)
    base = {}
    grads = []
    for s in range(steps):
        row = []
        for w_ in range(world):
            g = torch.full((total,), SENT, dtype=torch.float32)
            for i, (o, r, c, k) in enumerate(tensors):
                if kind == "zeros":
                    v = torch.zeros(r * c)
                elif kind == "rank1" and c > 1:
                    if (w_, i) not in base:
                        u = torch.randint(-8, 9, (r, 1), generator=gen).float()
                        w = torch.randint(-8, 9, (1, c), generator=gen).float()
                        u[0, 0], w[0, 0] = 3.0, -5.0
                        base[(w_, i)] = (u @ w).reshape(-1)
                    v = base[(w_, i)] * float(s + 1)
                else:
                    v = torch.randn(r * c, generator=gen)
                    if kind == "scaled":
                        v = v * 65536.0
                g[o:o + r * c] = v
            row.append(g)
        grads.append(row)
    return grads


class _Rank:
    """One rank's device side of the kernel-level cases: its own plan, staging / Q / state with sentinel tails, g, e."""

    def __init__(self, dtc, cuda, tensors, total, error_feedback=True):
        self.dtc, self.tensors, self.total = dtc, tensors, total
        self.plan = dtc.ops.psgd_plan(tensors, device=cuda)
        p = self.plan
        self.staging = torch.full((p.n_staging + 64,), SENT, dtype=torch.float32, device=cuda)
        self.q = torch.full((2 * p.q_stride + 64,), SENT, dtype=torch.float32, device=cuda)
        init = torch.randn(p.n_q, generator=torch.Generator().manual_seed(SEED), dtype=torch.float32)
        self.q[:p.n_q] = init.to(cuda)
        self.state = torch.zeros(4, dtype=torch.int32, device=cuda)
        self.g = torch.full((total,), SENT, dtype=torch.float32, device=cuda)
        self.e = None
        if error_feedback:
            e = torch.full((total,), SENT, dtype=torch.float32)
            e[_mask(tensors, total)] = 0.0
            self.e = e.to(cuda)

    def step(self, g_cpu, c=1.0, allreduce=None, eps=0.0):
        self.g.copy_(g_cpu)
        self.dtc.ops.psgd_step(self.plan, self.g, self.e, self.staging, self.q, self.state, c, eps, allreduce)

    def warm_q(self):
        """the warm start the next step will read (state[0] chooses the copy), on the CPU"""
        p, sel = self.plan, int(self.state[0].item())
        return self.q[sel * p.q_stride:sel * p.q_stride + p.n_q].cpu()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _yardstick(tensors, got, ref64, ref32, what, worst):
    """per compressed tensor: max|gpu - f64| <= 2 * max|f32 - f64|; returns the worst ratio seen so far"""
    for i, (o, r, c, k) in enumerate(tensors):
        if not k:
            continue
        want = ref64[i].reshape(-1)
        err = float((got[o:o + r * c].double() - want).abs().max())
        yard = float((ref32[i].reshape(-1).double() - want).abs().max())
        scale = float(want.abs().max())
        print(f"{what} tensor {r}x{c} r{k}: gpu {err:.3e} f32 {yard:.3e} max|ref| {scale:.3e}")
        assert err <= 2.0 * yard, (what, (r, c, k), err, yard)
        if yard > 0:
            worst = max(worst, err / yard)
    return worst


# ----------------------------------------------------------------------------- (a) steps against the reference
@pytest.mark.parametrize("kind", ["normal", "scaled", "rank1", "zeros"])
@pytest.mark.parametrize("rank", [1, 2, 4])
def test_steps_against_reference(dtc, cuda, rank, kind):
    """Three warm-started steps with error feedback, one rank. Measured worst gpu / f32 error ratio on an MI355X
    (bound 2): normal and scaled 0.976 / 0.508 / 0.518 at ranks 1 / 2 / 4, rank-1 inputs 1.000 / 0.286 / 0.182."""
    tensors, total = _tensors(dtc, rank)
    assert (tensors[0][3] != 0) == (rank == 1) and all(t[3] for t in tensors if t[2] > 1 and t[1] * t[2] > 48)
    grads = _inputs(tensors, total, kind, 1, 3)
    ref64 = PowerSGDRef(tensors, 1, SEED, torch.float64)
    ref32 = PowerSGDRef(tensors, 1, SEED, torch.float32)
    dev = _Rank(dtc, cuda, tensors, total)
    worst = 0.0
    for s, (g,) in enumerate(grads):
        dev.step(g)
        got, e = dev.g.cpu(), dev.e.cpu()
        w64, w32 = ref64.step([g]), ref32.step([g])
        assert torch.isfinite(got[_mask(tensors, total)]).all()
        worst = _yardstick(tensors, got, w64, w32, f"{kind} r{rank} step {s}", worst)
        for i, (o, r, c, k) in enumerate(tensors):
            if k == 0:  # one rank: an uncompressed tensor returns as it was
                assert _same_bits(got[o:o + r * c], g[o:o + r * c])
            elif kind == "zeros":
                assert not got[o:o + r * c].any() and not e[o:o + r * c].any()
            elif kind == "rank1":
                # recovered, nothing left for the error buffer: P, Ph, Q and gh are each rounded to fp32 once
                # (2^-24 relative), the sums are formed in double; 64 roundings of the largest element leave room
                # for their accumulation over the three steps through e
                amax = float(g[o:o + r * c].abs().max())
                assert float((got[o:o + r * c] - g[o:o + r * c]).abs().max()) <= 64 * 2.0 ** -24 * amax
                assert float(e[o:o + r * c].abs().max()) <= 64 * 2.0 ** -24 * amax
    print(f"{kind} r{rank}: worst ratio {worst:.3f}")


# ----------------------------------------------------------------------------- (b) the error identity
@pytest.mark.parametrize("c", [1.0, 0.5])
@pytest.mark.parametrize("rank", [1, 2, 4])
def test_error_identity_and_padding(dtc, cuda, rank, c):
    tensors, total = _tensors(dtc, rank)
    mask = _mask(tensors, total)
    comp = torch.zeros(total, dtype=torch.bool)
    for o, r, cc, k in tensors:
        if k:
            comp[o:o + r * cc] = True
    dev = _Rank(dtc, cuda, tensors, total)
    p = dev.plan
    for s, (g,) in enumerate(_inputs(tensors, total, "normal", 1, 3, seed=13)):
        e_old = dev.e.cpu()
        dev.step(g, c=c)
        gh, e_new = dev.g.cpu(), dev.e.cpu()
        want = (g + e_old) - c * gh  # three separately rounded fp32 operations
        assert _same_bits(e_new[comp], want[comp]), s
        assert _same_bits(e_new[mask & ~comp], e_old[mask & ~comp])  # uncompressed tensors keep no error
        for t in (gh, e_new):
            assert (t[~mask] == SENT).all()
        assert (dev.staging[p.n_staging:] == SENT).all() and (dev.q[2 * p.q_stride:] == SENT).all()
        assert int(dev.state[0]) == 1 and int(dev.state[1]) == 0


def test_without_error_feedback(dtc, cuda):
    tensors, total = _tensors(dtc, 2)
    dev = _Rank(dtc, cuda, tensors, total, error_feedback=False)
    ref64 = PowerSGDRef(tensors, 1, SEED, torch.float64, error_feedback=False)
    ref32 = PowerSGDRef(tensors, 1, SEED, torch.float32, error_feedback=False)
    for s, (g,) in enumerate(_inputs(tensors, total, "normal", 1, 2, seed=17)):
        dev.step(g)
        _yardstick(tensors, dev.g.cpu(), ref64.step([g]), ref32.step([g]), f"no-ef step {s}", 0.0)


# ----------------------------------------------------------------------------- thread group
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


def _rank_ordered_sum(parts):
    """((g_0 + g_1) + ...) + g_{W-1}: fp32 adds in rank order, as the thread-group collective forms them"""
    s = parts[0].clone()
    for p in parts[1:]:
        s = s + p
    return s


def _group_run(dtc, cuda, tensors, total, grads, world, steps=None):
    """every rank's (g, e, warm Q, state, found_inf) after each of `steps` (indices into grads) over a thread group"""
    comms = dtc.parallel.Comm.thread_group(cuda.index or 0, world)
    torch.cuda.synchronize()
    steps = list(range(len(grads))) if steps is None else steps

    def rank(r):
        dev = _Rank(dtc, cuda, tensors, total)
        found = torch.zeros(1, dtype=torch.int32, device=cuda)
        out = []
        for s in steps:
            dev.step(grads[s][r], c=1.0 / world, allreduce=comms[r].allreduce_sum_)
            found.zero_()
            dtc.ops.amp_check_finite(dev.g, found)
            torch.cuda.current_stream().synchronize()
            out.append((dev.g.cpu(), dev.e.cpu(), dev.warm_q(), dev.state.cpu(), int(found.item())))
        return out

    try:
        return _run_ranks(rank, world)
    finally:
        for cm in comms:
            cm.close()


@pytest.mark.parametrize("world", [2, 3])
def test_thread_group_distinct_data(dtc, cuda, world):
    """(c) Measured worst gpu / f32 error ratio on an MI355X (bound 2): 0.465 with 2 ranks, 0.442 with 3."""
    rank = 2
    tensors, total = _tensors(dtc, rank)
    grads = _inputs(tensors, total, "normal", world, 3, seed=19 + world)
    for row in grads:  # the arena stands for pre-divided gradients; the padding must stay finite for the check below
        for g in row:
            g[~_mask(tensors, total)] = 1.0
    res = _group_run(dtc, cuda, tensors, total, grads, world)
    ref64 = PowerSGDRef(tensors, world, SEED, torch.float64)
    ref32 = PowerSGDRef(tensors, world, SEED, torch.float32)
    worst = 0.0
    for s, row in enumerate(grads):
        w64, w32 = ref64.step(row), ref32.step(row)
        g0, _, q0, st0, found0 = res[0][s]
        assert found0 == 0 and int(st0[0]) == 1
        for r in range(1, world):
            g, _, q, _, _ = res[r][s]
            assert torch.equal(g[_mask(tensors, total)], g0[_mask(tensors, total)]) and torch.equal(q, q0), (s, r)
        worst = _yardstick(tensors, g0, w64, w32, f"W{world} step {s}", worst)
        for o, r_, c, k in tensors:
            if k == 0:
                assert _same_bits(g0[o:o + r_ * c], _rank_ordered_sum([g[o:o + r_ * c] for g in row])), (s, o)
    print(f"W{world}: worst ratio {worst:.3f}")


def test_non_finite_step_is_skipped_everywhere(dtc, cuda):
    """(d) an inf in rank 1's gradient at the second step"""
    world, rank = 2, 2
    tensors, total = _tensors(dtc, rank)
    mask = _mask(tensors, total)
    grads = _inputs(tensors, total, "normal", world, 3, seed=29)
    for row in grads:
        for g in row:
            g[~mask] = 1.0
    o, r, c, k = tensors[3]
    assert (r, c) == (100, 512) and k == 2
    grads[1][1][o + 7 * c + 33] = float("inf")
    full = _group_run(dtc, cuda, tensors, total, grads, world)
    skip = _group_run(dtc, cuda, tensors, total, grads, world, steps=[0, 2])
    for rk in range(world):
        (g1, e1, q1, st1, f1), (g2, e2, q2, st2, f2), (g3, e3, q3, st3, f3) = full[rk]
        assert (f1, f2, f3) == (0, 1, 0)  # amp_check_finite trips on every rank
        assert int(st1[0]) == 1 and (int(st2[0]), int(st2[1])) == (0, 1) and (int(st3[0]), int(st3[1])) == (1, 0)
        assert _same_bits(e2, e1) and _same_bits(q2, q1)  # e and the warm-start Q are as before the step
        for o_, r_, c_, k_ in tensors:
            seg = g2[o_:o_ + r_ * c_]
            if k_:
                assert torch.isnan(seg).all()
            else:
                assert _same_bits(seg, _rank_ordered_sum([g[o_:o_ + r_ * c_] for g in grads[1]]))
        (_, _, _, _, _), (gs, es, qs, sts, fs) = skip[rk]
        assert fs == 0 and _same_bits(g3, gs) and _same_bits(e3, es) and _same_bits(q3, qs)


def test_repeatable(dtc, cuda):
    """(e) two runs, bit for bit -- also across whichever workgroup folds the back-project slots"""
    tensors, total = _tensors(dtc, 4)
    grads = _inputs(tensors, total, "normal", 1, 3, seed=31)
    runs = []
    for _ in range(2):
        dev = _Rank(dtc, cuda, tensors, total)
        out = []
        for (g,) in grads:
            dev.step(g)
            out.append((dev.g.cpu(), dev.e.cpu(), dev.q.cpu(), dev.staging.cpu()))
        runs.append(out)
    for a, b in zip(*runs):
        assert all(_same_bits(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- (f) through the model
def _model(dtc, cuda):
    torch.manual_seed(42)
    return dtc.ResNet18().to(cuda)


def _batches(cuda, n, batch=8, seed=23):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(batch, 3, 32, 32, generator=g).to(cuda) for _ in range(n)]
    ys = [torch.randint(0, 100, (batch,), generator=g).to(cuda) for _ in range(n)]
    return xs, ys


def test_through_the_model_two_ranks(dtc, cuda):
    """Iterations are counted as torch's `state.iter`, from 0: with start_powerSGD_iter = 2 iterations 0 and 1 ride
    the native Reducer and equal a hook-less DDP bit for bit; from iteration 2 on the step is PowerSGD's. No
    optimizer step is taken, so every iteration sees the same local gradients (the step is bit-reproducible).
    Measured worst gpu / f32 error ratio on an MI355X (bound 2): 0.477."""
    world = 2
    xs, ys = _batches(cuda, world)
    comms = dtc.parallel.Comm.thread_group(cuda.index or 0, world)
    models = [_model(dtc, cuda) for _ in range(world)]
    torch.cuda.synchronize()
    crit = dtc.CrossEntropyLoss()

    def rank(r):
        m = models[r]
        ddp = dtc.DistributedDataParallel(m, device_ids=[0], comm=comms[r])

        def backward(local=False):
            with dtc.autocast():
                loss = crit(ddp(xs[r]), ys[r])
            if local:
                with m.local_grads():
                    loss.backward()
            else:
                loss.backward()
            torch.cuda.current_stream().synchronize()
            return m.flat.grads.cpu()

        local = backward(local=True)  # this rank's own gradient, already divided by the world size
        plain = backward()            # hook-less DDP
        state = dtc.parallel.PowerSGDState(matrix_approximation_rank=2, start_powerSGD_iter=2, random_seed=SEED)
        ddp.register_comm_hook(state, dtc.parallel.powerSGD_hook)
        its = [backward() for _ in range(4)]
        assert state.iter == 4
        return local, plain, its, m._powersgd.plan.tensors

    try:
        res = _run_ranks(rank, world)
    finally:
        for cm in comms:
            cm.close()
    tensors = res[0][3]
    assert sum(1 for t in tensors if t[3]) == 21
    locals_ = [res[r][0] for r in range(world)]
    plain = res[0][1]
    ref64 = PowerSGDRef(tensors, world, SEED, torch.float64)
    ref32 = PowerSGDRef(tensors, world, SEED, torch.float32)
    worst = 0.0
    for it in range(4):
        g0 = res[0][2][it]
        assert torch.isfinite(g0).all()
        assert _same_bits(res[1][2][it], g0), it  # both ranks hold the same gradients
        if it < 2:
            assert _same_bits(g0, plain) and _same_bits(res[1][1], plain), it
            continue
        assert not _same_bits(g0, plain)
        worst = _yardstick(tensors, g0, ref64.step(locals_), ref32.step(locals_), f"model it {it}", worst)
        for o, r_, c, k in tensors:
            if k == 0:  # the plain mean, exactly
                assert _same_bits(g0[o:o + r_ * c], plain[o:o + r_ * c]), (it, o)
    print(f"model: worst ratio {worst:.3f}")


def test_loopback_log_two_small_allreduces(dtc, cuda):
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 2.0, world=2)
    try:
        m = _model(dtc, cuda)
        (x,), (y,) = _batches(cuda, 1)
        m._comm, m._grad_scale = comm, 0.5
        state = dtc.parallel.PowerSGDState(matrix_approximation_rank=2, start_powerSGD_iter=2)
        m._powersgd, m.grad_compression = dtc.nn.PowerSGD(state), "powersgd"
        crit = dtc.CrossEntropyLoss()
        logs = []
        for _ in range(4):
            comm.clear_log()
            with dtc.autocast():
                crit(m(x), y).backward()
            torch.cuda.synchronize()
            logs.append(comm.log())
        buckets = m.buckets()
        for it in (0, 1):  # the native Reducer: every bucket of the gradient buffer
            assert [((a - m.flat.grads.data_ptr()) // 4, n) for a, n, is_bucket in logs[it] if is_bucket] == buckets
        ps = m._powersgd
        want = [(ps.staging.data_ptr(), 19500), (ps.q[1].data_ptr(), 63030)]
        for it in (2, 3):  # exactly two all-reduces per compressed step
            assert [(a, n) for a, n, _ in logs[it]] == want, it
        assert torch.isfinite(m.flat.grads).all()
    finally:
        m._comm = None
        comm.close()


# ----------------------------------------------------------------------------- (g) a no_sync() window of 2
def test_no_sync_window(dtc, cuda):
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 1.0, world=1)  # the identity, logged
    try:
        m = _model(dtc, cuda)
        xs, ys = _batches(cuda, 2, seed=37)
        crit = dtc.CrossEntropyLoss()
        m.grad_accum_steps = 2

        def window():
            comm.clear_log()
            with dtc.autocast():
                with m.accumulate():  # DistributedDataParallel.no_sync()
                    crit(m(xs[0]), ys[0]).backward()
                torch.cuda.synchronize()
                inside = list(comm.log())
                crit(m(xs[1]), ys[1]).backward()
            torch.cuda.synchronize()
            return inside, m.flat.grads.clone()

        _, mean = window()  # no hook, no communicator: the window's mean gradient
        m._comm = comm
        state = dtc.parallel.PowerSGDState(matrix_approximation_rank=2, start_powerSGD_iter=2, random_seed=SEED)
        m._powersgd, m.grad_compression = dtc.nn.PowerSGD(state), "powersgd"
        for _ in range(2):  # the two plain windows torch's counter asks for
            inside, g = window()
            assert inside == [] and _same_bits(g, mean)
        assert state.iter == 2  # backwards inside the window are not counted
        inside, got = window()
        assert inside == [] and [n for _, n, _ in comm.log()] == [19500, 63030] and state.iter == 3
        # PowerSGD of the window's mean: the same kernels on `mean`, from the same seed
        plan = dtc.ops.psgd_plan(m.flat.layout, 2, 2, cuda)
        staging, q, st = dtc.ops.psgd_buffers(plan, SEED, cuda)
        want, e = mean.clone(), torch.zeros_like(mean)
        dtc.ops.psgd_step(plan, want, e, staging, q, st, 1.0, 0.0, None)
        torch.cuda.synchronize()
        assert _same_bits(got, want) and not _same_bits(got, mean)
        assert _same_bits(m.flat.grad_err, e)
    finally:
        m._comm = None
        comm.close()


# ----------------------------------------------------------------------------- (h) the trainer, one rank
def test_trainer_world_size_one(dtc, cuda, tmp_path):
    import json
    import math
    import os

    import torch.distributed as dist

    par = dtc.parallel
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/rendezvous", rank=0, world_size=1)
    t = None
    try:
        dtc.data.fix_seed(42)
        args = ["--max-steps", "4", "--epoch", "1", "--synthetic-train", "64", "--synthetic-test", "16",
                "--batch-size", "8", "--workers", "0", "--ckpt-path", str(tmp_path / "ckpt"), "--world-size", "1",
                "--grad-compress", "powersgd", "--powersgd-rank", "2", "--powersgd-start-iter", "2"]
        t = dtc.trainer.Trainer(dtc.trainer.load_config(args, "ddp"), dtc.ResNet18(), None, rank=cuda.index or 0,
                                ngpus_per_node=1, distributed=True)
        t.fit()
        mod = t.model.module
        assert t.global_step == 4 and mod.grad_compression == "powersgd"
        assert mod._powersgd.state.iter == 4 and mod._powersgd.plan is not None  # two plain, two compressed steps
        assert int(mod._powersgd.dev_state[0]) == 1 and mod.flat.grad_err.abs().max() > 0
        rows = [json.loads(line) for line in open(os.path.join(t.save_path, "scalars.jsonl"))]
        losses = [r for r in rows if r["tag"] == "loss/epoch"]
        assert len(losses) == 1 and math.isfinite(losses[0]["train"]) and math.isfinite(losses[0]["val"])
        assert torch.isfinite(mod.flat.params).all()
    finally:
        if t is not None and getattr(t.model, "comm", None) is not None:
            if par._WORLD_COMM[0] is t.model.comm:
                par._WORLD_COMM[0] = None
            t.model.comm.close()
        dist.destroy_process_group()
