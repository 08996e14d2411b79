"""bf16 gradient compression: the flat kernels (dtc_grad_compress_bf16 / dtc_grad_decompress_bf16), the bf16
all-reduce of the loopback, thread-group and RCCL transports, the executor's bucket-point hook
(dtc_rn18_set_grad_compress), ResNet.grad_compression and DistributedDataParallel.register_comm_hook.

Everything here is bit-exact: "equal" compares uint16 / uint32 words. The rounding reference is oracle.ops.bf16_bits
(round to nearest even), widening is `bits << 16`, the fp32 adds and multiplies are numpy float32's (one IEEE
operation each), and the backward itself is bit-reproducible, so the gradients of a plain backward are
the operands of every executor reference. A NaN is only checked to be a NaN.
"""
import threading

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import bounds

pytestmark = pytest.mark.gpu

# compress.hip / kernels.h: a workgroup of DTC_COMPRESS_THREADS takes DTC_COMPRESS_UNROLL rows of 8 elements per
# thread and trip (decompress: twice as many rows of 4, the same trip), the grid is capped at DTC_COMPRESS_MAX_BLOCKS
# workgroups
THREADS, UNROLL, MAX_BLOCKS = 256, 4, 1024
TRIP = THREADS * UNROLL * 8  # elements of one workgroup trip
# n = 4, 8, 12 (head / tail rows only, one body row); one trip - 4, exactly one, + 4; ~1.1 M elements (134 full
# chunks and a ragged one); one full grid-stride trip of the capped grid, a second partial one and a ragged last
# chunk with a 4-element row left over
LENGTHS = [4, 8, 12, TRIP - 4, TRIP, TRIP + 4, 1_100_004, (MAX_BLOCKS + 3) * TRIP + 1028]

B16_PAT = np.uint16(bounds._PAT[2])


def _specials():
    """ties to even (down onto an even, up onto an even, just above / below a tie), the two values around the bf16
    overflow threshold, +-inf, NaNs (quiet, signalling with a high and with a low-only payload, negative),
    subnormals, +-0"""
    bits = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0xBF808000, 0xBF818000, 0x7F800000, 0xFF800000,
                     0x7FC00000, 0x7FA00000, 0x7F800001, 0xFFC12345, 0x00000001, 0x80000001, 0x00400000, 0x007FFFFF,
                     0x00008000, 0x00018000, 0x00000000, 0x80000000], dtype=np.uint32).view(np.float32)
    edge = np.array([3.3961776e38, 3.38e38, -3.3961776e38, -3.38e38], dtype=np.float32)
    return np.concatenate([edge, bits])


def _values(rng, n):
    """normals over +-30 decades, random sign, with the special values at the front and again at the very end (the
    last trip, the ragged chunk and the tail row)"""
    v = (10.0 ** rng.uniform(-30.0, 30.0, n)).astype(np.float32)
    v = np.where(rng.random(n) < 0.5, -v, v).astype(np.float32)
    s = _specials()
    k = min(s.size, n)
    v[:k] = s[:k]
    v[n - k:] = s[s.size - k:]
    return v


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _u32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


def _f32_arena(vals, cuda):
    like = torch.from_numpy(vals.copy()).to(cuda)
    return bounds.arena((vals.size,), torch.float32, cuda, like=like)


def _c_arena(n, cuda, shift):
    """a bf16 destination of n words `shift` elements into a (256-byte aligned) arena view: shift 0 is 16-byte
    aligned, shift 4 only 8-byte aligned; the words of the view around it must keep the pattern too"""
    a, view = bounds.arena((n + 8,), torch.bfloat16, cuda)
    c = view[shift:shift + n]
    assert c.data_ptr() % 16 == (8 if shift == 4 else 0)
    return a, view, c


def _assert_c_surroundings(a, view, shift, n):
    assert a.dirty() == 0
    w = _u16(view)
    assert (w[:shift] == B16_PAT).all() and (w[shift + n:] == B16_PAT).all()


def test_reference_rounds_the_overflow_edge_as_the_issue_states():
    got = O.bf16_bits(np.array([3.3961776e38, 3.38e38], dtype=np.float32))
    assert got[0] == 0x7F80 and got[1] == 0x7F7E


@pytest.mark.parametrize("shift", [0, 4], ids=["c16", "c8"])
@pytest.mark.parametrize("with_acc", [False, True], ids=["plain", "acc"])
@pytest.mark.parametrize("n", LENGTHS)
def test_compress_bit_exact(dtc, cuda, n, with_acc, shift):
    rng = np.random.default_rng(7 * n % 1009 + 2 * with_acc + shift)
    g = _values(rng, n)
    ga, dg = _f32_arena(g, cuda)
    acc = da = aa = None
    if with_acc:
        acc = _values(rng, n)[::-1].copy()  # specials meet normals and each other
        aa, da = _f32_arena(acc, cuda)
    ca, cview, dc = _c_arena(n, cuda, shift)
    dtc.ops.grad_compress_bf16(dg, dc, acc=da)
    torch.cuda.synchronize()
    with np.errstate(over="ignore", invalid="ignore"):
        src = (g + acc).astype(np.float32) if with_acc else g
    want, got = O.bf16_bits(src), _u16(dc)
    nan = np.isnan(src)
    assert nan.any() or n < 16
    assert np.array_equal(got[~nan], want[~nan])
    assert ((got[nan] & 0x7F80) == 0x7F80).all() and ((got[nan] & 0x007F) != 0).all()  # a NaN stays a NaN
    if not with_acc and n >= 64:
        assert got[0] == 0x7F80 and got[1] == 0x7F7E and got[2] == 0xFF80 and got[3] == 0xFF7E
    _assert_c_surroundings(ca, cview, shift, n)
    # the operands bit-unchanged, their guard bands intact
    assert np.array_equal(_u32(dg), g.view(np.uint32)) and ga.dirty() == 0
    if with_acc:
        assert np.array_equal(_u32(da), acc.view(np.uint32)) and aa.dirty() == 0


@pytest.mark.parametrize("shift", [0, 4], ids=["c16", "c8"])
@pytest.mark.parametrize("n", LENGTHS)
def test_decompress_bit_exact(dtc, cuda, n, shift):
    rng = np.random.default_rng(11 * n % 1013 + shift)
    words = rng.integers(0, 1 << 16, n, dtype=np.uint16)  # every pattern: NaN payloads, inf, -0, subnormals
    k = min(8, n)
    words[n - k:] = np.array([0x7FC1, 0xFF81, 0x7F80, 0xFF80, 0x8000, 0x0001, 0x807F, 0x0000], dtype=np.uint16)[8 - k:]
    ca, cview, dc = _c_arena(n, cuda, shift)
    dc.view(torch.int16).copy_(torch.from_numpy(words.view(np.int16).copy()).to(cuda))
    ga, dg = bounds.arena((n,), torch.float32, cuda)
    dtc.ops.grad_decompress_bf16(dc, dg)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(dg), words.astype(np.uint32) << 16)  # payloads included
    assert ga.dirty() == 0
    assert np.array_equal(_u16(dc), words)
    _assert_c_surroundings(ca, cview, shift, n)


def test_fused_compress_equals_finish_then_compress(dtc, cuda):
    n = TRIP + 12
    rng = np.random.default_rng(3)
    g = torch.from_numpy(_values(rng, n)).to(cuda)
    acc = torch.from_numpy(_values(rng, n)[::-1].copy()).to(cuda)
    fused = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    dtc.ops.grad_compress_bf16(g, fused, acc=acc)
    summed = g.clone()
    dtc.ops.grad_accum_flat(acc.clone(), summed, dtc.ops.ACCUM_FINISH)
    two = torch.zeros(n, dtype=torch.bfloat16, device=cuda)
    dtc.ops.grad_compress_bf16(summed, two)
    a, b = _u16(fused), _u16(two)
    nan = np.isnan(O.from_bf16_bits(b))
    assert np.array_equal(a[~nan], b[~nan]) and np.isnan(O.from_bf16_bits(a[nan])).all()


def test_overflow_to_inf_reaches_the_finiteness_check(dtc, cuda):
    """AMP: a finite fp32 gradient at the bf16 overflow threshold is inf after the compressed all-reduce; the
    decompress brings that inf into the fp32 gradients, where dtc_amp_check_finite (GradScaler) sees it."""
    g = torch.full((4096,), 0.5, device=cuda)
    g[1234] = 3.3961776e38
    found = torch.zeros(1, dtype=torch.int32, device=cuda)
    dtc.ops.amp_check_finite(g, found)
    assert int(found.item()) == 0
    c = torch.zeros(4096, dtype=torch.bfloat16, device=cuda)
    dtc.ops.grad_compress_bf16(g, c)
    dtc.ops.grad_decompress_bf16(c, g)
    dtc.ops.amp_check_finite(g, found)
    assert int(found.item()) == 1 and float(g[1234]) == float("inf") and float(g[0]) == 0.5


# ----------------------------------------------------------------------------- transports
def _bf16_words(rng, n):
    """bf16 words of normals over +-15 decades, with values that overflow when doubled or summed, inf and zeros"""
    v = (10.0 ** rng.uniform(-15.0, 15.0, n)).astype(np.float32)
    v = np.where(rng.random(n) < 0.5, -v, v).astype(np.float32)
    v[:6] = np.array([3.0e38, -2.0e38, np.inf, 0.0, -0.0, 1.17e-38], dtype=np.float32)
    return O.bf16_bits(v)


def _words_to_dev(words, cuda):
    return torch.from_numpy(words.view(np.int16).copy()).to(cuda).view(torch.bfloat16)


@pytest.mark.parametrize("factor", [2.0, 3.0])
def test_loopback_allreduce_bf16(dtc, cuda, factor):
    n = 4100
    words = _bf16_words(np.random.default_rng(int(factor)), n)
    t = _words_to_dev(words, cuda)
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, factor, world=2)
    try:
        comm.allreduce_sum_(t)
        torch.cuda.synchronize()
        with np.errstate(over="ignore"):
            want = O.bf16_bits(O.from_bf16_bits(words) * np.float32(factor))
        assert np.array_equal(_u16(t), want)
        assert comm.log() == [(t.data_ptr(), n, False)]
    finally:
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


def _rank_ordered_sum(words):
    """bf16 words of ((widen(c_0) + widen(c_1)) + ...) + widen(c_{W-1}): fp32 adds in rank order, rounded once"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = O.from_bf16_bits(words[0])
        for w in words[1:]:
            s = (s + O.from_bf16_bits(w)).astype(np.float32)
    return O.bf16_bits(s), np.isnan(s)


def test_thread_group_allreduce_bf16_three_ranks(dtc, cuda):
    world, n = 3, 4100
    words = [_bf16_words(np.random.default_rng(40 + r), n) for r in range(world)]
    words[1][2] = 0xFF80  # inf + -inf: a NaN on every rank
    want, nan = _rank_ordered_sum(words)
    assert nan.sum() == 1
    comms = dtc.parallel.Comm.thread_group(cuda.index or 0, world)
    torch.cuda.synchronize()

    def rank(r):
        t = _words_to_dev(words[r], cuda)
        comms[r].allreduce_sum_(t)
        torch.cuda.current_stream().synchronize()
        return _u16(t)

    for r, got in enumerate(_run_ranks(rank, world)):
        assert np.array_equal(got[~nan], want[~nan]), r
        assert np.isnan(O.from_bf16_bits(got[nan])).all(), r


# ----------------------------------------------------------------------------- executor
def _model(dtc, cuda, cap_mb=1.0):
    torch.manual_seed(42)
    m = dtc.ResNet18().to(cuda)
    m.set_bucket_cap_mb(cap_mb)
    return m


def _batches(cuda, n, batch=8, seed=23):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(batch, 3, 32, 32, generator=g).to(cuda) for _ in range(n)]
    ys = [torch.randint(0, 100, (batch,), generator=g).to(cuda) for _ in range(n)]
    return xs, ys


def _backward(dtc, model, x, y):
    dtc.CrossEntropyLoss()(model(x), y).backward()
    torch.cuda.synchronize()
    return _u32(model.flat.grads).view(np.float32).copy()


def _round_trip(g, factor=None):
    """widen(bf16(g)), or widen(bf16(widen(bf16(g)) * factor)) (the loopback collective between the two)"""
    r = O.from_bf16_bits(O.bf16_bits(g))
    if factor is not None:
        r = O.from_bf16_bits(O.bf16_bits(r * np.float32(factor)))
    return r


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _bucket_log(comm, base, itemsize):
    return [((a - base) // itemsize, n) for a, n, is_bucket in comm.log() if is_bucket]


@pytest.mark.parametrize("on_side", [0, 1])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_executor_loopback_two_ranks(dtc, cuda, precision, on_side):
    lib = dtc._native.lib
    prev = lib.dtc_get_option(b"comm_on_side")
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 2.0, world=2)
    try:
        lib.dtc_set_option(b"comm_on_side", on_side)
        model = _model(dtc, cuda)
        model.precision = precision
        buckets = model.buckets()
        assert len(buckets) == 7
        (x,), (y,) = _batches(cuda, 1)
        g_plain = _backward(dtc, model, x, y)
        assert np.isfinite(g_plain).all() and np.count_nonzero(g_plain) > g_plain.size // 2
        flat = model.flat
        # compressed: every bucket staged, reduced in the staging tensor and widened back
        model._comm, model.grad_compression = comm, "bf16"
        comm.clear_log()
        got = _backward(dtc, model, x, y)
        want = _round_trip(g_plain, 2.0)
        assert not _same_bits(want, g_plain * np.float32(2.0))
        assert _same_bits(got, want)
        assert _bucket_log(comm, flat.grad_c16.data_ptr(), 2) == buckets  # each bucket once, inside the staging tensor
        assert np.array_equal(_u16(flat.grad_c16), O.bf16_bits(want))
        # back to OFF: the fp32 loopback on the gradients themselves
        model.grad_compression = None
        comm.clear_log()
        got = _backward(dtc, model, x, y)
        assert _same_bits(got, g_plain * np.float32(2.0))
        assert _bucket_log(comm, flat.grads.data_ptr(), 4) == buckets
        # BF16 without a communicator: nothing compressed, the staging tensor untouched
        model._comm, model.grad_compression = None, "bf16"
        flat.grad_c16.view(torch.int16).fill_(0x7FD5)
        got = _backward(dtc, model, x, y)
        assert _same_bits(got, g_plain)
        assert (_u16(flat.grad_c16) == 0x7FD5).all()
    finally:
        lib.dtc_set_option(b"comm_on_side", prev)
        comm.close()


def test_with_accumulation_fused_finish(dtc, cuda):
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 2.0, world=2)
    try:
        model = _model(dtc, cuda)
        model.grad_accum_steps = 3
        xs, ys = _batches(cuda, 3, seed=29)
        with dtc.autocast():
            g1, g2, g3 = (_backward(dtc, model, xs[i], ys[i]) for i in range(3))
            model._comm, model.grad_compression = comm, "bf16"
            comm.clear_log()
            with model.accumulate():
                _backward(dtc, model, xs[0], ys[0])
                _backward(dtc, model, xs[1], ys[1])
            assert comm.log() == []
            acc_before = _u32(model.flat.grad_acc).copy()
            got = _backward(dtc, model, xs[2], ys[2])
        total = (g3 + (g1 + g2).astype(np.float32)).astype(np.float32)
        assert _same_bits(acc_before.view(np.float32), (g1 + g2).astype(np.float32))
        assert _same_bits(got, _round_trip(total, 2.0))
        assert not _same_bits(got, _round_trip(g3, 2.0))
        assert np.array_equal(_u32(model.flat.grad_acc), acc_before)  # the closing step reads the sum only
        assert _bucket_log(comm, model.flat.grad_c16.data_ptr(), 2) == model.buckets()
    finally:
        comm.close()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_with_distinct_data_through_ddp_hook(dtc, cuda, world):
    cap_mb, steps = 1.0, 2
    xs, ys = _batches(cuda, world, seed=31 + world)
    # rank r's own gradient with DDP's pre-scale 1 / W, without a communicator
    ref = _model(dtc, cuda, cap_mb)
    ref._grad_scale = 1.0 / world
    local = []
    for r in range(world):
        with dtc.autocast():
            local.append(_backward(dtc, ref, xs[r], ys[r]))
    want_words, nan = _rank_ordered_sum([O.bf16_bits(g) for g in local])
    assert not nan.any()
    want = O.from_bf16_bits(want_words)
    # derived, not measured: one rounding of each operand costs 2^-8 |g_r|, one rounding of the sum
    # 2^-8 |sum bf16(g_r)|, the fp32 adds are absorbed by the 1.01; for every element
    exact = np.sum([g.astype(np.float64) for g in local], axis=0)
    bound = 1.01 * 2.0 ** -7 * np.sum([np.abs(g.astype(np.float64)) for g in local], axis=0)

    comms = dtc.parallel.Comm.thread_group(cuda.index or 0, world)
    models = [_model(dtc, cuda, cap_mb) for _ in range(world)]
    n_buckets = len(models[0].buckets())

    def rank(r):
        m = models[r]
        ddp = dtc.DistributedDataParallel(m, device_ids=[0], bucket_cap_mb=cap_mb, comm=comms[r])
        ddp.register_comm_hook(None, dtc.parallel.bf16_compress_hook)
        assert m.grad_compression == "bf16"
        comms[r].clear_log()
        crit = dtc.CrossEntropyLoss()
        grads = []
        for _ in range(steps):
            with dtc.autocast():
                loss = crit(ddp(xs[r]), ys[r])
            dtc._native.call("dtc_barrier", comms[r].handle, dtc._native.stream_ptr())  # the per-step barrier
            loss.backward()
            torch.cuda.current_stream().synchronize()
            grads.append(_u32(m.flat.grads).view(np.float32).copy())
        return grads, _bucket_log(comms[r], m.flat.grad_c16.data_ptr(), 2)

    res = _run_ranks(rank, world)
    for r in range(world):
        grads, log = res[r]
        for got in grads:
            assert _same_bits(got, want), r  # hence all ranks identical
            worst = bounds.assert_within(got, exact, bound, f"rank {r} of {world}")
        assert log == models[r].buckets() * steps, (r, len(log), n_buckets)
    print(f"W = {world}: worst |got - sum| / bound {worst:.4f}")


def test_real_rccl_one_rank(dtc, cuda):
    """The identity all-reduce of a one-rank RCCL communicator: ncclBfloat16 on the collective's stream with the
    decompress behind it."""
    comm = dtc.parallel.Comm(0, 1, dtc.parallel.Comm.unique_id(), cuda.index or 0)
    try:
        model = _model(dtc, cuda)
        (x,), (y,) = _batches(cuda, 1, seed=37)
        with dtc.autocast():
            g_plain = _backward(dtc, model, x, y)
            model._comm, model.grad_compression = comm, "bf16"
            got = _backward(dtc, model, x, y)
        assert _same_bits(got, _round_trip(g_plain))
        assert not _same_bits(got, g_plain)
        model._comm = None
    finally:
        comm.close()


def test_graph_modes_plain_compressed_plain(dtc, cuda):
    lib = dtc._native.lib
    (x,), (y,) = _batches(cuda, 1, seed=41)

    def run(model, compression):
        model.grad_compression = compression
        with dtc.autocast():
            return _backward(dtc, model, x, y)

    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 2.0, world=2)
    prev = lib.dtc_get_option(b"graphs")
    try:
        eager = _model(dtc, cuda)
        eager._comm = comm
        eager_compressed = run(eager, "bf16")
        lib.dtc_set_option(b"graphs", 1)
        model = _model(dtc, cuda)
        model._comm = comm
        plain_a = run(model, None)
        compressed = run(model, "bf16")
        plain_b = run(model, None)
        assert _same_bits(plain_a, plain_b)
        assert _same_bits(compressed, eager_compressed)
        assert not _same_bits(compressed, plain_a)
    finally:
        lib.dtc_set_option(b"graphs", prev)
        comm.close()


def test_data_parallel_refuses_compression(dtc, cuda):
    model = _model(dtc, cuda)
    dp = dtc.DataParallel(model, device_ids=[cuda.index or 0, cuda.index or 0])
    x = torch.randn(8, 3, 32, 32, device=cuda)
    model.grad_compression = "bf16"
    with pytest.raises(dtc.NativeError, match="gradient compression"):
        dp(x)
    model.grad_compression = None
    out = dp(x)  # the plain path still runs
    model.grad_compression = "bf16"  # set between the forward and the backward
    with pytest.raises(dtc.NativeError, match="gradient compression"):
        out.sum().backward()
