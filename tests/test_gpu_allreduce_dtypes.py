"""The loopback and thread-group all-reduce in all four dtypes at the sizes where their grid-stride kernels branch:
one element, one workgroup plus one element, and 2048 * 256 + 1 elements, where the capped grid (2048 workgroups of
256 threads) wraps and one thread takes a second trip. Bit-exact against numpy: the loopback is one fp32 multiply
(bf16: widened, multiplied, rounded to nearest even once; int64 and fp64 in their own arithmetic), the thread group
adds the ranks' buffers in rank order (bf16: fp32 adds of the widened words, rounded once). The words behind the
reduced range must stay as they were.
"""
import threading

import numpy as np
import pytest
import torch

from oracle import ops as O

pytestmark = pytest.mark.gpu

SIZES = [1, 257, 2048 * 256 + 1]
DTYPES = ["f32", "bf16", "i64", "f64"]
GUARD = 64  # elements behind the range that no kernel may touch


def _host(rng, n, dtype):
    """n + GUARD finite values that neither overflow when tripled nor when three of them are summed; bf16 as words"""
    m = n + GUARD
    if dtype == "i64":
        return rng.integers(-(1 << 60), 1 << 60, m, dtype=np.int64)
    v = 10.0 ** rng.uniform(-15.0, 15.0, m) * np.where(rng.random(m) < 0.5, -1.0, 1.0)
    if dtype == "f64":
        return v
    v = v.astype(np.float32)
    return O.bf16_bits(v) if dtype == "bf16" else v


def _to_dev(a, cuda):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).to(cuda).view(torch.bfloat16)
    return torch.from_numpy(a.copy()).to(cuda)


def _to_host(t):
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _tripled(a):
    if a.dtype == np.uint16:
        return O.bf16_bits(O.from_bf16_bits(a) * np.float32(3.0))
    return a * a.dtype.type(3)


def _rank_ordered_sum(parts):
    if parts[0].dtype == np.uint16:
        s = O.from_bf16_bits(parts[0])
        for p in parts[1:]:
            s = (s + O.from_bf16_bits(p)).astype(np.float32)
        return O.bf16_bits(s)
    s = parts[0].copy()
    for p in parts[1:]:
        s = s + p
    return s


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_loopback_allreduce_factor_three(dtc, cuda, dtype, n):
    a = _host(np.random.default_rng(n % 1000 + DTYPES.index(dtype)), n, dtype)
    full = _to_dev(a, cuda)
    comm = dtc.parallel.Comm.loopback(cuda.index or 0, 3.0, world=2)
    try:
        comm.allreduce_sum_(full[:n])
        torch.cuda.synchronize()
    finally:
        comm.close()
    got = _to_host(full)
    assert np.array_equal(_bits(got[:n]), _bits(_tripled(a[:n])))
    assert np.array_equal(_bits(got[n:]), _bits(a[n:]))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_thread_group_allreduce_three_ranks(dtc, cuda, dtype, n):
    world = 3
    parts = [_host(np.random.default_rng(100 * r + n % 1000 + DTYPES.index(dtype)), n, dtype) for r in range(world)]
    want = _rank_ordered_sum([p[:n] for p in parts])
    comms = dtc.parallel.Comm.thread_group(cuda.index or 0, world)
    torch.cuda.synchronize()
    out, errs = [None] * world, [None] * world
    streams = [torch.cuda.Stream() for _ in range(world)]

    def body(r):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(streams[r]):
                full = _to_dev(parts[r], cuda)
                comms[r].allreduce_sum_(full[:n])
                torch.cuda.current_stream().synchronize()
                out[r] = _to_host(full)
        except BaseException as e:  # noqa: BLE001 - re-raised below
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
    for r in range(world):
        assert np.array_equal(_bits(out[r][:n]), _bits(want)), r
        assert np.array_equal(_bits(out[r][n:]), _bits(parts[r][n:])), r
