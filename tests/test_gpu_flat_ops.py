"""The flat-buffer kernels around the optimizer (csrc/optim.hip) beyond one size and one set of scalars.

* dtc_sgd_nesterov_flat: three consecutive steps at n = 4 (one vector), 1028 and 2,097,156 = 2048 * 256 * 4 + 4 (one
  vector in the second grid-stride trip), each step against float64 arithmetic on the kernel's own previous p and
  m within tests/bounds.py's sgd_tol, the bf16 shadow bit-equal to the round-to-nearest-even of the kernel's own p,
  with and without the GradScaler inputs, the skipped step, the launcher's alignment / size refusals, and
  p, m and the shadow inside guard-band arenas.
* The shadow's rounding on exact ties, through SGD with lr = wd = g = 0 (p is then bit-unchanged).
* dtc_cast_f32_bf16 bit for bit against oracle.ops.bf16_bits on ties, infinities, subnormals and random data, at
  n = 1, 7 and 524,289 = 2048 * 256 + 1, aligned and on views offset by one element.
* dtc_amp_scale bit-equal to the numpy float32 product, overflow to inf included.
* dtc_amp_update_scale over a 40-step clean / overflow sequence against torch._amp_update_scale_.
"""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import bounds as B

pytestmark = pytest.mark.gpu

EINVAL = r"code -1\)"
# exact ties with an even / odd upper half, both signs; one ulp either side of each tie; +-0; the smallest normal;
# the largest finite value (rounds to inf)
TIES = [0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,
        0xBF807FFF, 0xBF808001, 0xBF817FFF, 0xBF818001, 0x00000000, 0x80000000, 0x00800000, 0x7F7FFFFF]
INFS = [0x7F800000, 0xFF800000]
SUBNORMALS = [0x00000001, 0x00008000, 0x007FFFFF, 0x80000001, 0x80008000, 0x807FFFFF]
NANS = [0x7FC00000, 0x7F800001, 0xFFC12345]


def _f32(words):
    return np.array(words, np.uint32).view(np.float32)


def _bits16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _bits32(t):
    return t.view(torch.int32).cpu().numpy().view(np.uint32)


class _Sgd:
    """p, m and the shadow in arenas; g a plain tensor."""

    def __init__(self, dtc, dev, p0):
        n = p0.shape[0]
        self.ops, self.dev = dtc.ops, dev
        self.ap, self.p = B.arena((n,), torch.float32, dev, like=torch.from_numpy(p0).to(dev))
        self.am, self.m = B.arena((n,), torch.float32, dev, zero=True)
        self.apb, self.pb = B.arena((n,), torch.bfloat16, dev)

    def step(self, g, lr, wd, mu, inv=None, found=None):
        self.ops.sgd_nesterov_flat(self.p, torch.from_numpy(g).to(self.dev), self.m, self.pb, lr, wd, mu, inv, found)

    def host(self):
        return self.p.cpu().numpy(), self.m.cpu().numpy(), _bits16(self.pb)

    def guards_intact(self):
        torch.cuda.synchronize()
        return self.ap.dirty() == 0 and self.am.dirty() == 0 and self.apb.dirty() == 0


@pytest.mark.parametrize("amp", [False, True], ids=["plain", "gradscaler"])
@pytest.mark.parametrize("n", [4, 1028, 2_097_156])
def test_sgd_nesterov_flat_three_steps_within_bound(dtc, cuda, n, amp):
    worst = [0.0, 0.0]
    for (wd, mu) in ((0.0, 0.0), (5e-4, 0.9)):
        for lr in (0.1, 3.2):
            g_ = np.random.default_rng(n % 1000 + int(lr * 10) + int(mu * 100))
            s = _Sgd(dtc, cuda, g_.standard_normal(n).astype(np.float32))
            is_ = 1.0 / 65536 if amp else 1.0
            inv = torch.full((1,), is_, device=cuda) if amp else None
            found = torch.zeros(1, dtype=torch.int32, device=cuda) if amp else None
            p, m, _ = s.host()
            for step in range(3):
                g = g_.standard_normal(n).astype(np.float32) * np.float32(65536.0 if amp else 1.0)
                s.step(g, lr, wd, mu, inv, found)
                p2, m2, pb2 = s.host()
                (p_ref, m_ref), (tp, tm) = B.sgd_ref(p, g, m, lr, wd, mu, is_), B.sgd_tol(p, g, m, lr, wd, mu, is_)
                what = f"sgd n={n} amp={amp} wd={wd} mu={mu} lr={lr} step {step}"
                worst[0] = max(worst[0], B.assert_within(p2, p_ref, tp, what + " p"))
                worst[1] = max(worst[1], B.assert_within(m2, m_ref, tm, what + " m"))
                np.testing.assert_array_equal(pb2, O.bf16_bits(p2), err_msg=what + " shadow")
                assert np.any(p2 != p)
                p, m = p2, m2
            if amp:  # an overflow step is skipped whole
                found.fill_(1)
                s.step(g, lr, wd, mu, inv, found)
                for was, now in zip((p, m), s.host()[:2]):
                    np.testing.assert_array_equal(was.view(np.uint32), now.view(np.uint32))
                np.testing.assert_array_equal(s.host()[2], pb2)
                assert int(found.item()) == 1
            assert s.guards_intact(), "guard words overwritten"
    print(f"sgd_nesterov_flat n={n} amp={amp}: worst |err|/tol p {worst[0]:.3f}, m {worst[1]:.3f}")


def test_sgd_nesterov_flat_refuses_misaligned_and_odd_sizes(dtc, cuda):
    """p, g, momentum 16-byte and p_bf16 8-byte aligned, n a positive multiple of 4: anything else is refused
    before any launch."""
    n = 8
    g_ = np.random.default_rng(3)
    base = [torch.from_numpy(g_.standard_normal(n + 4).astype(np.float32)).to(cuda) for _ in range(3)]
    base.append(torch.from_numpy(g_.standard_normal(n + 4).astype(np.float32)).to(cuda).bfloat16())
    before = [t.clone() for t in base]
    P, call = dtc._native.ptr, dtc._native.call

    def run(views, count):
        call("dtc_sgd_nesterov_flat", P(views[0]), P(views[1]), P(views[2]), P(views[3]), count, 0.1, 1e-4, 0.9, None,
             None, dtc._native.stream_ptr())

    for bad in range(4):
        views = [t[1:n + 1] if i == bad else t[:n] for i, t in enumerate(base)]
        assert views[bad].data_ptr() % (8 if bad == 3 else 16) != 0
        with pytest.raises(dtc._native.NativeError, match=EINVAL):
            run(views, n)
    for count in (6, 0):
        with pytest.raises(dtc._native.NativeError, match=EINVAL):
            run([t[:n] for t in base], count)
    torch.cuda.synchronize()
    for was, now in zip(before, base):
        assert torch.equal(was.view(torch.int16), now.view(torch.int16))
    run([t[:n] for t in base], n)  # the aligned call is accepted
    torch.cuda.synchronize()
    assert not torch.equal(before[0], base[0])


def test_sgd_shadow_rounds_ties_to_even(dtc, cuda):
    """lr = 0, wd = 0, g = 0: p is bit-unchanged and the shadow is the round-to-nearest-even of p, on exact ties
    (finite values only: an infinite p makes p * wd NaN)."""
    p0 = _f32(TIES)
    assert p0.shape[0] % 4 == 0 and np.isfinite(p0).all()
    s = _Sgd(dtc, cuda, p0)
    s.step(np.zeros_like(p0), 0.0, 0.0, 0.9)
    p, m, pb = s.host()
    np.testing.assert_array_equal(p.view(np.uint32), p0.view(np.uint32))
    assert not m.any()
    np.testing.assert_array_equal(pb, O.bf16_bits(p0))
    assert pb[0] == 0x3F80 and pb[1] == 0x3F82 and pb[-1] == 0x7F80  # even stays, odd goes up, the largest to inf
    assert s.guards_intact()


def _cast_data(n, seed):
    special = np.concatenate([_f32(TIES), _f32(INFS), _f32(SUBNORMALS), _f32(NANS)])
    if n <= special.shape[0]:
        last = special.shape[0] - n
        return [special[i:i + n] for i in list(range(0, last, n)) + [last]]
    g = np.random.default_rng(seed)
    r = g.standard_normal(n - special.shape[0]).astype(np.float32)
    r *= np.float32(10.0) ** g.integers(-30, 30, r.shape[0]).astype(np.float32)
    return [np.concatenate([r[:1000], special, r[1000:]])[::-1].copy()]  # the specials sit in the last trip too


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("n", [1, 7, 524_289])
def test_cast_f32_bf16_bit_exact(dtc, cuda, n, offset):
    """Every finite and infinite value converts to O.bf16_bits (round to nearest even; torch.Tensor.bfloat16()'s
    conversion), subnormals included; a NaN stays a NaN; nothing is written outside the destination."""
    for src in _cast_data(n, 17):
        assert src.shape[0] == n
        sd = torch.from_numpy(np.concatenate([np.zeros(offset, np.float32), src])).to(cuda)[offset:]
        a, dst_all = B.arena((n + offset,), torch.bfloat16, cuda)
        dst = dst_all[offset:]
        assert sd.data_ptr() % 8 == 4 * offset and dst.data_ptr() % 4 == 2 * offset
        dtc.ops.cast_f32_bf16(sd, dst)
        torch.cuda.synchronize()
        got, want = _bits16(dst), O.bf16_bits(src)
        nan = np.isnan(src)
        np.testing.assert_array_equal(got[~nan], want[~nan])
        assert np.all((got[nan] & 0x7F80) == 0x7F80) and np.all((got[nan] & 0x007F) != 0), "a NaN must stay a NaN"
        np.testing.assert_array_equal(got[~nan], _bits16(sd.bfloat16())[~nan])  # and torch's own conversion
        assert a.dirty() == 0
        if offset:
            assert int(_bits16(dst_all)[0]) == 0x7FD5  # the element before the view keeps the arena's pattern


@pytest.mark.parametrize("n", [1, 7, 262_145])
def test_amp_scale_bit_equal_to_fp32_product(dtc, cuda, n):
    g = np.random.default_rng(n)
    with np.errstate(over="ignore"):  # a few inputs are themselves inf
        x = g.standard_normal(n).astype(np.float32) * np.float32(10.0) ** g.integers(-38, 39, n).astype(np.float32)
    x[0] = np.float32(3e38)
    xd = torch.from_numpy(x).to(cuda)
    scale = torch.full((1,), 65536.0, device=cuda)
    for s in (65536.0, 3.0):
        scale.fill_(s)  # the kernel reads the device word
        out = dtc.ops.amp_scale(xd, scale)
        with np.errstate(over="ignore"):
            want = x * np.float32(s)
        np.testing.assert_array_equal(_bits32(out), want.view(np.uint32))
        assert np.isinf(want[0])
        if n > 7:
            assert np.isinf(want).sum() > 1 and np.isfinite(want).sum() > n // 2


def test_amp_update_scale_sequence_matches_torch(dtc, cuda):
    growth, backoff, interval = 2.0, 0.5, 3
    overflow = np.random.default_rng(40).random(40) < 0.3
    assert 5 < overflow.sum() < 20
    scale = torch.full((1,), 65536.0, device=cuda)
    inv = torch.zeros(1, device=cuda)
    tracker = torch.zeros(1, dtype=torch.int32, device=cuda)
    found = torch.zeros(1, dtype=torch.int32, device=cuda)
    t_scale, t_tracker = scale.clone(), tracker.clone()
    seen = set()
    for step, ov in enumerate(overflow):
        found.fill_(int(ov))
        dtc.ops.amp_update_scale(scale, inv, tracker, found, growth, backoff, interval)
        torch._amp_update_scale_(t_scale, t_tracker, torch.full((1,), float(ov), device=cuda), growth, backoff, interval)
        s, tr = float(scale), int(tracker)
        assert s == float(t_scale) and tr == int(t_tracker), (step, s, float(t_scale), tr, int(t_tracker))
        assert np.float32(float(inv)) == np.float32(1) / np.float32(s) and int(found) == 0, step
        seen.add(tr)
    assert seen == {0, 1, 2} and float(scale) != 65536.0
    # no growth to inf: the scale stays, the tracker restarts; inv_scale = NULL is accepted
    scale.fill_(2.0 ** 127)
    tracker.zero_()
    dtc.ops.amp_update_scale(scale, None, tracker, found, growth, backoff, 1)
    assert float(scale) == 2.0 ** 127 and int(tracker) == 0
    dtc.ops.amp_update_scale(scale, None, tracker, found, growth, backoff, 2)
    assert float(scale) == 2.0 ** 127 and int(tracker) == 1
    found.fill_(1)
    dtc.ops.amp_update_scale(scale, None, tracker, found, growth, backoff, 2)
    assert float(scale) == 2.0 ** 126 and int(tracker) == 0 and int(found) == 0
