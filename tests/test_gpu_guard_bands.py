"""Guard bands ("moats") around every tensor of the tiled conv / stem kernels.

Several kernels launch tiles that extend past the tensor (conv_halo's last tile, wgrad_halo's zero-fill DMA rows,
the general geometries' padded slots), and the caching allocator places tensors back to back: a store one row
past an output, or a load past an input that reaches an accumulator, would corrupt or borrow a neighbour's memory
without any other test noticing. Here each op runs once plainly and once with EVERY operand, output, statistics
accumulator and workspace embedded in an arena of its own (tests/bounds.py: a quiet-NaN bit pattern with at least
1 MiB of it on each side of the tensor, the workspace exactly the bytes the size query returns), under the same
options and therefore the same plan:

* the outputs are bit-identical between the two runs and hold no NaN (a moat value that reached an accumulator
  shows as NaN),
* the BN statistics totals are exactly equal,
* every guard word of every arena, the inputs' included, is bit-unchanged (a stray store shows there).

The shapes and forced options are those of the existing tests of each kernel (tests/test_gpu_ops.py); the head
cases (pool + Linear, cross-entropy backward into an embedded dlogits, the head backward through both of its paths)
are two of tests/test_gpu_head.py's: ragged image splits and class tiles, C below one 256-channel strip.
"""
import numpy as np
import pytest
import torch

from oracle import ops as O
from tests.bounds import arena

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


def _rand_bf16(shape, gen, scale=1.0):
    return O.bf16(gen.standard_normal(shape).astype(np.float32) * scale)


class _Plain:
    """Today's allocation: operands as ordinary device tensors, outputs / workspaces left to the wrappers."""

    def __init__(self, dtc, dev):
        self.dtc, self.dev = dtc, dev

    def inp(self, a, dtype=BF):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev).to(dtype)

    def out(self, shape, dtype=BF):
        return None

    def stats(self, c):
        return self.dtc.ops.new_stats(c, self.dev)

    def ws(self, nbytes):
        return None

    def check(self):
        pass


class _Moat(_Plain):
    def __init__(self, dtc, dev):
        super().__init__(dtc, dev)
        self.arenas = []

    def _new(self, *a, **k):
        ar, view = arena(*a, **k)
        self.arenas.append(ar)
        return view

    def inp(self, a, dtype=BF):
        t = super().inp(a, dtype)
        return self._new(t.shape, dtype, self.dev, like=t)

    def out(self, shape, dtype=BF):
        return self._new(shape, dtype, self.dev)

    def stats(self, c):
        return self._new((int(self.dtc._native.lib.dtc_bn_stat_words(c)),), torch.int64, self.dev, zero=True)

    def ws(self, nbytes):
        if nbytes == 0:
            return None
        assert nbytes % 4 == 0
        return self._new((nbytes // 4,), F32, self.dev)

    def check(self):
        torch.cuda.synchronize()
        dirty = {i: a.dirty() for i, a in enumerate(self.arenas)}
        assert not any(dirty.values()), f"guard words overwritten (arena index: count): " \
                                        f"{ {i: n for i, n in dirty.items() if n} }"


# Each op(dtc, a) allocates through `a` (_Plain or _Moat) and returns (outputs, [(statistics, channels)]).
def _fwd(x, w, st, pad):
    def op(dtc, a):
        N, H, W, C = x.shape
        K, R = w.shape[:2]
        d = dtc.ops.conv_desc(N, H, W, C, K, R, R, st, pad)
        P, Q = dtc.ops.conv_out_hw(H, W, R, R, st, pad)
        s = a.stats(K)
        y = dtc.ops.conv2d_fwd(a.inp(x), a.inp(w), st, pad, stats=s, out=a.out((N, P, Q, K)),
                               workspace=a.ws(dtc._native.lib.dtc_conv2d_workspace_size(d, 0)))
        return [y], [(s, K)]
    return op


def _dgrad(dy, w, hw, st, pad, res):
    def op(dtc, a):
        N = dy.shape[0]
        K, R, _, C = w.shape
        d = dtc.ops.conv_desc(N, hw[0], hw[1], C, K, R, R, st, pad)
        dx = dtc.ops.conv2d_dgrad(a.inp(dy), a.inp(w), hw, st, pad, res=None if res is None else a.inp(res),
                                  out=a.out((N, hw[0], hw[1], C)),
                                  workspace=a.ws(dtc._native.lib.dtc_conv2d_workspace_size(d, 1)))
        return [dx], []
    return op


def _wgrad(x, dy, R, st, pad):
    def op(dtc, a):
        N, H, W, C = x.shape
        K = dy.shape[3]
        d = dtc.ops.conv_desc(N, H, W, C, K, R, R, st, pad)
        dw = dtc.ops.conv2d_wgrad(a.inp(x), a.inp(dy), R, R, st, pad, scale=0.5, out=a.out((K, R, R, C), F32),
                                  workspace=a.ws(dtc._native.lib.dtc_conv2d_workspace_size(d, 2)))
        return [dw], []
    return op


def _fwd_sc(x, w, wsc):
    def op(dtc, a):
        N, H, W, C = x.shape
        K = w.shape[0]
        s1, s2 = a.stats(K), a.stats(K)
        y, ysc = dtc.ops.conv2d_fwd_sc(a.inp(x), a.inp(w), a.inp(wsc.reshape(K, C)), stats=s1, stats_sc=s2,
                                       out=(a.out((N, H // 2, W // 2, K)), a.out((N, H // 2, W // 2, K)))
                                       if isinstance(a, _Moat) else None)
        return [y, ysc], [(s1, K), (s2, K)]
    return op


def _dgrad_sc(dy, w, dsc, wsc, hw):
    def op(dtc, a):
        N = dy.shape[0]
        K, _, _, C = w.shape
        dx = dtc.ops.conv2d_dgrad_sc(a.inp(dy), a.inp(w), a.inp(dsc), a.inp(wsc.reshape(K, C)), hw,
                                     out=a.out((N, hw[0], hw[1], C)))
        return [dx], []
    return op


def _wgrad_sc(x, dy, dsc):
    def op(dtc, a):
        N, H, W, C = x.shape
        K = dy.shape[3]
        nb = dtc._native.lib.dtc_conv2d_wgrad_sc_workspace_size(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 2, 1))
        assert nb > 0  # the fused plan exists for this geometry (test_conv_wgrad_stride2_halo_and_shortcut)
        dw, dwsc = dtc.ops.conv2d_wgrad_sc(a.inp(x), a.inp(dy), a.inp(dsc), scale=0.5, workspace=a.ws(nb),
                                           out=(a.out((K, 3, 3, C), F32), a.out((K, C), F32))
                                           if isinstance(a, _Moat) else None)
        return [dw, dwsc], []
    return op


def _wgrad_batch(xs, dys):
    def op(dtc, a):
        n = len(xs)
        N, H, W, C = xs[0].shape
        K = dys[0].shape[3]
        nb = dtc._native.lib.dtc_conv2d_wgrad_batch_workspace_size(dtc.ops.conv_desc(N, H, W, C, K, 3, 3, 1, 1), n)
        assert nb > 0
        dws = dtc.ops.conv2d_wgrad_batch([a.inp(v) for v in xs], [a.inp(v) for v in dys], scale=0.25,
                                         workspace=a.ws(nb),
                                         out=[a.out((K, 3, 3, C), F32) for _ in range(n)]
                                         if isinstance(a, _Moat) else None)
        return list(dws), []
    return op


def _stem(x, w27, dy):
    def op(dtc, a):
        n, _, h, w = x.shape
        s = a.stats(64)
        xd = a.inp(x, F32)
        y = dtc.ops.stem_fwd(xd, a.inp(w27.reshape(64, 27)), s, out=a.out((n, h, w, 64)))
        dw = dtc.ops.stem_wgrad(xd, a.inp(dy), scale=0.5, out=a.out((64, 27), F32),
                                workspace=a.ws(dtc._native.lib.dtc_stem_wgrad_workspace_size(n, h, w)))
        return [y, dw], [(s, 64)]
    return op


def _head(act, w, bias, labels):
    """head_fwd -> xent_bwd -> head_bwd: activations, weights, bias, dlogits, feat, every output and the workspace
    embedded."""
    def op(dtc, a):
        N, h, w_, C = act.shape
        ncls = w.shape[0]
        moat = isinstance(a, _Moat)
        wd = a.inp(w)
        feat, logits = dtc.ops.head_fwd(a.inp(act), wd, a.inp(bias, F32),
                                        out=(a.out((N, C), F32), a.out((N, ncls), F32)) if moat else None)
        lab = torch.from_numpy(labels).to(a.dev)
        _, lse = dtc.ops.xent_fwd(logits, lab)
        dl = dtc.ops.xent_bwd(logits, lab, lse, torch.full((1,), 16.0, device=a.dev), out=a.out((N, ncls), F32))
        dw, db, dact = dtc.ops.head_bwd(dl, feat, wd, (h, w_), scale=0.25,
                                        out=(a.out((ncls, C), F32), a.out((ncls,), F32), a.out((N, h, w_, C)))
                                        if moat else None,
                                        workspace=a.ws(dtc._native.lib.dtc_head_bwd_workspace_size(N, C, ncls)))
        return [feat, logits, dl, dw, db, dact], []
    return op


def _head_ops(case, seed):
    N, h, w_, C, ncls = case
    g = np.random.default_rng(seed)
    return [_head(O.relu(_rand_bf16((N, h, w_, C), g)), _rand_bf16((ncls, C), g, 0.05),
                  g.standard_normal(ncls).astype(np.float32), g.integers(0, ncls, N))]


def _conv_ops(case, seed, modes="fdw"):
    """FWD (+ statistics), DGRAD + residual and WGRAD of one (N, H, W, C, K, R, stride) geometry."""
    N, H, W, C, K, R, st = case
    pad = 1 if R == 3 else 0
    P, Q = (H + 2 * pad - R) // st + 1, (W + 2 * pad - R) // st + 1
    g = np.random.default_rng(seed)
    x, w = _rand_bf16((N, H, W, C), g), _rand_bf16((K, R, R, C), g, 0.05)
    dy, res = _rand_bf16((N, P, Q, K), g), _rand_bf16((N, H, W, C), g)
    ops = {"f": _fwd(x, w, st, pad), "d": _dgrad(dy, w, (H, W), st, pad, res), "w": _wgrad(x, dy, R, st, pad)}
    return [ops[m] for m in modes]


def _s2_ops(case, seed, which):
    N, H, W, C, K = case
    g = np.random.default_rng(seed)
    x = _rand_bf16((N, H, W, C), g)
    dy, dsc = _rand_bf16((N, H // 2, W // 2, K), g), _rand_bf16((N, H // 2, W // 2, K), g)
    w, wsc = _rand_bf16((K, 3, 3, C), g, 0.05), _rand_bf16((K, 1, 1, C), g, 0.1)
    return {"fwd_sc": lambda: [_fwd(x, w, 2, 1), _fwd_sc(x, w, wsc)],
            "dgrad": lambda: [_dgrad(dy, w, (H, W), 2, 1, None), _dgrad_sc(dy, w, dsc, wsc, (H, W))],
            "dgrad_sc": lambda: [_dgrad_sc(dy, w, dsc, wsc, (H, W))],
            "wgrad_sc": lambda: [_wgrad(x, dy, 3, 2, 1), _wgrad_sc(x, dy, dsc)]}[which]()


def _wgrad_ops(case, seed):
    N, H, W, C, K = case
    g = np.random.default_rng(seed)
    return [_wgrad(_rand_bf16((N, H, W, C), g), _rand_bf16((N, H, W, K), g), 3, 1, 1)]


def _batch_ops(case, seed):
    N, H, W, C, K, n = case
    g = np.random.default_rng(seed)
    return [_wgrad_batch([_rand_bf16((N, H, W, C), g) for _ in range(n)],
                         [_rand_bf16((N, H, W, K), g) for _ in range(n)])]


def _stem_ops(shape, seed):
    n, h, w = shape
    g = np.random.default_rng(seed)
    return [_stem(g.standard_normal((n, 3, h, w)).astype(np.float32), _rand_bf16((64, 3, 3, 3), g, 0.2),
                  _rand_bf16((n, h, w, 64), g))]


# (id, forced options as the kernel's own test sets them, the ops)
CASES = [
    ("igemm-1x5x7", {}, lambda: _conv_ops((1, 5, 7, 64, 64, 3, 1), 1)),
    ("igemm-ragged-splitk-s2", {}, lambda: _conv_ops((3, 4, 4, 256, 512, 3, 2), 1)),
    # odd extents (tests/test_gpu_odd_extents.py): stride 2 at P = (H + 1) / 2, where tap r = 2 of the last output
    # row is padding, and the stride-1 conv of the 7x7 map behind it (49 pixels per image: no halo tile fits)
    ("igemm-odd-3x7x7-s2", {}, lambda: _conv_ops((3, 7, 7, 256, 512, 3, 2), 61)),
    ("igemm-odd-2x9x11-s2", {}, lambda: _conv_ops((2, 9, 11, 128, 256, 3, 2), 62)),
    ("igemm-odd-3x7x7-s1", {}, lambda: _conv_ops((3, 7, 7, 256, 256, 3, 1), 63)),
    ("halo-5x8x8-auto", {"halo_split": 0}, lambda: _conv_ops((5, 8, 8, 256, 256, 3, 1), 21, "fd")),
    ("halo-5x8x8-split2", {"halo_split": 2}, lambda: _conv_ops((5, 8, 8, 256, 256, 3, 1), 21, "fd")),
    ("halo-9x4x4-auto", {"halo_split": 0}, lambda: _conv_ops((9, 4, 4, 512, 256, 3, 1), 21, "fd")),
    ("halo-9x4x4-split2", {"halo_split": 2}, lambda: _conv_ops((9, 4, 4, 512, 256, 3, 1), 21, "fd")),
    ("halo-general-3x4x56", {}, lambda: _conv_ops((3, 4, 56, 64, 128, 3, 1), 41, "fd")),
    ("c64-forced-3x16x16", {"conv_c64": 2}, lambda: _conv_ops((3, 16, 16, 64, 64, 3, 1), 31, "fd")),
    ("c64-forced-general-2x40x96", {"conv_c64": 2}, lambda: _conv_ops((2, 40, 96, 64, 64, 3, 1), 33, "fd")),
    ("halo-s2-fwd-sc-cfg2", {"halo_s2": 2}, lambda: _s2_ops((5, 16, 16, 128, 256), 3, "fwd_sc")),
    ("dgrad-s2-subpixel-3x16x16", {"dgrad_s2h": 2}, lambda: _s2_ops((3, 16, 16, 128, 256), 34, "dgrad")),
    ("dgrad-s2-subpixel-5x8x8", {"dgrad_s2h": 2}, lambda: _s2_ops((5, 8, 8, 256, 512), 36, "dgrad")),
    ("dgrad-classes-sc-fused", {"dgrad_scf": 1}, lambda: _s2_ops((5, 16, 16, 128, 256), 9, "dgrad_sc")),
    ("wgrad-halo-3x8x8", {}, lambda: _wgrad_ops((3, 8, 8, 64, 128), 7)),
    ("wgrad-halo-12x4x4", {}, lambda: _wgrad_ops((12, 4, 4, 512, 512), 7)),
    ("wgrad-halo-3x4x4", {}, lambda: _wgrad_ops((3, 4, 4, 64, 64), 7)),
    ("wgrad-halo-1x5x40", {}, lambda: _wgrad_ops((1, 5, 40, 64, 64), 7)),
    ("wgrad-halo-2x14x224-trim0", {"wgrad_trim": 0}, lambda: _wgrad_ops((2, 14, 224, 64, 64), 23)),
    ("wgrad-halo-2x14x224-trim1", {"wgrad_trim": 1}, lambda: _wgrad_ops((2, 14, 224, 64, 64), 23)),
    ("wgrad-batch-n3", {}, lambda: _batch_ops((2, 14, 28, 128, 128, 3), 11)),
    ("wgrad-s2-sc-fused", {"wgrad_s2": 1}, lambda: _s2_ops((5, 16, 16, 128, 256), 7, "wgrad_sc")),
    ("stem-3x7x9", {}, lambda: _stem_ops((3, 7, 9), 12)),
    ("head-33x7x7x512x128-fused", {"head_fused": 1}, lambda: _head_ops((33, 7, 7, 512, 128), 51)),
    ("head-33x7x7x512x128-unfused", {"head_fused": 0}, lambda: _head_ops((33, 7, 7, 512, 128), 51)),
    ("head-70x2x3x96x129-fused", {"head_fused": 1}, lambda: _head_ops((70, 2, 3, 96, 129), 52)),
    ("head-70x2x3x96x129-unfused", {"head_fused": 0}, lambda: _head_ops((70, 2, 3, 96, 129), 52)),
]


def test_out_and_workspace_are_validated(dtc, cuda):
    """A caller's `out` must have the op's shape and dtype and be contiguous, a `workspace` the queried size: a
    wrong one is refused before any launch."""
    g = np.random.default_rng(0)
    a = _Plain(dtc, cuda)
    x, w = a.inp(_rand_bf16((3, 4, 4, 256), g)), a.inp(_rand_bf16((512, 3, 3, 256), g, 0.05))
    for bad in (torch.empty(3, 2, 2, 256, dtype=BF, device=cuda), torch.empty(3, 2, 2, 512, dtype=F32, device=cuda),
                torch.empty(3, 2, 2, 1024, dtype=BF, device=cuda)[..., ::2]):
        with pytest.raises(ValueError, match="out must be contiguous"):
            dtc.ops.conv2d_fwd(x, w, 2, 1, out=bad)
    assert dtc._native.lib.dtc_conv2d_workspace_size(dtc.ops.conv_desc(3, 4, 4, 256, 512, 3, 3, 2, 1), 0) > 16
    with pytest.raises(ValueError, match="workspace must be contiguous and hold"):
        dtc.ops.conv2d_fwd(x, w, 2, 1, workspace=torch.empty(4, dtype=F32, device=cuda))
    with pytest.raises(ValueError, match="out must list 2 tensors"):
        xb, dyb = a.inp(_rand_bf16((3, 8, 8, 64), g)), a.inp(_rand_bf16((3, 8, 8, 128), g))  # test_conv_wgrad_batch's
        dtc.ops.conv2d_wgrad_batch([xb, xb], [dyb, dyb], out=[None])
    with pytest.raises(dtc._native.NativeError):
        dtc.ops.conv2d_fwd(x, w, 2, 1, out=torch.empty(3, 2, 2, 512, dtype=BF))  # a host tensor


@pytest.mark.parametrize("name,opts,make", CASES, ids=[c[0] for c in CASES])
def test_guard_bands(dtc, cuda, name, opts, make):
    lib = dtc._native.lib
    prev = {k: lib.dtc_get_option(k.encode()) for k in opts}
    try:
        for k, v in opts.items():
            lib.dtc_set_option(k.encode(), v)
        for i, op in enumerate(make()):
            plain = _Plain(dtc, cuda)
            moat = _Moat(dtc, cuda)
            outs0, stats0 = op(dtc, plain)
            outs1, stats1 = op(dtc, moat)
            moat.check()
            assert len(moat.arenas) >= 3
            for j, (o0, o1) in enumerate(zip(outs0, outs1)):
                what = f"{name} op {i} output {j}"
                assert o1.data_ptr() != o0.data_ptr() and o0.shape == o1.shape, what
                assert not torch.isnan(o1).any() and not torch.isnan(o0).any(), what + ": NaN"
                bits = torch.int16 if o0.dtype == BF else torch.int32
                assert torch.equal(o0.view(bits), o1.view(bits)), what + ": embedded run differs from the plain run"
            for (s0, c), (s1, _) in zip(stats0, stats1):
                t0, t1 = dtc.ops.stat_totals(s0, c), dtc.ops.stat_totals(s1, c)
                assert t0.abs().sum() > 0 and torch.equal(t0, t1), f"{name} op {i}: BN statistics totals differ"
    finally:
        for k, v in prev.items():
            lib.dtc_set_option(k.encode(), v)
