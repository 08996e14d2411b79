#!/usr/bin/env python3
"""Which kernels every bf16 conv entry point launches, and the SHA-256 of what they write, for comparing two builds.

    python tools/conv_digest.py [--out FILE]           on the GPU: one line per (entry point, shape, option set)
    python tools/conv_digest.py --sizes [--out FILE]   no GPU needed: the workspace-size queries over the same grid
    python tools/conv_digest.py --routes [--out FILE]  no GPU needed: the router's answers (below)
    DTC_LIB=/path/to/other/libdtc_amd.so python tools/conv_digest.py ...    the other build; then cmp the files

A GPU line holds the dtc:: kernel names in launch order (tools/step_digest.py's kernels_of; one profiler session per
(shape, option set), the entry points separated by a one-element cast launch) and the digest of every output buffer;
an entry point the library refuses prints `refused`. Inputs come from numpy.random.default_rng(seed of the shape).
Entry points: fwd, fwd_sc, dgrad, dgrad with residual, dgrad_bn (one BN and two), dgrad_sc, wgrad, wgrad_sc,
wgrad_batch (2 and 4 problems), and fwd / dgrad / wgrad with no workspace straight through _native.call.
Shapes, the smallest that reach each route: the ResNet-18 layer shapes at batch 8 on 32x32, two split-K shapes at
batch 256, the 224x224 model's maps at batch 1, and S2_ODD / S1_ODD of tests/test_gpu_odd_extents.py. Option sets:
the defaults; that test's S1_FORCED on the stride-1 3x3 shapes and S2_FORCED on the stride-2 3x3 shapes of the
32x32 and odd groups; the routing options (OTHER below) on the 32x32 and split-K groups.
--sizes prints dtc_conv2d_workspace_size (three passes), dtc_conv2d_wgrad_sc_workspace_size,
dtc_conv2d_wgrad_batch_workspace_size (1..4) for every shape (also at batch 32 / 256 on 32x32, batch 8 on 224x224,
and the descriptors the ABI rejects) under EVERY option set, and dtc_rn18_workspace_bytes of four networks.
--routes prints one line per dtc_conv2d_route_query answer (workspace unlimited) over the whole GRID of
tests/test_conv_route.py, under every option set of that test, for every (pass, flags, nprob) of its _requests:
kernel, tile, splits, halo_cfg, halo_gen, sc_ok, refused, slab_wanted and slab_used."""
import argparse
import ctypes as C
import hashlib
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dtc_import  # noqa: E402

dtc = dtc_import.load()
lib, ops = dtc._native.lib, dtc.ops

S2_ODD = [(3, 7, 7, 256, 512), (2, 9, 11, 128, 256), (2, 5, 6, 256, 512), (3, 18, 21, 64, 128), (3, 15, 17, 64, 128),
          (2, 3, 3, 256, 512), (4, 1, 1, 256, 512), (9, 13, 15, 64, 128)]
S1_ODD = [(3, 7, 7, 256, 256), (3, 9, 11, 128, 128), (3, 5, 6, 256, 256), (3, 3, 3, 512, 512), (3, 2, 3, 512, 512),
          (2, 15, 17, 64, 64), (2, 14, 14, 128, 128)]
_S2_ALONE = [{"halo_s2": 2}, {"halo_s2": 3}, {"halo_s2": 4}, {"dgrad_s2h": 2}, {"wgrad_s2": 1}, {"dgrad_scf": 1}]
S2_FORCED = _S2_ALONE + [{"halo_s2": k, "dgrad_s2h": 2, "wgrad_s2": 1, "dgrad_scf": 1} for k in (2, 3, 4)]
S1_FORCED = [{"halo_conv": 2 + cfg, "halo_split": split} for cfg in range(8) for split in (0, 2)] + \
            [{"conv_c64": 2}, {"wgrad_halo": 0}, {"wgrad_gen": 0}, {"halo_small": 0}, {"halo_gen": 0}]
OTHER = [{"dgrad_classes": 0}, {"igemm_tile": 1}, {"igemm_tile": 2}, {"igemm_tile": 3}, {"igemm_split": 2},
         {"wgrad_s2": 0}, {"wgrad_s2": 1}, {"wgrad_s2": 2}, {"wgrad_halo": 0}, {"splitk_ink": 0}, {"sc_fuse": 2},
         {"sc_fuse": 3}]
REJECTED = [(8, 32, 32, 3, 64, 3, 3, 1, 1), (8, 32, 32, 64, 100, 3, 3, 1, 1), (8, 32, 32, 64, 64, 5, 5, 1, 2),
            (8, 32, 32, 64, 64, 3, 3, 3, 1), (0, 32, 32, 64, 64, 3, 3, 1, 1), (8, 1, 1, 64, 64, 3, 3, 1, 0)]


def layer_shapes(b, h):
    """The ten conv descriptors (n, h, w, c, k, r, s, stride, pad) of the residual layers for a b x 3 x h x h input."""
    out = [(b, h, h, 64, 64, 3, 3, 1, 1)]
    c = 64
    for _ in range(3):
        out += [(b, h, h, c, 2 * c, 3, 3, 2, 1), (b, h, h, c, 2 * c, 1, 1, 2, 0), (b, h // 2, h // 2, 2 * c, 2 * c, 3, 3, 1, 1)]
        c, h = 2 * c, h // 2
    return out


def odd_shapes():
    return [(n, h, w, c, k, r, r, 2, r // 2) for (n, h, w, c, k) in S2_ODD for r in (3, 1)] + \
           [(n, h, w, c, k, 3, 3, 1, 1) for (n, h, w, c, k) in S1_ODD]


SPLITK = [(256, 4, 4, 512, 512, 3, 3, 1, 1), (256, 8, 8, 256, 256, 3, 3, 1, 1)]


def oid(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "defaults"


class Options:
    def __init__(self, opts):
        self.opts, self.saved = opts, {}

    def __enter__(self):
        for k, v in self.opts.items():
            self.saved[k.encode()] = lib.dtc_get_option(k.encode())
            dtc._native.call("dtc_set_option", k.encode(), int(v))

    def __exit__(self, *exc):
        for key, v in self.saved.items():
            lib.dtc_set_option(key, v)


# ---------------------------------------------------------------------------------------------- workspace sizes (CPU)
def sizes(emit):
    shapes = [s for b in (8, 32, 256) for s in layer_shapes(b, 32)] + [s for b in (1, 8) for s in layer_shapes(b, 224)] + \
        SPLITK + odd_shapes() + REJECTED
    for o in [{}] + S1_FORCED + S2_FORCED + OTHER:
        with Options(o):
            for s in shapes:
                d = dtc._native.ConvDesc(*s)
                ws = [lib.dtc_conv2d_workspace_size(d, p) for p in range(3)]
                emit(f"{oid(o)} | {s} | ws={ws} wgrad_sc={lib.dtc_conv2d_wgrad_sc_workspace_size(d)} "
                     f"wgrad_batch={[lib.dtc_conv2d_wgrad_batch_workspace_size(d, n) for n in range(1, 5)]}")
            for (b, h, w) in [(8, 32, 32), (32, 32, 32), (256, 32, 32), (8, 224, 224)]:
                net = C.c_void_p()
                dtc._native.call("dtc_rn18_create", C.byref(net), b, h, w, 100, 25.0)
                emit(f"{oid(o)} | rn18 {(b, h, w)} | workspace={lib.dtc_rn18_workspace_bytes(net)}")
                lib.dtc_rn18_destroy(net)


# ---------------------------------------------------------------------------------------------- routes (CPU)
def routes(emit):
    import importlib.util

    spec = importlib.util.spec_from_file_location("test_conv_route", os.path.join(ROOT, "tests", "test_conv_route.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    N = dtc._native
    q, r, unlimited = lib.dtc_conv2d_route_query, N.ConvRoute(), C.c_size_t(-1).value >> 1
    for o in t.OPTION_SETS:
        with Options(o):
            for shape in t.GRID:
                d = N.ConvDesc(*shape)
                for mode, flags, nprob in t._requests(shape):
                    if q(d, mode, flags, nprob, t.WS, unlimited, C.byref(r)) != 0:
                        emit(f"{oid(o)} | {shape} | {mode} {flags} {nprob} | error: {N.last_error()}")
                        continue
                    emit(f"{oid(o)} | {shape} | {mode} {flags} {nprob} | {N.CONV_KERNELS[r.kernel]} {r.gemm_bm}x{r.gemm_bn} "
                         f"splits={r.splits} halo_cfg={r.halo_cfg} halo_gen={r.halo_gen} sc_ok={r.sc_ok} "
                         f"refused={r.refused} slab_wanted={r.slab_wanted} slab_used={r.slab_used}")


# ---------------------------------------------------------------------------------------------- launches (GPU)
def sha(t):
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:20]


class Problem:
    def __init__(self, shape, seed):
        self.shape = shape
        n, h, w, c, k, r, s, st, pad = shape
        self.p, self.q = ops.conv_out_hw(h, w, r, s, st, pad)
        g, dev = np.random.default_rng(seed), torch.device("cuda:0")

        def bf(*dims, scale=1.0):
            return torch.from_numpy((g.standard_normal(dims) * scale).astype(np.float32)).to(dev).bfloat16()

        def f32(*dims, lo=0.0):
            return torch.from_numpy((g.random(dims) + lo).astype(np.float32)).to(dev)

        self.x, self.w, self.dy = bf(n, h, w, c), bf(k, r, s, c, scale=0.05), bf(n, self.p, self.q, k)
        self.res, self.ym, self.x1, self.x2 = bf(n, h, w, c), bf(n, h, w, c), bf(n, h, w, c), bf(n, h, w, c)
        self.mean1, self.mean2, self.inv1, self.inv2 = f32(c, lo=-0.5), f32(c, lo=-0.5), f32(c, lo=0.5), f32(c, lo=0.5)
        self.wsc, self.dsc = bf(k, c, scale=0.05), bf(n, self.p, self.q, k)
        self.desc = dtc._native.ConvDesc(*shape)

    def entries(self):
        n, h, w, c, k, r, s, st, pad = self.shape
        P, ptr, sp, dev = self, dtc._native.ptr, dtc._native.stream_ptr, self.x.device
        yield "fwd", lambda: _fwd(P)
        yield "dgrad", lambda: {"dx": ops.conv2d_dgrad(P.dy, P.w, (h, w), st, pad)}
        yield "dgrad_res", lambda: {"dx": ops.conv2d_dgrad(P.dy, P.w, (h, w), st, pad, res=P.res)}
        yield "dgrad_bn", lambda: _named(("dz", "acc1", "acc2"), ops.conv2d_dgrad_bn(
            P.dy, P.w, (h, w), st, pad, P.ym, P.x1, P.mean1, P.inv1))
        yield "dgrad_bn2", lambda: _named(("dz", "acc1", "acc2"), ops.conv2d_dgrad_bn(
            P.dy, P.w, (h, w), st, pad, P.ym, P.x1, P.mean1, P.inv1, P.x2, P.mean2, P.inv2, res=P.res))
        yield "wgrad", lambda: {"dw": ops.conv2d_wgrad(P.x, P.dy, r, s, st, pad, scale=0.5)}
        if r == 3 and st == 2:
            yield "fwd_sc", lambda: _fwd_sc(P)
            yield "dgrad_sc", lambda: {"dx": ops.conv2d_dgrad_sc(P.dy, P.w, P.dsc, P.wsc, (h, w))}
            yield "wgrad_sc", lambda: _named(("dw", "dw_sc"), ops.conv2d_wgrad_sc(P.x, P.dy, P.dsc, scale=0.5))
        if r == 3 and st == 1:
            for nb in (2, 4):
                yield f"wgrad_batch{nb}", lambda nb=nb: _named(
                    [f"dw{i}" for i in range(nb)],
                    ops.conv2d_wgrad_batch([torch.roll(P.x, i, 2) for i in range(nb)],
                                           [torch.roll(P.dy, i, 2) for i in range(nb)], scale=0.5))
        # no workspace at all: the one-split / separate-reduction fallbacks (wgrad requires one: refused)
        y = torch.zeros(n, P.p, P.q, k, dtype=torch.bfloat16, device=dev)
        dx = torch.zeros(n, h, w, c, dtype=torch.bfloat16, device=dev)
        dw = torch.zeros(k, r, s, c, dtype=torch.float32, device=dev)
        yield "fwd_nows", lambda: (dtc._native.call("dtc_conv2d_fwd", P.desc, ptr(P.x), ptr(P.w), ptr(y), None, None, 0,
                                                    sp()), {"y": y})[1]
        yield "dgrad_nows", lambda: (dtc._native.call("dtc_conv2d_dgrad", P.desc, ptr(P.dy), ptr(P.w), ptr(dx), None,
                                                      None, 0, sp()), {"dx": dx})[1]
        yield "wgrad_nows", lambda: (dtc._native.call("dtc_conv2d_wgrad", P.desc, ptr(P.x), ptr(P.dy), ptr(dw),
                                                      C.c_float(0.5), None, 0, sp()), {"dw": dw})[1]


def _named(names, tensors):
    return {nm: t for nm, t in zip(names, tensors) if t is not None}


def _fwd(P):
    stats = ops.new_stats(P.shape[4], P.x.device)
    return {"y": ops.conv2d_fwd(P.x, P.w, P.shape[7], P.shape[8], stats=stats), "stats": stats}


def _fwd_sc(P):
    st, st2 = ops.new_stats(P.shape[4], P.x.device), ops.new_stats(P.shape[4], P.x.device)
    y, ysc = ops.conv2d_fwd_sc(P.x, P.w, P.wsc, stats=st, stats_sc=st2)
    return {"y": y, "ysc": ysc, "stats": st, "stats_sc": st2}


def run_gpu(emit):
    from tools.step_digest import kernels_of

    one, one_bf = torch.zeros(4, device="cuda:0"), torch.zeros(4, dtype=torch.bfloat16, device="cuda:0")

    def mark():
        ops.cast_f32_bf16(one, one_bf)

    marker = kernels_of(mark)[0][0]
    small = layer_shapes(8, 32)
    groups = [({}, small + SPLITK + layer_shapes(1, 224) + odd_shapes())]
    groups += [(o, [s for s in small + odd_shapes() if s[5] == 3 and s[7] == 1]) for o in S1_FORCED]
    groups += [(o, [s for s in small + odd_shapes() if s[5] == 3 and s[7] == 2]) for o in S2_FORCED]
    groups += [(o, small + SPLITK) for o in OTHER]
    problems = {}
    for o, shapes in groups:
        with Options(o):
            for s in shapes:
                if s not in problems:
                    problems[s] = Problem(s, seed=zlib.crc32(repr(s).encode()))
                names, outs = [], []

                def body():
                    for nm, fn in problems[s].entries():
                        names.append(nm)
                        try:
                            outs.append(fn())
                        except (dtc._native.NativeError, ValueError):
                            outs.append(None)
                        mark()

                seqs = kernels_of(body)
                flat = seqs[0] if len(seqs) == 1 else [f"STREAMS {seqs}"]
                per, cur = [], []
                for kname in flat:
                    if kname == marker:
                        per.append(cur)
                        cur = []
                    else:
                        cur.append(kname)
                for i, nm in enumerate(names):
                    ks = per[i] if len(per) == len(names) else ["?"]
                    res = "refused" if outs[i] is None else " ".join(f"{k}={sha(v)}" for k, v in outs[i].items())
                    emit(f"{nm} | {s} | {oid(o)} | {' '.join(ks)} | {res}")
        if len(problems) > 24:  # device memory: keep only the shapes the option groups share
            problems = {k: v for k, v in problems.items() if k in small + SPLITK or k in odd_shapes()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--routes", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    f = open(a.out, "w") if a.out else None

    def emit(line):
        print(line, flush=not a.routes)  # (--routes prints over a million lines)
        if f:
            f.write(line + "\n")
            if not a.routes:
                f.flush()

    (sizes if a.sizes else routes if a.routes else run_gpu)(emit)


if __name__ == "__main__":
    main()
