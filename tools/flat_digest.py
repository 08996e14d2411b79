"""SHA-256 digests of everything the flat-buffer kernels write, for comparing two builds bit for bit.

    python tools/flat_digest.py [--seed 0] [--out FILE]

Only dtc.ops and the communicator API are used; inputs come from numpy.random.default_rng(seed). One JSON line per
(operation, shape) with the digest of every output buffer. Run it from two trees, each with its own built library,
and compare the files: equal files mean equal bits. Shapes are the smallest that reach each branch: for the chunked
kernels the LENGTHS of tests/test_gpu_grad_accum.py and tests/test_gpu_grad_compress.py, for the grid-stride kernels
1, 257 and cap * 256 + 1 rows (one thread takes a second trip)."""
import argparse
import hashlib
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dtc_import  # noqa: E402

ROWS = [1, 257, 2048 * 256 + 1]
ACCUM_TRIP, COMPRESS_TRIP = 256 * 4 * 4, 256 * 4 * 8
ACCUM_LENGTHS = [4, ACCUM_TRIP - 4, ACCUM_TRIP, ACCUM_TRIP + 4, 1_100_004, (2 * 1024 + 3) * ACCUM_TRIP + 1028]
COMPRESS_LENGTHS = [4, 8, 12, COMPRESS_TRIP - 4, COMPRESS_TRIP, COMPRESS_TRIP + 4, 1_100_004,
                    (1024 + 3) * COMPRESS_TRIP + 1028]
ODD_SEGMENTS = [(0, 5, True), (8, 8193, True), (8204, 3, False), (8208, 70001, True), (78212, 16386, False)]


def sha(t):
    torch.cuda.synchronize()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    dtc = dtc_import.load()
    ops, dev = dtc.ops, torch.device("cuda:0")
    rng = np.random.default_rng(a.seed)
    lines = []

    def f32(n, scale=1.0):
        return torch.from_numpy((rng.standard_normal(n) * scale).astype(np.float32)).to(dev)

    def bf16(n):
        return torch.zeros(n, dtype=torch.bfloat16, device=dev)

    def emit(op, shape, **bufs):
        lines.append(json.dumps({"op": op, "shape": shape, "sha256": {k: sha(v) for k, v in bufs.items()}}))

    found = torch.zeros(1, dtype=torch.int32, device=dev)
    inv = torch.full((1,), 1.0 / 1024.0, device=dev)

    for n in [4 * r for r in ROWS]:
        for scaled in (False, True):
            p, m, pb = f32(n), torch.zeros(n, device=dev), bf16(n)
            for _ in range(3):
                ops.sgd_nesterov_flat(p, f32(n, 1024.0 if scaled else 1.0), m, pb, 0.1, 1e-4, 0.9,
                                      inv if scaled else None, found if scaled else None)
            emit("sgd_nesterov_flat", {"n": n, "inv_scale": scaled}, p=p, m=m, pb=pb)
        for decoupled in (False, True):
            p, m, v, pb, st = f32(n), torch.zeros(n, device=dev), torch.zeros(n, device=dev), bf16(n), ops.adam_state(dev)
            for _ in range(3):
                ops.adam_flat(p, f32(n, 1024.0), m, v, pb, st, 1e-3, 0.9, 0.999, 1e-8, 1e-2, decoupled, inv, found)
            emit("adam_flat", {"n": n, "decoupled": decoupled}, p=p, m=m, v=v, pb=pb, state=st)
    for n in [4, 4 * 1025, 4 * (256 * 1024 + 1), 4 * (4 * 256 * 1024 + 5)]:
        tn, gm = ops.grad_norm_clip(f32(n, 1024.0), 1.0, inv_scale=inv)
        emit("grad_norm_clip", {"n": n}, total_norm=tn, grad_mult=gm)

    for name, plan in (("model", ops.seg_plan(dtc.nn.Layout(), dev)), ("odd", ops.seg_plan(ODD_SEGMENTS, dev))):
        n = (plan.end + 63) // 64 * 64
        p, g = f32(n), f32(n, 1024.0)
        emit("seg_norms", {"layout": name}, out=ops.seg_norms(plan, p, g, gmul=inv))
        for nesterov in (False, True):
            q, m, pb, so = p.clone(), torch.zeros(n, device=dev), bf16(n), torch.zeros(plan.nseg, 3, device=dev)
            for _ in range(2):
                ops.lars_flat(plan, q, g, m, pb, 0.1, 1e-4, 0.9, nesterov=nesterov, inv_scale=inv, found_inf=found,
                              seg_out=so)
            emit("lars_flat", {"layout": name, "nesterov": nesterov}, p=q, m=m, pb=pb, seg_out=so)

    for warmup in (False, True):
        sizes = [4 * 257, 4 * 300_001, 4 * 400_003]
        ema, src = [f32(n) for n in sizes], [f32(n) for n in sizes]
        shadow = [bf16(sizes[0]), None, bf16(sizes[2])]
        st = ops.ema_state(dev)
        for _ in range(3):
            ops.ema_update(list(zip(ema, src, shadow)), st, 0.9998, warmup=warmup, found_inf=found)
        emit("ema_update", {"n": sizes, "warmup": warmup}, ema0=ema[0], ema1=ema[1], ema2=ema[2], bf0=shadow[0],
             bf2=shadow[2], state=st)

    for n in ACCUM_LENGTHS:
        for mode in (ops.ACCUM_STORE, ops.ACCUM_ADD, ops.ACCUM_FINISH):
            acc, g = f32(n), f32(n)
            ops.grad_accum_flat(acc, g, mode)
            emit("grad_accum_flat", {"n": n, "mode": mode}, acc=acc, g=g)
    for n in COMPRESS_LENGTHS:
        for shift in (0, 4):  # c 16-byte aligned, c only 8-byte aligned
            for with_acc in (False, True):
                g, c = f32(n), bf16(n + 8)
                ops.grad_compress_bf16(g, c[shift:shift + n], acc=f32(n) if with_acc else None)
                emit("grad_compress_bf16", {"n": n, "c_shift": shift, "acc": with_acc}, c=c)
            g = torch.zeros(n, device=dev)
            c = torch.from_numpy(rng.integers(-(1 << 15), 1 << 15, n + 8, dtype=np.int16)).to(dev).view(torch.bfloat16)
            ops.grad_decompress_bf16(c[shift:shift + n], g)
            emit("grad_decompress_bf16", {"n": n, "c_shift": shift}, g=g)

    for n in ROWS + [1024 * 256 + 1]:
        src, dst = f32(n), bf16(n)
        ops.cast_f32_bf16(src, dst)
        emit("cast_f32_bf16", {"n": n}, dst=dst)
        emit("amp_scale", {"n": n}, out=ops.amp_scale(src, torch.full((1,), 1024.0, device=dev)))
    for n in [1, 3, 4 * 257 + 2, 4 * (4 * 1024 * 256 + 1) + 3]:
        for shift in (0, 1):  # the float4 kernel, the scalar kernel
            for bad in (None, 0, n - 1):
                g = f32(n + 1)[shift:shift + n]
                if bad is not None:
                    g[bad] = float("inf")
                flag = torch.zeros(1, dtype=torch.int32, device=dev)
                ops.amp_check_finite(g, flag)
                emit("amp_check_finite", {"n": n, "shift": shift, "bad": bad}, found=flag)

    def operand(n, dtype):
        if dtype == torch.int64:
            return torch.from_numpy(rng.integers(-(1 << 60), 1 << 60, n, dtype=np.int64)).to(dev)
        return f32(n).to(dtype)

    for dtype in (torch.float32, torch.bfloat16, torch.int64, torch.float64):
        for n in ROWS:
            t = operand(n, dtype)
            comm = dtc.parallel.Comm.loopback(0, 3.0, world=2)
            comm.allreduce_sum_(t)
            torch.cuda.synchronize()
            comm.close()
            emit("loopback_allreduce", {"n": n, "dtype": str(dtype), "factor": 3.0}, t=t)
            world = 3
            parts = [operand(n, dtype) for _ in range(world)]
            comms = dtc.parallel.Comm.thread_group(0, world)
            streams = [torch.cuda.Stream() for _ in range(world)]
            torch.cuda.synchronize()
            errs = []

            def body(r):
                try:
                    torch.cuda.set_device(0)
                    with torch.cuda.stream(streams[r]):
                        comms[r].allreduce_sum_(parts[r])
                        torch.cuda.current_stream().synchronize()
                except BaseException as e:  # noqa: BLE001 - reported below
                    errs.append(repr(e))

            ts = [threading.Thread(target=body, args=(r,)) for r in range(world)]
            for th in ts:
                th.start()
            for th in ts:
                th.join(120)
            if errs or any(th.is_alive() for th in ts):
                raise RuntimeError(f"thread-group all-reduce failed: {errs}")
            emit("thread_group_allreduce", {"n": n, "dtype": str(dtype), "world": world},
                 **{f"rank{r}": parts[r] for r in range(world)})

    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
