"""Gradient accumulation at the bench defaults: eager AMP training micro-steps in windows of N against plain steps.

    python tools/accum_bench.py [--accum-steps 4] [--windows 10] [--warmup 3] [--batch 256] [--out profiles/accum_bench.json]

One process, one model (B = 256, 32 x 32, bf16 under autocast, bucket cap 25 MB, SGD with GradScaler): `windows`
windows of N micro-steps (N - 1 backwards inside ResNet.accumulate(), one outside, then scaler.step / update), then
the same number of micro-batches as plain steps (forward, backward, step each). Wall time per micro-step of both,
the host synchronised only around each timed region. The accumulate launches overlap the backward, so their own
device time is read from a kernel trace of this run instead:

    rocprofv3 --kernel-trace --stats -d DIR -o accum -- python tools/accum_bench.py

    python tools/accum_bench.py --summarise DIR [--csv profiles/accum_kernel_times.csv]

The second form reads DIR's trace (tools/prof_summary.py's reader) and prints, per kernel of interest --
grad_accum_kernel<1|2|3> (STORE, ADD, FINISH: one launch per gradient bucket and micro-step; STORE moves 8 B per
gradient element, ADD and FINISH 12 B), sgd_nesterov_kernel, amp_check_finite4_kernel -- calls, total, mean, min and
max device time. The run prints one JSON line with the micro-step counts to divide the totals by and writes it to
--out.

    python tools/accum_bench.py --flat [--out profiles/accum_flat_bench.json]

The kernel alone, as tools/ema_bench.py times its kernel: dtc_grad_accum_flat in each mode over the whole gradient
buffer against dtc_sgd_nesterov_flat over the same buffers, 200 launches each in alternating blocks of 20
back-to-back launches between two device events, median of the blocks (the buffers fit the Infinity Cache: rates of
repeated passes, not of a cold pass inside a step)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


KERNELS = ("grad_accum_kernel<1>", "grad_accum_kernel<2>", "grad_accum_kernel<3>", "sgd_nesterov_kernel",
           "amp_check_finite4_kernel")


def summarise(src, out_csv):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import prof_summary

    rows = prof_summary.load_rows(src)
    lines = ["kernel,calls,total_us,mean_us,min_us,max_us"]
    for k in KERNELS:
        mangled = k.replace("<", "ILi").replace(">", "E")  # a trace that kept the mangled names
        d = [(e - s) / 1e3 for s, e, n in rows if k in n or mangled in n]
        if d:
            lines.append(f"{k},{len(d)},{sum(d):.2f},{sum(d) / len(d):.3f},{min(d):.3f},{max(d):.3f}")
    text = "\n".join(lines)
    print(text, flush=True)
    if out_csv:
        with open(out_csv, "w") as f:
            f.write(text + "\n")


def flat_bench(out, launches=200, inner=20, warmup=20):
    import statistics

    import torch

    import dtc_import

    dtc = dtc_import.load()
    ops = dtc.ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = dtc.ResNet18().to(dev)
    flat = model.flat
    n = flat.grads.numel()
    flat.grads.normal_(0, 1e-2)
    acc = flat.grad_acc
    mom = torch.zeros_like(flat.params)
    kernels = {
        "accum_store": (lambda: ops.grad_accum_flat(acc, flat.grads, ops.ACCUM_STORE), 8 * n),
        "accum_add": (lambda: ops.grad_accum_flat(acc, flat.grads, ops.ACCUM_ADD), 12 * n),
        "accum_finish": (lambda: ops.grad_accum_flat(acc, flat.grads, ops.ACCUM_FINISH), 12 * n),
        "sgd_nesterov": (lambda: ops.sgd_nesterov_flat(flat.params, flat.grads, mom, flat.params_bf16, 1e-3, 1e-4, 0.9,
                                                       None, None), 22 * n),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / inner  # us per launch

    for _ in range(warmup):
        for fn, _ in kernels.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in kernels}
    for _ in range(launches // inner):
        for k, (fn, _) in kernels.items():
            flat.grads.normal_(0, 1e-2)  # (repeated ADD / FINISH passes would otherwise run the sums up to inf)
            acc.zero_()
            us[k].append(timed(fn))
    line = {"what": "dtc_grad_accum_flat per mode over the whole flat gradient buffer against dtc_sgd_nesterov_flat, us "
                    "per launch (device events around blocks of back-to-back launches, blocks alternating)",
            "flat_numel": n, "launches": launches, "inner": inner, "warmup": warmup, "kernels": {}}
    for k, (_, nbytes) in kernels.items():
        med = statistics.median(us[k])
        line["kernels"][k] = {"median_us": med, "min_us": min(us[k]), "max_us": max(us[k]), "bytes": nbytes,
                              "TBps_median": nbytes / (med * 1e-6) / 1e12, "of_8TBps_peak": nbytes / (med * 1e-6) / 8e12}
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise", type=str, default=None, help="a rocprofv3 output directory of an earlier run")
    ap.add_argument("--csv", type=str, default=None, help="--summarise: also write the table here")
    ap.add_argument("--flat", action="store_true", help="time the kernel alone over the whole gradient buffer")
    ap.add_argument("--accum-steps", type=int, default=4)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", type=str, default=None, help="default: profiles/accum_bench.json (--flat: accum_flat_bench.json)")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise, a.csv)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "accum_flat_bench.json" if a.flat else "accum_bench.json")
    if a.flat:
        return flat_bench(a.out)
    if a.accum_steps < 2:
        ap.error("--accum-steps must be >= 2")

    import contextlib

    import torch

    import dtc_import

    dtc = dtc_import.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = dtc.ResNet18().to(dev)
    crit = dtc.CrossEntropyLoss()
    opt = dtc.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)
    scaler = dtc.GradScaler()
    n = a.accum_steps
    xs = [torch.randn(a.batch, 3, 32, 32, device=dev) for _ in range(n)]
    ys = [torch.randint(0, 100, (a.batch,), device=dev) for _ in range(n)]

    def micro(k, hold):
        with dtc.autocast():
            loss = crit(model(xs[k]), ys[k])
        with model.accumulate() if hold else contextlib.nullcontext():
            scaler.scale(loss).backward()

    def window():
        for k in range(n):
            micro(k, k < n - 1)
        scaler.step(opt)
        scaler.update()

    def plain():
        for k in range(n):
            micro(k, False)
            scaler.step(opt)
            scaler.update()

    def timed(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.windows):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (a.windows * steps)

    model.grad_accum_steps = n
    for _ in range(a.warmup):
        window()
    accum_ms = timed(window, n)
    model.grad_accum_steps = 1
    for _ in range(a.warmup):
        plain()
    plain_ms = timed(plain, n)
    buckets = model.buckets()
    numel = model.flat.grads.numel()
    total = a.windows + a.warmup
    line = {"what": "eager AMP micro-steps in windows of N (ResNet.accumulate) against plain steps, wall ms per "
                    "micro-step; per-mode accumulate launches in this run for a kernel trace's totals",
            "batch": a.batch, "accum_steps": n, "windows": a.windows, "warmup": a.warmup,
            "flat_numel": numel, "buckets": len(buckets), "bucket_numel": [b[1] for b in buckets],
            "ms_per_micro_step_accum": accum_ms, "ms_per_micro_step_plain": plain_ms,
            "micro_steps": {"store": total, "add": total * (n - 2), "finish": total},
            "launches": {"store": total * len(buckets), "add": total * (n - 2) * len(buckets),
                         "finish": total * len(buckets)},
            "bytes_per_micro_step": {"store": 8 * numel, "add": 12 * numel, "finish": 12 * numel}}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
