"""bf16 gradient compression: the flat kernels alone, and the step with compression on and off.

    python tools/compress_bench.py --flat [--out profiles/compress_flat_bench.json]

The kernels alone, by the method of tools/accum_bench.py --flat: dtc_grad_compress_bf16 (plain and with `acc`) and
dtc_grad_decompress_bf16 over the whole flat gradient buffer against dtc_grad_accum_flat STORE over the same
buffers -- existing code of the same launch shape, the yardstick of the session. 200 launches each in alternating
blocks of 20 back-to-back launches between two device events, median of the blocks (the buffers fit the Infinity
Cache: rates of repeated passes, not of a cold pass inside a step).

    python tools/compress_bench.py [--batch 256] [--steps 40] [--blocks 6] [--warmup 10] [--out profiles/compress_bench.json]

The B = 256 eager AMP training step (forward, backward through Comm.loopback(world=2), SGD under GradScaler) with
compression on and off in alternating blocks, wall ms per step, median of the blocks. A placement check, not a wire
measurement: the loopback "collective" is a kernel over the bucket on this GPU, and over a bf16 bucket it moves half
the bytes too, so the difference says what the compress / decompress launches cost where they sit, not what xGMI
would save.

    python tools/compress_bench.py --curve [--out profiles/grad_compress_curve.json]

Loss curve, recorded only: W = 2 ranks of Comm.thread_group on one GPU (one host thread each, distinct data through
the product Reducer), batch 32 per rank, 50 SGD steps (lr 0.1, momentum 0.9, weight decay 1e-4, Nesterov, bf16
autocast) on data.synthetic_batch -- rank r takes batch W * step + r -- once with the fp32 all-reduce and once
bf16-compressed on the same build. Writes both curves (rank 0's loss per step) and the relative difference of the mean
of the last 10 losses."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _write(line, out):
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


def flat_bench(out, launches=200, inner=20, warmup=20):
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
    acc.normal_(0, 1e-2)
    c16 = flat.grad_c16
    ops.grad_compress_bf16(flat.grads, c16)
    kernels = {
        "compress": (lambda: ops.grad_compress_bf16(flat.grads, c16), 6 * n),
        "compress_acc": (lambda: ops.grad_compress_bf16(flat.grads, c16, acc=acc), 10 * n),
        "decompress": (lambda: ops.grad_decompress_bf16(c16, flat.grads), 6 * n),
        "accum_store": (lambda: ops.grad_accum_flat(acc, flat.grads, ops.ACCUM_STORE), 8 * n),
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
            us[k].append(timed(fn))
    line = {"what": "dtc_grad_compress_bf16 (plain, with acc) and dtc_grad_decompress_bf16 over the whole flat gradient "
                    "buffer against dtc_grad_accum_flat STORE, us per launch (device events around blocks of "
                    "back-to-back launches, blocks alternating)",
            "flat_numel": n, "launches": launches, "inner": inner, "warmup": warmup, "kernels": {}}
    for k, (_, nbytes) in kernels.items():
        med = statistics.median(us[k])
        line["kernels"][k] = {"median_us": med, "min_us": min(us[k]), "max_us": max(us[k]), "bytes": nbytes,
                              "TBps_median": nbytes / (med * 1e-6) / 1e12, "of_8TBps_peak": nbytes / (med * 1e-6) / 8e12}
    store = line["kernels"]["accum_store"]["TBps_median"]
    for k in ("compress", "compress_acc", "decompress"):
        line["kernels"][k]["of_accum_store_rate"] = line["kernels"][k]["TBps_median"] / store
    _write(line, out)


def step_bench(a):
    import torch

    import dtc_import

    dtc = dtc_import.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = dtc.ResNet18().to(dev)
    comm = dtc.parallel.Comm.loopback(0, 1.0, world=2)  # factor 1: the parameters stay where training puts them
    model._comm = comm
    model._grad_scale = 0.5
    crit = dtc.CrossEntropyLoss()
    opt = dtc.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)
    scaler = dtc.GradScaler()
    x = torch.randn(a.batch, 3, 32, 32, device=dev)
    y = torch.randint(0, 100, (a.batch,), device=dev)

    def step():
        with dtc.autocast():
            loss = crit(model(x), y)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    def block(compression, steps):
        model.grad_compression = compression
        step()  # the mode switch itself
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for mode in (None, "bf16"):
        block(mode, a.warmup)
    ms = {"off": [], "bf16": []}
    for _ in range(a.blocks):
        ms["off"].append(block(None, a.steps))
        ms["bf16"].append(block("bf16", a.steps))
    comm.clear_log()
    line = {"what": "eager AMP training step through Comm.loopback(world=2), bf16 gradient compression off / on in "
                    "alternating blocks, wall ms per step. A placement check, not a wire measurement: the loopback's "
                    "own kernel moves half the bytes over a bf16 bucket too",
            "batch": a.batch, "steps_per_block": a.steps, "blocks": a.blocks, "warmup": a.warmup,
            "buckets": len(model.buckets()), "flat_numel": model.flat.grads.numel(),
            "ms_per_step_off": ms["off"], "ms_per_step_bf16": ms["bf16"],
            "median_ms_off": statistics.median(ms["off"]), "median_ms_bf16": statistics.median(ms["bf16"])}
    _write(line, a.out)
    comm.close()


def curve_bench(out, world=2, batch=32, steps=50):
    import threading

    import torch

    import dtc_import

    dtc = dtc_import.load()
    dev = torch.device("cuda:0")
    templates = dtc.data.class_templates(100, 32, 32, 1234)
    data = [[dtc.data.synthetic_batch(world * s + r, batch, device=dev, templates=templates) for s in range(steps)]
            for r in range(world)]
    torch.cuda.synchronize()

    def run(compression):
        comms = dtc.parallel.Comm.thread_group(0, world)
        models = []
        for _ in range(world):
            torch.manual_seed(42)
            models.append(dtc.ResNet18().to(dev))
        losses, errs = [None] * world, [None] * world
        streams = [torch.cuda.Stream() for _ in range(world)]

        def rank(r):
            try:
                torch.cuda.set_device(0)
                with torch.cuda.stream(streams[r]):
                    ddp = dtc.DistributedDataParallel(models[r], device_ids=[0], comm=comms[r],
                                                      gradient_compression=compression)
                    crit = dtc.CrossEntropyLoss()
                    opt = dtc.SGD(ddp.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
                    mine = []
                    for x, y in data[r]:
                        opt.zero_grad()
                        with dtc.autocast():
                            loss = crit(ddp(x), y)
                        dtc._native.call("dtc_barrier", comms[r].handle, dtc._native.stream_ptr())
                        loss.backward()
                        opt.step()
                        mine.append(loss)
                    torch.cuda.current_stream().synchronize()
                    losses[r] = [float(v) for v in mine]
            except BaseException as e:  # noqa: BLE001 - re-raised below
                errs[r] = e

        ts = [threading.Thread(target=rank, args=(r,)) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(600)
        for e in errs:
            if e is not None:
                raise e
        return losses[0]

    fp32 = run(None)
    bf16 = run("bf16")
    tail = lambda v: sum(v[-10:]) / 10.0
    line = {"what": "rank 0's training loss per step, W = 2 thread-group ranks with distinct data, batch 32 per rank, SGD "
                    "lr 0.1 momentum 0.9 wd 1e-4 Nesterov, bf16 autocast, data.synthetic_batch(W * step + rank): fp32 "
                    "bucket all-reduce against bf16-compressed, same build; recorded only",
            "world": world, "batch_per_rank": batch, "steps": steps, "loss_fp32_allreduce": fp32,
            "loss_bf16_compressed": bf16, "mean_last10_fp32": tail(fp32), "mean_last10_bf16": tail(bf16),
            "rel_diff_mean_last10": (tail(bf16) - tail(fp32)) / tail(fp32)}
    _write(line, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flat", action="store_true", help="time the kernels alone over the whole gradient buffer")
    ap.add_argument("--curve", action="store_true", help="50-step loss curves, fp32 all-reduce against bf16-compressed")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None,
                    help="default: profiles/compress_bench.json (--flat: compress_flat_bench.json, --curve: "
                         "grad_compress_curve.json)")
    a = ap.parse_args()
    if a.out is None:
        name = "compress_flat_bench.json" if a.flat else "grad_compress_curve.json" if a.curve else "compress_bench.json"
        a.out = os.path.join(ROOT, "profiles", name)
    if a.flat:
        return flat_bench(a.out)
    if a.curve:
        return curve_bench(a.out)
    return step_bench(a)


if __name__ == "__main__":
    main()
