"""Weight-EMA kernel timing: dtc_ema_update over the model's two ranges against dtc_sgd_nesterov_flat over the same
parameter buffer.

    python tools/ema_bench.py [--launches 200] [--inner 20] [--warmup 20] [--out profiles/ema_bench.json]

One process, the model's own flat buffers (11.22 M parameters + slot padding; the EMA also covers the 9600-element
running-statistics buffer in the same launch). After `warmup` launches of each, `launches` launches of each are
timed in blocks of `inner` back-to-back launches between two device events, the blocks of the two kernels
ALTERNATING, so both see the same machine state. ema_update's time includes its one-thread tick launch (what a
step pays). Bytes by the algorithm: ema 4 + 4 + 4 + 2 = 14 B per parameter and 12 B per running statistic (no bf16
copy), sgd 5 x 4 + 2 = 22 B per parameter. Target: ema_us <= sgd_us x (14 / 22) x 1.25 -- the margin is for the
launch ramp and the tick, a larger share of a shorter kernel. Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ema_bench.json"))
    a = ap.parse_args()
    if a.launches % a.inner:
        ap.error("--launches must be a multiple of --inner")

    import torch

    import dtc_import

    dtc = dtc_import.load()
    ops = dtc.ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = dtc.ResNet18().to(dev)
    flat = model.flat
    n, nb = flat.params.numel(), flat.bufs.numel()
    flat.grads.normal_(0, 1e-2)
    mom = torch.zeros_like(flat.params)
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    inv = torch.ones(1, device=dev)
    ema = dtc.ModelEma(model, decay=0.9998)

    kernels = {
        "ema_update": (lambda: ema.update(found_inf=found), 14 * n + 12 * nb),
        "sgd_nesterov": (lambda: ops.sgd_nesterov_flat(flat.params, flat.grads, mom, flat.params_bf16, 1e-3, 1e-4, 0.9,
                                                       inv, found), 22 * n),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.inner  # us per launch

    for _ in range(a.warmup):
        for fn, _ in kernels.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in kernels}
    for _ in range(a.launches // a.inner):
        for k, (fn, _) in kernels.items():
            us[k].append(timed(fn))
    line = {"what": "dtc_ema_update (parameters + running statistics, tick included) against dtc_sgd_nesterov_flat "
                    "over the model's flat parameter buffer, us per launch (device events around blocks of "
                    "back-to-back launches, blocks alternating)",
            "flat_numel": n, "bufs_numel": nb, "parameters": sum(p.numel for p in flat.layout.params),
            "launches": a.launches, "inner": a.inner, "warmup": a.warmup, "ema_updates_counted": ema.num_updates,
            "kernels": {}}
    for k, (_, nbytes) in kernels.items():
        med = statistics.median(us[k])
        line["kernels"][k] = {"median_us": med, "min_us": min(us[k]), "max_us": max(us[k]),
                              "all_us": [round(x, 3) for x in us[k]], "bytes": nbytes,
                              "TBps_median": nbytes / (med * 1e-6) / 1e12,
                              "TBps_best": nbytes / (min(us[k]) * 1e-6) / 1e12}
    ema_us, sgd_us = line["kernels"]["ema_update"]["median_us"], line["kernels"]["sgd_nesterov"]["median_us"]
    line["ema_us"], line["sgd_us"] = ema_us, sgd_us
    line["ema_over_sgd"] = ema_us / sgd_us
    line["target_ema_over_sgd"] = 14 / 22 * 1.25
    line["target_met"] = ema_us <= sgd_us * (14 / 22) * 1.25
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
