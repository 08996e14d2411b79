#!/usr/bin/env python3
"""Time of the fp32 (no autocast) training step of the native ResNet-18, for comparing two builds of the library.

    python tools/f32_step_bench.py [--batch 256] [--steps 40] [--warmup 10] [--opt f32_split=4]
    LAB_CMD="python tools/f32_step_bench.py --opt f32_split=4" tools/lib_ab.sh 3 parent=... new=...

One step = forward, cross entropy, backward, Nesterov SGD on fixed synthetic 32x32 data; the clock runs around
`steps` steps between two device synchronisations. Prints one JSON line; "value" is images per second."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import dtc_import  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--opt", action="append", default=[], help="native option NAME=VALUE, set before the executor exists")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("f32_step_bench: no GPU")
    dtc = dtc_import.load()
    for o in a.opt:
        name, value = o.split("=")
        dtc._native.call("dtc_set_option", name.encode(), int(value))
    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    model = dtc.ResNet18().to(dev)
    model.precision = "fp32"
    crit = dtc.CrossEntropyLoss()
    opt = dtc.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    x = torch.randn(a.batch, 3, 32, 32, device=dev)
    y = torch.randint(0, 100, (a.batch,), device=dev)

    def step():
        crit(model(x), y).backward()
        opt.step()

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"value": round(a.batch * a.steps / dt, 2), "unit": "images/s", "ms_per_step": round(1e3 * dt / a.steps, 4),
                      "batch": a.batch, "steps": a.steps, "precision": "fp32", "options": a.opt}))


if __name__ == "__main__":
    main()
