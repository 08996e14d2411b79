"""PowerSGD: the five launches of one compressed step at ResNet-18's real layout, one rank (no collectives).

    python tools/powersgd_bench.py [--ranks 1,2,4] [--launches 200] [--out profiles/powersgd_bench.json]

For every rank r: the plan of the model's Layout (ops.psgd_plan, torch's compression rule), gradients and an error
buffer of N(0, 1e-2), then each phase alone -- orthonormalize(Q), project, orthonormalize(P), back-project,
reconstruct -- and the whole step, by the method of tools/compress_bench.py --flat: `launches` launches in blocks of
20 back-to-back between two device events after a warm-up, median of the blocks (the 44.9 MB buffers fit the
Infinity Cache: rates of repeated passes, not of a cold pass inside a training step).

Reported per rank: us per phase and per step, and the step's share of the streaming bound: with error feedback the
algorithm reads g and e twice (project, back-project), reads and writes both once more (reconstruct) -- eight passes
over the flat buffer -- at the 6.3 TB/s achievable HBM rate. A measurement; no threshold is set anywhere."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # bytes / s
PARENT_STEP_MS = 1.78    # the training step this cost would be added to


def _time(fn, launches, inner, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(max(1, launches // inner)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        blocks.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(blocks)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", type=lambda v: [int(r) for r in v.split(",")], default=[1, 2, 4])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", type=str, default="")
    a = ap.parse_args()

    import torch

    import dtc_import

    dtc = dtc_import.load()
    ops = dtc.ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    flat = dtc.ResNet18().to(dev).flat
    n = flat.grads.numel()
    g0 = torch.empty_like(flat.grads).normal_(0, 1e-2)
    e0 = torch.empty_like(flat.grads).normal_(0, 1e-2)
    bound_us = 8 * n * 4 / HBM_ACHIEVABLE * 1e6
    line = {"bench": "powersgd", "device": torch.cuda.get_device_name(0), "flat_numel": n,
            "bytes_8_passes": 8 * n * 4, "streaming_bound_us": round(bound_us, 2), "launches": a.launches,
            "parent_step_ms": PARENT_STEP_MS, "ranks": {}}
    for r in a.ranks:
        plan = ops.psgd_plan(flat.layout, r, 2, dev)
        staging, q, state = ops.psgd_buffers(plan, 0, dev)
        g, e = g0.clone(), e0.clone()
        ops.psgd_step(plan, g, e, staging, q, state)  # leaves finite P, Ph, Q behind for the phases alone
        g.copy_(g0)
        e.copy_(e0)
        phases = {
            "orthonormalize_q": lambda: ops.psgd_orthonormalize(plan, ops.PSGD_Q, q, staging, state),
            "project": lambda: ops.psgd_project(plan, g, e, q, staging),
            "orthonormalize_p": lambda: ops.psgd_orthonormalize(plan, ops.PSGD_P, q, staging, state),
            "backproject": lambda: ops.psgd_backproject(plan, g, e, staging, q),
            "reconstruct": lambda: ops.psgd_reconstruct(plan, g, e, staging, q, state),
            "step": lambda: ops.psgd_step(plan, g, e, staging, q, state),
        }
        us = {k: round(_time(f, a.launches, a.inner, a.warmup), 2) for k, f in phases.items()}
        assert int(state[1]) == 0, "a benchmark step was not finite"
        line["ranks"][str(r)] = {"us": us, "share_of_streaming_bound": round(bound_us / us["step"], 3),
                                 "step_over_parent_step": round(us["step"] / (PARENT_STEP_MS * 1e3), 3),
                                 "allreduce_elements": [plan.n_staging, plan.n_q]}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
