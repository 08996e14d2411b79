"""Trainer.validate() timing and launch counting: the default path against --fused-eval.

    python tools/eval_bench.py [--reps 7] [--batch-size 256] [--precision fp32|bf16] [--out FILE]
        Two trainers on the same weights and the same 5,000-image validation split (--device-data); after a
        warm-up of each, validate() of the two is timed alternately (host clock around a final device
        synchronise), `reps` times each. Prints one JSON line: medians, min / max, the per-repetition times and
        both paths' results (which must be equal).
    python tools/eval_bench.py --only default|fused [--evals 3]
        The same set-up, then `evals` evaluations of ONE path between two marker prints -- the process to put
        under `rocprofv3 --kernel-trace --stats` (and, in a run of its own, `--memory-copy-trace`) to count
        kernel launches and device-to-host copies per evaluation batch (tools/eval_trace_counts.py).

The reference trainer evaluates outside autocast, i.e. in fp32; --precision bf16 forces the bf16 executor."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--synthetic-train", type=int, default=50000)
    ap.add_argument("--precision", choices=["fp32", "bf16"], default="fp32")
    ap.add_argument("--only", choices=["default", "fused"], default=None)
    ap.add_argument("--evals", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()

    import torch

    import dtc_import

    dtc = dtc_import.load()
    tmp = tempfile.mkdtemp(prefix="eval_bench_")
    base = ["--device-data", "--synthetic-train", str(a.synthetic_train), "--synthetic-test", "256",
            "--batch-size", str(a.batch_size), "--ckpt-path", tmp]
    trainers = {}
    state = None
    for name, extra in (("default", []), ("fused", ["--fused-eval"])):
        if a.only and name != a.only:
            continue
        dtc.data.fix_seed(42)  # as trainer._run: the train / validation split is drawn from numpy's global RNG
        t = dtc.trainer.Trainer(dtc.trainer.load_config(base + extra, "single"), dtc.ResNet18(), None)
        if state is None:
            state = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
        t.model.load_state_dict(state)
        if a.precision == "bf16":
            t.model.precision = "bf16"
        trainers[name] = t
    nb = len(next(iter(trainers.values())).val_loader)

    def run(t):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = t.validate(0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    if a.only:
        t = trainers[a.only]
        for _ in range(a.warmup):
            run(t)
        print(f"EVAL_BENCH_BEGIN path={a.only} evals={a.evals} batches_per_eval={nb}", flush=True)
        for _ in range(a.evals):
            ms, r = run(t)
        print(f"EVAL_BENCH_END ms_last={ms:.3f} result={r}", flush=True)
        return
    for _ in range(a.warmup):
        for t in trainers.values():
            run(t)
    times = {k: [] for k in trainers}
    results = {}
    for _ in range(a.reps):
        for k, t in trainers.items():  # alternate the two paths
            ms, results[k] = run(t)
            times[k].append(ms)
    line = {"what": "Trainer.validate() over the validation split, ms per evaluation", "precision": a.precision,
            "batch_size": a.batch_size, "batches": nb, "reps": a.reps,
            "equal_results": results["default"] == results["fused"], "results": results}
    for k, v in times.items():
        line[k] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                   "all_ms": [round(x, 3) for x in v]}
    line["fused_over_default"] = line["fused"]["median_ms"] / line["default"]["median_ms"]
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
