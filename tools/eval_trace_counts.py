"""Launches and device-to-host copies per evaluation batch from a rocprofv3 trace of tools/eval_bench.py --only.

usage: python tools/eval_trace_counts.py <rocprof output dir> <evaluation batches in the run> <out.md> [title]

Reads *kernel_trace.csv (and *memory_copy_trace.csv when the run had --memory-copy-trace) under the directory.
The batch count is (warmup + evals) x batches_per_eval of the traced process; the trainer's construction
(parameter upload, dataset upload) adds a few launches and copies that are not evaluation work, so kernels that
run once per batch show as 1.00 and set-up work as a small fraction."""
import csv
import glob
import os
import sys
from collections import Counter


def short(name):
    n = name.replace("void ", "").split("(")[0]
    return n if len(n) <= 90 else n[:87] + "..."


def main():
    src, batches, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    title = sys.argv[4] if len(sys.argv) > 4 else os.path.basename(os.path.normpath(src))
    kt = glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True)
    assert kt, f"no kernel_trace.csv under {src}"
    kernels, dur = Counter(), Counter()
    with open(kt[0]) as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            kernels[k] += 1
            dur[k] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    lines = [f"# Evaluation launch counts: {title}", "",
             f"{batches} evaluation batches in the traced process; {sum(kernels.values())} kernel launches = "
             f"{sum(kernels.values()) / batches:.2f} per batch.", "",
             "| kernel | launches | per batch | avg us |", "|---|---|---|---|"]
    for k, c in sorted(kernels.items(), key=lambda kv: (-kv[1], kv[0])):
        lines.append(f"| `{k}` | {c} | {c / batches:.2f} | {dur[k] / c / 1e3:.2f} |")
    mc = glob.glob(os.path.join(src, "**", "*memory_copy_trace.csv"), recursive=True)
    if mc:
        dirs = Counter()
        with open(mc[0]) as f:
            for r in csv.DictReader(f):
                dirs[r.get("Direction", "?")] += 1
        lines += ["", "| memory copy direction | copies | per batch |", "|---|---|---|"]
        for d, c in sorted(dirs.items()):
            lines.append(f"| {d} | {c} | {c / batches:.2f} |")
    else:
        lines += ["", "(no memory-copy trace in this run)"]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
