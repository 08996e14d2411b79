"""Optimizer-stage timing: adam_flat and lars_flat against sgd_nesterov, grad_norm_clip against amp_check_finite,
and the training step with AdamW + clip and with LARS against SGD.

    python tools/optim_bench.py [--reps 20] [--inner 20] [--steps 40] [--batch 256] [--sam] [--out FILE]

Kernels: the model's own flat buffers (11.22 M parameters + slot padding). After a warm-up of every kernel,
each repetition times `inner` back-to-back launches of one kernel between two device events, and the
repetitions of the kernels of a pair ALTERNATE, so both see the same machine state. Bytes per element by the
algorithm: sgd 5 x 4 + 2 = 22 B, adam 7 x 4 + 2 = 30 B, lars sgd's 22 B + the norm pass's 8 B = 30 B, seg_norms
(lars_flat's first two launches on their own: the norm pass over p and g and the ratios) 8 B, the two read passes
4 B. adam_flat's time includes its one-thread tick launch, lars_flat's all three of its launches, grad_norm_clip's
its finalize launch (what a step pays).

Step: bench.py's single-GPU loop body (autocast forward + CrossEntropy, scaler.scale(loss).backward(),
scaler.step, scaler.update, loss.item()) at batch 256, bf16, with SGD, with AdamW + unscale_ + clip_grad_norm_
and with LARS (the SGD arm's hyper-parameters plus the trust ratio), `steps` steps each in alternating blocks.

--sam runs the SAM arms instead, by the same method: sam_perturb (its three launches; plain 4 B norm pass + 18 B
update = 22 B, adaptive 8 + 18 = 26 B) and sam_restore (10 B), both with the model's two keep ranges, alternating
with sgd_nesterov; and the step with SAM(SGD, rho 0.05) -- two forward / backward passes -- against plain SGD. The
perturb arms run at rho = 1e-6 (the time does not depend on rho; back-to-back perturbs without a restore then leave
the weights where they were to six digits).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "all_ms": [round(x, 5) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=3, help="alternating blocks of --steps steps per optimizer")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--sam", action="store_true", help="the SAM perturb / restore and two-pass step arms instead")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()

    import torch

    import dtc_import

    dtc = dtc_import.load()
    ops = dtc.ops
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = dtc.ResNet18().to(dev)
    flat = model.flat
    n, nparam = flat.params.numel(), sum(p.numel for p in flat.layout.params)
    flat.grads.normal_(0, 1e-2)
    mom, m, v = (torch.zeros_like(flat.params) for _ in range(3))
    state = ops.adam_state(dev)
    found = torch.zeros(1, dtype=torch.int32, device=dev)
    inv = torch.ones(1, device=dev)
    ws = ops.grad_norm_workspace(n, dev)
    tn, gm = torch.empty(1, device=dev), torch.empty(1, device=dev)
    plan = ops.seg_plan(flat.layout, dev)
    seg_out = torch.empty(plan.nseg, 3, device=dev)

    kernels = {
        "sgd_nesterov": (lambda: ops.sgd_nesterov_flat(flat.params, flat.grads, mom, flat.params_bf16, 1e-3, 1e-4, 0.9,
                                                       inv, found), 22),
        "adam_flat": (lambda: ops.adam_flat(flat.params, flat.grads, m, v, flat.params_bf16, state, 1e-3, 0.9, 0.999,
                                            1e-8, 1e-2, True, inv, found), 30),
        "lars_flat": (lambda: ops.lars_flat(plan, flat.params, flat.grads, mom, flat.params_bf16, 1e-3, 1e-4, 0.9, True,
                                            1e-3, 1e-8, False, inv, found, seg_out), 30),
        "seg_norms": (lambda: ops.seg_norms(plan, flat.params, flat.grads, inv, seg_out), 8),
        "amp_check_finite": (lambda: ops.amp_check_finite(flat.grads, found), 4),
        "grad_norm_clip": (lambda: ops.grad_norm_clip(flat.grads, 1.0, inv, ws, tn, gm), 4),
    }
    sets = (("sgd_nesterov", "adam_flat", "lars_flat", "seg_norms"), ("amp_check_finite", "grad_norm_clip"))
    if a.sam:
        saved, sam_state, sam_ws = torch.empty_like(flat.params), ops.sam_state(dev), ops.sam_workspace(n, dev)
        keep = [(flat.bufs, torch.empty_like(flat.bufs)), (flat.nbt, torch.empty_like(flat.nbt))]

        def perturb(adaptive):
            return lambda: ops.sam_perturb(flat.params, flat.grads, saved, flat.params_bf16, sam_state, 1e-6,
                                           adaptive, 1e-12, inv, keep, sam_ws)

        kernels = {"sgd_nesterov": kernels["sgd_nesterov"], "sam_perturb": (perturb(False), 22),
                   "sam_perturb_adaptive": (perturb(True), 26),
                   "sam_restore": (lambda: ops.sam_restore(flat.params, saved, flat.params_bf16, sam_state, keep,
                                                           found), 10)}
        sets = (tuple(kernels),)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for fn, _ in kernels.values():  # warm-up: code objects loaded, buffers touched
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in kernels}
    for pair in sets:
        for _ in range(a.reps):
            for k in pair:
                times[k].append(timed(kernels[k][0]))
    line = {"what": "optimizer-stage kernels over the model's flat buffers, ms per call (device events)",
            "flat_numel": n, "parameters": nparam, "reps": a.reps, "inner": a.inner, "kernels": {}}
    for k, (_, bpe) in kernels.items():
        s = _stats(times[k])
        s["bytes_per_element"] = bpe
        s["bytes"] = bpe * n
        s["TBps_median"] = bpe * n / (s["median_ms"] * 1e-3) / 1e12
        s["TBps_best"] = bpe * n / (s["min_ms"] * 1e-3) / 1e12
        line["kernels"][k] = s
    ks = line["kernels"]
    if a.sam:
        line["sam_pair_over_sgd_time"] = ((ks["sam_perturb"]["median_ms"] + ks["sam_restore"]["median_ms"]) /
                                          ks["sgd_nesterov"]["median_ms"])
    else:
        line["adam_over_sgd_bandwidth"] = ks["adam_flat"]["TBps_median"] / ks["sgd_nesterov"]["TBps_median"]
        line["lars_over_sgd_bandwidth"] = ks["lars_flat"]["TBps_median"] / ks["sgd_nesterov"]["TBps_median"]
        line["lars_over_adam_time"] = ks["lars_flat"]["median_ms"] / ks["adam_flat"]["median_ms"]
        line["norm_over_check_bandwidth"] = (ks["grad_norm_clip"]["TBps_median"] /
                                             ks["amp_check_finite"]["TBps_median"])

    if not a.no_step:
        del model, flat, mom, m, v, plan, kernels
        templates = dtc.data.class_templates(100, 32, 32)
        pool = [tuple(t.contiguous() for t in dtc.data.synthetic_batch(i, a.batch, 32, 32, 100, dev, templates))
                for i in range(4)]
        crit = dtc.CrossEntropyLoss()
        runs = {}
        for name in (("sgd", "sam") if a.sam else ("sgd", "adamw_clip", "lars")):
            torch.manual_seed(42)
            net = dtc.ResNet18().to(dev)
            if name in ("sgd", "sam"):
                opt = dtc.SGD(net.parameters(), lr=0.1, weight_decay=1e-4, momentum=0.9, nesterov=True)
                if name == "sam":
                    opt = dtc.SAM(opt, rho=0.05)
            elif name == "lars":
                opt = dtc.LARS(net.parameters(), lr=0.1, weight_decay=1e-4, momentum=0.9, nesterov=True)
            else:
                opt = dtc.AdamW(net.parameters(), lr=1e-3, weight_decay=1e-2)
            runs[name] = (net, opt, dtc.GradScaler())

        def step(name, i):
            net, opt, scaler = runs[name]
            img, label = pool[i % len(pool)]
            opt.zero_grad()
            with dtc.autocast():
                loss = crit(net(img), label)
            if name == "sam":  # the first pass: this model's own gradient, then w + e and the same batch again
                with net.local_grads():
                    scaler.scale(loss).backward()
                opt.first_step(scaler)
                with dtc.autocast():
                    second = crit(net(img), label)
                scaler.scale(second).backward()
            else:
                scaler.scale(loss).backward()
            if name == "adamw_clip":
                scaler.unscale_(opt)
                dtc.clip_grad_norm_(net.parameters(), 1.0, scaler=scaler)
            scaler.step(opt)
            scaler.update()
            return loss.item()

        for name in runs:
            for i in range(10):
                step(name, i)
        step_ms = {k: [] for k in runs}
        last = {}
        for _ in range(a.blocks):
            for name in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    last[name] = step(name, i)
                torch.cuda.synchronize()
                step_ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        line["step"] = {"what": f"training step, batch {a.batch}, 32x32, bf16 + GradScaler, ms per step (host clock "
                                f"around {a.steps} steps ending in a device synchronise)",
                        "last_loss": last, **{k: _stats(v) for k, v in step_ms.items()}}
        for name in runs:
            if name != "sgd":
                line["step"][f"{name}_over_sgd"] = line["step"][name]["median_ms"] / line["step"]["sgd"]["median_ms"]
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
