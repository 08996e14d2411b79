"""Soft-target loss and mixed input launch against their plain counterparts, and the training step with label
smoothing + Mixup + CutMix against the default step.

    python tools/soft_mix_bench.py [--reps 20] [--inner 20] [--steps 40] [--blocks 3] [--batch 256] [--out FILE]

Kernels: after a warm-up of every arm, each repetition times `inner` back-to-back calls of one arm between two
device events, and the repetitions of the arms of a pair ALTERNATE, so both see the same machine state.
  loss      dtc_xent_fwd_ex against dtc_xent_soft_fwd_ex (eps 0.1, labels_b + lam), batch x 100 logits
  backward  the whole eager backward call, dtc_rn18_xent_backward against dtc_rn18_xent_soft_backward: the two
            differ in the head backward kernel's instantiation only (<T, true> against <T, true, true>)
  input     cifar_augment against cifar_augment_mix, Mixup and CutMix, batch x 32 x 32
Step: the single-GPU --amp --device-data loop body (DeviceLoader batch, autocast forward + loss,
scaler.scale(loss).backward(), scaler.step, scaler.update, loss.item()) with the default flags and with
--label-smoothing 0.1 --mixup-alpha 1 --cutmix-alpha 1, `steps` steps each in alternating blocks. One JSON line."""
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
    ap.add_argument("--blocks", type=int, default=3, help="alternating blocks of --steps steps per configuration")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import dtc_import

    dtc = dtc_import.load()
    ops, call = dtc.ops, dtc._native.call
    dev = torch.device("cuda:0")
    B = a.batch
    g = torch.Generator().manual_seed(0)
    z = (torch.randn(B, 100, generator=g) * 3).to(dev)
    ya = torch.randint(0, 100, (B,), generator=g).to(dev)
    yb = torch.randint(0, 100, (B,), generator=g).to(dev)
    lam = torch.rand(B, generator=g).to(dev)
    scale = torch.full((1,), 65536.0, device=dev)
    loss, scaled = torch.empty((), device=dev), torch.empty((), device=dev)
    lse = torch.empty(B, device=dev)
    host = torch.zeros(1).pin_memory()
    st = dtc._native.stream_ptr

    imgs, tg = dtc.data.synthetic_cifar_u8(n=4096, seed=1)
    imgs_d, tg_d = torch.from_numpy(imgs).to(dev), torch.from_numpy(tg).to(dev)
    idx = torch.randint(0, 4096, (B,), generator=g).to(dev)
    crop = torch.randint(0, 9, (B, 2), generator=g, dtype=torch.uint8).to(dev)
    flip = torch.randint(0, 2, (B,), generator=g, dtype=torch.uint8).to(dev)
    box = torch.tensor([[4, 24, 6, 26]], dtype=torch.uint8).repeat(B, 1).to(dev)
    out = torch.empty(B, 3, 32, 32, device=dev)
    la_o, lb_o = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    mean, std = dtc.data.CIFAR_MEAN, dtc.data.CIFAR_STD

    dtc._native.lib.dtc_set_option(b"graphs", 0)  # the fused head backward runs in the eager backward
    torch.manual_seed(0)
    model = dtc.ResNet18().to(dev)
    x = torch.randn(B, 3, 32, 32, device=dev)
    exe = model.executor(B, 32, 32, "bf16")
    logits = torch.empty(B, 100, device=dev)
    exe.forward(x, logits, True)
    ops.xent_soft_fwd(logits, ya, yb, lam, 0.1)
    soft = dtc.nn._Soft(ya, yb, lam, 0.1)
    _, lse_m, _ = ops.xent_soft_fwd(logits, ya, yb, lam, 0.1)

    arms = {
        "xent_fwd_ex": lambda: call("dtc_xent_fwd_ex", z.data_ptr(), ya.data_ptr(), B, 100, loss.data_ptr(),
                                    lse.data_ptr(), scale.data_ptr(), scaled.data_ptr(), host.data_ptr(), st()),
        "xent_soft_fwd_ex": lambda: call("dtc_xent_soft_fwd_ex", z.data_ptr(), ya.data_ptr(), yb.data_ptr(),
                                         lam.data_ptr(), 0.1, B, 100, loss.data_ptr(), lse.data_ptr(),
                                         scale.data_ptr(), scaled.data_ptr(), host.data_ptr(), st()),
        "backward_hard": lambda: exe.xent_backward(logits, ya, lse_m, scale, 1.0, None),
        "backward_soft": lambda: exe.xent_soft_backward(logits, soft, lse_m, scale, 1.0, None),
        "cifar_augment": lambda: ops.cifar_augment(imgs_d, idx, crop, flip, mean, std, 4, targets=tg_d, out=out,
                                                   labels=la_o),
        "cifar_augment_mixup": lambda: ops.cifar_augment_mix(imgs_d, idx, crop, flip, mean, std, 4, targets=tg_d,
                                                             mode=1, lam=lam, out=out, labels=la_o, labels_b=lb_o),
        "cifar_augment_cutmix": lambda: ops.cifar_augment_mix(imgs_d, idx, crop, flip, mean, std, 4, targets=tg_d,
                                                              mode=2, box=box, out=out, labels=la_o, labels_b=lb_o),
    }

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for fn in arms.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for group in (("xent_fwd_ex", "xent_soft_fwd_ex"), ("backward_hard", "backward_soft"),
                  ("cifar_augment", "cifar_augment_mixup", "cifar_augment_cutmix")):
        for _ in range(a.reps):
            for k in group:
                times[k].append(timed(arms[k]))
    ks = {k: _stats(v) for k, v in times.items()}
    line = {"what": "soft-target / mixed-input launches against their plain counterparts, ms per call (device "
                    "events around back-to-back calls)", "batch": B, "reps": a.reps, "inner": a.inner, "kernels": ks,
            "soft_over_hard_loss": ks["xent_soft_fwd_ex"]["median_ms"] / ks["xent_fwd_ex"]["median_ms"],
            "soft_over_hard_backward": ks["backward_soft"]["median_ms"] / ks["backward_hard"]["median_ms"],
            "backward_soft_minus_hard_ms": ks["backward_soft"]["median_ms"] - ks["backward_hard"]["median_ms"],
            "mixup_over_plain_input": ks["cifar_augment_mixup"]["median_ms"] / ks["cifar_augment"]["median_ms"],
            "cutmix_over_plain_input": ks["cifar_augment_cutmix"]["median_ms"] / ks["cifar_augment"]["median_ms"]}
    dtc._native.lib.dtc_set_option(b"graphs", 4)

    if not a.no_step:
        del model, exe
        runs = {}
        for name, eps, kw in (("default", 0.0, {}),
                              ("smooth_mixup_cutmix", 0.1, dict(mixup_alpha=1.0, cutmix_alpha=1.0))):
            torch.manual_seed(42)
            net = dtc.ResNet18().to(dev)
            opt = dtc.SGD(net.parameters(), lr=0.1, weight_decay=1e-4, momentum=0.9, nesterov=True)
            loader = dtc.data.DeviceLoader(imgs, tg, B, device=dev, seed=0, **kw)
            runs[name] = [net, opt, dtc.GradScaler(), dtc.CrossEntropyLoss(label_smoothing=eps), loader, None]

        def batch_of(run):
            while True:
                if run[5] is None:
                    run[5] = iter(run[4])
                try:
                    return next(run[5])
                except StopIteration:
                    run[5] = None

        def step(name):
            run = runs[name]
            net, opt, scaler, crit = run[:4]
            img, label = batch_of(run)
            label = label.to(dev)
            opt.zero_grad()
            with dtc.autocast():
                lo = crit(net(img), label)
            scaler.scale(lo).backward()
            scaler.step(opt)
            scaler.update()
            return lo.item()

        for name in runs:
            for _ in range(12):
                step(name)
        step_ms = {k: [] for k in runs}
        last = {}
        for _ in range(a.blocks):
            for name in runs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    last[name] = step(name)
                torch.cuda.synchronize()
                step_ms[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
        line["step"] = {"what": f"training step fed by a DeviceLoader, batch {B}, 32x32, bf16 + GradScaler, ms per "
                                f"step (host clock around {a.steps} steps ending in a device synchronise)",
                        "last_loss": last, **{k: _stats(v) for k, v in step_ms.items()}}
        line["step"]["soft_over_default"] = (line["step"]["smooth_mixup_cutmix"]["median_ms"] /
                                             line["step"]["default"]["median_ms"])
        assert all(np.isfinite(v) for v in last.values()), last
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
