"""Throughput of the on-device CIFAR pipeline kernel (ops.cifar_augment) against HBM peak, and
of the DeviceLoader feeding the native training step. Prints one JSON line.

Algorithmic bytes per image: h*w*3 (uint8 read) + 3*h*w*4 (fp32 write) + 8 (index) + 2 (crop)
+ 1 (flip) + 8 (label read) + 8 (label write) = 15,395 B at 32x32.

Beside the plain launch: the policy launch (ops.cifar_augment_policy, RandAugment draws with two ops per image
at magnitude 9 and RandomErasing 0.25) and the policy launch writing uint8 followed by the CutMix launch, as the
DeviceLoader composes them; and the loader with the policy on against resident input."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dtc_import  # noqa: E402

HBM_PEAK_GBS = 8000.0


def timed_us(fn, iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    dtc = dtc_import.load()
    dev = torch.device("cuda:0")
    imgs, tg = dtc.data.synthetic_cifar_u8()
    images = torch.from_numpy(imgs).to(dev)
    targets = torch.from_numpy(tg).to(dev)
    res, pol_res = {}, {}
    for B in (256, 4096, 45000):
        idx = torch.randint(0, images.shape[0], (B,), device=dev)
        crop = torch.randint(0, 9, (B, 2), dtype=torch.uint8, device=dev)
        flip = torch.randint(0, 2, (B,), dtype=torch.uint8, device=dev)
        out = torch.empty(B, 3, 32, 32, device=dev)
        lab = torch.empty(B, dtype=torch.int64, device=dev)
        args = (images, idx, crop, flip, dtc.data.CIFAR_MEAN, dtc.data.CIFAR_STD, 4)
        iters = 200 if B < 10000 else 40
        us = timed_us(lambda: dtc.ops.cifar_augment(*args, targets=targets, out=out, labels=lab), iters)
        gbs = B * 15395 / (us * 1e-6) / 1e9
        res[str(B)] = {"us_per_launch": round(us, 2), "GB_s": round(gbs, 1), "frac_hbm": round(gbs / HBM_PEAK_GBS, 4),
                       "images_per_s": round(B / (us * 1e-6))}
        if B > 4096:
            continue
        rng = np.random.default_rng(B)
        pol = dtc.data.policy_params(1, B, 32, 32, "randaugment", 2, 9, rng)
        p_ops, p_args = torch.from_numpy(pol.ops[0]).to(dev), torch.from_numpy(pol.args[0]).to(dev)
        erase = torch.from_numpy(dtc.data.erase_params(1, B, 32, 32, 0.25, rng)[0]).to(dev)
        mix = dtc.data.mix_params(1, B, 32, 32, 0.0, 1.0, 1.0, rng)
        box = torch.from_numpy(mix.box[0]).to(dev)
        u8 = torch.empty(B, 32, 32, 3, dtype=torch.uint8, device=dev)
        lab_b = torch.empty(B, dtype=torch.int64, device=dev)

        def policy():
            dtc.ops.cifar_augment_policy(*args, targets=targets, ops=p_ops, args=p_args, erase=erase, out=out,
                                         labels=lab)

        def policy_then_mix():
            dtc.ops.cifar_augment_policy(*args, targets=targets, ops=p_ops, args=p_args, to_u8=True, out=u8, labels=lab)
            dtc.ops.cifar_augment_mix(u8, None, None, None, *args[4:], targets=lab, mode=2, box=box, out=out,
                                      labels=lab, labels_b=lab_b)

        us_p, us_pm = timed_us(policy, iters), timed_us(policy_then_mix, iters)
        pol_res[str(B)] = {"policy_n_ops_2_us": round(us_p, 2), "policy_then_mix_us": round(us_pm, 2),
                           "policy_over_plain": round(us_p / us, 2)}
    # DeviceLoader feeding the native train step (batch 256), vs resident synthetic input
    torch.manual_seed(42)
    model = dtc.ResNet18().to(dev)
    crit = dtc.CrossEntropyLoss()
    opt = dtc.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    loader = dtc.data.DeviceLoader(imgs, tg, 256, device=dev)
    pol_loader = dtc.data.DeviceLoader(imgs, tg, 256, device=dev, policy="randaugment", erase_prob=0.25)

    def run(batches):
        n = 0
        for x, y in batches:
            opt.zero_grad()
            loss = crit(model(x), y)
            loss.backward()
            opt.step()
            n += x.shape[0]
        return n

    def rate(batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = run(batches)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    run(b for _, b in zip(range(5), loader))
    fed = rate(b for _, b in zip(range(60), loader))
    x0, y0 = next(iter(loader))
    resident = rate((x0, y0) for _ in range(60))
    run(b for _, b in zip(range(5), pol_loader))
    pol_fed = rate(b for _, b in zip(range(60), pol_loader))
    resident2 = rate((x0, y0) for _ in range(60))
    print(json.dumps({"kernel": "cifar_augment", "bytes_per_image": 15395, "peak_GB_s": HBM_PEAK_GBS, "by_batch": res,
                      "train_step_images_per_s": {"device_loader": round(fed, 1), "resident": round(resident, 1)},
                      "policy_by_batch": pol_res,
                      "policy_train_step_images_per_s": {"device_loader": round(pol_fed, 1),
                                                         "resident": round(resident2, 1)}}),
          flush=True)


if __name__ == "__main__":
    main()
