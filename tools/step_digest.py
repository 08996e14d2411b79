#!/usr/bin/env python3
"""Digests of two training steps of the native ResNet-18 under every option the executor branches on.

For each configuration: two steps (forward, loss, backward, Nesterov SGD) at batch 8, 32x32, fixed seeds; one
line per step with the SHA-256 of logits, flat gradients, flat parameters and the running-statistics buffers
(and of the capture slots where parity capture is on), then the dtc:: kernels of a step: the launch count per
kernel name, and the names in launch order per stream (torch.profiler, from the second step on; a trace now and
then loses events, so the ordered list is marked UNCONFIRMED unless two steps gave it). The step is bit-reproducible, so two builds of the library run the same
step if and only if their outputs are equal line for line:

    python tools/step_digest.py > new.txt
    DTC_LIB=/path/to/other/libdtc_amd.so python tools/step_digest.py > old.txt
    cmp old.txt new.txt

`--only SUBSTRING` runs the configurations whose name contains it; `--list` prints the names.
"""
import argparse
import collections
import ctypes as C
import hashlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dtc_import  # noqa: E402

dtc = dtc_import.load()
lib = dtc._native.lib
DEV = torch.device("cuda:0")


def sha(t):
    a = t.detach().contiguous().cpu()
    if a.dtype == torch.bfloat16:
        a = a.view(torch.int16)
    return hashlib.sha256(a.numpy().tobytes()).hexdigest()[:20]


class Options:
    """Library options for one configuration; every one is restored on exit."""

    def __init__(self, opts):
        self.opts, self.saved = opts, {}

    def __enter__(self):
        for k, v in self.opts.items():
            key = k.encode()
            self.saved[key] = lib.dtc_get_option(key)
            dtc._native.call("dtc_set_option", key, int(v))

    def __exit__(self, *exc):
        for key, v in self.saved.items():
            lib.dtc_set_option(key, v)


def kernels_of(fn):
    """The dtc:: kernels fn launches, in start order within each stream; streams ordered by their sequences
    (stream numbers and the interleaving across streams depend on timing, the per-stream order does not)."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    streams = {}
    for e in prof.profiler.kineto_results.events():
        if "CUDA" not in str(e.device_type()) or "dtc::" not in e.name():
            continue
        start = e.start_ns() if hasattr(e, "start_ns") else e.start_us()
        streams.setdefault(e.device_resource_id(), []).append((start, e.name()))
    return sorted([name.split("(")[0] for _, name in sorted(v)] for v in streams.values())


def data(batch):
    g = np.random.default_rng(11)
    x = torch.from_numpy(g.standard_normal((batch, 3, 32, 32)).astype(np.float32)).to(DEV)
    ya, yb = g.integers(0, 100, batch), g.integers(0, 100, batch)
    lam = g.random(batch).astype(np.float32)
    lam[0], lam[1] = 1.0, 0.0
    return x, torch.from_numpy(ya).to(DEV), torch.from_numpy(yb).to(DEV), torch.from_numpy(lam).to(DEV)


def make_model(precision="bf16", capture=False, cap_mb=None):
    torch.manual_seed(42)
    model = dtc.ResNet18().to(DEV)
    model.precision = precision
    if capture:
        model.enable_capture(True)
    if cap_mb is not None:
        model.set_bucket_cap_mb(cap_mb)
    return model


def train_config(name, batch=8, precision="bf16", capture=False, soft=False, sync=False, comm=False):
    model = make_model(precision, capture, 1.0 if comm else None)
    x, ya, yb, lam = data(batch)
    crit = dtc.CrossEntropyLoss(label_smoothing=0.1) if soft else dtc.CrossEntropyLoss()
    target = dtc.MixedTarget(ya, yb, lam) if soft else ya
    opt = dtc.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    comms = []
    if sync:
        comms.append(dtc.parallel.Comm.loopback(0, 1.0, world=1))
        dtc.SyncBatchNorm.convert_sync_batchnorm(model)
        model.set_sync_bn(comms[-1])
    if comm:
        comms.append(dtc.parallel.Comm.loopback(0, 2.0))
        model._comm, model._grad_scale = comms[-1], 0.5
    out = {}

    def step():
        logits = model(x)
        crit(logits, target).backward()
        opt.step()
        out["logits"] = logits

    try:
        for k in range(2):
            if k == 1:
                seqs = kernels_of(step)
            else:
                step()
            torch.cuda.synchronize()
            flat = model.flat
            line = (f"{name} | step {k} | logits={sha(out['logits'])} grads={sha(flat.grads)} "
                    f"params={sha(flat.params)} bufs={sha(flat.bufs)} nbt={sha(flat.nbt)}")
            if capture:
                caps = model.executor(batch, 32, 32, precision).activations(captures=True)
                h = hashlib.sha256()
                for nm in sorted(caps):
                    h.update(nm.encode() + sha(caps[nm]).encode())
                line += f" captures[{len(caps)}]={h.hexdigest()[:20]}"
            print(line, flush=True)
        # The profiler loses events of a trace now and then, more often the more kernels a step has. The ordered
        # list is the longest capture of up to 10 steps, confirmed once a second capture equals it; the launch
        # count per kernel name is the maximum over the captures (a lost event only ever lowers a count).
        caps, confirmed = [seqs], False
        while len(caps) < 10 and not confirmed:
            caps.append(kernels_of(step))
            best = max(caps, key=lambda s: sum(map(len, s)))
            confirmed = caps.count(best) >= 2
        counts = {}
        for s in caps:
            for nm, c in collections.Counter(k for seq in s for k in seq).items():
                counts[nm] = max(counts.get(nm, 0), c)
        print(f"{name} | kernel counts | {json.dumps(counts, sort_keys=True)}", flush=True)
        print(f"{name} | kernels {'confirmed' if confirmed else 'UNCONFIRMED'} | {json.dumps(best)}", flush=True)
    finally:
        if sync:
            model.set_sync_bn(None)
        model._comm, model._grad_scale = None, 1.0
        torch.cuda.synchronize()
        del model
        for c in comms:
            c.close()


def eval_config(name):
    model = make_model()
    x, ya, _, _ = data(8)
    exe = model.executor(8, 32, 32, "bf16")
    other = types.SimpleNamespace(params=model.flat.params * 1.5, bufs=model.flat.bufs.clone() + 0.25,
                                  params_bf16=torch.empty_like(model.flat.params_bf16))
    dtc.ops.cast_f32_bf16(other.params, other.params_bf16)
    for tag, weights in (("eval_batch", None), ("eval_batch_weights", other)):
        rec = torch.zeros(4, dtype=torch.int32, device=DEV)
        logits = torch.zeros(8, 100, dtype=torch.float32, device=DEV)
        exe.eval_batch(x, ya, 5, 5, rec, logits, weights=weights)
        torch.cuda.synchronize()
        print(f"{name} | {tag} | logits={sha(logits)} record={rec.cpu().tolist()} bufs={sha(model.flat.bufs)}", flush=True)


def profiled_config(name):
    model = make_model()
    x, ya, _, _ = data(8)
    crit = dtc.CrossEntropyLoss()
    crit(model(x), ya).backward()
    exe = model.executor(8, 32, 32, "bf16")
    dtc._native.call("dtc_rn18_profile_begin", exe.handle, 1)
    crit(model(x), ya).backward()
    ms, work, cnt = (C.c_double * 4)(), (C.c_double * 4)(), (C.c_int * 4)()
    dtc._native.call("dtc_rn18_profile_end_ex", exe.handle, 4, ms, work, cnt)
    torch.cuda.synchronize()
    print(f"{name} | count_by_kind={list(cnt)} work_by_kind={[float(w).hex() for w in work]} "
          f"grads={sha(model.flat.grads)}", flush=True)


def comm_timed_config(name):
    model = make_model(cap_mb=1.0)
    x, ya, _, _ = data(8)
    crit = dtc.CrossEntropyLoss()
    comm = dtc.parallel.Comm.loopback(0, 2.0)
    model._comm, model._grad_scale = comm, 0.5
    try:
        crit(model(x), ya).backward()
        exe = model.executor(8, 32, 32, "bf16")
        nb = len(model.buckets())
        dtc._native.call("dtc_rn18_comm_timing", exe.handle, 1)
        crit(model(x), ya).backward()
        torch.cuda.synchronize()
        bus, exu, nst = (C.c_double * (3 * nb))(), (C.c_double * 5)(), C.c_int(0)
        dtc._native.call("dtc_rn18_comm_timing_result", exe.handle, nb, bus, exu, C.byref(nst))
        timed = sum(1 for i in range(nb) if bus[3 * i + 1] > 0)
        print(f"{name} | steps={nst.value} joined={int(exu[4])} buckets={nb} buckets_timed={timed} "
              f"grads={sha(model.flat.grads)}", flush=True)
    finally:
        model._comm, model._grad_scale = None, 1.0
        torch.cuda.synchronize()
        del model
        comm.close()


def configs():
    T = train_config
    yield "defaults", {}, T, {}
    yield "batch64", {}, T, {"batch": 64}
    yield "bn_mask=0", {"bn_mask": 0}, T, {}
    yield "unfused", {"bn_fused_fin": 0, "dgrad_scf": 0, "bn_cg": 0, "wgrad_s2": 0}, T, {}
    for opt in ("bn_cg", "stem_direct", "stem_bn_fuse", "sc_fuse", "sc_compact", "bwd_streams", "fork_lazy",
                "xent_fuse"):
        yield f"{opt}=0", {opt: 0}, T, {}
    yield "wgrad_batch=1", {"wgrad_batch": 1}, T, {}
    yield "soft xent_fuse=1", {"xent_fuse": 1}, T, {"soft": True}
    yield "soft xent_fuse=0", {"xent_fuse": 0}, T, {"soft": True}
    yield "fp32", {}, T, {"precision": "fp32"}
    yield "capture bf16", {}, T, {"capture": True}
    yield "capture fp32", {}, T, {"capture": True, "precision": "fp32"}
    for g in (1, 2, 3):
        yield f"graphs={g}", {"graphs": g}, T, {}
    yield "syncbn one rank", {}, T, {"sync": True}
    for g in (0, 1):
        for side in (1, 0):
            yield f"comm 1MB graphs={g} comm_on_side={side}", {"graphs": g, "comm_on_side": side}, T, {"comm": True}
    yield "comm 1MB comm_tail_inline=0", {"comm_tail_inline": 0}, T, {"comm": True}
    yield "eval", {}, eval_config, {}
    yield "profiled step", {}, profiled_config, {}
    yield "comm-timed step", {}, comm_timed_config, {}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--only", default=None)
    ap.add_argument("--list", action="store_true")
    args = ap.parse_args()
    for name, opts, fn, kw in configs():
        if args.list:
            print(name)
            continue
        if args.only is not None and args.only not in name:
            continue
        with Options(opts):
            fn(name, **kw)


if __name__ == "__main__":
    main()
