"""Time the fp32 3x3 stride-1 convs of ResNet-18 (forward, data gradient and weight gradient) on the exact kernel
(conv_f32, algo 0) and on the split-bf16 kernels (conv_f32x / conv_f32x_wgrad, algo 1), interleaved in one process;
then the transition blocks' conv1 + shortcut pair (fwd_sc / dgrad_sc: two conv_f32 launches against conv_f32x_s2;
wgrad_sc: the two conv_f32 weight gradients against the one conv_f32x_s2_wgrad launch, its reduces included).
--gen-cases: the same three passes at the 224x224 model's rows (g1 .. g4: 224 / 112 / 56 / 28 wide), which the split
kernels serve on their general (row-segment) tiles and steps under option f32x_gen.

As tools/conv_bench.py: each (layer, pass, algo) is captured ITERS times into a graph on preallocated buffers (raw
C-ABI calls), so a replay measures device time only; ROUNDS interleaved rounds per case. Prints the median us, the
spread over the rounds (min .. max), TF/s of the algorithmic 2 N H W C 9 K FLOPs and the exact / split ratio."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dtc_import  # noqa: E402

LAYERS = [("l1", 32, 64), ("l2", 16, 128), ("l3", 8, 256), ("l4", 4, 512)]  # (name, H = W, C = K)
GEN_LAYERS = [("g1", 224, 64), ("g2", 112, 128), ("g3", 56, 256), ("g4", 28, 512),  # the 224x224 model's layers 1-4
              ("g5", 14, 512), ("g6", 7, 512)]  # (not in the default cases) narrower rows: 98 and 49 of a tile's 128 slots
TRANSITIONS = [("t2", 32, 64, 128), ("t3", 16, 128, 256), ("t4", 8, 256, 512)]  # (name, H = W in, C, K): layers 2-4, block 0


def time_interleaved(fns, iters, rounds):
    """us per call of each fn: `iters` calls captured into a graph, `rounds` interleaved rounds of one timed replay."""
    us = {a: [] for a in fns}
    for _ in range(rounds):
        for algo, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    for _ in range(iters):
                        fn()
            g.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            us[algo].append(e0.elapsed_time(e1) * 1e3 / iters)
            del g
    return us


def report(label, pname, us, flops, note=""):
    m = {a: statistics.median(v) for a, v in us.items()}
    cell = {a: f"{m[a]:8.1f} ({min(us[a]):.1f}..{max(us[a]):.1f})" for a in us}
    print(f"{label:10s} {pname:8s} {cell[0]:>26s} {flops / m[0] / 1e6:6.1f} {cell[1]:>26s} "
          f"{flops / m[1] / 1e6:6.1f} {m[0] / m[1]:11.2f}{note}", flush=True)


def transition_cases(dtc, cases, iters, rounds, passes=(("fwd_sc", 0), ("dgrad_sc", 1))):
    """conv1 (3x3 stride 2) + the 1x1 stride-2 shortcut of a transition block: algo 0 is the exact pair (two conv_f32
    launches per call, what the executor pays), algo 1 the one conv_f32x_s2 / conv_f32x_s2_wgrad launch (wgrad_sc: each
    side on the workspace its size query asks for)."""
    ops, nat = dtc.ops, dtc._native
    dev, P_ = torch.device("cuda:0"), nat.ptr
    geo = {n: (h, c, k) for n, h, c, k in TRANSITIONS}
    for case in cases.split(","):
        name, B = case.split(":")[0], int(case.split(":")[1])
        H, C, K = geo[name]
        x = torch.randn(B, H, H, C, device=dev)
        dy, dsc = torch.randn(B, H // 2, H // 2, K, device=dev), torch.randn(B, H // 2, H // 2, K, device=dev)
        w, wsc = torch.randn(K, 3, 3, C, device=dev) * 0.05, torch.randn(K, C, device=dev) * 0.1
        wts = {0: (w, wsc), 1: (ops.f32_split3(w), ops.f32_split3(wsc))}
        y, ysc, dx = torch.empty_like(dy), torch.empty_like(dy), torch.empty_like(x)
        st, st_sc = ops.new_stats(K, dev), ops.new_stats(K, dev)
        d = ops.conv_desc(B, H, H, C, K, 3, 3, 2, 1)
        flops = 2.0 * B * (H // 2) ** 2 * C * 10 * K
        dw, dwsc = torch.empty(K, 3, 3, C, device=dev), torch.empty(K, C, device=dev)
        wsz = {a: int(nat.lib.dtc_conv2d_f32_wgrad_sc_workspace_size(d, a)) for a in (0, 1)}
        nat.call("dtc_set_option", b"f32x_s2_wgrad", 2)  # (the buffer holds the fused kernel's slab where it is refused too)
        ws = torch.empty(max(wsz[0], int(nat.lib.dtc_conv2d_f32_wgrad_sc_workspace_size(d, 1)), 16), dtype=torch.uint8,
                         device=dev)
        nat.call("dtc_set_option", b"f32x_s2_wgrad", 1)
        for pname, mode in passes:
            note = ""
            if mode == 2:
                if ops.conv2d_f32_wgrad_sc_route(d, 1) != "split":  # refused by default: timed with the predicate opened
                    nat.call("dtc_set_option", b"f32x_s2_wgrad", 2)
                    note = "  (refused by default)"
                assert ops.conv2d_f32_wgrad_sc_route(d, 1) == "split", case
                wsz[1] = int(nat.lib.dtc_conv2d_f32_wgrad_sc_workspace_size(d, 1))
                fns = {algo: lambda algo=algo: nat.call(
                    "dtc_conv2d_f32_wgrad_sc", d, P_(x), P_(dy), P_(dsc), P_(dw), P_(dwsc), 1.0, algo,
                    P_(ws) if wsz[algo] else None, wsz[algo], nat.stream_ptr()) for algo in (0, 1)}
                report(f"{name} B={B}", pname, time_interleaved(fns, iters, rounds), flops, note)
                nat.call("dtc_set_option", b"f32x_s2_wgrad", 1)
                continue
            if ops.conv2d_f32_sc_route(d, mode, 1) != "split":  # refused by default: timed with the predicate opened
                nat.call("dtc_set_option", b"f32x_s2_fwd", 2)
                note = "  (refused by default)"
            assert ops.conv2d_f32_sc_route(d, mode, 1) == "split", case
            fns = {}
            for algo, (wt, wsct) in wts.items():
                if mode == 0:
                    fns[algo] = lambda algo=algo, wt=wt, wsct=wsct: nat.call(
                        "dtc_conv2d_f32_fwd_sc", d, P_(x), P_(wt), P_(y), P_(st), P_(wsct), P_(ysc), P_(st_sc), algo,
                        nat.stream_ptr())
                else:
                    fns[algo] = lambda algo=algo, wt=wt, wsct=wsct: nat.call(
                        "dtc_conv2d_f32_dgrad_sc", d, P_(dy), P_(wt), P_(dx), P_(dsc), P_(wsct), algo, nat.stream_ptr())
            report(f"{name} B={B}", pname, time_interleaved(fns, iters, rounds), flops, note)
            nat.call("dtc_set_option", b"f32x_s2_fwd", 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="l1:256,l2:256,l3:256,l4:256,l3:32,l4:32", help="layer:batch, ...; empty: none")
    ap.add_argument("--sc-cases", default="t2:256,t3:256,t4:256,t2:32,t3:32,t4:32",
                    help="transition blocks (conv1 + shortcut in one call), name:batch, ...; empty: none")
    ap.add_argument("--wgrad-sc-cases", default=",".join(f"t{l}:{b}" for b in (256, 128, 64, 32) for l in (2, 3, 4)),
                    help="transition blocks' fused weight gradients (wgrad_sc rows), name:batch, ...; empty: none")
    ap.add_argument("--gen-cases", default=",".join(f"g{l}:{b}" for b in (32, 128) for l in (1, 2, 3, 4)),
                    help="general-geometry rows (all three passes under option f32x_gen), name:batch, ...; empty: none")
    ap.add_argument("--passes", default="", help="of fwd,dgrad,wgrad for --cases / --gen-cases; empty: all")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    dtc = dtc_import.load()
    ops, nat = dtc.ops, dtc._native
    dev = torch.device("cuda:0")
    geo = {n: (h, c) for n, h, c in LAYERS + GEN_LAYERS}
    print(f"{'case':10s} {'pass':8s} {'exact us (min..max)':>26s} {'TF/s':>6s} {'split us (min..max)':>26s} {'TF/s':>6s} "
          f"{'exact/split':>11s}")
    for case in filter(None, (args.cases + "," + args.gen_cases).split(",")):
        name, B = case.split(":")[0], int(case.split(":")[1])
        H, C = geo[name]
        gen, refused = name.startswith("g"), set()
        if gen:  # timed with every feasible general tile admitted; the note says what the default rule (1) does
            nat.call("dtc_set_option", b"f32x_gen", 1)
            d1 = ops.conv_desc(B, H, H, C, C, 3, 3, 1, 1)
            refused = {m for m in (0, 1, 2)
                       if (ops.conv2d_f32_wgrad_route(d1, 1) if m == 2 else ops.conv2d_f32_route(d1, m, 1)) != "split"}
            nat.call("dtc_set_option", b"f32x_gen", 2)
        x = torch.randn(B, H, H, C, device=dev)
        w = torch.randn(C, 3, 3, C, device=dev) * 0.05
        wpl = ops.f32_split3(w)
        out = torch.empty(B, H, H, C, device=dev)
        stats = ops.new_stats(C, dev)
        d = ops.conv_desc(B, H, H, C, C, 3, 3, 1, 1)
        flops = 2.0 * B * H * H * C * 9 * C
        P_ = nat.ptr
        dw = torch.empty(C, 3, 3, C, device=dev)
        wsz = {a: int(nat.lib.dtc_conv2d_f32_wgrad_workspace_size(d, a)) for a in (0, 1)}
        ws = torch.empty(max(wsz.values()), dtype=torch.uint8, device=dev)
        for pname, mode in (("fwd", 0), ("dgrad", 1), ("wgrad", 2)):
            if args.passes and pname not in args.passes.split(","):
                continue
            note = "  (refused at f32x_gen = 1)" if mode in refused else ""
            assert (ops.conv2d_f32_wgrad_route(d, 1) if mode == 2 else ops.conv2d_f32_route(d, mode, 1)) == "split", case
            fns = {}
            for algo, wt in ((0, w), (1, wpl)):
                if mode == 2:  # x against a dy of the same shape (C = K), each kernel on the slab its size query asks for
                    fns[algo] = lambda algo=algo: nat.call("dtc_conv2d_f32_wgrad", d, P_(x), P_(out), P_(dw), 1.0, algo,
                                                           P_(ws), wsz[algo], nat.stream_ptr())
                elif mode == 0:
                    fns[algo] = lambda algo=algo, wt=wt: nat.call("dtc_conv2d_f32_fwd", d, P_(x), P_(wt), P_(out),
                                                                  P_(stats), algo, None, 0, nat.stream_ptr())
                else:
                    fns[algo] = lambda algo=algo, wt=wt: nat.call("dtc_conv2d_f32_dgrad", d, P_(x), P_(wt), P_(out),
                                                                  None, algo, None, 0, nat.stream_ptr())
            us = time_interleaved(fns, args.iters, args.rounds)
            report(f"{name} B={B}", pname, us, flops, note)
        nat.call("dtc_set_option", b"f32x_gen", 0)
        del x, w, wpl, out, dw, ws
    if args.sc_cases:
        transition_cases(dtc, args.sc_cases, args.iters, args.rounds)
    if args.wgrad_sc_cases:
        transition_cases(dtc, args.wgrad_sc_cases, args.iters, args.rounds, (("wgrad_sc", 2),))


if __name__ == "__main__":
    main()
