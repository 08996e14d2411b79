#!/usr/bin/env python3
"""Everything the executor's planner exposes, as sorted JSON, for a fixed list of configurations.

Runs without a GPU (the planner makes no device call). Two builds of the library plan the same if and only
if their dumps are byte-identical:

    python tools/plan_dump.py > new.json
    DTC_LIB=/path/to/other/libdtc_amd.so python tools/plan_dump.py > old.json
    cmp old.json new.json
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dtc_import  # noqa: E402

SHAPES = [(8, 32, 32, 100), (256, 32, 32, 100), (8, 8, 8, 10), (2, 224, 224, 1000), (5, 40, 24, 100)]
MODES = [("bf16", 0, 0), ("fp32", 1, 0), ("bf16+capture", 0, 1), ("fp32+capture", 1, 1)]
CAPS_MB = [1.0, 5.0, 25.0]


def _acts(lib, h, count, info):
    out = []
    for i in range(count(h)):
        name, off, shape = C.c_char_p(), C.c_size_t(), (C.c_int32 * 4)()
        assert info(h, i, C.byref(name), C.byref(off), shape) == 0
        out.append({"name": name.value.decode(), "offset": off.value, "shape": list(shape)})
    return out


def dump_one(nat, batch, height, width, ncls, fp32, capture, cap_mb):
    lib = nat.lib
    h = C.c_void_p()
    nat.call("dtc_rn18_create", C.byref(h), batch, height, width, ncls, cap_mb)
    try:
        if fp32:
            nat.call("dtc_rn18_set_precision", h, 1)
        if capture:
            nat.call("dtc_rn18_enable_capture", h)
        params = []
        for i in range(lib.dtc_rn18_num_params(h)):
            name, off, numel, ndim = C.c_char_p(), C.c_int64(), C.c_int64(), C.c_int32()
            shape, stride = (C.c_int64 * 4)(), (C.c_int64 * 4)()
            nat.call("dtc_rn18_param_info", h, i, C.byref(name), C.byref(off), C.byref(numel), C.byref(ndim), shape,
                     stride)
            params.append({"name": name.value.decode(), "offset": off.value, "numel": numel.value, "ndim": ndim.value,
                           "shape": list(shape), "stride": list(stride)})
        bns = []
        for i in range(lib.dtc_rn18_num_bn(h)):
            prefix, ch, mo, vo = C.c_char_p(), C.c_int32(), C.c_int64(), C.c_int64()
            nat.call("dtc_rn18_bn_info", h, i, C.byref(prefix), C.byref(ch), C.byref(mo), C.byref(vo))
            bns.append({"prefix": prefix.value.decode(), "channels": ch.value, "mean_offset": mo.value,
                        "var_offset": vo.value})
        buckets = []
        for i in range(lib.dtc_rn18_num_buckets(h)):
            off, numel = C.c_int64(), C.c_int64()
            nat.call("dtc_rn18_bucket_info", h, i, C.byref(off), C.byref(numel))
            buckets.append([off.value, numel.value])
        dl = C.c_size_t()
        nat.call("dtc_rn18_dlogits_buffer", h, C.byref(dl))
        return {
            "precision": lib.dtc_rn18_precision(h),
            "params": params,
            "bns": bns,
            "flat_numel": lib.dtc_rn18_flat_numel(h),
            "bufs_numel": lib.dtc_rn18_bufs_numel(h),
            "workspace_bytes": lib.dtc_rn18_workspace_bytes(h),
            "buckets": buckets,
            "activations": _acts(lib, h, lib.dtc_rn18_num_activations, lib.dtc_rn18_activation_info),
            "captures": _acts(lib, h, lib.dtc_rn18_num_captures, lib.dtc_rn18_capture_info),
            "dlogits_offset": dl.value,
        }
    finally:
        lib.dtc_rn18_destroy(h)


def main():
    nat = dtc_import.load()._native
    lib = nat.lib
    defaults = {k: lib.dtc_get_option(k) for k in (b"stem_direct", b"bucket_tail")}
    out = {}
    try:
        for stem_direct in (0, 1):
            for bucket_tail in (0, 1):
                nat.call("dtc_set_option", b"stem_direct", stem_direct)
                nat.call("dtc_set_option", b"bucket_tail", bucket_tail)
                for (b, hh, ww, ncls) in SHAPES:
                    for (mode, fp32, capture) in MODES:
                        for cap_mb in CAPS_MB:
                            key = (f"stem_direct={stem_direct} bucket_tail={bucket_tail} B={b} {hh}x{ww} "
                                   f"classes={ncls} {mode} cap={cap_mb:g}MB")
                            out[key] = dump_one(nat, b, hh, ww, ncls, fp32, capture, cap_mb)
    finally:
        for k, v in defaults.items():
            lib.dtc_set_option(k, v)
    json.dump(out, sys.stdout, sort_keys=True, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
