"""Tensor-level wrappers over the per-op C ABI (include/dtc.h).

Each function takes torch tensors that already live on the GPU (torch is the allocator and
stream provider only), enqueues the native kernel on the current stream and returns output
tensors. bf16 tensors are passed as torch.bfloat16 (same bits as the ABI's uint16_t words).
Nothing here computes on the host and there is no fallback path.
"""
from __future__ import annotations

import ctypes as C

import torch

from ._native import (CONV_KERNELS, CONV_ROUTE_RES, CONV_ROUTE_SC, SAM_MAX_KEEP, SEG_ADAPT, ConvDesc, ConvRoute, EmaRange,
                      NativeError, PsgdTensor, SamKeep, Seg, call, lib, ptr, require_cuda, stream_ptr)



def conv_desc(n, h, w, c, k, r, s, stride, pad) -> ConvDesc:
    return ConvDesc(n, h, w, c, k, r, s, stride, pad)


def conv_out_hw(h, w, r, s, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def conv_route_info(desc, mode, res=False, sc=False, nprob=1, ws=None, ws_bytes=0):
    """dtc_conv2d_route_query as a dict: the kernel (a CONV_KERNELS name), tile, splits and slab bytes the entry point
    named by (mode, res, sc, nprob) would run with for a workspace of `ws_bytes` at device address `ws` (an int; it is
    never dereferenced; None: no workspace). Host code: nothing is launched."""
    r = ConvRoute()
    call("dtc_conv2d_route_query", desc, mode, (CONV_ROUTE_RES if res else 0) | (CONV_ROUTE_SC if sc else 0), nprob,
         ws, ws_bytes, C.byref(r))
    out = {n: getattr(r, n) for n, _ in ConvRoute._fields_ if n != "reserved"}
    out["kernel"] = CONV_KERNELS[r.kernel]
    return out


def _ws(desc, mode, device, workspace=None):
    nbytes = lib.dtc_conv2d_workspace_size(desc, mode)
    if nbytes == 0:
        return None, 0
    if workspace is not None:
        return _given_ws(workspace, nbytes), nbytes
    return torch.empty(nbytes // 4 + 1, dtype=torch.float32, device=device), nbytes


def _given_ws(workspace, nbytes):
    """A caller's workspace: contiguous, on the GPU, at least the `nbytes` the size query returned."""
    require_cuda(workspace)
    if not workspace.is_contiguous() or workspace.numel() * workspace.element_size() < nbytes:
        raise ValueError(f"workspace must be contiguous and hold {nbytes} bytes, got "
                         f"{workspace.numel() * workspace.element_size()}")
    return workspace


def _out(out, shape, dtype, device, what):
    """The output tensor: a fresh one (the default), or the caller's `out` checked for shape, dtype, contiguity."""
    if out is None:
        return torch.empty(*shape, dtype=dtype, device=device)
    require_cuda(out)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"{what}: out must be contiguous {dtype} {tuple(shape)}, got {out.dtype} {tuple(out.shape)}")
    return out


def conv2d_fwd(x, w, stride, pad, stats=None, out=None, workspace=None):
    """x [N,H,W,C] bf16, w [K,R,S,C] bf16 -> y [N,P,Q,K] bf16 (nn.Conv2d forward, net.py:18). Here and in the
    other conv / stem wrappers, `out` (a tuple / list where several tensors are returned) and `workspace` (at
    least the bytes the size query returns) replace the tensors allocated by default."""
    require_cuda(x, w)
    N, H, W, Cc = x.shape
    K, R, S, _ = w.shape
    d = conv_desc(N, H, W, Cc, K, R, S, stride, pad)
    P, Q = conv_out_hw(H, W, R, S, stride, pad)
    y = _out(out, (N, P, Q, K), torch.bfloat16, x.device, "conv2d_fwd")
    ws, nb = _ws(d, 0, x.device, workspace)
    call("dtc_conv2d_fwd", d, ptr(x), ptr(w), ptr(y), ptr(stats), ptr(ws), nb, stream_ptr())
    return y


def conv2d_fwd_sc(x, w, wsc, stats=None, stats_sc=None, out=None):
    """3x3 stride-2 conv + the 1x1 stride-2 projection shortcut of the same x in one launch (net.py:18-19,
    29-36): x [N,H,W,C], w [K,3,3,C], wsc [K,C] bf16 -> (y, ysc) [N,H/2,W/2,K] bf16."""
    require_cuda(x, w, wsc)
    N, H, W, Cc = x.shape
    K = w.shape[0]
    d = conv_desc(N, H, W, Cc, K, 3, 3, 2, 1)
    P, Q = conv_out_hw(H, W, 3, 3, 2, 1)
    y, ysc = (_out(o, (N, P, Q, K), torch.bfloat16, x.device, "conv2d_fwd_sc") for o in (out if out is not None else (None, None)))
    call("dtc_conv2d_fwd_sc", d, ptr(x), ptr(w), ptr(y), ptr(stats), ptr(wsc), ptr(ysc), ptr(stats_sc), stream_ptr())
    return y, ysc


def conv2d_dgrad(dy, w, in_hw, stride, pad, res=None, out=None, workspace=None):
    """dy [N,P,Q,K] bf16, w [K,R,S,C] -> dx [N,H,W,C] bf16 (+ res)."""
    require_cuda(dy, w)
    N = dy.shape[0]
    K, R, S, Cc = w.shape
    H, W = in_hw
    d = conv_desc(N, H, W, Cc, K, R, S, stride, pad)
    dx = _out(out, (N, H, W, Cc), torch.bfloat16, dy.device, "conv2d_dgrad")
    ws, nb = _ws(d, 1, dy.device, workspace)
    call("dtc_conv2d_dgrad", d, ptr(dy), ptr(w), ptr(dx), ptr(res), ptr(ws), nb, stream_ptr())
    return dx


def conv2d_dgrad_bn(dy, w, in_hw, stride, pad, ymask, x1, mean1, invstd1, x2=None, mean2=None, invstd2=None,
                    res=None, out=None):
    """conv2d_dgrad fused with bn_bwd_reduce (dtc_conv2d_dgrad_bn): returns (dz, acc1, acc2) where
    dz = bf16(dx [+ res]) * [ymask > 0]; `out` may be `res` (in place)."""
    require_cuda(dy, w)
    N = dy.shape[0]
    K, R, S, Cc = w.shape
    H, W = in_hw
    d = conv_desc(N, H, W, Cc, K, R, S, stride, pad)
    dz = out if out is not None else torch.empty(N, H, W, Cc, dtype=torch.bfloat16, device=dy.device)
    acc1 = new_stats(Cc, dy.device)
    acc2 = new_stats(Cc, dy.device) if x2 is not None else None
    ws, nb = _ws(d, 1, dy.device)
    call("dtc_conv2d_dgrad_bn", d, ptr(dy), ptr(w), ptr(dz), ptr(res), ptr(ymask), ptr(x1), ptr(mean1), ptr(invstd1),
         ptr(acc1), ptr(x2), ptr(mean2), ptr(invstd2), ptr(acc2), ptr(ws), nb, stream_ptr())
    return dz, acc1, acc2


def conv2d_wgrad(x, dy, r, s, stride, pad, scale=1.0, out=None, workspace=None):
    """x [N,H,W,C] bf16, dy [N,P,Q,K] bf16 -> dw [K,R,S,C] fp32 (scaled)."""
    require_cuda(x, dy)
    N, H, W, Cc = x.shape
    K = dy.shape[3]
    d = conv_desc(N, H, W, Cc, K, r, s, stride, pad)
    dw = _out(out, (K, r, s, Cc), torch.float32, x.device, "conv2d_wgrad")
    ws, nb = _ws(d, 2, x.device, workspace)
    call("dtc_conv2d_wgrad", d, ptr(x), ptr(dy), ptr(dw), float(scale), ptr(ws), nb, stream_ptr())
    return dw


def conv2d_dgrad_sc(dy, w, dsc, wsc, in_hw, out=None):
    """dx through a projection block's conv1 (3x3 stride 2) and its 1x1 stride-2 shortcut in one launch
    (dtc_conv2d_dgrad_sc): dy / dsc [N,P,Q,K], w [K,3,3,C], wsc [K,C] bf16 -> dx [N,H,W,C] bf16."""
    require_cuda(dy, w, dsc, wsc)
    N, _, _, K = dy.shape
    Cc = w.shape[3]
    H, W = in_hw
    d = conv_desc(N, H, W, Cc, K, 3, 3, 2, 1)
    dx = _out(out, (N, H, W, Cc), torch.bfloat16, dy.device, "conv2d_dgrad_sc")
    call("dtc_conv2d_dgrad_sc", d, ptr(dy), ptr(w), ptr(dx), ptr(dsc), ptr(wsc), stream_ptr())
    return dx


def conv2d_wgrad_sc(x, dy, dsc, scale=1.0, out=None, workspace=None):
    """Weight gradients of a projection block's 3x3 stride-2 conv1 and its 1x1 stride-2 shortcut in one
    launch (dtc_conv2d_wgrad_sc): x [N,H,W,C], dy / dsc [N,H/2,W/2,K] bf16 -> (dw [K,3,3,C], dw_sc [K,C])."""
    require_cuda(x, dy, dsc)
    N, H, W, Cc = x.shape
    K = dy.shape[3]
    d = conv_desc(N, H, W, Cc, K, 3, 3, 2, 1)
    nb = lib.dtc_conv2d_wgrad_sc_workspace_size(d)
    if nb == 0:
        raise ValueError(f"conv2d_wgrad_sc: no fused plan for {(N, H, W, Cc, K)}")
    ws = _given_ws(workspace, nb) if workspace is not None else \
        torch.empty(nb // 4 + 64, dtype=torch.float32, device=x.device)
    o = out if out is not None else (None, None)
    dw = _out(o[0], (K, 3, 3, Cc), torch.float32, x.device, "conv2d_wgrad_sc")
    dw_sc = _out(o[1], (K, Cc), torch.float32, x.device, "conv2d_wgrad_sc")
    call("dtc_conv2d_wgrad_sc", d, ptr(x), ptr(dy), ptr(dsc), ptr(dw), ptr(dw_sc), float(scale), ptr(ws), nb,
         stream_ptr())
    return dw, dw_sc


def conv2d_wgrad_batch(xs, dys, scale=1.0, out=None, workspace=None):
    """n (<= 4) same-shape 3x3 stride-1 weight gradients in one launch (dtc_conv2d_wgrad_batch):
    xs[i] [N,H,W,C] bf16, dys[i] [N,H,W,K] bf16 -> list of dw [K,3,3,C] fp32 (scaled)."""
    require_cuda(*xs, *dys)
    n = len(xs)
    N, H, W, Cc = xs[0].shape
    K = dys[0].shape[3]
    d = conv_desc(N, H, W, Cc, K, 3, 3, 1, 1)
    nb = lib.dtc_conv2d_wgrad_batch_workspace_size(d, n)
    if nb == 0:
        raise ValueError(f"conv2d_wgrad_batch: no batched halo plan for {(N, H, W, Cc, K)} x {n}")
    ws = _given_ws(workspace, nb) if workspace is not None else \
        torch.empty(nb // 4 + 64, dtype=torch.float32, device=xs[0].device)
    if out is not None and len(out) != n:
        raise ValueError(f"conv2d_wgrad_batch: out must list {n} tensors, got {len(out)}")
    dws = [_out(o, (K, 3, 3, Cc), torch.float32, xs[0].device, "conv2d_wgrad_batch") for o in (out if out is not None else [None] * n)]
    arr = C.c_void_p * n
    call("dtc_conv2d_wgrad_batch", d, n, arr(*[ptr(t) for t in xs]), arr(*[ptr(t) for t in dys]),
         arr(*[ptr(t) for t in dws]), float(scale), ptr(ws), nb, stream_ptr())
    return dws


def new_stats(c, device):
    """A zeroed BN statistics accumulator for c channels (dtc_bn_stat_words(c) int64 words: exact fixed-point
    sums, common.h): conv epilogues and BN-backward reductions ADD into it."""
    return torch.zeros(int(lib.dtc_bn_stat_words(c)), dtype=torch.int64, device=device)


def stat_totals(stats, c):
    """The two per-channel totals an accumulator holds, as the BN kernels form them (dtc_bn_stat_totals, host
    code): float64 [2, c] on the CPU -- row 0 sum x (sum dz), row 1 sum x^2 (sum dz * xhat)."""
    host = stats.detach().to("cpu", torch.int64).contiguous()
    if host.numel() != int(lib.dtc_bn_stat_words(c)):
        raise ValueError(f"stat_totals: {host.numel()} words is not an accumulator of {c} channels")
    out = torch.empty(2, c, dtype=torch.float64)
    call("dtc_bn_stat_totals", ptr(host), c, ptr(out))
    return out


def stat_from_totals(s, q, device):
    """An accumulator holding the given per-channel totals (float64 arrays of c values; test input for the
    finalize kernels): each total goes into slot 0 in the fixed-point format of common.h."""
    import numpy as np

    s, q = np.asarray(s, np.float64), np.asarray(q, np.float64)
    c = s.shape[0]
    words = np.zeros(int(lib.dtc_bn_stat_words(c)), np.int64)
    hdr = 2 * int(lib.dtc_bn_stat_words(1)) - int(lib.dtc_bn_stat_words(2))  # header words (common.h DTC_STAT_HDR)
    for j, v in enumerate((s, q)):
        d = v * 256.0
        if not np.all(np.abs(d) < 2.0 ** 55):
            raise ValueError("stat_from_totals: total out of range")
        h = np.floor(d)
        words[hdr + (2 * j) * c:hdr + (2 * j + 1) * c] = h.astype(np.int64)
        words[hdr + (2 * j + 1) * c:hdr + (2 * j + 2) * c] = np.floor((d - h) * 2.0 ** 44).astype(np.int64)
    return torch.from_numpy(words).to(device)


def bn_fwd_finalize(stats, count, gamma, beta, running_mean=None, running_var=None, nbt=None, momentum=0.1,
                    eps=1e-5):
    c = gamma.numel()
    dev = gamma.device
    mean, invstd, scale, shift = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(4))
    call("dtc_bn_fwd_finalize", ptr(stats), c, int(count), ptr(gamma), ptr(beta), ptr(running_mean),
         ptr(running_var), ptr(nbt), float(momentum), float(eps), ptr(mean), ptr(invstd), ptr(scale), ptr(shift),
         stream_ptr())
    return mean, invstd, scale, shift


def bn_apply_relu(x, scale, shift):
    y = torch.empty_like(x)
    m, c = x.numel() // x.shape[-1], x.shape[-1]
    call("dtc_bn_apply_relu", ptr(x), ptr(scale), ptr(shift), ptr(y), m, c, stream_ptr())
    return y


def bn_apply_add_relu(x, scale, shift, res):
    y = torch.empty_like(x)
    m, c = x.numel() // x.shape[-1], x.shape[-1]
    call("dtc_bn_apply_add_relu", ptr(x), ptr(scale), ptr(shift), ptr(res), ptr(y), m, c, stream_ptr())
    return y


def bn_apply_dual_relu(x, scale, shift, x2, scale2, shift2):
    y = torch.empty_like(x)
    m, c = x.numel() // x.shape[-1], x.shape[-1]
    call("dtc_bn_apply_dual_relu", ptr(x), ptr(scale), ptr(shift), ptr(x2), ptr(scale2), ptr(shift2), ptr(y), m, c,
         stream_ptr())
    return y


def bn_bwd_reduce(dy, ymask, x1, mean1, invstd1, x2=None, mean2=None, invstd2=None):
    c = x1.shape[-1]
    m = x1.numel() // c
    acc1 = new_stats(c, x1.device)
    acc2 = new_stats(c, x1.device) if x2 is not None else None
    dz = torch.empty_like(dy) if ymask is not None else None
    call("dtc_bn_bwd_reduce", ptr(dy), ptr(ymask), ptr(x1), ptr(mean1), ptr(invstd1), ptr(acc1), ptr(x2), ptr(mean2),
         ptr(invstd2), ptr(acc2), ptr(dz), m, c, stream_ptr())
    return (dz if dz is not None else dy), acc1, acc2


def bn_bwd_finalize(acc, count, gamma, mean, invstd, gscale=1.0):
    c = gamma.numel()
    dev = gamma.device
    dgamma = torch.empty(c, dtype=torch.float32, device=dev)
    dbeta = torch.empty(c, dtype=torch.float32, device=dev)
    coef = torch.empty(3, c, dtype=torch.float32, device=dev)
    call("dtc_bn_bwd_finalize", ptr(acc), c, int(count), ptr(gamma), ptr(mean), ptr(invstd), float(gscale),
         ptr(dgamma), ptr(dbeta), ptr(coef), stream_ptr())
    return dgamma, dbeta, coef


def bn_bwd_apply(dz, x1, coef1, x2=None, coef2=None):
    c = x1.shape[-1]
    m = x1.numel() // c
    dx1 = torch.empty_like(x1)
    dx2 = torch.empty_like(x2) if x2 is not None else None
    call("dtc_bn_bwd_apply", ptr(dz), ptr(x1), ptr(coef1), ptr(dx1), ptr(x2), ptr(coef2), ptr(dx2), m, c, stream_ptr())
    return dx1, dx2


def bn_fin_apply(mode, x, stats, count, gamma, beta, running_mean=None, running_var=None, nbt=None, x2=None, bn2=None,
                 momentum=0.1, eps=1e-5, want_mask=True):
    """The fused forward BN (dtc_bn_fin_apply): mode 1 relu(bn(x)), 2 relu(bn(x) + x2), 3 relu(bn(x) + bn2(x2)) with
    bn2 = dict(stats=, gamma=, beta=, running_mean=, running_var=, nbt=) of the second BatchNorm. The running
    statistics and nbt are updated in place. Returns (y, mask bits or None, (mean, invstd), (mean2, invstd2) or
    None)."""
    require_cuda(x, stats, gamma, beta, x2)
    c = x.shape[-1]
    m = x.numel() // c
    dev = x.device
    y = torch.empty_like(x)
    mask = torch.empty(m * c // 8, dtype=torch.uint8, device=dev) if want_mask else None
    mean, invstd = (torch.empty(c, dtype=torch.float32, device=dev) for _ in range(2))
    b2 = bn2 or {}
    mean2, invstd2 = (torch.empty(c, dtype=torch.float32, device=dev) if bn2 else None for _ in range(2))
    call("dtc_bn_fin_apply", int(mode), ptr(x), ptr(stats), int(count), ptr(gamma), ptr(beta), ptr(running_mean),
         ptr(running_var), ptr(nbt), float(momentum), float(eps), ptr(mean), ptr(invstd), ptr(x2), ptr(b2.get("stats")),
         ptr(b2.get("gamma")), ptr(b2.get("beta")), ptr(b2.get("running_mean")), ptr(b2.get("running_var")),
         ptr(b2.get("nbt")), ptr(mean2), ptr(invstd2), ptr(y), ptr(mask), m, c, stream_ptr())
    return y, mask, (mean, invstd), ((mean2, invstd2) if bn2 else None)


def bn_bwd_mask(dy, mask_bits, x1, gamma1, mean1, invstd1, x2=None, gamma2=None, mean2=None, invstd2=None, count=None,
                gscale=1.0, one_launch=False, dz_out=None, acc=None):
    """The mask-bit BN backward (dtc_bn_bwd_mask), two launches through the accumulator `acc` (a zeroed one is
    made when None) or one (`one_launch`). dz_out: None, or a tensor to receive dz = dy * bit (may be dy itself).
    Returns dict(dx1, dgamma1, dbeta1, acc [, dx2, dgamma2, dbeta2])."""
    require_cuda(dy, mask_bits, x1, gamma1, mean1, invstd1, x2, dz_out)
    c = x1.shape[-1]
    m = x1.numel() // c
    dev = x1.device
    dual = x2 is not None
    out = {"dx1": torch.empty_like(x1)}
    for k in ("dgamma1", "dbeta1") + (("dgamma2", "dbeta2") if dual else ()):
        out[k] = torch.empty(c, dtype=torch.float32, device=dev)
    if dual:
        out["dx2"] = torch.empty_like(x2)
    if acc is None and not one_launch:
        acc = torch.zeros((2 if dual else 1) * int(lib.dtc_bn_stat_words(c)), dtype=torch.int64, device=dev)
    out["acc"] = acc
    call("dtc_bn_bwd_mask", ptr(dy), ptr(mask_bits), ptr(dz_out), ptr(x1), ptr(gamma1), ptr(mean1), ptr(invstd1),
         ptr(out["dgamma1"]), ptr(out["dbeta1"]), ptr(out["dx1"]), ptr(x2), ptr(gamma2), ptr(mean2), ptr(invstd2),
         ptr(out.get("dgamma2")), ptr(out.get("dbeta2")), ptr(out.get("dx2")), int(m if count is None else count),
         float(gscale), int(bool(one_launch)), ptr(acc), 0 if acc is None else acc.numel(), m, c, stream_ptr())
    return out


def bn_mask_bits(y):
    """ReLU mask bits of a post-ReLU NHWC tensor as the forward BN apply writes them: one byte per 8
    channels, bit k = channel 8j+k > 0."""
    c = y.shape[-1]
    b = (y.reshape(-1, c // 8, 8) > 0).to(torch.int32)
    w = torch.tensor([1 << k for k in range(8)], dtype=torch.int32, device=y.device)
    return (b * w).sum(-1).to(torch.uint8).contiguous()


def stem_im2col(x):
    n, _, h, w = x.shape
    cols = torch.empty(n, h, w, 64, dtype=torch.bfloat16, device=x.device)
    call("dtc_stem_im2col", ptr(x), ptr(cols), n, h, w, stream_ptr())
    return cols


def stem_fwd(x, w27, stats=None, out=None):
    """Direct stem conv (dtc_stem_fwd): x [N,3,H,W] fp32, w27 [64,27] bf16 (KRSC) -> y [N,H,W,64] bf16."""
    n, _, h, w = x.shape
    y = _out(out, (n, h, w, 64), torch.bfloat16, x.device, "stem_fwd")
    call("dtc_stem_fwd", ptr(x), ptr(w27), ptr(y), ptr(stats), n, h, w, stream_ptr())
    return y


def stem_wgrad(x, dy, scale=1.0, out=None, workspace=None):
    """Direct stem weight gradient (dtc_stem_wgrad): x [N,3,H,W] fp32, dy [N,H,W,64] bf16 -> [64,27] fp32."""
    n, _, h, w = x.shape
    nb = lib.dtc_stem_wgrad_workspace_size(n, h, w)
    ws = _given_ws(workspace, nb) if workspace is not None else \
        torch.empty(nb // 4 + 64, dtype=torch.float32, device=x.device)
    dw = _out(out, (64, 27), torch.float32, x.device, "stem_wgrad")
    call("dtc_stem_wgrad", ptr(x), ptr(dy), ptr(dw), float(scale), n, h, w, ptr(ws), nb, stream_ptr())
    return dw


def stem_pack_weight(w27):
    k = w27.shape[0]
    w64 = torch.empty(k, 64, dtype=torch.bfloat16, device=w27.device)
    call("dtc_stem_pack_weight", ptr(w27), ptr(w64), k, stream_ptr())
    return w64


def head_fwd(act, wfc, bfc, out=None):
    """act [N,h,w,C] bf16, wfc [ncls,C] bf16, bfc [ncls] fp32 -> (feat fp32 [N,C], logits fp32 [N,ncls]);
    `out`: a (feat, logits) pair to write instead of fresh tensors."""
    require_cuda(act, wfc, bfc)
    n, h, w, c = act.shape
    ncls = wfc.shape[0]
    o = out if out is not None else (None, None)
    feat = _out(o[0], (n, c), torch.float32, act.device, "head_fwd")
    logits = _out(o[1], (n, ncls), torch.float32, act.device, "head_fwd")
    call("dtc_head_fwd", ptr(act), n, h * w, c, ptr(wfc), ptr(bfc), ncls, ptr(feat), ptr(logits), stream_ptr())
    return feat, logits


def head_bwd(dlogits, feat, wfc, hw, scale=1.0, out=None, workspace=None):
    """dlogits [N,ncls] fp32, feat [N,C] fp32, wfc [ncls,C] bf16 -> (dw fp32 [ncls,C], db fp32 [ncls], dact bf16
    [N,h,w,C]); `out`: a (dw, db, dact) triple, `workspace`: at least dtc_head_bwd_workspace_size bytes (the
    default is exactly that many)."""
    require_cuda(dlogits, feat, wfc)
    n, c = feat.shape
    ncls = wfc.shape[0]
    h, w = hw
    o = out if out is not None else (None, None, None)
    dw = _out(o[0], (ncls, c), torch.float32, feat.device, "head_bwd")
    db = _out(o[1], (ncls,), torch.float32, feat.device, "head_bwd")
    dact = _out(o[2], (n, h, w, c), torch.bfloat16, feat.device, "head_bwd")
    nb = lib.dtc_head_bwd_workspace_size(n, c, ncls)
    ws = _given_ws(workspace, nb) if workspace is not None else \
        torch.empty(nb // 4, dtype=torch.float32, device=feat.device)
    call("dtc_head_bwd", ptr(dlogits), ptr(feat), ptr(wfc), n, h * w, c, ncls, float(scale), ptr(dw), ptr(db),
         ptr(dact), ptr(ws), nb, stream_ptr())
    return dw, db, dact


def xent_fwd(logits, labels):
    n, ncls = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    lse = torch.empty(n, dtype=torch.float32, device=logits.device)
    call("dtc_xent_fwd", ptr(logits), ptr(labels), n, ncls, ptr(loss), ptr(lse), stream_ptr())
    return loss, lse


def eval_metrics(logits, labels, topk=5, out=None):
    """One evaluation batch's metrics in one launch, no host sync (dtc_eval_metrics): logits fp32 [n, ncls],
    labels int64 [n] -> an int32 [4] device tensor viewing one 16-byte record (loss, n, top1, topk): word 0
    holds the fp32 mean cross-entropy's bits (``rec[:1].view(torch.float32)``), bit-identical to
    ``xent_fwd``'s; top1 / topk count the rows whose label ranks < 1 / < topk (ties to the lower index).
    `out`: a contiguous int32 [4] device tensor to write (e.g. one slot of a record buffer)."""
    require_cuda(logits, labels, out)
    n, ncls = logits.shape
    rec = torch.empty(4, dtype=torch.int32, device=logits.device) if out is None else out
    if rec.dtype != torch.int32 or rec.numel() != 4 or not rec.is_contiguous():
        raise NativeError("eval_metrics: out must be a contiguous int32 [4] tensor")
    call("dtc_eval_metrics", ptr(logits), ptr(labels), n, ncls, int(topk), ptr(rec), stream_ptr())
    return rec


def xent_bwd(logits, labels, lse, gscale=None, out=None):
    n, ncls = logits.shape
    dl = torch.empty_like(logits) if out is None else out
    call("dtc_xent_bwd", ptr(logits), ptr(labels), ptr(lse), ptr(gscale), n, ncls, ptr(dl), stream_ptr())
    return dl


def _soft_check(logits, labels_a, labels_b, lam):
    require_cuda(logits, labels_a, labels_b, lam)
    n = logits.shape[0]
    if (labels_b is None) != (lam is None):
        raise ValueError("labels_b and lam go together (both or neither)")
    for t, dt in ((labels_a, torch.int64), (labels_b, torch.int64), (lam, torch.float32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != (n,) or not t.is_contiguous()):
            raise ValueError(f"expected contiguous {dt} ({n},), got {t.dtype} {tuple(t.shape)}")
    if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError(f"logits must be contiguous fp32 [n, ncls], got {logits.dtype} {tuple(logits.shape)}")


def xent_soft_fwd(logits, labels_a, labels_b=None, lam=None, smoothing=0.0, scale=None, host=None):
    """Mean cross-entropy against the soft target q = (1 - smoothing) * (lam * onehot(labels_a) + (1 - lam) *
    onehot(labels_b)) + smoothing / ncls per row (label smoothing, Mixup, CutMix; labels_b = lam = None: lam = 1).
    Returns (loss, lse, scaled): n <= 4096 is one launch (dtc_xent_soft_fwd_ex) that also stores loss * scale
    (`scale`: a device fp32 scalar) into `scaled` and the loss into `host` (a pinned host word); beyond, the
    two-launch form (no scale / host there). lse is bit-identical to xent_fwd's."""
    _soft_check(logits, labels_a, labels_b, lam)
    n, ncls = logits.shape
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    lse = torch.empty(n, dtype=torch.float32, device=logits.device)
    if n > 4096:
        if scale is not None or host is not None:
            raise NativeError("xent_soft_fwd: scale / host need n <= 4096")
        call("dtc_xent_soft_fwd", ptr(logits), ptr(labels_a), ptr(labels_b), ptr(lam), float(smoothing), n, ncls,
             ptr(loss), ptr(lse), stream_ptr())
        return loss, lse, None
    scaled = torch.empty((), dtype=torch.float32, device=logits.device) if scale is not None else None
    call("dtc_xent_soft_fwd_ex", ptr(logits), ptr(labels_a), ptr(labels_b), ptr(lam), float(smoothing), n, ncls,
         ptr(loss), ptr(lse), ptr(scale), ptr(scaled), ptr(host), stream_ptr())
    return loss, lse, scaled


def xent_soft_bwd(logits, labels_a, labels_b, lam, smoothing, lse, gscale=None, out=None):
    """dlogits = (softmax(logits) - q) * gscale / n for xent_soft_fwd's q."""
    _soft_check(logits, labels_a, labels_b, lam)
    n, ncls = logits.shape
    dl = torch.empty_like(logits) if out is None else out
    call("dtc_xent_soft_bwd", ptr(logits), ptr(labels_a), ptr(labels_b), ptr(lam), float(smoothing), ptr(lse),
         ptr(gscale), n, ncls, ptr(dl), stream_ptr())
    return dl


def sgd_nesterov_flat(p, g, mom, pb, lr, weight_decay, momentum, inv_scale=None, found_inf=None):
    call("dtc_sgd_nesterov_flat", ptr(p), ptr(g), ptr(mom), ptr(pb), p.numel(), float(lr), float(weight_decay),
         float(momentum), ptr(inv_scale), ptr(found_inf), stream_ptr())


def adam_state(device):
    """The zeroed device state record of one adam_flat optimizer (word 0: the int32 step count)."""
    return torch.zeros(lib.dtc_adam_state_words(), dtype=torch.int32, device=device)


def adam_flat(p, g, m, v, pb, state, lr, beta1, beta2, eps, weight_decay, decoupled, inv_scale=None, found_inf=None):
    """One torch.optim.Adam (decoupled=False) / AdamW (decoupled=True) step over flat fp32 buffers, the bf16
    shadow `pb` refreshed in the same pass; `state` from adam_state() carries the device-side step count."""
    call("dtc_adam_flat", ptr(p), ptr(g), ptr(m), ptr(v), ptr(pb), p.numel(), ptr(state), float(lr), float(beta1),
         float(beta2), float(eps), float(weight_decay), int(bool(decoupled)), ptr(inv_scale), ptr(found_inf),
         stream_ptr())


def grad_norm_workspace(n, device):
    return torch.empty(max(1, lib.dtc_grad_norm_workspace_bytes(int(n)) // 8), dtype=torch.float64, device=device)


def grad_norm_clip(g, max_norm, inv_scale=None, workspace=None, total_norm=None, grad_mult=None):
    """(total_norm, grad_mult), two fp32 [1] device tensors: the L2 norm of g * inv_scale and inv_scale *
    min(1, max_norm / (total_norm + 1e-6)) (torch.nn.utils.clip_grad_norm_'s coefficient with the GradScaler
    factor folded in). No host synchronisation; bit-identical from run to run."""
    if workspace is None:
        workspace = grad_norm_workspace(g.numel(), g.device)
    if total_norm is None:
        total_norm = torch.empty(1, dtype=torch.float32, device=g.device)
    if grad_mult is None:
        grad_mult = torch.empty(1, dtype=torch.float32, device=g.device)
    call("dtc_grad_norm_clip", ptr(g), g.numel(), ptr(inv_scale), float(max_norm), ptr(workspace), ptr(total_norm),
         ptr(grad_mult), stream_ptr())
    return total_norm, grad_mult


class SegPlan:
    """A segment plan (dtc_segplan) with the device memory it is bound to. `names` follow the segments, which are
    in offset order; `end` is the first element past the last segment (the least size of a flat buffer)."""

    def __init__(self, segments, names=None, device=None):
        segments = [(int(o), int(n), bool(a)) for o, n, a in segments]
        table = (Seg * max(1, len(segments)))(*[Seg(o, n, SEG_ADAPT if a else 0, 0) for o, n, a in segments])
        self.handle = C.c_void_p()
        self._destroy = lib.dtc_segplan_destroy  # held here: module globals are gone at interpreter exit
        call("dtc_segplan_create", C.byref(self.handle), table, len(segments))
        self.nseg = len(segments)
        self.names = list(names) if names is not None else [str(i) for i in range(self.nseg)]
        self.segments = segments
        self.end = segments[-1][0] + segments[-1][1]
        self.mem = None
        if device is not None:
            self.bind(device)

    def bind(self, device):
        """Upload the tables into fresh device memory (the only copy: nothing is copied per step)."""
        nbytes = lib.dtc_segplan_device_bytes(self.handle)
        self.mem = torch.empty(nbytes, dtype=torch.uint8, device=device)  # the allocator aligns to 512 bytes
        require_cuda(self.mem)
        call("dtc_segplan_bind", self.handle, ptr(self.mem), nbytes, stream_ptr())

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            self._destroy(h)


def seg_plan(layout_or_segments, device=None) -> SegPlan:
    """The segment plan of a model's Layout (one segment per parameter, ADAPT for those with more than one
    dimension: conv and linear weights) or of a list of (offset, numel, adapt) triples in offset order, bound to
    fresh memory on `device` (None: left unbound)."""
    params = getattr(layout_or_segments, "params", None)
    if params is None:
        return SegPlan(layout_or_segments, None, device)
    params = sorted(params, key=lambda q: q.offset)
    return SegPlan([(q.offset, q.numel, len(q.shape) > 1) for q in params], [q.name for q in params], device)


def _seg_check(plan, *flat):
    require_cuda(*flat)
    if plan.mem is None:
        raise NativeError("the segment plan is not bound to a device (ops.seg_plan(..., device))")
    for t in flat:
        if t is not None and (t.numel() < plan.end or not t.is_contiguous() or t.device != plan.mem.device):
            raise NativeError(f"flat buffers must be contiguous, on the plan's device and hold the plan's "
                              f"{plan.end} elements, got {t.numel()} on {t.device}")


def _seg_out(plan, out):
    return _out(out, (plan.nseg, 3), torch.float32, plan.mem.device, "seg_out")


def seg_norms(plan, p, g, gmul=None, out=None):
    """Per-tensor L2 norms over flat buffers: fp32 [nseg, 3] = (||p_s||, |gmul| * ||g_s||, ||p_s|| / that) on the
    device, double accumulation in a fixed order (bit-identical run to run), no host synchronisation."""
    _seg_check(plan, p, g)
    out = _seg_out(plan, out)
    call("dtc_seg_norms", plan.handle, ptr(p), ptr(g), ptr(gmul), ptr(out), stream_ptr())
    return out


def lars_flat(plan, p, g, mom, pb, lr, weight_decay, momentum, nesterov=False, trust_coef=1e-3, eps=1e-8,
              trust_clip=False, inv_scale=None, found_inf=None, seg_out=None):
    """One LARS step over the plan's segments of the flat fp32 buffers (include/dtc.h: dtc_lars_flat), the bf16
    shadow `pb` refreshed in the same pass. `seg_out` (optional fp32 [nseg, 3]) receives the norms and the trust
    ratio of every segment."""
    _seg_check(plan, p, g, mom, pb)
    if seg_out is not None:
        seg_out = _seg_out(plan, seg_out)
    call("dtc_lars_flat", plan.handle, ptr(p), ptr(g), ptr(mom), ptr(pb), float(lr), float(weight_decay),
         float(momentum), int(bool(nesterov)), float(trust_coef), float(eps), int(bool(trust_clip)), ptr(inv_scale),
         ptr(found_inf), ptr(seg_out), stream_ptr())


def eval_batch_weights(net, params, params_bf16, bufs, x, labels, n_valid, topk, rec, logits=None):
    """dtc_rn18_eval_batch_weights on the executor handle `net`: one evaluation batch read from the given flat
    parameter / bf16 shadow / running-statistics tensors (the bound buffers' layout) instead of the bound ones."""
    require_cuda(params, params_bf16, bufs, x, labels, rec, logits)
    if params.dtype != torch.float32 or params_bf16.dtype != torch.bfloat16 or bufs.dtype != torch.float32:
        raise NativeError("eval_batch_weights: params / bufs must be fp32 tensors, params_bf16 a bf16 tensor")
    if not (params.is_contiguous() and params_bf16.is_contiguous() and bufs.is_contiguous()):
        raise NativeError("eval_batch_weights: contiguous weight tensors only")
    call("dtc_rn18_eval_batch_weights", net, ptr(params), ptr(params_bf16), ptr(bufs), ptr(x), ptr(labels),
         int(n_valid), int(topk), ptr(logits), ptr(rec), stream_ptr())


def ema_state(device):
    """The zeroed device state record of one EMA (word 0: the int32 count of updates, word 1: the fp32 weight
    1 - decay_t of the last update)."""
    return torch.zeros(lib.dtc_ema_state_words(), dtype=torch.int32, device=device)


def ema_update(ranges, state, decay, warmup=False, found_inf=None):
    """One EMA update over 1..4 flat ranges in one launch behind a one-thread tick (include/dtc.h: dtc_ema_update).
    `ranges`: (ema, src, ema_bf16 or None) triples of contiguous tensors -- ema += (src - ema) * w, ema_bf16 =
    bf16(ema); `state` from ema_state(). Nothing changes when `found_inf` (a device int32 word) is non-zero."""
    ranges = list(ranges)
    table = (EmaRange * max(1, len(ranges)))()
    for k, (ema, src, bf) in enumerate(ranges):
        require_cuda(ema, src, bf)
        if ema.dtype != torch.float32 or src.dtype != torch.float32 or (bf is not None and bf.dtype != torch.bfloat16):
            raise NativeError("ema_update: ema and src must be fp32 tensors, ema_bf16 a bf16 tensor")
        if src.numel() != ema.numel() or (bf is not None and bf.numel() != ema.numel()):
            raise NativeError(f"ema_update: range {k}: ema, src and ema_bf16 must have one size")
        if not (ema.is_contiguous() and src.is_contiguous() and (bf is None or bf.is_contiguous())):
            raise NativeError(f"ema_update: range {k}: contiguous tensors only")
        table[k] = EmaRange(ptr(ema), ptr(src), ptr(bf), ema.numel())
    require_cuda(state, found_inf)
    call("dtc_ema_update", table, len(ranges), ptr(state), float(decay), int(bool(warmup)), ptr(found_inf),
         stream_ptr())


ACCUM_OFF, ACCUM_STORE, ACCUM_ADD, ACCUM_FINISH = 0, 1, 2, 3  # include/dtc.h DTC_ACCUM_*


def grad_accum_flat(acc, g, mode):
    """One gradient-accumulation launch over two contiguous fp32 tensors of one size (include/dtc.h:
    dtc_grad_accum_flat): ACCUM_STORE acc = g, ACCUM_ADD acc = acc + g, ACCUM_FINISH g = g + acc -- one rounded fp32
    add per element, the other operand untouched."""
    require_cuda(acc, g)
    if acc.dtype != torch.float32 or g.dtype != torch.float32:
        raise NativeError("grad_accum_flat: acc and g must be fp32 tensors")
    if acc.numel() != g.numel() or not (acc.is_contiguous() and g.is_contiguous()):
        raise NativeError("grad_accum_flat: acc and g must be contiguous tensors of one size")
    call("dtc_grad_accum_flat", ptr(acc), ptr(g), g.numel(), int(mode), stream_ptr())


COMPRESS_OFF, COMPRESS_BF16 = 0, 1  # include/dtc.h DTC_COMPRESS_*


def _bf16_words(c, name):
    if c.dtype not in (torch.bfloat16, torch.uint16, torch.int16) or not c.is_contiguous():
        raise NativeError(f"{name}: c must be a contiguous tensor of 16-bit words (bfloat16, uint16 or int16)")


def grad_compress_bf16(g, c, acc=None):
    """c = bf16(g), or bf16(g + acc) with `acc` (one rounded fp32 add, then one round-to-nearest-even; include/dtc.h:
    dtc_grad_compress_bf16). g, acc: contiguous fp32 tensors; c: 16-bit words of the same element count."""
    require_cuda(g, c)
    _bf16_words(c, "grad_compress_bf16")
    if g.dtype != torch.float32 or not g.is_contiguous() or c.numel() != g.numel():
        raise NativeError("grad_compress_bf16: g must be a contiguous fp32 tensor of c's element count")
    if acc is not None:
        require_cuda(acc)
        if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.numel() != g.numel():
            raise NativeError("grad_compress_bf16: acc must be a contiguous fp32 tensor of g's size")
    call("dtc_grad_compress_bf16", ptr(g), None if acc is None else ptr(acc), ptr(c), g.numel(), stream_ptr())


def grad_decompress_bf16(c, g):
    """g = widen(c): the bf16 words shifted into the upper half of fp32, exact (dtc_grad_decompress_bf16)."""
    require_cuda(g, c)
    _bf16_words(c, "grad_decompress_bf16")
    if g.dtype != torch.float32 or not g.is_contiguous() or c.numel() != g.numel():
        raise NativeError("grad_decompress_bf16: g must be a contiguous fp32 tensor of c's element count")
    call("dtc_grad_decompress_bf16", ptr(c), ptr(g), g.numel(), stream_ptr())


# ----------------------------------------------------------------------------- PowerSGD
PSGD_P, PSGD_Q, PSGD_UNCOMPRESSED, PSGD_STAGING, PSGD_QSTRIDE = 0, 1, 2, 3, 4  # include/dtc.h DTC_PSGD_*
PSGD_MAX_RANK = 4


def psgd_should_compress(rows, cols, rank, min_compression_rate=2):
    """torch's ``powerSGD_hook._should_compress``: a rows x cols tensor is compressed at `rank` when the P and Q
    blocks together, times the rate, are smaller than the tensor."""
    return (rows + cols) * rank * min_compression_rate < rows * cols


class PsgdPlan:
    """A PowerSGD plan (dtc_psgd_plan) with the device memory it is bound to. `tensors`: (offset, rows, cols, rank)
    in offset order, rank 0 = all-reduced uncompressed. n_p / n_q / n_unc / n_staging / q_stride: the element
    counts of include/dtc.h; `end`: the first element past the last tensor."""

    def __init__(self, tensors, names=None, device=None):
        tensors = [(int(o), int(r), int(c), int(k)) for o, r, c, k in tensors]
        table = (PsgdTensor * max(1, len(tensors)))(*[PsgdTensor(o, r, c, k, 0) for o, r, c, k in tensors])
        self.handle = C.c_void_p()
        self._destroy = lib.dtc_psgd_plan_destroy  # held here: module globals are gone at interpreter exit
        call("dtc_psgd_plan_create", C.byref(self.handle), table, len(tensors))
        self.tensors = tensors
        self.names = list(names) if names is not None else [str(i) for i in range(len(tensors))]
        self.n_p, self.n_q, self.n_unc, self.n_staging, self.q_stride = (
            int(lib.dtc_psgd_plan_numel(self.handle, w))
            for w in (PSGD_P, PSGD_Q, PSGD_UNCOMPRESSED, PSGD_STAGING, PSGD_QSTRIDE))
        self.end = tensors[-1][0] + tensors[-1][1] * tensors[-1][2]
        self.mem = None
        if device is not None:
            self.bind(device)

    def bind(self, device):
        """Upload the tables into fresh device memory (the only copy: nothing is copied per step)."""
        nbytes = lib.dtc_psgd_plan_device_bytes(self.handle)
        self.mem = torch.empty(nbytes, dtype=torch.uint8, device=device)  # the allocator aligns to 512 bytes
        require_cuda(self.mem)
        call("dtc_psgd_plan_bind", self.handle, ptr(self.mem), nbytes, stream_ptr())

    def q_blocks(self):
        """[(tensor index, Q offset, cols, rank)] of the compressed tensors: where each Q block lies in a Q copy."""
        out, off = [], 0
        for i, (_, _, c, k) in enumerate(self.tensors):
            if k:
                out.append((i, off, c, k))
                off += c * k
        return out

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h:
            self._destroy(h)


def psgd_plan(layout_or_tensors, rank=1, min_compression_rate=2, device=None) -> PsgdPlan:
    """The PowerSGD plan of a model's Layout -- every parameter with more than one dimension is the row-major
    shape[0] x (numel / shape[0]) matrix it is stored as (conv weights: K x R*S*C) and is compressed at
    min(rows, cols, rank) when torch's rule (psgd_should_compress) says so; everything else is rank 0 -- or of a
    list of (offset, rows, cols, rank) in offset order. Bound to fresh memory on `device` (None: left unbound)."""
    params = getattr(layout_or_tensors, "params", None)
    if params is None:
        return PsgdPlan(layout_or_tensors, None, device)
    if not isinstance(rank, int) or not 1 <= rank <= PSGD_MAX_RANK:
        raise ValueError(f"PowerSGD rank must be an integer in [1, {PSGD_MAX_RANK}], not {rank!r}")
    tensors = []
    params = sorted(params, key=lambda q: q.offset)
    for q in params:
        rows = q.shape[0] if len(q.shape) > 1 else q.numel
        cols = q.numel // rows
        k = min(rows, cols, rank) if len(q.shape) > 1 and psgd_should_compress(rows, cols, rank,
                                                                               min_compression_rate) else 0
        tensors.append((q.offset, rows, cols, k))
    return PsgdPlan(tensors, [q.name for q in params], device)


def psgd_buffers(plan, seed=0, device=None):
    """(staging, q, state) of one PowerSGD plan on its device: staging fp32 [n_staging] = [uncompressed | P]; q fp32
    [2, q_stride] with q[0] = torch.randn(n_q) drawn on the CPU from `seed` (the same on every rank; per tensor a
    row-major cols x rank block, columns in storage order) and uploaded once; state int32 [4], zeroed."""
    device = device if device is not None else plan.mem.device
    staging = torch.zeros(max(plan.n_staging, 4), dtype=torch.float32, device=device)
    q = torch.zeros(2, max(plan.q_stride, 4), dtype=torch.float32, device=device)  # (4: only without any Q)
    init = torch.randn(plan.n_q, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)
    q[0, :plan.n_q].copy_(init)
    return staging, q, torch.zeros(4, dtype=torch.int32, device=device)


def _psgd_check(plan, g, e, staging, q, state=None):
    require_cuda(g, e, staging, q, state)
    if plan.mem is None:
        raise NativeError("the PowerSGD plan is not bound to a device (ops.psgd_plan(..., device))")
    for t in (g, e):
        if t is not None and (t.dtype != torch.float32 or t.numel() < plan.end or not t.is_contiguous()):
            raise NativeError(f"PowerSGD: g and e must be contiguous fp32 tensors of at least the plan's {plan.end} "
                              "elements")
    if staging.dtype != torch.float32 or staging.numel() < plan.n_staging or not staging.is_contiguous():
        raise NativeError(f"PowerSGD: staging must be a contiguous fp32 tensor of {plan.n_staging} elements")
    if q.dtype != torch.float32 or q.numel() < 2 * plan.q_stride or not q.is_contiguous():
        raise NativeError(f"PowerSGD: q must be a contiguous fp32 tensor of 2 x {plan.q_stride} elements")
    if state is not None and (state.dtype != torch.int32 or state.numel() < 4):
        raise NativeError("PowerSGD: state must be an int32 tensor of 4 words")


def psgd_orthonormalize(plan, what, q, staging, state, eps=0.0):
    """Modified Gram-Schmidt of every Q block (what = PSGD_Q: warm start -> q[1]) or P block (PSGD_P: in staging)."""
    _psgd_check(plan, None, None, staging, q, state)
    call("dtc_psgd_orthonormalize", plan.handle, int(what), ptr(q), ptr(staging), ptr(state), float(eps),
         stream_ptr())


def psgd_project(plan, g, e, q, staging):
    """staging = [uncompressed tensors of g | P = (g + e) Qh] (e may be None)."""
    _psgd_check(plan, g, e, staging, q)
    call("dtc_psgd_project", plan.handle, ptr(g), ptr(e), ptr(q), ptr(staging), stream_ptr())


def psgd_backproject(plan, g, e, staging, q):
    """q[1] = (g + e)^T Ph, Ph the orthonormalised P blocks in staging."""
    _psgd_check(plan, g, e, staging, q)
    call("dtc_psgd_backproject", plan.handle, ptr(g), ptr(e), ptr(staging), ptr(q), stream_ptr())


def psgd_reconstruct(plan, g, e, staging, q, state, c=1.0):
    """g = Ph Q^T, e = (g + e) - c * that, uncompressed tensors scattered back from staging; NaN and nothing else
    when the all-reduced P or Q was not finite."""
    _psgd_check(plan, g, e, staging, q, state)
    call("dtc_psgd_reconstruct", plan.handle, ptr(g), ptr(e), ptr(staging), ptr(q), ptr(state), float(c),
         stream_ptr())


def psgd_step(plan, g, e, staging, q, state, c=1.0, eps=0.0, allreduce=None):
    """One PowerSGD step on the current stream: the five launches with the two SUM all-reduces `allreduce(tensor)`
    between them (None: one rank, the collectives elided): [uncompressed | P], then Q."""
    psgd_orthonormalize(plan, PSGD_Q, q, staging, state, eps)
    psgd_project(plan, g, e, q, staging)
    if allreduce is not None and plan.n_staging:
        allreduce(staging[:plan.n_staging])
    psgd_orthonormalize(plan, PSGD_P, q, staging, state, eps)
    psgd_backproject(plan, g, e, staging, q)
    if allreduce is not None and plan.n_q:
        allreduce(q.view(-1)[plan.q_stride:plan.q_stride + plan.n_q])
    psgd_reconstruct(plan, g, e, staging, q, state, c)


def sam_state(device):
    """The device record of one SAM optimizer (include/dtc.h: dtc_sam_perturb), int32 [4]: word 0 the fp32 coef,
    word 1 the fp32 gradient norm of the last perturb, word 2 `skipped` (1: the norm was not finite and nothing
    moved). Every perturb writes it whole."""
    return torch.zeros(lib.dtc_sam_state_words(), dtype=torch.int32, device=device)


def sam_workspace(n, device):
    return torch.empty(max(1, lib.dtc_sam_workspace_bytes(int(n)) // 8), dtype=torch.float64, device=device)


def _sam_keep(keep, who):
    """The dtc_sam_keep table of (live, saved) tensor pairs: contiguous, one size in bytes, a multiple of 8."""
    keep = list(keep or ())
    if len(keep) > SAM_MAX_KEEP:
        raise NativeError(f"{who}: at most {SAM_MAX_KEEP} keep ranges, got {len(keep)}")
    table = (SamKeep * max(1, len(keep)))()
    for k, (live, saved) in enumerate(keep):
        require_cuda(live, saved)
        nbytes = live.numel() * live.element_size()
        if not (live.is_contiguous() and saved.is_contiguous()) or saved.numel() * saved.element_size() != nbytes:
            raise NativeError(f"{who}: keep {k}: live and saved must be contiguous tensors of one size in bytes")
        table[k] = SamKeep(ptr(live), ptr(saved), nbytes)
    return table, len(keep)


def _sam_check(who, p, p_saved, pb, g=None):
    require_cuda(p, p_saved, pb, g)
    fp32 = [t for t in (p, p_saved, g) if t is not None]
    if any(t.dtype != torch.float32 for t in fp32) or pb.dtype != torch.bfloat16:
        raise NativeError(f"{who}: p, g and p_saved must be fp32 tensors, p_bf16 a bf16 tensor")
    if any(t.numel() != p.numel() or not t.is_contiguous() for t in fp32 + [pb]):
        raise NativeError(f"{who}: p, g, p_saved and p_bf16 must be contiguous tensors of one size")


def sam_perturb(p, g, p_saved, pb, state, rho, adaptive=False, eps=1e-12, gmul=None, keep=None, workspace=None):
    """The SAM / ASAM ascent step over flat fp32 buffers (include/dtc.h: dtc_sam_perturb): p_saved = p, then
    p += coef * g (adaptive: * p * p) with coef = rho * m / (|m| * ||g|| + eps) (adaptive: ||p * g||), m = *gmul, and
    the bf16 shadow `pb` refreshed; a non-finite norm moves nothing and sets state's `skipped`. `keep`: up to 4
    (live, saved) pairs of small tensors copied live -> saved in the same launches. `state` from sam_state()."""
    _sam_check("sam_perturb", p, p_saved, pb, g)
    if workspace is None:
        workspace = sam_workspace(p.numel(), p.device)
    require_cuda(state, gmul, workspace)
    table, nkeep = _sam_keep(keep, "sam_perturb")
    call("dtc_sam_perturb", ptr(p), ptr(g), ptr(p_saved), ptr(pb), p.numel(), float(rho), float(eps),
         int(bool(adaptive)), ptr(gmul), table, nkeep, ptr(state), ptr(workspace), stream_ptr())


def sam_restore(p, p_saved, pb, state, keep=None, found_inf=None):
    """The way back (dtc_sam_restore), one launch: p = p_saved bit for bit, pb = bf16(p), every keep pair copied
    saved -> live, and *found_inf = 1 (an int32 device word, never cleared here) if the perturb was skipped."""
    _sam_check("sam_restore", p, p_saved, pb)
    require_cuda(state, found_inf)
    table, nkeep = _sam_keep(keep, "sam_restore")
    call("dtc_sam_restore", ptr(p), ptr(p_saved), ptr(pb), p.numel(), table, nkeep, ptr(state), ptr(found_inf),
         stream_ptr())


def cast_f32_bf16(src, dst):
    call("dtc_cast_f32_bf16", ptr(src), ptr(dst), src.numel(), stream_ptr())


def amp_check_finite(g, found_inf):
    call("dtc_amp_check_finite", ptr(g), g.numel(), ptr(found_inf), stream_ptr())


def amp_scale(x, scale):
    """GradScaler.scale(x) (main.py:25, trainer.py:157) on the native kernel: x * scale, device-side."""
    out = torch.empty_like(x)
    call("dtc_amp_scale", ptr(x), ptr(scale), ptr(out), x.numel(), stream_ptr())
    return out


def amp_update_scale(scale, inv_scale, tracker, found_inf, growth, backoff, interval):
    call("dtc_amp_update_scale", ptr(scale), ptr(inv_scale), ptr(tracker), ptr(found_inf), float(growth),
         float(backoff), int(interval), stream_ptr())


def cifar_augment(images, index, crop, flip, mean, std, pad=4, targets=None, out=None, labels=None, status=None):
    """Gather + RandomCrop(pad) + RandomHorizontalFlip + ToTensor + Normalize on the GPU
    (reference src/ddp/dataset.py:43-64). images: uint8 [N,H,W,3]; index: int64 [n] (None: 0..n-1);
    crop: uint8 [n,2] (None: centre); flip: uint8 [n] (None: no flip). Returns (fp32 [n,3,H,W],
    int64 labels [n] or None)."""
    require_cuda(images, index, crop, flip, targets, out, labels, status)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError(f"images must be contiguous uint8 [N,H,W,3], got {images.dtype} {tuple(images.shape)}")
    n_images, h, w, _ = images.shape
    n = index.numel() if index is not None else (crop.shape[0] if crop is not None else n_images)
    for t, shape, dt in ((index, (n,), torch.int64), (crop, (n, 2), torch.uint8), (flip, (n,), torch.uint8),
                         (targets, (n_images,), torch.int64)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"expected contiguous {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    if out is None:
        out = torch.empty(n, 3, h, w, dtype=torch.float32, device=images.device)
    if targets is not None and labels is None:
        labels = torch.empty(n, dtype=torch.int64, device=images.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    call("dtc_cifar_augment", ptr(images), ptr(targets), n_images, ptr(index), ptr(crop), ptr(flip), n, h, w, int(pad),
         m, s, ptr(out), ptr(labels), ptr(status), stream_ptr())
    return out, labels


def cifar_augment_mix(images, index, crop, flip, mean, std, pad=4, targets=None, partner=None, mode=1, lam=None,
                      box=None, out=None, labels=None, labels_b=None, status=None):
    """cifar_augment plus Mixup (mode 1: out[b] = A_b * lam[b] + A_p * (1 - lam[b])) or CutMix (mode 2: out[b] = A_p
    inside box[b] = (y0, y1, x0, x1), A_b outside) in the same launch, A the augmented batch and p = partner[b]
    (int32 [n], None: b - 1 cyclically, batch.roll(1, 0)). lam: fp32 [n]; box: uint8 [n, 4]. Returns (fp32
    [n,3,H,W], labels, labels_b) with labels_b[b] = targets[index[partner[b]]] (None without targets)."""
    require_cuda(images, index, crop, flip, targets, partner, lam, box, out, labels, labels_b, status)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError(f"images must be contiguous uint8 [N,H,W,3], got {images.dtype} {tuple(images.shape)}")
    n_images, h, w, _ = images.shape
    n = index.numel() if index is not None else (crop.shape[0] if crop is not None else n_images)
    for t, shape, dt in ((index, (n,), torch.int64), (crop, (n, 2), torch.uint8), (flip, (n,), torch.uint8),
                         (targets, (n_images,), torch.int64), (partner, (n,), torch.int32),
                         (lam, (n,), torch.float32), (box, (n, 4), torch.uint8)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"expected contiguous {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    if out is None:
        out = torch.empty(n, 3, h, w, dtype=torch.float32, device=images.device)
    if targets is not None and labels is None:
        labels = torch.empty(n, dtype=torch.int64, device=images.device)
    if targets is not None and labels_b is None:
        labels_b = torch.empty(n, dtype=torch.int64, device=images.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    call("dtc_cifar_augment_mix", ptr(images), ptr(targets), n_images, ptr(index), ptr(crop), ptr(flip), n, h, w,
         int(pad), m, s, ptr(partner), int(mode), ptr(lam), ptr(box), ptr(out), ptr(labels), ptr(labels_b),
         ptr(status), stream_ptr())
    return out, labels, labels_b


def cifar_augment_policy(images, index, crop, flip, mean, std, pad=4, targets=None, ops=None, args=None, erase=None,
                         to_u8=False, out=None, labels=None, status=None):
    """cifar_augment with a chain of policy ops per image between the flip and Normalize (RandAugment /
    TrivialAugmentWide; op codes and their arithmetic: include/dtc.h, dtc_cifar_augment_policy) and an optional
    RandomErasing box zeroed after Normalize, in one launch. ops: uint8 [n, N], N in 0..4 (None: no ops); args:
    fp32 [n, N, 6]; erase: uint8 [n, 4] = (y0, y1, x0, x1), half open (None: none). Returns (fp32 [n,3,H,W], labels)
    or, with to_u8, (uint8 [n,H,W,3] before Normalize, labels) -- the `images` of a following cifar_augment_mix
    with index = crop = flip = None and targets = these labels."""
    require_cuda(images, index, crop, flip, targets, ops, args, erase, out, labels, status)
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError(f"images must be contiguous uint8 [N,H,W,3], got {images.dtype} {tuple(images.shape)}")
    n_images, h, w, _ = images.shape
    n = index.numel() if index is not None else (crop.shape[0] if crop is not None else n_images)
    if (ops is None) != (args is None):
        raise ValueError("cifar_augment_policy: ops and args go together")
    n_ops = 0
    if ops is not None:
        if ops.dim() != 2:
            raise ValueError(f"ops must be uint8 [n, N], got {tuple(ops.shape)}")
        n_ops = int(ops.shape[1])
    if to_u8 and erase is not None:
        raise ValueError("cifar_augment_policy: erase applies to the normalized output, not with to_u8")
    for t, shape, dt in ((index, (n,), torch.int64), (crop, (n, 2), torch.uint8), (flip, (n,), torch.uint8),
                         (targets, (n_images,), torch.int64), (ops, (n, n_ops), torch.uint8),
                         (args, (n, n_ops, 6), torch.float32), (erase, (n, 4), torch.uint8)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"expected contiguous {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    if n_ops == 0:
        ops = args = None
    if to_u8:
        out = _out(out, (n, h, w, 3), torch.uint8, images.device, "cifar_augment_policy")
    else:
        out = _out(out, (n, 3, h, w), torch.float32, images.device, "cifar_augment_policy")
    if targets is not None and labels is None:
        labels = torch.empty(n, dtype=torch.int64, device=images.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(v) for v in std])
    call("dtc_cifar_augment_policy", ptr(images), ptr(targets), n_images, ptr(index), ptr(crop), ptr(flip), n, h, w,
         int(pad), m, s, ptr(ops), ptr(args), n_ops, ptr(erase), None if to_u8 else ptr(out),
         ptr(out) if to_u8 else None, ptr(labels), ptr(status), stream_ptr())
    return out, labels
