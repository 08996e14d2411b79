"""The head kernels (csrc/head.hip: pool + Linear, and their backward) at the shapes where they branch.

tests/test_gpu_ops.py runs N=6, 4x4, C=512, 100 classes, which selects the specialised paths (the weight prefetch
of head_fwd_kernel and the register path of head_dact_image, both C == 512 && ncls <= 128). The shapes here reach
the generic Linear loop and its second 64-chunk round (C > 512), pools whose thread rows do not divide the
workgroup or outnumber the pixels, the generic dact loop, the dW strips at C < 256 and C > 256, the three-kernel
backward's ragged image splits and class tiles, and ncls > 1024, where head_bwd leaves the one-launch path whatever
option head_fused says.

Every output is held element-wise to the derived bounds of tests/bounds.py against a float64 reference: feat
against the pooled mean, logits teacher-forced from the kernel's own feat, dW / db / dact from the dlogits and
feat the kernel was given. Both backward paths are checked against the reference, not against each other. The
workspace sits in a guard-band arena: the one-launch path must leave it untouched, the three-kernel path must
fill it, which also pins which path ran (head_fused 2: one launch up to 64 images).

The bias is drawn at the logits' own size: an unrounded bias differs from bf16(b) by at most 2^-9 |b|, which
shows beside the output's half-ulp only then (tests/test_bounds_cpu.py).
"""
import re

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import bounds as B
from tests.conftest import rel_err

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
EINVAL = r"code -1\)"


def _rand_bf16(shape, gen, scale=1.0):
    return O.bf16(gen.standard_normal(shape).astype(np.float32) * scale)


def _dev(a, dev, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)


FWD_CASES = [
    (3, 7, 7, 512, 128),   # prefetch path at its class limit; 49 pixels = 3 unrolled pool trips + remainder
    (2, 1, 1, 512, 10),    # prefetch path; groups (4) > HW: three pool groups sum nothing
    (3, 4, 4, 512, 129),   # one class past the limit: generic Linear at C = 512
    (2, 3, 5, 96, 129),    # tpr = 12 does not divide 256 (threads 252..255 idle); lanes r8 >= nch idle
    (5, 8, 8, 32, 7),      # smallest C: 64 pool groups; one partial 32-class pass
    (2, 4, 4, 1024, 1000),  # nch = 128: the second 64-chunk round; 32 class passes, last ragged
    (2, 2, 2, 2048, 33),   # largest C: tpr = 256, one pool group
]


@pytest.mark.parametrize("case", FWD_CASES, ids=["x".join(map(str, c)) for c in FWD_CASES])
def test_head_fwd_elementwise(dtc, cuda, case):
    N, h, w_, C, ncls = case
    g = np.random.default_rng(1000 + C + ncls)
    act = O.relu(_rand_bf16((N, h, w_, C), g))
    w = _rand_bf16((ncls, C), g, 0.05)
    bias = g.standard_normal(ncls).astype(np.float32)
    af, feat = B.arena((N, C), F32, cuda)
    al, logits = B.arena((N, ncls), F32, cuda)
    dtc.ops.head_fwd(_dev(act, cuda, BF), _dev(w, cuda, BF), _dev(bias, cuda), out=(feat, logits))
    torch.cuda.synchronize()
    feat, logits = feat.cpu().numpy(), logits.cpu().numpy()
    f_ref = act.astype(np.float64).mean(axis=(1, 2))
    rf = B.assert_within(feat, f_ref, B.head_feat_tol(f_ref, act), f"head_fwd {case} feat")
    np.testing.assert_array_equal(feat, O.bf16(feat))  # bf16 values
    l_ref, l_tol = B.head_logits_ref_tol(feat, w, bias)
    rl = B.assert_within(logits, l_ref, l_tol, f"head_fwd {case} logits")
    np.testing.assert_array_equal(logits, O.bf16(logits))
    print(f"head_fwd {case}: worst |err|/tol feat {rf:.3f}, logits {rl:.3f}; rel_err feat {rel_err(feat, f_ref):.2e}, "
          f"logits {rel_err(logits, l_ref):.2e}")
    assert af.dirty() == 0 and al.dirty() == 0, "guard words overwritten"


BWD_CASES = [
    (1, 1, 1, 512, 10),      # one image: three of the four summing waves idle
    (33, 7, 7, 512, 128),    # unfused: 2 image splits, the second holding 1 image; register dact path at its limit
    (70, 2, 3, 96, 129),     # generic dact; dW strip with 24 live lanes; 16-class tile ragged; 3 ragged splits
    (5, 4, 4, 1024, 1000),   # four 256-channel strips; dact two 64-chunk rounds; ncls <= 1024 still fused
    (3, 1, 2, 2048, 1025),   # ncls > 1024: unfused whatever head_fused says; maximum C
]
# head_fused 2: one launch up to 64 images, three kernels beyond (the first shape's geometry at both sides)
BOUNDARY = [(64, 1, 1, 512, 10), (65, 1, 1, 512, 10)]


def _bwd_inputs(dtc, cuda, case):
    N, h, w_, C, ncls = case
    g = np.random.default_rng(2000 + N + ncls)
    feat = O.relu(_rand_bf16((N, C), g))
    w = _rand_bf16((ncls, C), g, 0.05)
    logits = _dev(g.standard_normal((N, ncls)).astype(np.float32) * 3, cuda)
    lab = torch.from_numpy(g.integers(0, ncls, N)).to(cuda)
    _, lse = dtc.ops.xent_fwd(logits, lab)
    dl = dtc.ops.xent_bwd(logits, lab, lse, torch.full((1,), 16.0, device=cuda))
    return feat, w, dl


def _run_bwd(dtc, cuda, case, head_fused, fused_expected):
    N, h, w_, C, ncls = case
    scale = 0.25
    feat, w, dl = _bwd_inputs(dtc, cuda, case)
    lib = dtc._native.lib
    nb = lib.dtc_head_bwd_workspace_size(N, C, ncls)
    assert nb == ((N + 31) // 32) * ncls * (C + 1) * 4
    arenas, outs = zip(*(B.arena(s, dt, cuda) for s, dt in (((ncls, C), F32), ((ncls,), F32), ((N, h, w_, C), BF),
                                                           ((nb // 4,), F32))))
    prev = lib.dtc_get_option(b"head_fused")
    lib.dtc_set_option(b"head_fused", head_fused)
    try:
        dw, db, dact = dtc.ops.head_bwd(dl, _dev(feat, cuda), _dev(w, cuda, BF), (h, w_), scale=scale, out=outs[:3],
                                        workspace=outs[3])
        torch.cuda.synchronize()
    finally:
        lib.dtc_set_option(b"head_fused", prev)
    ws_nan = int(torch.isnan(outs[3]).sum())
    assert ws_nan == (nb // 4 if fused_expected else 0), \
        f"workspace: {ws_nan} of {nb // 4} words untouched; expected the {'one-launch' if fused_expected else 'three-kernel'} path"
    dln = dl.cpu().numpy()
    dw_ref, db_ref, dact_ref = O.head_bwd(dln, feat, w, (h, w_))
    dw_ref, db_ref = scale * dw_ref, scale * db_ref
    what = f"head_bwd {case} head_fused={head_fused}"
    dw, db, dact = dw.cpu().numpy(), db.cpu().numpy(), dact.float().cpu().numpy()
    r = (B.assert_within(dw, dw_ref, B.head_dw_tol(dln, feat, scale), what + " dW"),
         B.assert_within(db, db_ref, B.head_db_tol(dln, scale), what + " db"),
         B.assert_within(dact, dact_ref, B.head_dact_tol(dact_ref, dln, w, (h, w_)), what + " dact"))
    print(f"{what}: worst |err|/tol dW {r[0]:.3f}, db {r[1]:.3f}, dact {r[2]:.3f}; rel_err dW {rel_err(dw, dw_ref):.2e}, "
          f"db {rel_err(db, db_ref):.2e}, dact {rel_err(dact, dact_ref):.2e}")
    assert np.linalg.norm(dw_ref) > 0 and np.linalg.norm(dact_ref) > 0
    assert not any(a.dirty() for a in arenas), "guard words overwritten"


@pytest.mark.parametrize("head_fused", [1, 0])
@pytest.mark.parametrize("case", BWD_CASES, ids=["x".join(map(str, c)) for c in BWD_CASES])
def test_head_bwd_elementwise(dtc, cuda, case, head_fused):
    _run_bwd(dtc, cuda, case, head_fused, fused_expected=head_fused == 1 and case[4] <= 1024)


@pytest.mark.parametrize("case", BOUNDARY, ids=["x".join(map(str, c)) for c in BOUNDARY])
def test_head_bwd_fused_up_to_64_images(dtc, cuda, case):
    _run_bwd(dtc, cuda, case, 2, fused_expected=case[0] <= 64)


def _pattern_unchanged(arenas):
    torch.cuda.synchronize()
    return all(a.dirty() == 0 and bool((a.bits[a.g:a.g + a.n] == a.pat).all()) for a in arenas)


def test_head_refuses_unsupported_shapes(dtc, cuda):
    """DTC_EINVAL before any launch: the outputs keep their NaN pattern bit for bit."""
    P, call, st = dtc._native.ptr, dtc._native.call, dtc._native.stream_ptr
    NativeError = dtc._native.NativeError
    for C in (520, 4096):
        act = torch.zeros(1, 1, 1, C, dtype=BF, device=cuda)
        w, b = torch.zeros(4, C, dtype=BF, device=cuda), torch.zeros(4, device=cuda)
        (af, feat), (al, logits) = B.arena((1, C), F32, cuda), B.arena((1, 4), F32, cuda)
        with pytest.raises(NativeError, match=EINVAL):
            call("dtc_head_fwd", P(act), 1, 1, C, P(w), P(b), 4, P(feat), P(logits), st())
        assert _pattern_unchanged((af, al))

    def bwd(N, C, ncls, head_fused=1, short=0):
        dl, feat = torch.zeros(N, ncls, device=cuda), torch.zeros(N, C, device=cuda)
        w = torch.zeros(ncls, C, dtype=BF, device=cuda)
        nb = ((N + 31) // 32) * ncls * (C + 1) * 4
        arenas, outs = zip(*(B.arena(s, dt, cuda) for s, dt in (((ncls, C), F32), ((ncls,), F32), ((N, 1, 1, C), BF),
                                                               ((nb // 4,), F32))))
        lib = dtc._native.lib
        prev = lib.dtc_get_option(b"head_fused")
        lib.dtc_set_option(b"head_fused", head_fused)
        err = None
        try:
            call("dtc_head_bwd", P(dl), P(feat), P(w), N, 1, C, ncls, 0.25, P(outs[0]), P(outs[1]), P(outs[2]),
                 P(outs[3]), nb - short, st())
        except NativeError as e:
            err = str(e)
        finally:
            lib.dtc_set_option(b"head_fused", prev)
        return arenas, err

    for N, C, ncls in ((2, 100, 4), (2, 4096, 4), (2, 512, 4097)):
        arenas, err = bwd(N, C, ncls)
        assert err and re.search(EINVAL, err), (N, C, ncls, err)
        assert _pattern_unchanged(arenas)
    assert dtc._native.lib.dtc_head_bwd_workspace_size(33, 512, 10) == 2 * 10 * 513 * 4
    arenas, err = bwd(33, 512, 10, head_fused=0, short=4)
    assert err and re.search(EINVAL + ".*workspace too small", err), err
    assert _pattern_unchanged(arenas)
    arenas, err = bwd(33, 512, 10, head_fused=0)  # the exact size is accepted: every output and the workspace written
    torch.cuda.synchronize()
    assert err is None
    assert not any(bool(torch.isnan(a.view.float()).any()) for a in arenas) and not any(a.dirty() for a in arenas)
