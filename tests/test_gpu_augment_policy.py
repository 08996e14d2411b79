"""The augmentation-policy input launch (dtc_cifar_augment_policy: RandAugment / TrivialAugmentWide op chains and
RandomErasing between the existing crop / flip and Normalize): BIT-EXACT against the numpy restatement
tests/policy_ref.py, whose crop, flip and Normalize parts are the existing oracle's; the status flagging, stray
stores, the uint8 output that feeds the Mixup / CutMix launch, and the DeviceLoader's epoch stream.

Images are drawn in [40, 200): on full-range noise AutoContrast is the identity. Every (op, shape) case is checked
against being vacuous: the reference must change at least a quarter of the batch's pixels (Equalize at 8 x 12 has
step == 0 and must be exactly the identity, the early-out path)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import ops as O
from tests import policy_ref as P
from tests.bounds import Arena

pytestmark = pytest.mark.gpu

MEAN, STD = O.CIFAR_MEAN, O.CIFAR_STD
SHAPES = [(32, 32, 4, 37), (8, 12, 2, 19), (32, 32, 4, 5), (32, 32, 4, 1)]  # ten workgroups, ragged last; non-square
NAN = float("nan")


def _rot(deg, scale=1.0):
    t = np.deg2rad(deg)
    return [scale * np.cos(t), -scale * np.sin(t), 0, scale * np.sin(t), scale * np.cos(t), 0]


# per op: the args of row r are ARGS[op][r % len]; the first entry is a nominal one (the n = 1 shape runs it alone),
# the edge rows follow: blends with g0 = 1, g1 = 0; Solarize 0 and 256; Posterize 0 and 255; the identity matrix; a
# translation that moves the image out entirely. Ops 0, 8 and 9 read no arg: theirs are garbage.
_BLEND = [[1.27, -0.27], [0.4, 0.6], [1.5, -0.5], [1, 0], [1.9, -0.9], [0, 1], [0.73, 0.27]]
ARGS = {
    0: [[NAN, float("inf"), -1e30, 7, NAN, 3]],
    1: [_rot(20), [1, 0.3, 0, 0, 1, 0], [1, 0, -3, 0, 1, 2], [1, 0, 0, 0, 1, 0], [1, 0, 100, 0, 1, 0],
        [1, 0, 0, -0.3, 1, 0], _rot(-135, 1.2), [1, 0, 0, 0, 1, -40]],
    6: [[0xF0], [0x80], [0xFE], [0], [255], [0xC0], [0xE0]],
    7: [[128], [100], [150], [0], [256], [60], [178.5]],
    8: [[NAN] * 6],
    9: [[NAN, NAN, float("-inf"), 1, 2, 3]],
}
for _op in (2, 3, 4, 5):
    ARGS[_op] = _BLEND


def _args_of(op, r):
    g = list(ARGS[op][r % len(ARGS[op])])
    return g + [0.0] * (6 - len(g))


def _data(h, w, n_img=50, seed=0):
    g = np.random.default_rng(seed)
    return g.integers(40, 200, (n_img, h, w, 3), dtype=np.uint8), g.integers(0, 100, n_img, dtype=np.int64)


def _params(n, pad, n_img=50, seed=1):
    g = np.random.default_rng(seed)
    idx = g.integers(0, n_img, n)
    crop = g.integers(0, 2 * pad + 1, (n, 2)).astype(np.uint8)
    crop[0] = (0, 2 * pad)
    flip = g.integers(0, 2, n).astype(np.uint8)
    return g, idx, crop, flip


def _D(cuda):
    return lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run(dtc, cuda, imgs, tg, idx, crop, flip, pad, ops=None, args=None, erase=None, **kw):
    """(out, labels, status) of one launch, as numpy."""
    D = _D(cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    out, lab = dtc.ops.cifar_augment_policy(D(imgs), D(idx), D(crop), D(flip), MEAN, STD, pad, targets=D(tg),
                                            ops=D(ops), args=D(args), erase=D(erase), status=status, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lab.cpu().numpy(), int(status.item())


def single_op_case(op, h, w, pad, n):
    """(inputs, ops, args, reference) of `op` alone on every row, args varied per row."""
    imgs, tg = _data(h, w)
    _, idx, crop, flip = _params(n, pad)
    ops = np.full((n, 1), op, np.uint8)
    args = np.array([[_args_of(op, r)] for r in range(n)], np.float32)
    before = P.crop_flip(imgs, idx, crop, flip, pad)
    ref, lab, u8 = P.augment_policy(imgs, tg, idx, crop, flip, MEAN, STD, pad, ops, args)
    return (imgs, tg, idx, crop, flip), ops, args, (ref, lab, u8, before)


def chain_case(n_ops, h, w, pad, n, seed=7):
    """Random op sequences per row. The first workgroup's four images start in four different reduce / table /
    apply classes (Contrast, AutoContrast, Equalize, an element-wise op); the last row -- in the ragged last
    workgroup at every test shape -- runs AutoContrast then Equalize."""
    imgs, tg = _data(h, w)
    g, idx, crop, flip = _params(n, pad)
    ops = g.integers(0, 10, (n, n_ops)).astype(np.uint8)
    ops[:4, 0] = [4, 8, 9, 2][:min(n, 4)]
    if n > 4:
        ops[n - 1, 0] = 8
    ops[n - 1, 1] = 9
    args = np.array([[_args_of(int(ops[r, k]), int(g.integers(0, 64))) for k in range(n_ops)] for r in range(n)],
                    np.float32)
    return (imgs, tg, idx, crop, flip), ops, args


@pytest.mark.parametrize("h,w,pad,n", SHAPES)
def test_identity_equals_the_plain_launch(dtc, cuda, h, w, pad, n):
    imgs, tg = _data(h, w)
    _, idx, crop, flip = _params(n, pad)
    ref, ref_lab = O.cifar_augment(imgs, tg, idx, crop, flip, MEAN, STD, pad)
    out, lab, st = _run(dtc, cuda, imgs, tg, idx, crop, flip, pad)
    assert np.array_equal(out, ref) and np.array_equal(lab, ref_lab) and st == 0
    ops = np.zeros((n, 3), np.uint8)
    args = np.array([[_args_of(0, 0)] * 3] * n, np.float32)  # garbage, NaN and inf included: Identity reads none
    out, lab, st = _run(dtc, cuda, imgs, tg, idx, crop, flip, pad, ops, args)
    assert np.array_equal(out, ref) and np.array_equal(lab, ref_lab) and st == 0
    # and without index / crop / flip (the valid transform's centre window)
    D = _D(cuda)
    out, lab = dtc.ops.cifar_augment_policy(D(imgs), None, None, None, MEAN, STD, pad, targets=D(tg))
    ref, ref_lab = O.cifar_augment(imgs, tg, None, None, None, MEAN, STD, pad)
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(lab.cpu().numpy(), ref_lab)


@pytest.mark.parametrize("h,w,pad,n", SHAPES)
@pytest.mark.parametrize("op", range(1, 10))
def test_each_op_alone(dtc, cuda, op, h, w, pad, n):
    inputs, ops, args, (ref, ref_lab, u8, before) = single_op_case(op, h, w, pad, n)
    changed = float((u8 != before).mean())
    print(f"op {op} {h}x{w} n={n}: reference changes {changed:.3f} of the pixels")
    if op == 9 and h * w < 255:
        assert changed == 0.0  # step == 0: the early out, exactly the identity
    else:
        assert changed >= 0.25
    out, lab, st = _run(dtc, cuda, *inputs, pad, ops, args)
    assert out.dtype == np.float32 and ref.dtype == np.float32
    assert np.array_equal(out, ref), (op, int((out != ref).sum()))
    assert np.array_equal(lab, ref_lab) and st == 0


@pytest.mark.parametrize("h,w,pad,n", SHAPES)
@pytest.mark.parametrize("n_ops", [2, 3, 4])
def test_chains(dtc, cuda, n_ops, h, w, pad, n):
    inputs, ops, args = chain_case(n_ops, h, w, pad, n)
    if n >= 4:
        assert sorted(ops[:4, 0].tolist()) == [2, 4, 8, 9]
    assert n % 4 != 0 and set(ops[n - 1, :2].tolist()) & {4, 8, 9}  # a reduce op in the ragged last workgroup
    ref, ref_lab, u8 = P.augment_policy(*inputs, MEAN, STD, pad, ops, args)
    out, lab, st = _run(dtc, cuda, *inputs, pad, ops, args)
    assert np.array_equal(out, ref), int((out != ref).sum())
    assert np.array_equal(lab, ref_lab) and st == 0
    got_u8, lab, st = _run(dtc, cuda, *inputs, pad, ops, args, to_u8=True)
    assert got_u8.dtype == np.uint8 and np.array_equal(got_u8, u8) and st == 0


@pytest.mark.parametrize("h,w,pad,n", [(64, 64, 4, 3), (32, 48, 4, 5), (16, 32, 2, 9)])
def test_fewer_images_per_workgroup(dtc, cuda, h, w, pad, n):
    """Above 3 KiB per image a workgroup holds fewer than four: one at 64 x 64 (the 12 KiB limit, both LDS buffers
    full), two at 32 x 48 (ragged at n = 5); 16 x 32 holds four of 1.5 KiB. Every op alone, then chains of four with
    an erase box, fp32 and uint8 outputs."""
    for op in range(1, 10):
        inputs, ops, args, (ref, ref_lab, u8, before) = single_op_case(op, h, w, pad, n)
        assert (u8 != before).mean() >= 0.25
        out, lab, st = _run(dtc, cuda, *inputs, pad, ops, args)
        assert np.array_equal(out, ref), op
        assert np.array_equal(lab, ref_lab) and st == 0
    inputs, ops, args = chain_case(4, h, w, pad, n, seed=29)
    box = _boxes(np.random.default_rng(2), n, h, w)
    ref, ref_lab, u8 = P.augment_policy(*inputs, MEAN, STD, pad, ops, args, erase=box)
    out, lab, st = _run(dtc, cuda, *inputs, pad, ops, args, erase=box)
    assert np.array_equal(out, ref) and np.array_equal(lab, ref_lab) and st == 0
    got_u8, _, st = _run(dtc, cuda, *inputs, pad, ops, args, to_u8=True)
    assert np.array_equal(got_u8, u8) and st == 0
    with pytest.raises(dtc.NativeError, match="bad shape"):
        _run(dtc, cuda, *_data(64, 68, 4)[:2], None, None, None, pad)


def _boxes(g, n, h, w):
    y = np.sort(g.integers(0, h + 1, (n, 2)), 1)
    x = np.sort(g.integers(0, w + 1, (n, 2)), 1)
    box = np.concatenate([y, x], 1).astype(np.uint8)
    box[0] = (0, h, 0, w)  # the whole image
    if n > 2:
        box[n // 2] = (3, 3, 0, w)  # empty
        box[n - 1] = (0, h, 2, 2)   # empty
    return box


@pytest.mark.parametrize("h,w,pad,n", SHAPES)
def test_erase(dtc, cuda, h, w, pad, n):
    inputs, ops, args = chain_case(2, h, w, pad, n, seed=9)
    box = _boxes(np.random.default_rng(11), n, h, w)
    plain, _, _ = P.augment_policy(*inputs, MEAN, STD, pad, ops, args)
    ref, ref_lab, _ = P.augment_policy(*inputs, MEAN, STD, pad, ops, args, erase=box)
    out, lab, st = _run(dtc, cuda, *inputs, pad, ops, args, erase=box)
    assert np.array_equal(out, ref) and np.array_equal(lab, ref_lab) and st == 0
    ys, xs = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    b = box.astype(np.int64)
    inside = (ys >= b[:, 0, None, None]) & (ys < b[:, 1, None, None]) & (xs >= b[:, 2, None, None]) \
        & (xs < b[:, 3, None, None])
    inside = np.broadcast_to(inside[:, None], out.shape)
    assert not out[inside].any() and not np.signbit(out[inside]).any()  # exactly +0.0f
    assert np.array_equal(out[~inside], plain[~inside])  # untouched outside
    assert inside[0].all() and (n <= 2 or not inside[n // 2].any())
    # erase alone, no ops: the plain launch outside the boxes
    ref0, _ = O.cifar_augment(*inputs, MEAN, STD, pad)
    out0, _, st = _run(dtc, cuda, *inputs, pad, erase=box)
    assert st == 0 and not out0[inside].any() and np.array_equal(out0[~inside], ref0[~inside])


def test_bad_erase_boxes_flag_status_and_leave_the_row(dtc, cuda):
    h, w, pad, n = 32, 32, 4, 11
    inputs, ops, args = chain_case(2, h, w, pad, n, seed=13)
    box = _boxes(np.random.default_rng(12), n, h, w)
    plain, _, _ = P.augment_policy(*inputs, MEAN, STD, pad, ops, args)
    for bad in ((9, 4, 0, 8), (0, 8, 20, 10), (0, 33, 0, 8), (0, 8, 0, 200)):  # inverted, leaves the image
        bb = box.copy()
        bb[6] = bad
        out, _, st = _run(dtc, cuda, *inputs, pad, ops, args, erase=bb)
        assert st == 1, bad
        assert np.array_equal(out[6], plain[6])  # unerased
        assert np.array_equal(out, P.augment_policy(*inputs, MEAN, STD, pad, ops, args, erase=bb)[0])
    with pytest.raises(ValueError):
        _run(dtc, cuda, *inputs, pad, ops, args, erase=box, to_u8=True)


@pytest.mark.parametrize("h,w,pad,n", SHAPES)
def test_u8_output_feeds_the_plain_and_mix_launches(dtc, cuda, h, w, pad, n):
    inputs, ops, args = chain_case(3, h, w, pad, n, seed=17)
    ref, ref_lab, u8 = P.augment_policy(*inputs, MEAN, STD, pad, ops, args)
    D = _D(cuda)
    got, lab = dtc.ops.cifar_augment_policy(*(D(a) for a in inputs[:1]), *(D(a) for a in inputs[2:]), MEAN, STD, pad,
                                            targets=D(inputs[1]), ops=D(ops), args=D(args), to_u8=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
    assert np.array_equal(got.cpu().numpy(), u8) and np.array_equal(lab.cpu().numpy(), ref_lab)
    out, lab2 = dtc.ops.cifar_augment(got, None, None, None, MEAN, STD, pad, targets=lab)
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(lab2.cpu().numpy(), ref_lab)
    # CutMix of the augmented batch with itself rolled by one row, as the DeviceLoader composes it
    box = _boxes(np.random.default_rng(5), n, h, w)
    x, la, lb = dtc.ops.cifar_augment_mix(got, None, None, None, MEAN, STD, pad, targets=lab, mode=2, box=D(box))
    assert np.array_equal(x.cpu().numpy(), _cutmix(ref, box))
    assert np.array_equal(la.cpu().numpy(), ref_lab) and np.array_equal(lb.cpu().numpy(), np.roll(ref_lab, 1))


def _cutmix(A, box):
    """The numpy CutMix rule of test_gpu_mix_augment.py with the partner b - 1 (cyclically)."""
    h, w = A.shape[2:]
    ys, xs = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    b = np.asarray(box).astype(np.int64)
    m = (ys >= b[:, 0, None, None]) & (ys < b[:, 1, None, None]) & (xs >= b[:, 2, None, None]) & (xs < b[:, 3, None, None])
    return np.where(m[:, None], np.roll(A, 1, 0), A)


@pytest.mark.parametrize("what,op,g", [("op code 10", 10, [1, 0, 0, 0, 0, 0]), ("op code 255", 255, [0] * 6),
                                       ("NaN blend arg", 2, [1.2, NAN, 0, 0, 0, 0]),
                                       ("inf affine arg", 1, [1, 0, 0, 0, 1, float("inf")]),
                                       ("Posterize 3.5", 6, [3.5, 0, 0, 0, 0, 0]),
                                       ("Posterize 256", 6, [256, 0, 0, 0, 0, 0]),
                                       ("Posterize -1", 6, [-1, 0, 0, 0, 0, 0]),
                                       ("NaN Solarize", 7, [NAN, 0, 0, 0, 0, 0])])
def test_bad_ops_flag_status_and_act_as_identity(dtc, cuda, what, op, g):
    h, w, pad, n = 32, 32, 4, 11
    inputs, ops, args = chain_case(3, h, w, pad, n, seed=19)
    ops[6, 1], args[6, 1] = op, g
    assert not P.op_is_valid(op, g)
    ref, ref_lab, _ = P.augment_policy(*inputs, MEAN, STD, pad, ops, args)  # the reference skips the bad op
    out, lab, st = _run(dtc, cuda, *inputs, pad, ops, args)
    assert st == 1, what
    assert np.array_equal(out, ref) and np.array_equal(lab, ref_lab)  # row 6 and every other row
    ops[6, 1], args[6, 1] = 0, 0  # ... which is the same chain with the Identity in its place
    assert np.array_equal(ref, P.augment_policy(*inputs, MEAN, STD, pad, ops, args)[0])


def test_wrapper_and_index_status(dtc, cuda):
    imgs, tg = _data(32, 32)
    _, idx, crop, flip = _params(9, 4)
    bad = idx.copy()
    bad[2] = 50
    assert _run(dtc, cuda, imgs, tg, bad, crop, flip, 4)[2] == 1
    D = _D(cuda)
    ops, args = np.zeros((9, 5), np.uint8), np.zeros((9, 5, 6), np.float32)
    with pytest.raises(dtc.NativeError, match="n_ops"):
        dtc.ops.cifar_augment_policy(D(imgs), D(idx), D(crop), D(flip), MEAN, STD, 4, ops=D(ops), args=D(args))
    with pytest.raises(ValueError):
        dtc.ops.cifar_augment_policy(D(imgs), D(idx), D(crop), D(flip), MEAN, STD, 4, ops=D(ops[:, :2]))
    with pytest.raises(ValueError):
        dtc.ops.cifar_augment_policy(D(imgs), D(idx), D(crop), D(flip), MEAN, STD, 4, ops=D(ops[:8, :2]),
                                     args=D(args[:8, :2]))


@pytest.mark.parametrize("h,w,pad,n", SHAPES[:2])
def test_no_stray_stores(dtc, cuda, h, w, pad, n):
    inputs, ops, args = chain_case(4, h, w, pad, n, seed=23)
    box = _boxes(np.random.default_rng(3), n, h, w)
    ref, ref_lab, u8 = P.augment_policy(*inputs, MEAN, STD, pad, ops, args, erase=box)
    D = _D(cuda)
    dev = [D(a) for a in inputs]
    a_out, a_lab = Arena((n, 3, h, w), torch.float32, cuda), Arena((n,), torch.int64, cuda)
    dtc.ops.cifar_augment_policy(dev[0], dev[2], dev[3], dev[4], MEAN, STD, pad, targets=dev[1], ops=D(ops),
                                 args=D(args), erase=D(box), out=a_out.view, labels=a_lab.view)
    torch.cuda.synchronize()
    assert a_out.dirty() == 0 and a_lab.dirty() == 0
    assert np.array_equal(a_out.view.cpu().numpy(), ref) and np.array_equal(a_lab.view.cpu().numpy(), ref_lab)
    # the uint8 output, embedded as the bytes of an int32 arena
    a_u8, a_lab = Arena((n * h * w * 3 // 4,), torch.int32, cuda), Arena((n,), torch.int64, cuda)
    view = a_u8.view.view(torch.uint8).view(n, h, w, 3)
    dtc.ops.cifar_augment_policy(dev[0], dev[2], dev[3], dev[4], MEAN, STD, pad, targets=dev[1], ops=D(ops),
                                 args=D(args), to_u8=True, out=view, labels=a_lab.view)
    torch.cuda.synchronize()
    assert a_u8.dirty() == 0 and a_lab.dirty() == 0
    assert np.array_equal(view.cpu().numpy(), u8)


# ----------------------------------------------------------------------------- DeviceLoader
def _loader(dtc, cuda, imgs, tg, seed=1, **kw):
    return dtc.data.DeviceLoader(imgs, tg, 16, device=cuda, seed=seed, **kw)


def _np(t):
    return None if t is None else t.cpu().numpy()


def test_device_loader_policy_epoch(dtc, cuda):
    """64 images, batch 16, RandAugment (3 ops) with RandomErasing 0.5: every batch equals the reference applied
    with last_params and last_policy, which are the epoch's host draws from default_rng([seed + epoch, 1]); the
    crop / flip stream is the plain loader's; equal (seed, epoch) give one stream, epochs differ."""
    imgs, tg = _data(32, 32, 64, seed=4)
    kw = dict(policy="randaugment", policy_num_ops=3, policy_magnitude=12, erase_prob=0.5)
    plain = _loader(dtc, cuda, imgs, tg)
    streams = []
    for rep in range(2):
        loader = _loader(dtc, cuda, imgs, tg, **kw)
        stream = []
        for epoch in (0, 1):
            loader.set_epoch(epoch)
            plain.set_epoch(epoch)
            rng = np.random.default_rng([1 + epoch, 1])
            want = dtc.data.policy_params(4, 16, 32, 32, "randaugment", 3, 12, rng)
            want_erase = dtc.data.erase_params(4, 16, 32, 32, 0.5, rng)
            it = iter(plain)
            for k, (x, y) in enumerate(loader):
                next(it)
                assert len(loader.last_params) == 3
                for a, b in zip(loader.last_params, plain.last_params):
                    assert torch.equal(a, b)
                idx, crop, flip = (_np(t) for t in loader.last_params)
                ops, args, erase = (_np(t) for t in loader.last_policy)
                assert np.array_equal(ops, want.ops[k]) and np.array_equal(args, want.args[k])
                assert np.array_equal(erase, want_erase[k])
                ref, lab, _ = P.augment_policy(imgs, tg, idx, crop, flip, MEAN, STD, 4, ops, args, erase)
                assert np.array_equal(x.cpu().numpy(), ref) and np.array_equal(y.cpu().numpy(), lab)
                stream.append((x.cpu().numpy(), y.cpu().numpy()))
            assert k == 3
        assert int(loader.status.item()) == 0
        streams.append(stream)
    for a, b in zip(streams[0], streams[1]):
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert not np.array_equal(streams[0][0][0], streams[0][4][0])  # epoch 1 differs from epoch 0
    with pytest.raises(ValueError):
        _loader(dtc, cuda, imgs, tg, train=False, policy="randaugment")


def test_device_loader_policy_then_cutmix(dtc, cuda):
    """TrivialAugmentWide with a CutMix alpha: the mixed batch is the existing numpy mix (the partner b - 1) of the
    policy-augmented batch; the Mixup / CutMix parameter stream is the one of a loader without a policy."""
    imgs, tg = _data(32, 32, 64, seed=4)
    loader = _loader(dtc, cuda, imgs, tg, policy="trivialwide", cutmix_alpha=1.0)
    nopol = _loader(dtc, cuda, imgs, tg, cutmix_alpha=1.0)
    expect = dtc.data.mix_params(4, 16, 32, 32, 0.0, 1.0, 1.0, np.random.default_rng(1))
    it = iter(nopol)
    for k, (x, y) in enumerate(loader):
        next(it)
        idx, crop, flip, mix = loader.last_params
        assert mix["mode"] == 2 and nopol.last_params[3]["mode"] == 2
        assert torch.equal(mix["box"], nopol.last_params[3]["box"]) and np.array_equal(_np(mix["box"]), expect.box[k])
        ops, args, erase = (_np(t) for t in loader.last_policy)
        assert erase is None and ops.shape == (16, 1)
        A, lab, _ = P.augment_policy(imgs, tg, _np(idx), _np(crop), _np(flip), MEAN, STD, 4, ops, args)
        assert isinstance(y, dtc.MixedTarget)
        assert np.array_equal(x.cpu().numpy(), _cutmix(A, expect.box[k]))
        assert np.array_equal(_np(y.labels_a), lab) and np.array_equal(_np(y.labels_b), np.roll(lab, 1))
        assert np.array_equal(_np(y.lam), expect.lam[k])
    assert k == 3 and int(loader.status.item()) == 0


def test_device_loader_defaults_issue_todays_launches(dtc, cuda):
    imgs, tg = _data(32, 32, 64, seed=4)
    a = _loader(dtc, cuda, imgs, tg)
    b = _loader(dtc, cuda, imgs, tg, policy="none", policy_num_ops=2, policy_magnitude=9, erase_prob=0.0)
    b._ops = types.SimpleNamespace(cifar_augment=dtc.ops.cifar_augment)  # any other launch would be an error
    for (xa, ya), (xb, yb) in zip(a, b):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
        assert len(b.last_params) == 3 and b.last_policy is None
        ref, lab = O.cifar_augment(imgs, tg, *(_np(t) for t in a.last_params), MEAN, STD, 4)
        assert np.array_equal(xa.cpu().numpy(), ref) and np.array_equal(ya.cpu().numpy(), lab)


def test_single_trainer_with_policy_flags(dtc, cuda, tmp_path):
    """`train.py single --amp --device-data --auto-augment randaugment --random-erasing 0.25 --epoch 1 --max-steps 3
    --synthetic-train 2048`: three steps, a finite training loss."""
    flags = ["--amp", "--device-data", "--auto-augment", "randaugment", "--random-erasing", "0.25", "--epoch", "1",
             "--max-steps", "3", "--synthetic-train", "2048", "--synthetic-test", "128", "--ckpt-path", str(tmp_path)]
    t = dtc.trainer.main(flags, "single")
    assert t.train_loader.policing and not t.val_loader.policing and not t.test_loader.policing
    assert t.global_step == 3 and int(t.train_loader.status.item()) == 0
    ops, args, erase = t.train_loader.last_policy
    assert tuple(ops.shape[1:]) == (2,) and tuple(erase.shape[1:]) == (4,) and t.val_loader.last_policy is None
    t._scalars.flush()
    with open(os.path.join(t.save_path, "scalars.jsonl")) as f:
        rows = [json.loads(line) for line in f]
    train = [r["train"] for r in rows if r["tag"] == "loss/epoch"]
    assert len(train) == 1 and np.isfinite(train[0]) and train[0] > 0
    assert torch.isfinite(t.model.flat.params).all().item()
