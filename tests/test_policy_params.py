"""The host side of the augmentation policies (CPU only): the numpy restatement tests/policy_ref.py on hand-worked
micro-cases, and the per-epoch draws data.policy_params / data.erase_params. The launch that consumes them is
tested in test_gpu_augment_policy.py."""
import numpy as np
import pytest

from tests import policy_ref as P


def _rgb(plane):
    """One plane repeated on the three channels, uint8 [h, w, 3]."""
    return np.repeat(np.asarray(plane, np.uint8)[..., None], 3, -1)


# ----------------------------------------------------------------------------- policy_ref, hand-worked
def test_ref_equalize_and_autocontrast_on_few_level_images():
    # 32 x 16 = 512 pixels: 128 x 100, 128 x 150, 256 x 200. last bin 200, step = (512 - 256) // 255 = 1,
    # exclusive cumsum 0 / 128 / 256 -> lut 0 / 128 / min(255, 256)
    plane = np.concatenate([np.full(128, 100), np.full(128, 150), np.full(256, 200)]).reshape(32, 16)
    got = P.apply_op(_rgb(plane), P.EQUALIZE, np.zeros(6))
    want = np.concatenate([np.full(128, 0), np.full(128, 128), np.full(256, 255)]).reshape(32, 16)
    assert np.array_equal(got, _rgb(want))
    # two levels, half each: 100 -> 0, 200 -> min(255, 256)
    two = np.concatenate([np.full(256, 100), np.full(256, 200)]).reshape(32, 16)
    assert np.array_equal(P.apply_op(_rgb(two), P.EQUALIZE, np.zeros(6)), _rgb(np.where(two == 100, 0, 255)))
    # 4 x 4: step = (16 - 8) // 255 = 0, the early out
    small = _rgb(np.where(np.arange(16).reshape(4, 4) < 8, 100, 200))
    assert np.array_equal(P.apply_op(small, P.EQUALIZE, np.zeros(6)), small)
    # AutoContrast: lo 100, hi 185, scale 255 / 85 = 3 exactly: 100 -> 0, 117 -> 51, 185 -> 255; a constant
    # channel (lo == hi) stays
    img = _rgb([[100, 117], [185, 185]])
    img[..., 2] = 77
    got = P.apply_op(img, P.AUTOCONTRAST, np.zeros(6))
    assert np.array_equal(got[..., 0], [[0, 51], [255, 255]]) and np.array_equal(got[..., 1], got[..., 0])
    assert np.array_equal(got[..., 2], img[..., 2])


def test_ref_sharpness_3x3():
    # neighbours 10+20+30+40+60+70+80+90 = 400, + 5 * 100 + 6 = 906, // 13 = 69; the border is its own blur
    plane = np.array([[10, 20, 30], [40, 100, 60], [70, 80, 90]])
    blur = plane.copy()
    blur[1, 1] = 69
    assert np.array_equal(P.blur(_rgb(plane)), _rgb(blur))
    assert np.array_equal(P.apply_op(_rgb(plane), P.SHARPNESS, [0, 1, 0, 0, 0, 0]), _rgb(blur))
    sharp = plane.copy()
    sharp[1, 1] = 2 * 100 - 69
    assert np.array_equal(P.apply_op(_rgb(plane), P.SHARPNESS, [2, -1, 0, 0, 0, 0]), _rgb(sharp))


def test_ref_affine_rotation_translation_and_fill():
    a = np.arange(48, dtype=np.uint8).reshape(4, 4, 3)
    # [0, -1, 0, 1, 0, 0]: sx = -Y, sy = X, so rx = 3 - oy, ry = ox: out[oy][ox] = a[ox][3 - oy], a quarter turn
    want = np.empty_like(a)
    for oy in range(4):
        for ox in range(4):
            want[oy, ox] = a[ox, 3 - oy]
    assert np.array_equal(want, np.rot90(a, 1))
    assert np.array_equal(P.apply_op(a, P.AFFINE, [0, -1, 0, 1, 0, 0]), want)
    th = np.deg2rad(90.0)  # cos is 6e-17 here, not 0: the rounding to the nearest pixel absorbs it
    assert np.array_equal(P.apply_op(a, P.AFFINE, [np.cos(th), -np.sin(th), 0, np.sin(th), np.cos(th), 0]), want)
    assert np.array_equal(P.apply_op(a, P.AFFINE, [1, 0, 0, 0, 1, 0]), a)
    # TranslateX(1) = [1, 0, -1, 0, 1, 0]: rx = ox - 1, the image moves right and column 0 is filled with 0
    right = np.zeros_like(a)
    right[:, 1:] = a[:, :-1]
    assert np.array_equal(P.apply_op(a, P.AFFINE, [1, 0, -1, 0, 1, 0]), right)
    assert not P.apply_op(a, P.AFFINE, [1, 0, 4, 0, 1, 0]).any()  # moved out entirely
    assert not P.apply_op(a, P.AFFINE, [1, 0, 3e38, 3e38, 1, 0]).any()  # overflow to inf / NaN reads as outside


def test_ref_blends_and_pointwise_ops():
    px = np.array([[[200, 100, 50], [255, 255, 255]]], np.uint8)  # gray: trunc(124.18) = 124, trunc(254.97) = 254
    assert np.array_equal(P.gray(px), [[124, 254]])
    assert np.array_equal(P.apply_op(px, P.COLOR, [0, 1, 0, 0, 0, 0]), _rgb([[124, 254]]))
    # Contrast: m = (124 + 254) / 2 = 189
    assert np.array_equal(P.apply_op(px, P.CONTRAST, [0, 1, 0, 0, 0, 0]), _rgb([[189, 189]]))
    assert np.array_equal(P.apply_op(px, P.CONTRAST, [0.5, 0.5, 0, 0, 0, 0])[0, 0], [194, 144, 119])  # trunc(.5)
    assert np.array_equal(P.apply_op(px, P.BRIGHTNESS, [1.5, -0.5, 0, 0, 0, 0])[0], [[255, 150, 75], [255] * 3])
    assert np.array_equal(P.apply_op(px, P.BRIGHTNESS, [-1, 2, 0, 0, 0, 0]), np.zeros_like(px))  # clamped at 0
    assert np.array_equal(P.apply_op(px, P.POSTERIZE, [0xF0] + [0] * 5)[0], [[192, 96, 48], [240] * 3])
    assert np.array_equal(P.apply_op(px, P.SOLARIZE, [128] + [0] * 5)[0], [[55, 100, 50], [0] * 3])
    assert np.array_equal(P.apply_op(px, P.SOLARIZE, [256] + [0] * 5), px)
    assert np.array_equal(P.apply_op(px, P.SOLARIZE, [0] + [0] * 5), 255 - px)
    for op, g in ((10, [0] * 6), (P.BRIGHTNESS, [np.nan, 0, 0, 0, 0, 0]), (P.POSTERIZE, [3.5, 0, 0, 0, 0, 0]),
                  (P.POSTERIZE, [256, 0, 0, 0, 0, 0]), (P.SOLARIZE, [np.inf, 0, 0, 0, 0, 0])):
        assert not P.op_is_valid(op, g) and np.array_equal(P.apply_op(px, op, g), px)
    assert P.op_is_valid(P.SOLARIZE, [1, np.nan, 0, 0, 0, 0])  # an arg the op does not read


def test_ref_whole_launch_composes_with_the_existing_oracle():
    from oracle import ops as O

    g = np.random.default_rng(0)
    imgs, tg = g.integers(0, 256, (6, 8, 12, 3), dtype=np.uint8), g.integers(0, 100, 6)
    idx, crop, flip = g.integers(0, 6, 5), g.integers(0, 5, (5, 2)), g.integers(0, 2, 5)
    out, lab, u8 = P.augment_policy(imgs, tg, idx, crop, flip, O.CIFAR_MEAN, O.CIFAR_STD, 2)
    ref, ref_lab = O.cifar_augment(imgs, tg, idx, crop, flip, O.CIFAR_MEAN, O.CIFAR_STD, 2)
    assert np.array_equal(out, ref) and np.array_equal(lab, ref_lab)
    erase = np.array([[0, 8, 0, 12], [2, 2, 0, 12], [1, 3, 4, 9], [5, 2, 0, 4], [0, 9, 0, 4]], np.uint8)
    out2 = P.augment_policy(imgs, tg, idx, crop, flip, O.CIFAR_MEAN, O.CIFAR_STD, 2, erase=erase)[0]
    assert not out2[0].any() and np.array_equal(out2[[1, 3, 4]], ref[[1, 3, 4]])  # whole, empty, inverted, outside
    assert not out2[2, :, 1:3, 4:9].any() and np.array_equal(out2[2, :, 3:], ref[2, :, 3:])


# ----------------------------------------------------------------------------- policy_params
def test_randaugment_bin_zero_is_the_identity(dtc):
    """At magnitude bin 0 every op whose args depend on the magnitude is the identity under the reference
    (AutoContrast and Equalize take no magnitude; Solarize's threshold 255 still inverts a pixel of 255, so the
    image stays below it)."""
    p = dtc.data.policy_params(2, 64, 8, 12, "randaugment", 4, 0, np.random.default_rng(0))
    img = np.random.default_rng(1).integers(0, 255, (8, 12, 3), dtype=np.uint8)
    seen = set()
    for name, op, g in zip(p.name.ravel(), p.ops.ravel(), p.args.reshape(-1, 6)):
        if name < 12:
            seen.add(int(name))
            assert np.array_equal(P.apply_op(img, op, g), img), dtc.data.POLICY_OPS[name]
    assert seen == set(range(12))


def test_randaugment_draws(dtc):
    D = dtc.data
    p = D.policy_params(4, 256, 32, 32, "randaugment", 2, 9, np.random.default_rng(5))
    assert p.ops.shape == (4, 256, 2) and p.ops.dtype == np.uint8
    assert p.args.shape == (4, 256, 2, 6) and p.args.dtype == np.float32
    assert set(p.name.ravel().tolist()) == set(range(14))  # all 14 named ops occur
    kernel_op = {0: 0, 1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 2, 7: 3, 8: 4, 9: 5, 10: 6, 11: 7, 12: 8, 13: 9}
    assert all(kernel_op[int(n)] == int(o) for n, o in zip(p.name.ravel(), p.ops.ravel()))
    a, name = p.args.reshape(-1, 6), p.name.ravel()
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)
    # bin 9 of 31: shear 0.3 * 9/30, translate trunc(150/331 * 32 * 9/30) = trunc(4.35), rotate 9 degrees, blends
    # 0.27, 8 - round(9 / 7.5) = 7 bits, threshold 255 - 255 * 9/30
    s, c = np.sin(np.deg2rad(9.0)), np.cos(np.deg2rad(9.0))
    want = {1: [1, 0.09, 0, 0, 1, 0], 2: [1, 0, 0, 0.09, 1, 0], 3: [1, 0, -4, 0, 1, 0], 4: [1, 0, 0, 0, 1, -4],
            5: [c, -s, 0, s, c, 0], 6: [1.27, -0.27, 0, 0, 0, 0], 10: [0xFE, 0, 0, 0, 0, 0],
            11: [178.5, 0, 0, 0, 0, 0], 12: [0] * 6, 0: [0] * 6}
    neg = {1: [1, -0.09, 0, 0, 1, 0], 2: [1, 0, 0, -0.09, 1, 0], 3: [1, 0, 4, 0, 1, 0], 4: [1, 0, 0, 0, 1, 4],
           5: [c, s, 0, -s, c, 0], 6: [0.73, 0.27, 0, 0, 0, 0]}
    for k, w in want.items():
        rows = a[name == k]
        pos = np.all(np.isclose(rows, f32(w), rtol=1e-6, atol=1e-7), axis=1)
        if k in neg:  # signed ops: both signs occur, about half each (>= 100 draws per op here)
            ng = np.all(np.isclose(rows, f32(neg[k]), rtol=1e-6, atol=1e-7), axis=1)
            assert np.all(pos | ng) and len(rows) >= 100 and 0.3 < pos.mean() < 0.7, (k, pos.mean())
        else:
            assert np.all(pos), k
    for k in (7, 8, 9):  # the other blends share Brightness's pair
        assert set(np.round(a[name == k][:, 0].astype(np.float64), 5).tolist()) == {1.27, 0.73}
    q = D.policy_params(4, 256, 32, 32, "randaugment", 2, 9, np.random.default_rng(5))
    assert all(np.array_equal(u, v) for u, v in zip(p, q))  # equal seeds, equal arrays
    r = D.policy_params(4, 256, 32, 32, "randaugment", 2, 9, np.random.default_rng(6))
    assert not np.array_equal(p.ops, r.ops)
    for bad in (dict(policy="none"), dict(policy="autoaugment"), dict(num_ops=0), dict(num_ops=5),
                dict(magnitude=31), dict(magnitude=-1)):
        with pytest.raises(ValueError):
            D.policy_params(1, 4, 32, 32, **{"policy": "randaugment", **bad})


def test_trivialwide_stays_inside_its_ranges(dtc):
    D = dtc.data
    p = D.policy_params(8, 256, 32, 32, "trivialwide", 3, 9, np.random.default_rng(2))
    assert p.ops.shape == (8, 256, 1)  # one op per sample whatever num_ops says
    a, name = p.args.reshape(-1, 6).astype(np.float64), p.name.ravel()
    assert set(name.tolist()) == set(range(14))
    eps = 1e-6
    sh = np.concatenate([a[name == 1][:, 1], a[name == 2][:, 3]])
    assert np.abs(sh).max() <= 0.99 + eps and sh.min() < 0 < sh.max() and len(set(np.round(sh, 4))) > 20
    tr = np.concatenate([a[name == 3][:, 2], a[name == 4][:, 5]])
    assert np.abs(tr).max() <= 32 and np.array_equal(tr, np.trunc(tr)) and tr.min() < 0 < tr.max()
    rot = a[name == 5]
    ang = np.rad2deg(np.arctan2(rot[:, 3], rot[:, 0]))
    assert np.abs(ang).max() <= 135 + 1e-4 and np.abs(ang).max() > 90 and ang.min() < 0 < ang.max()
    assert np.allclose(rot[:, 0], rot[:, 4]) and np.allclose(rot[:, 1], -rot[:, 3])
    assert np.allclose(rot[:, 0] ** 2 + rot[:, 3] ** 2, 1, atol=1e-6)
    bl = a[(name >= 6) & (name <= 9)]
    assert bl[:, 0].min() >= 0.01 - eps and bl[:, 0].max() <= 1.99 + eps and np.allclose(bl[:, 0] + bl[:, 1], 1)
    # 8 - round(arange(31) / 5): 8 down to 2 bits
    assert set(a[name == 10][:, 0].tolist()) == {float(0xFF & (0xFF << (8 - b))) for b in range(2, 9)}
    so = a[name == 11][:, 0]
    assert so.min() >= 0 and so.max() <= 255 and len(set(so.tolist())) > 20
    assert not a[(name == 0) | (name >= 12)].any()
    q = D.policy_params(8, 256, 32, 32, "trivialwide", 1, 0, np.random.default_rng(2))
    assert all(np.array_equal(u, v) for u, v in zip(p, q))  # num_ops and magnitude play no part


# ----------------------------------------------------------------------------- erase_params
def test_erase_params(dtc):
    """Boxes lie inside the image; a box of round(sqrt(A r)) x round(sqrt(A / r)) with A in [0.02, 0.33] h w and r
    in [0.3, 3.3] has an area within A -/+ (0.5 sqrt(A) (sqrt(r) + 1 / sqrt(r)) + 0.25) of A (each side is within
    0.5 of its root, and sqrt(r) + 1 / sqrt(r) <= 2.38 on that interval): [15.35, 360.1] at 32 x 32.
    An attempt fits unless round(sqrt(A r)) >= 32 or round(sqrt(A / r)) >= 32, which needs r >= 2.93 or
    r <= 0.341: at most 0.102 of the log-uniform draws, so ten attempts all fail with probability <= 1.2e-10 and
    prob = 1 leaves no sample of the 8192 here without a box (measured share of empty boxes: 0.0)."""
    D = dtc.data
    h = w = 32
    box = D.erase_params(32, 256, h, w, 1.0, np.random.default_rng(3)).astype(np.int64)
    assert box.shape == (32, 256, 4)
    y0, y1, x0, x1 = (box[..., i] for i in range(4))
    assert np.all((0 <= y0) & (y0 <= y1) & (y1 <= h) & (0 <= x0) & (x0 <= x1) & (x1 <= w))
    assert np.all((y1 - y0 < h) & (x1 - x0 < w))
    area = (y1 - y0) * (x1 - x0)
    empty = area == 0
    print("share of empty boxes at prob = 1:", empty.mean())
    assert empty.mean() == 0.0
    slack = lambda A: 0.5 * np.sqrt(A) * 2.38 + 0.25
    lo, hi = 0.02 * h * w, 0.33 * h * w
    assert area.min() >= lo - slack(lo) and area.max() <= hi + slack(hi)
    assert area.min() < 40 and area.max() > 250  # the scale range is used
    ratio = (y1 - y0) / (x1 - x0)
    assert (ratio < 0.5).any() and (ratio > 2).any()
    assert y0.min() == 0 and x0.min() == 0 and y1.max() == h and x1.max() == w  # corners reach every edge
    half = D.erase_params(32, 256, h, w, 0.25, np.random.default_rng(3))
    share = (half.reshape(-1, 4).astype(np.int64) @ [-1, 1, 0, 0] > 0).mean()
    assert 0.2 < share < 0.3  # 8192 Bernoulli(0.25) draws: sd 0.005
    assert not D.erase_params(4, 16, h, w, 0.0, np.random.default_rng(3)).any()
    again = D.erase_params(32, 256, h, w, 1.0, np.random.default_rng(3))
    assert np.array_equal(again, box.astype(np.uint8))
    small = D.erase_params(8, 64, 8, 12, 1.0, np.random.default_rng(4)).astype(np.int64)
    assert np.all((small[..., 1] <= 8) & (small[..., 3] <= 12) & (small[..., 0] <= small[..., 1])
                  & (small[..., 2] <= small[..., 3]))
    for bad in (dict(prob=1.5), dict(prob=-0.1), dict(h=256)):
        with pytest.raises(ValueError):
            D.erase_params(1, 4, **{"h": 32, "w": 32, "prob": 0.5, **bad})
