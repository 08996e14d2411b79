"""From-scratch numpy restatement of the policy ops of dtc_cifar_augment_policy (include/dtc.h): the oracle of
tests/test_gpu_augment_policy.py. It follows torchvision's uint8 tensor path with two deliberate departures, both
for exactness: Sharpness's blur is rounded in integers, (sum + 6) // 13, and the affine ops take the nearest source
pixel by the rule stated below. torchvision is not installed where this suite runs, so parity with it is unpinned.

Every fp32 expression is evaluated in the written order, one rounding per operation (numpy float32 arithmetic
never fuses a multiply with an add). Conversions to uint8 clamp to [0, 255], then truncate toward zero.
Images are uint8 [h, w, 3]; `g` holds the op's six fp32 args.
"""
import numpy as np

from oracle import ops as O

F = np.float32
IDENTITY, AFFINE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE = range(10)
N_READ = {0: 0, 1: 6, 2: 2, 3: 2, 4: 2, 5: 2, 6: 1, 7: 1, 8: 0, 9: 0}  # args the op reads


def to_u8(s):
    """clamp to [0, 255], truncate."""
    s = np.asarray(s, F)
    return np.where(s >= 0, np.where(s <= 255, s, F(255)), F(0)).astype(np.int64).astype(np.uint8)


def gray(a):
    """trunc((0.2989 R + 0.587 G) + 0.114 B) per pixel, int64 [h, w]."""
    r, g, b = (a[..., c].astype(F) for c in range(3))
    return ((F(0.2989) * r + F(0.587) * g) + F(0.114) * b).astype(np.int64)


def blend(a, other, g0, g1):
    """g0 * a + g1 * other: two rounded products, one rounded add."""
    return to_u8(F(g0) * a.astype(F) + F(g1) * np.asarray(other, F))


def affine(a, g):
    h, w, _ = a.shape
    g = np.asarray(g, F)
    ox, oy = np.arange(w, dtype=F)[None, :], np.arange(h, dtype=F)[:, None]
    X = (ox + F(0.5)) - F(0.5) * F(w)
    Y = (oy + F(0.5)) - F(0.5) * F(h)
    with np.errstate(over="ignore", invalid="ignore"):
        sx = (g[0] * X + g[1] * Y) + g[2]
        sy = (g[3] * X + g[4] * Y) + g[5]
        rx = np.rint(sx + (F(0.5) * F(w) - F(0.5)))
        ry = np.rint(sy + (F(0.5) * F(h) - F(0.5)))
        inside = (rx >= 0) & (rx <= F(w) - F(1)) & (ry >= 0) & (ry <= F(h) - F(1))
    ix = np.where(inside, rx, 0).astype(np.int64)
    iy = np.where(inside, ry, 0).astype(np.int64)
    return np.where(inside[..., None], a[iy, ix], 0).astype(np.uint8)


def blur(a):
    """a on the border; inside (8 neighbours + 5 * centre + 6) // 13 in integers."""
    h, w, _ = a.shape
    out = a.astype(np.int64)
    if h < 3 or w < 3:
        return out
    v = a.astype(np.int64)
    s = np.zeros((h - 2, w - 2, 3), np.int64)
    for dy in range(3):
        for dx in range(3):
            s += v[dy:dy + h - 2, dx:dx + w - 2] * (5 if dy == 1 and dx == 1 else 1)
    out[1:-1, 1:-1] = (s + 6) // 13
    return out


def autocontrast(a):
    out = a.copy()
    for c in range(3):
        lo, hi = int(a[..., c].min()), int(a[..., c].max())
        if lo != hi:
            scale = F(255.0) / F(hi - lo)
            out[..., c] = to_u8((a[..., c].astype(F) - F(lo)) * scale)
    return out


def equalize(a):
    h, w, _ = a.shape
    out = a.copy()
    for c in range(3):
        hist = np.bincount(a[..., c].ravel(), minlength=256).astype(np.int64)
        last = int(np.flatnonzero(hist)[-1])
        step = (h * w - int(hist[last])) // 255
        if step == 0:
            continue
        excl = np.cumsum(hist) - hist
        lut = np.minimum(255, (excl + step // 2) // step).astype(np.uint8)
        out[..., c] = lut[a[..., c]]
    return out


def op_is_valid(op, g):
    g = np.asarray(g, F)
    if op > 9 or not np.all(np.isfinite(g[:N_READ.get(int(op), 0)])):
        return False
    if op == POSTERIZE and not (0 <= g[0] <= 255 and g[0] == np.trunc(g[0])):
        return False
    return True


def apply_op(a, op, g):
    """One op on one uint8 [h, w, 3] image; an invalid op (op_is_valid) is the Identity."""
    op = int(op)
    g = np.asarray(g, F)
    if op == IDENTITY or not op_is_valid(op, g):
        return a.copy()
    if op == AFFINE:
        return affine(a, g)
    if op == BRIGHTNESS:
        return blend(a, np.zeros(a.shape, F), g[0], g[1])
    if op == COLOR:
        return blend(a, gray(a)[..., None], g[0], g[1])
    if op == CONTRAST:
        h, w, _ = a.shape
        return blend(a, F(int(gray(a).sum())) / F(h * w), g[0], g[1])
    if op == SHARPNESS:
        return blend(a, blur(a), g[0], g[1])
    if op == POSTERIZE:
        return a & np.uint8(int(g[0]))
    if op == SOLARIZE:
        return np.where(a.astype(F) >= g[0], 255 - a, a).astype(np.uint8)
    if op == AUTOCONTRAST:
        return autocontrast(a)
    return equalize(a)


def crop_flip(images, index, crop, flip, pad):
    """The uint8 [n, h, w, 3] batch after gather, zero-padded crop and flip (oracle.ops.cifar_augment's rule)."""
    images = np.asarray(images, np.uint8)
    n_img, h, w, _ = images.shape
    index = np.arange(n_img) if index is None else np.asarray(index, np.int64)
    padded = np.zeros((n_img, h + 2 * pad, w + 2 * pad, 3), np.uint8)
    padded[:, pad:pad + h, pad:pad + w] = images
    out = np.empty((len(index), h, w, 3), np.uint8)
    for b, src in enumerate(index):
        i, j = (pad, pad) if crop is None else (int(crop[b][0]), int(crop[b][1]))
        img = padded[src, i:i + h, j:j + w]
        out[b] = img[:, ::-1] if flip is not None and flip[b] else img
    return out


def policy_u8(batch, ops, args):
    """The op chains on an already cropped and flipped uint8 batch: ops [n, N], args [n, N, 6]."""
    out = np.array(batch, np.uint8)
    for b in range(out.shape[0]):
        for k in range(0 if ops is None else ops.shape[1]):
            out[b] = apply_op(out[b], ops[b, k], args[b, k])
    return out


def erase_is_valid(box, h, w):
    y0, y1, x0, x1 = (int(v) for v in box)
    return y0 <= y1 <= h and x0 <= x1 <= w


def normalize_erase(u8, mean, std, erase=None):
    """ToTensor + Normalize through the existing oracle (centre window, no flip), then the boxes set to 0.0."""
    out, _ = O.cifar_augment(u8, None, None, None, None, mean, std, 0)
    if erase is not None:
        h, w = u8.shape[1:3]
        for b, box in enumerate(erase):
            if erase_is_valid(box, h, w):
                y0, y1, x0, x1 = (int(v) for v in box)
                out[b, :, y0:y1, x0:x1] = 0.0
    return out


def augment_policy(images, targets, index, crop, flip, mean, std, pad, ops=None, args=None, erase=None):
    """(fp32 [n, 3, h, w], labels, uint8 [n, h, w, 3] before Normalize) of the whole launch."""
    u8 = policy_u8(crop_flip(images, index, crop, flip, pad), ops, args)
    idx = np.arange(len(images)) if index is None else np.asarray(index, np.int64)
    labels = None if targets is None else np.asarray(targets, np.int64)[idx]
    return normalize_erase(u8, mean, std, erase), labels, u8
