"""Data-side plumbing of the reference, kept bit-compatible.

* ``fix_seed`` — src/ddp/utils.py:8-15.
* ``train_valid_split`` — the 45k/5k split of src/ddp/dataset.py:85-92: ``np.random.shuffle`` of
  ``list(range(50000))`` under the global numpy state seeded by fix_seed(42).
* ``shard_indices`` / ``DistributedSampler`` — the per-epoch sharding of
  ``torch.utils.data.distributed.DistributedSampler`` as used at src/ddp/dataset.py:98 with
  ``set_epoch(epoch)`` (src/ddp/trainer.py:125): ``randperm(n, Generator.manual_seed(seed+epoch))``,
  padded to a multiple of the world size, then ``[rank::world]``.
* ``SyntheticCIFAR100`` — CIFAR-100 is not downloadable here (dataset.py:70-82 uses
  ``download=True``), so training uses a seeded synthetic stand-in of the same shape
  (SURVEY.md §8(d)): ``x = 0.5*T[y] + N(0,1)`` with class templates ``T`` (seed 1234), which keeps
  the loss learnable for loss-curve checks.
"""
from __future__ import annotations

import math
import random
from typing import Iterator, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.utils.data as tud

CIFAR_MEAN = (0.4914, 0.4822, 0.4465)  # dataset.py:43-46
CIFAR_STD = (0.2023, 0.1994, 0.2010)
IMAGENET_MEAN = (0.485, 0.456, 0.406)  # dataset.py:139-142 (test loader)
IMAGENET_STD = (0.229, 0.224, 0.225)


def fix_seed(seed: int) -> None:
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def train_valid_split(num_train: int = 50000, valid_size: float = 0.1, shuffle: bool = True
                      ) -> Tuple[List[int], List[int]]:
    if not (0 <= valid_size <= 1):
        raise ValueError("[!] valid_size should be in the range [0, 1].")
    indices = list(range(num_train))
    split = int(np.floor(valid_size * num_train))
    if shuffle:
        np.random.shuffle(indices)
    return indices[split:], indices[:split]


def shard_indices(n: int, num_replicas: int, rank: int, epoch: int = 0, seed: int = 0, shuffle: bool = True,
                  drop_last: bool = False) -> List[int]:
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        indices = torch.randperm(n, generator=g).tolist()
    else:
        indices = list(range(n))
    if drop_last and n % num_replicas != 0:
        num_samples = math.ceil((n - num_replicas) / num_replicas)
    else:
        num_samples = math.ceil(n / num_replicas)
    total = num_samples * num_replicas
    if not drop_last:
        pad = total - len(indices)
        if pad <= len(indices):
            indices += indices[:pad]
        else:
            indices += (indices * math.ceil(pad / len(indices)))[:pad]
    else:
        indices = indices[:total]
    return indices[rank:total:num_replicas]


class DistributedSampler(tud.Sampler):
    """Same index stream as torch's DistributedSampler (dataset.py:98) with set_epoch()."""

    def __init__(self, dataset, num_replicas: Optional[int] = None, rank: Optional[int] = None, shuffle=True,
                 seed: int = 0, drop_last: bool = False):
        if num_replicas is None or rank is None:
            import torch.distributed as dist
            num_replicas = dist.get_world_size() if num_replicas is None else num_replicas
            rank = dist.get_rank() if rank is None else rank
        self.n = len(dataset)
        self.num_replicas, self.rank = num_replicas, rank
        self.shuffle, self.seed, self.drop_last = shuffle, seed, drop_last
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def __iter__(self) -> Iterator[int]:
        return iter(shard_indices(self.n, self.num_replicas, self.rank, self.epoch, self.seed, self.shuffle,
                                  self.drop_last))

    def __len__(self) -> int:
        if self.drop_last and self.n % self.num_replicas != 0:
            return math.ceil((self.n - self.num_replicas) / self.num_replicas)
        return math.ceil(self.n / self.num_replicas)


def class_templates(num_classes=100, height=32, width=32, seed=1234) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(num_classes, 3, height, width, generator=g)


class SyntheticCIFAR100(tud.Dataset):
    """Seeded CIFAR-100-shaped data: image i = 0.5*T[y_i] + N(0,1) (per-index generator), normalized
    like dataset.py:43-46 would leave it (zero-mean, unit-scale)."""

    def __init__(self, n: int = 50000, height: int = 32, width: int = 32, num_classes: int = 100, seed: int = 1234):
        self.n, self.h, self.w, self.num_classes, self.seed = n, height, width, num_classes, seed
        self.templates = class_templates(num_classes, height, width, seed)
        g = torch.Generator().manual_seed(seed + 1)
        self.labels = torch.randint(0, num_classes, (n,), generator=g)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        y = int(self.labels[i])
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        x = 0.5 * self.templates[y] + torch.randn(3, self.h, self.w, generator=g)
        return x, y


def synthetic_batch(step: int, batch: int, height: int = 32, width: int = 32, num_classes: int = 100,
                    device="cpu", templates: Optional[torch.Tensor] = None, seed: int = 1234):
    """One batch of the §8(d) stream: labels randint(seed+step), x = 0.5*T[y] + randn (CPU RNG, so
    the stream is identical on every machine), returned on `device`."""
    if templates is None:
        templates = class_templates(num_classes, height, width, seed)
    g = torch.Generator().manual_seed(seed + step)
    y = torch.randint(0, num_classes, (batch,), generator=g)
    x = 0.5 * templates[y] + torch.randn(batch, 3, height, width, generator=g)
    return x.to(device), y.to(device)


def get_trn_val_loader(batch_size: int, valid_size: float = 0.1, num_workers: int = 0, pin_memory: bool = True,
                       distributed: bool = True, dataset: Optional[tud.Dataset] = None, **_):
    """dataset.py:15-116 with the synthetic dataset; returns (train_loader, train_sampler, valid_loader)."""
    ds = dataset if dataset is not None else SyntheticCIFAR100()
    train_idx, valid_idx = train_valid_split(len(ds), valid_size, True)
    train_ds, valid_ds = tud.Subset(ds, train_idx), tud.Subset(ds, valid_idx)
    if distributed:
        sampler = DistributedSampler(train_ds)
        shuffle = False
    else:
        sampler = tud.SubsetRandomSampler(list(range(len(train_ds))))
        shuffle = False
    train_loader = tud.DataLoader(train_ds, batch_size=batch_size, sampler=sampler, num_workers=num_workers,
                                  pin_memory=pin_memory, drop_last=True, shuffle=shuffle)
    valid_loader = tud.DataLoader(valid_ds, batch_size=batch_size, num_workers=num_workers, pin_memory=pin_memory)
    return train_loader, sampler, valid_loader


def get_tst_loader(batch_size: int, num_workers: int = 0, pin_memory: bool = False, distributed: bool = True,
                   n: int = 10000, **_):
    """dataset.py:119-168 with a synthetic 10k test split (different seed)."""
    ds = SyntheticCIFAR100(n=n, seed=4321)
    sampler = DistributedSampler(ds) if distributed else None
    return tud.DataLoader(ds, batch_size=batch_size, shuffle=False, sampler=sampler, num_workers=num_workers,
                          pin_memory=pin_memory)


# ----------------------------------------------------------------------------- on-device input pipeline
def synthetic_cifar_u8(n: int = 50000, height: int = 32, width: int = 32, num_classes: int = 100, seed: int = 1234):
    """CIFAR-100 in its stored form (uint8 [n, h, w, 3] HWC + int64 targets), seeded synthetic:
    pixel = clip(128 + 48*T[y] + 40*N(0,1)) with per-class templates T (numpy, CPU-deterministic)."""
    rng = np.random.default_rng(seed)
    templates = rng.standard_normal((num_classes, height, width, 3), dtype=np.float32)
    targets = rng.integers(0, num_classes, n, dtype=np.int64)
    images = np.empty((n, height, width, 3), np.uint8)
    for s in range(0, n, 4096):  # bounded temporaries
        e = min(n, s + 4096)
        v = 128.0 + 48.0 * templates[targets[s:e]] + 40.0 * rng.standard_normal((e - s, height, width, 3),
                                                                                  dtype=np.float32)
        images[s:e] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return images, targets


class MixParams(NamedTuple):
    """One epoch's Mixup / CutMix parameters (host arrays, see mix_params)."""

    mode: np.ndarray  # int32 [n_batches]: 0 none, 1 Mixup, 2 CutMix
    lam: np.ndarray   # fp32 [n_batches, batch]: the weight of labels_a in the loss (and Mixup's blend weight)
    box: np.ndarray   # uint8 [n_batches, batch, 4]: CutMix's (y0, y1, x0, x1), half open
    draw: np.ndarray  # fp64 [n_batches]: the batch's Beta(alpha, alpha) draw (1 for mode 0)


def mix_params(n_batches: int, batch: int, h: int, w: int, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0,
               prob: float = 1.0, rng: Optional[np.random.Generator] = None) -> MixParams:
    """Mixup / CutMix parameters of a whole epoch, drawn on the host with a seeded numpy Generator
    (torchvision.transforms.v2.MixUp / CutMix's rules, one draw per batch, repeated over its rows):
    a batch is mixed with probability `prob`, by Mixup or CutMix -- each with probability 1/2 when both alphas
    are set; lam ~ Beta(alpha, alpha); CutMix's box has its centre uniform in the image and half sizes
    int(0.5 * sqrt(1 - lam) * W), int(0.5 * sqrt(1 - lam) * H), clamped to the image, and the loss then uses
    the adjusted lam = 1 - area / (H * W)."""
    if mixup_alpha < 0 or cutmix_alpha < 0 or not 0.0 <= prob <= 1.0:
        raise ValueError("mix_params: alphas must be >= 0 and prob in [0, 1]")
    if not (0 < h <= 255 and 0 < w <= 255):
        raise ValueError("mix_params: boxes are uint8, h and w must be in [1, 255]")
    rng = rng if rng is not None else np.random.default_rng()
    nb = int(n_batches)
    apply = rng.random(nb) < prob
    second = rng.random(nb) < 0.5
    draw_m = rng.beta(mixup_alpha, mixup_alpha, nb) if mixup_alpha > 0 else np.ones(nb)
    draw_c = rng.beta(cutmix_alpha, cutmix_alpha, nb) if cutmix_alpha > 0 else np.ones(nb)
    cy, cx = rng.integers(0, h, nb), rng.integers(0, w, nb)
    if mixup_alpha > 0 and cutmix_alpha > 0:
        kind = np.where(second, 2, 1)
    else:
        kind = np.full(nb, 1 if mixup_alpha > 0 else (2 if cutmix_alpha > 0 else 0))
    mode = np.where(apply, kind, 0).astype(np.int32)
    draw = np.where(mode == 1, draw_m, np.where(mode == 2, draw_c, 1.0))
    r = 0.5 * np.sqrt(1.0 - draw)
    hh, hw_ = (r * h).astype(np.int64), (r * w).astype(np.int64)
    y0, y1 = np.clip(cy - hh, 0, None), np.clip(cy + hh, None, h)
    x0, x1 = np.clip(cx - hw_, 0, None), np.clip(cx + hw_, None, w)
    cut = mode == 2
    box1 = np.where(cut[:, None], np.stack([y0, y1, x0, x1], 1), 0).astype(np.uint8)
    area = (box1[:, 1].astype(np.int64) - box1[:, 0]) * (box1[:, 3].astype(np.int64) - box1[:, 2])
    lam1 = np.where(cut, 1.0 - area / float(h * w), draw).astype(np.float32)
    return MixParams(mode, np.repeat(lam1[:, None], batch, 1), np.repeat(box1[:, None, :], batch, 1), draw)


class PolicyParams(NamedTuple):
    """One epoch's augmentation-policy draws (host arrays, see policy_params)."""

    ops: np.ndarray   # uint8 [n_batches, batch, N]: kernel op codes (include/dtc.h, dtc_cifar_augment_policy)
    args: np.ndarray  # fp32 [n_batches, batch, N, 6]: each op's g0..g5
    name: np.ndarray  # uint8 [n_batches, batch, N]: index into POLICY_OPS, the named op each entry was drawn as


POLICIES = ("none", "randaugment", "trivialwide")
# torchvision's RandAugment / TrivialAugmentWide op space, in its order
POLICY_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
              "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
_POLICY_BINS = 31
_KERNEL_OP = np.array([0, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 9], np.uint8)


def _policy_magnitudes(policy: str, h: int, w: int) -> np.ndarray:
    """fp64 [14, 31]: the magnitude of each named op at each bin (torchvision's _augmentation_space tables)."""
    nb = _POLICY_BINS
    lin = lambda a, b: np.linspace(a, b, nb)
    zero = np.zeros(nb)
    if policy == "randaugment":
        shear, tx, ty, rot, blend = lin(0, 0.3), lin(0, 150.0 / 331.0 * w), lin(0, 150.0 / 331.0 * h), lin(0, 30), \
            lin(0, 0.9)
        bits = 8 - np.round(np.arange(nb) / ((nb - 1) / 4))
    else:
        shear, tx, ty, rot, blend = lin(0, 0.99), lin(0, 32), lin(0, 32), lin(0, 135), lin(0, 0.99)
        bits = 8 - np.round(np.arange(nb) / ((nb - 1) / 6))
    return np.stack([zero, shear, shear, np.trunc(tx), np.trunc(ty), rot, blend, blend, blend, blend, bits,
                     lin(255, 0), zero, zero])


def policy_params(n_batches: int, batch: int, h: int, w: int, policy: str = "randaugment", num_ops: int = 2,
                  magnitude: int = 9, rng: Optional[np.random.Generator] = None) -> PolicyParams:
    """RandAugment / TrivialAugmentWide draws of a whole epoch, per sample, on the host (torchvision's rules over
    its 14 named ops, POLICY_OPS): ``randaugment`` draws `num_ops` ops uniformly, all at bin `magnitude` of 31;
    ``trivialwide`` draws one op and a uniform bin from its wider ranges. The geometric ops and the four blends
    are negated with probability 1/2. Each named op becomes a kernel op and six args (float64, then rounded to
    fp32): the shears, translations (whole pixels) and the rotation an Affine matrix, a blend of signed magnitude
    m the pair (1 + m, -m), Posterize its bit mask, Solarize its threshold."""
    if policy not in POLICIES[1:]:
        raise ValueError(f"policy_params: policy must be one of {POLICIES[1:]}, got {policy!r}")
    if not 1 <= int(num_ops) <= 4 or not 0 <= int(magnitude) < _POLICY_BINS:
        raise ValueError("policy_params: num_ops must be in [1, 4] and magnitude in [0, 30]")
    rng = rng if rng is not None else np.random.default_rng()
    shape = (int(n_batches), int(batch), int(num_ops) if policy == "randaugment" else 1)
    name = rng.integers(0, len(POLICY_OPS), shape)
    bins = rng.integers(0, _POLICY_BINS, shape)
    neg = rng.random(shape) < 0.5
    if policy == "randaugment":
        bins = np.full(shape, int(magnitude))
    m = _policy_magnitudes(policy, h, w)[name, bins]
    m = np.where(neg & (name >= 1) & (name <= 9), -m, m)
    args = np.zeros(shape + (6,), np.float64)
    affine = (name >= 1) & (name <= 5)
    args[..., 0] = np.where(affine, 1.0, args[..., 0])
    args[..., 4] = np.where(affine, 1.0, args[..., 4])
    args[..., 1] = np.where(name == 1, m, args[..., 1])   # ShearX
    args[..., 3] = np.where(name == 2, m, args[..., 3])   # ShearY
    args[..., 2] = np.where(name == 3, -m, args[..., 2])  # TranslateX
    args[..., 5] = np.where(name == 4, -m, args[..., 5])  # TranslateY
    rot = name == 5
    th = np.deg2rad(np.where(rot, m, 0.0))
    args[..., 0] = np.where(rot, np.cos(th), args[..., 0])
    args[..., 1] = np.where(rot, -np.sin(th), args[..., 1])
    args[..., 3] = np.where(rot, np.sin(th), args[..., 3])
    args[..., 4] = np.where(rot, np.cos(th), args[..., 4])
    blend = (name >= 6) & (name <= 9)
    args[..., 0] = np.where(blend, 1.0 + m, args[..., 0])
    args[..., 1] = np.where(blend, -m, args[..., 1])
    mask = 0xFF & (0xFF << (8 - np.where(name == 10, m, 8.0).astype(np.int64)))
    args[..., 0] = np.where(name == 10, mask, args[..., 0])
    args[..., 0] = np.where(name == 11, m, args[..., 0])
    return PolicyParams(_KERNEL_OP[name], args.astype(np.float32), name.astype(np.uint8))


def erase_params(n_batches: int, batch: int, h: int, w: int, prob: float, rng: Optional[np.random.Generator] = None,
                 scale=(0.02, 0.33), ratio=(0.3, 3.3)) -> np.ndarray:
    """RandomErasing boxes of a whole epoch, uint8 [n_batches, batch, 4] = (y0, y1, x0, x1), half open
    (torchvision.transforms.RandomErasing.get_params' rule): a sample is selected with probability `prob`; up to 10
    attempts draw an area of h * w * U(scale) and an aspect ratio log-uniform in `ratio`, giving a box of
    round(sqrt(area * ratio)) x round(sqrt(area / ratio)); the first attempt whose box is strictly smaller than the
    image in both extents is kept, at a uniform corner. A sample that is not selected, or with no fitting attempt,
    gets the empty box (0, 0, 0, 0)."""
    if not 0.0 <= prob <= 1.0:
        raise ValueError("erase_params: prob must be in [0, 1]")
    if not (0 < h <= 255 and 0 < w <= 255):
        raise ValueError("erase_params: boxes are uint8, h and w must be in [1, 255]")
    rng = rng if rng is not None else np.random.default_rng()
    shape = (int(n_batches), int(batch))
    selected = rng.random(shape) < prob
    area = h * w * rng.uniform(scale[0], scale[1], shape + (10,))
    aspect = np.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1]), shape + (10,)))
    u_y, u_x = rng.random(shape), rng.random(shape)
    eh = np.rint(np.sqrt(area * aspect)).astype(np.int64)
    ew = np.rint(np.sqrt(area / aspect)).astype(np.int64)
    fits = (eh < h) & (ew < w)
    first = np.argmax(fits, axis=-1)[..., None]
    eh, ew = np.take_along_axis(eh, first, -1)[..., 0], np.take_along_axis(ew, first, -1)[..., 0]
    keep = selected & fits.any(axis=-1)
    y0 = np.floor(u_y * (h - eh + 1)).astype(np.int64)
    x0 = np.floor(u_x * (w - ew + 1)).astype(np.int64)
    box = np.stack([y0, y0 + eh, x0, x0 + ew], -1)
    return np.where(keep[..., None], box, 0).astype(np.uint8)


class LastPolicy(NamedTuple):
    """The policy parameters of a DeviceLoader's last batch (device tensors; None where the part is off)."""

    ops: Optional[torch.Tensor]
    args: Optional[torch.Tensor]
    erase: Optional[torch.Tensor]


class DeviceLoader:
    """``DataLoader(Subset(dataset, subset_idx), batch_size, sampler=sampler, drop_last=...)`` with
    the reference's train (or valid/test) transform (src/ddp/dataset.py:43-64, 95-116) executed on
    the GPU: the uint8 dataset stays resident in HBM (153.6 MB for CIFAR's 50k images); per epoch
    the sampler's index list (bit-identical to torch's DistributedSampler) is composed with the
    Subset map on the host and uploaded once; per batch one HIP launch gathers, crops, flips and
    normalizes (``ops.cifar_augment``). Crop offsets / flips are drawn on the device from a
    generator seeded with ``seed + epoch`` (torchvision draws them with the worker processes' CPU
    RNG, which no run reproduces across worker counts either; distributions are the same:
    offsets uniform on [0, 2*pad], flip with p = 0.5). Out-of-range indices are detected on the
    device and raised at the end of the epoch (one host sync per epoch).

    ``mixup_alpha`` / ``cutmix_alpha`` > 0 (train loaders only): every batch is mixed with probability
    ``mix_prob`` by Mixup or CutMix with itself rolled by one row, in the same single launch
    (``ops.cifar_augment_mix``). The epoch's parameters are drawn on the host from ``seed + epoch``
    (``mix_params``) and uploaded once, like the index list; a mixed batch yields ``(images, nn.MixedTarget)``,
    an unmixed one the plain launch's ``(images, labels)``. ``last_params`` is then ``(index, crop, flip, mix)``
    with ``mix`` a dict of the batch's ``mode``, ``lam`` (the loss's), ``box`` and the Beta ``draw``.

    ``policy`` = ``"randaugment"`` / ``"trivialwide"`` and ``erase_prob`` > 0 (train loaders only): an augmentation
    policy's op chain per sample between the flip and Normalize, and RandomErasing after it, in the one launch of
    ``ops.cifar_augment_policy``. Both parameter sets are drawn once per epoch on the host from a generator of their
    own, ``default_rng([seed + epoch, 1])`` (``policy_params`` then ``erase_params``; the Mixup / CutMix stream is
    untouched), and uploaded once. A mixed batch is the policy launch writing the augmented uint8 batch, then the
    mix launch on that batch. ``last_policy`` holds the last batch's ``(ops, args, erase)``; RandomErasing does not
    combine with Mixup / CutMix. With the defaults the loader issues exactly the launches it issues without them."""

    def __init__(self, images, targets, batch_size: int, subset_idx=None, sampler=None, train: bool = True,
                 mean=CIFAR_MEAN, std=CIFAR_STD, pad: int = 4, drop_last: bool = True, seed: int = 0,
                 device=None, mixup_alpha: float = 0.0, cutmix_alpha: float = 0.0, mix_prob: float = 1.0,
                 policy: str = "none", policy_num_ops: int = 2, policy_magnitude: int = 9, erase_prob: float = 0.0):
        from . import ops

        self.mixup_alpha, self.cutmix_alpha, self.mix_prob = float(mixup_alpha), float(cutmix_alpha), float(mix_prob)
        self.mixing = self.mixup_alpha > 0 or self.cutmix_alpha > 0
        if self.mixing and not train:
            raise ValueError("DeviceLoader: Mixup / CutMix are training transforms (train=False with an alpha > 0)")
        if self.mixup_alpha < 0 or self.cutmix_alpha < 0 or not 0.0 <= self.mix_prob <= 1.0:
            raise ValueError("DeviceLoader: alphas must be >= 0 and mix_prob in [0, 1]")
        self.policy, self.policy_num_ops, self.policy_magnitude = str(policy), int(policy_num_ops), int(policy_magnitude)
        self.erase_prob = float(erase_prob)
        if self.policy not in POLICIES:
            raise ValueError(f"DeviceLoader: policy must be one of {POLICIES}, got {policy!r}")
        if not 1 <= self.policy_num_ops <= 4 or not 0 <= self.policy_magnitude < _POLICY_BINS:
            raise ValueError("DeviceLoader: policy_num_ops must be in [1, 4] and policy_magnitude in [0, 30]")
        if not 0.0 <= self.erase_prob <= 1.0:
            raise ValueError("DeviceLoader: erase_prob must be in [0, 1]")
        self.policing = self.policy != "none" or self.erase_prob > 0
        if self.policing and not train:
            raise ValueError("DeviceLoader: augmentation policies and RandomErasing are training transforms "
                             "(train=False with a policy or erase_prob > 0)")
        if self.erase_prob > 0 and self.mixing:
            raise ValueError("DeviceLoader: RandomErasing does not combine with Mixup / CutMix (erase_prob > 0 with "
                             "an alpha > 0)")

        self._ops = ops
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.images = torch.as_tensor(images).to(dev).contiguous()
        self.targets = torch.as_tensor(targets, dtype=torch.int64).to(dev).contiguous()
        self.subset_idx = (np.arange(self.images.shape[0], dtype=np.int64) if subset_idx is None
                           else np.asarray(subset_idx, np.int64))
        self.batch_size, self.sampler, self.train = int(batch_size), sampler, bool(train)
        self.mean, self.std, self.pad, self.drop_last = tuple(mean), tuple(std), int(pad), bool(drop_last)
        self.seed, self.device, self.epoch = int(seed), dev, 0
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.last_params = None  # (index, crop, flip) of the last batch, for tests
        self.last_policy = None  # LastPolicy(ops, args, erase) of the last batch (None without a policy / erasing)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)
        if self.sampler is not None and hasattr(self.sampler, "set_epoch"):
            self.sampler.set_epoch(epoch)

    def _rows(self) -> np.ndarray:
        order = np.fromiter(iter(self.sampler), np.int64) if self.sampler is not None else \
            np.arange(len(self.subset_idx), dtype=np.int64)
        return self.subset_idx[order]

    def __len__(self) -> int:
        n = len(self.sampler) if self.sampler is not None else len(self.subset_idx)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _policy_batch(self, k, idx, crop, flip, mix, lam_d, box_d, pol):
        """Batch k with a policy and / or erasing: one ops.cifar_augment_policy launch; a mixed batch is that launch
        writing the augmented uint8 batch and its labels, then the mix launch on that batch."""
        n = idx.numel()
        self.last_policy = pol
        common = dict(targets=self.targets, ops=pol.ops, args=pol.args, status=self.status)
        mode = 0
        if mix is not None:
            mode = int(mix.mode[k])
            self.last_params = (idx, crop, flip, {"mode": mode, "lam": lam_d[k, :n], "box": box_d[k, :n],
                                                  "draw": float(mix.draw[k])})
        else:
            self.last_params = (idx, crop, flip)
        if not mode:
            return self._ops.cifar_augment_policy(self.images, idx, crop, flip, self.mean, self.std, self.pad,
                                                  erase=pol.erase, **common)
        from .nn import MixedTarget

        u8, lab = self._ops.cifar_augment_policy(self.images, idx, crop, flip, self.mean, self.std, self.pad,
                                                 to_u8=True, **common)
        x, ya, yb = self._ops.cifar_augment_mix(u8, None, None, None, self.mean, self.std, self.pad, targets=lab,
                                                mode=mode, lam=lam_d[k, :n], box=box_d[k, :n], status=self.status)
        return x, MixedTarget(ya, yb, lam_d[k, :n])

    def __iter__(self):
        rows = torch.from_numpy(self._rows()).to(self.device)
        gen = torch.Generator(device=self.device)
        gen.manual_seed(self.seed + self.epoch)
        B = self.batch_size
        mix = lam_d = box_d = None
        if self.mixing:
            from .nn import MixedTarget

            mix = mix_params(len(self), B, self.images.shape[1], self.images.shape[2], self.mixup_alpha,
                             self.cutmix_alpha, self.mix_prob, np.random.default_rng(self.seed + self.epoch))
            lam_d = torch.from_numpy(mix.lam).to(self.device)
            box_d = torch.from_numpy(mix.box).to(self.device)
        pol_ops = pol_args = pol_erase = None
        if self.policing:
            h, w = self.images.shape[1], self.images.shape[2]
            prng = np.random.default_rng([self.seed + self.epoch, 1])
            if self.policy != "none":
                pol = policy_params(len(self), B, h, w, self.policy, self.policy_num_ops, self.policy_magnitude, prng)
                pol_ops = torch.from_numpy(pol.ops).to(self.device)
                pol_args = torch.from_numpy(pol.args).to(self.device)
            if self.erase_prob > 0:
                pol_erase = torch.from_numpy(erase_params(len(self), B, h, w, self.erase_prob, prng)).to(self.device)
        finished = False
        try:
            for k in range(len(self)):
                idx = rows[k * B:(k + 1) * B]
                n = idx.numel()
                crop = flip = None
                if self.train:
                    crop = torch.randint(0, 2 * self.pad + 1, (n, 2), dtype=torch.uint8, device=self.device,
                                         generator=gen)
                    flip = torch.randint(0, 2, (n,), dtype=torch.uint8, device=self.device, generator=gen)
                if self.policing:
                    yield self._policy_batch(k, idx, crop, flip, mix, lam_d, box_d, LastPolicy(
                        *(None if t is None else t[k, :n] for t in (pol_ops, pol_args, pol_erase))))
                    continue
                if mix is not None:
                    mode = int(mix.mode[k])
                    self.last_params = (idx, crop, flip, {"mode": mode, "lam": lam_d[k, :n], "box": box_d[k, :n],
                                                          "draw": float(mix.draw[k])})
                    if mode:
                        x, ya, yb = self._ops.cifar_augment_mix(
                            self.images, idx, crop, flip, self.mean, self.std, self.pad, targets=self.targets,
                            mode=mode, lam=lam_d[k, :n], box=box_d[k, :n], status=self.status)
                        yield x, MixedTarget(ya, yb, lam_d[k, :n])
                        continue
                else:
                    self.last_params = (idx, crop, flip)
                yield self._ops.cifar_augment(self.images, idx, crop, flip, self.mean, self.std, self.pad,
                                              targets=self.targets, status=self.status)
            finished = True
        finally:
            # checked however the epoch ends (also when the consumer breaks early, e.g. --max-steps),
            # and reset, so a bad index is reported for the epoch it happened in, never a later one
            if int(self.status.item()):
                self.status.zero_()
                msg = "DeviceLoader: a sampler index, crop offset or mix parameter was out of range this epoch"
                if finished:
                    raise IndexError(msg)
                import warnings

                warnings.warn(msg + " (epoch ended early)", RuntimeWarning)
