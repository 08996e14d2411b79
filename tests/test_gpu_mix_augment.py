"""Mixup / CutMix in the on-device input launch (dtc_cifar_augment_mix): BIT-EXACT against numpy on the existing
oracle's augmented batch (the mix of the augmented batch with a permutation of itself, each row keeping its own
crop and flip), the status flagging, and the DeviceLoader's mixed epoch stream."""
import numpy as np
import pytest
import torch

from oracle import ops as O

pytestmark = pytest.mark.gpu

MEAN, STD = O.CIFAR_MEAN, O.CIFAR_STD


def _data(n=50, h=32, w=32, seed=0):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (n, h, w, 3), dtype=np.uint8), g.integers(0, 100, n, dtype=np.int64)


def _D(cuda):
    return lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _box_mask(box, h, w):
    """[n, 1, h, w] bool: inside the half-open (y0, y1, x0, x1) box of each row."""
    ys, xs = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    b = box.astype(np.int64)
    m = (ys >= b[:, 0, None, None]) & (ys < b[:, 1, None, None]) & (xs >= b[:, 2, None, None]) & (xs < b[:, 3, None, None])
    return m[:, None]


def _mix_reference(A, partner, mode, lam, box):
    if mode == 1:
        lam = lam.astype(np.float32)
        return A * lam[:, None, None, None] + A[partner] * (1 - lam)[:, None, None, None]
    return np.where(_box_mask(box, A.shape[2], A.shape[3]), A[partner], A)


def _params(n, h, w, pad, seed=1):
    g = np.random.default_rng(seed)
    idx = g.integers(0, 50, n)
    crop = g.integers(0, 2 * pad + 1, (n, 2)).astype(np.uint8)
    crop[0] = (0, 2 * pad)
    flip = g.integers(0, 2, n).astype(np.uint8)
    lam = g.random(n).astype(np.float32)
    lam[0] = 1.0
    lam[n // 2] = 0.0
    y = np.sort(g.integers(0, h + 1, (n, 2)), 1)
    x = np.sort(g.integers(0, w + 1, (n, 2)), 1)
    box = np.concatenate([y, x], 1).astype(np.uint8)
    box[0] = (0, h, 0, w)       # the whole image
    box[n // 2] = (3, 3, 0, w)  # empty
    return g, idx, crop, flip, lam, box


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("explicit", [True, False])
@pytest.mark.parametrize("h,w,pad,n", [(32, 32, 4, 37), (8, 12, 2, 19), (32, 32, 4, 5), (32, 32, 4, 1)])
def test_mix_matches_numpy_bit_exact(dtc, cuda, h, w, pad, n, explicit, mode):
    """Rows whose partner sits in another workgroup (4 rows per workgroup at 32x32), a ragged last workgroup, the
    self-partner at n = 1; an explicit random partner array and NULL (b - 1 cyclically, batch.roll(1, 0))."""
    imgs, tg = _data(50, h, w)
    g, idx, crop, flip, lam, box = _params(n, h, w, pad)
    partner = g.integers(0, n, n).astype(np.int32) if explicit else ((np.arange(n) + n - 1) % n).astype(np.int32)
    A, lab = O.cifar_augment(imgs, tg, idx, crop, flip, MEAN, STD, pad)
    ref = _mix_reference(A, partner, mode, lam, box)
    if not explicit:
        assert np.array_equal(A[partner], np.roll(A, 1, 0))
    D = _D(cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    out, la, lb = dtc.ops.cifar_augment_mix(D(imgs), D(idx), D(crop), D(flip), MEAN, STD, pad, targets=D(tg),
                                            partner=D(partner) if explicit else None, mode=mode, lam=D(lam),
                                            box=D(box), status=status)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and ref.dtype == np.float32
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(la.cpu().numpy(), tg[idx]) and np.array_equal(la.cpu().numpy(), lab)
    assert np.array_equal(lb.cpu().numpy(), tg[idx[partner]])
    assert int(status.item()) == 0
    if n > 1:
        assert not np.array_equal(ref, A)  # the case does mix


@pytest.mark.parametrize("mode", [1, 2])
def test_mix_without_crop_and_flip(dtc, cuda, mode):
    """crop / flip / index NULL (the centre window of rows 0..n-1) mix the same way."""
    imgs, tg = _data(9)
    _, _, _, _, lam, box = _params(9, 32, 32, 4)
    A, lab = O.cifar_augment(imgs, tg, None, None, None, MEAN, STD, 4)
    partner = ((np.arange(9) + 8) % 9).astype(np.int32)
    D = _D(cuda)
    out, la, lb = dtc.ops.cifar_augment_mix(D(imgs), None, None, None, MEAN, STD, 4, targets=D(tg), mode=mode,
                                            lam=D(lam), box=D(box))
    assert np.array_equal(out.cpu().numpy(), _mix_reference(A, partner, mode, lam, box))
    assert np.array_equal(la.cpu().numpy(), tg) and np.array_equal(lb.cpu().numpy(), tg[partner])


def test_mix_flags_bad_rows_and_writes_them_unmixed(dtc, cuda):
    n, h, w, pad = 11, 32, 32, 4
    imgs, tg = _data(50, h, w)
    g, idx, crop, flip, lam, box = _params(n, h, w, pad)
    partner = g.integers(0, n, n).astype(np.int32)
    A, _ = O.cifar_augment(imgs, tg, idx, crop, flip, MEAN, STD, pad)
    D = _D(cuda)
    cases = []
    p2 = partner.copy(); p2[6] = n  # noqa: E702
    cases.append((1, p2, lam, box))
    p3 = partner.copy(); p3[6] = -1  # noqa: E702
    cases.append((2, p3, lam, box))
    b2 = box.copy(); b2[6] = (9, 4, 0, 8)  # noqa: E702  inverted
    cases.append((2, partner, lam, b2))
    b3 = box.copy(); b3[6] = (0, 33, 0, 8)  # noqa: E702  leaves the image
    cases.append((2, partner, lam, b3))
    l2 = lam.copy(); l2[6] = 1.5  # noqa: E702
    cases.append((1, partner, l2, box))
    l3 = lam.copy(); l3[6] = np.nan  # noqa: E702
    cases.append((1, partner, l3, box))
    for mode, pp, ll, bb in cases:
        status = torch.zeros(1, dtype=torch.int32, device=cuda)
        out, la, lb = dtc.ops.cifar_augment_mix(D(imgs), D(idx), D(crop), D(flip), MEAN, STD, pad, targets=D(tg),
                                                partner=D(pp), mode=mode, lam=D(ll), box=D(bb), status=status)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        assert int(status.item()) == 1, (mode, pp[6], ll[6], bb[6])
        assert np.array_equal(o[6], A[6])  # the plain augment's row
        assert int(lb[6]) == int(la[6]) == tg[idx[6]]
        good = np.arange(n) != 6
        safe = np.where(good, pp, 0)
        ref = _mix_reference(A, safe, mode, np.where(good, ll, 1).astype(np.float32), np.where(good[:, None], bb, 0))
        assert np.array_equal(o[good], ref[good])  # the other rows are unaffected
        assert np.array_equal(lb.cpu().numpy()[good], tg[idx[pp[good]]])
    # a good call leaves status alone; the existing conditions stay
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    dtc.ops.cifar_augment_mix(D(imgs), D(idx), D(crop), D(flip), MEAN, STD, pad, targets=D(tg), partner=D(partner),
                              mode=1, lam=D(lam), status=status)
    assert int(status.item()) == 0
    bad_idx = idx.copy(); bad_idx[2] = 50  # noqa: E702
    dtc.ops.cifar_augment_mix(D(imgs), D(bad_idx), D(crop), D(flip), MEAN, STD, pad, targets=D(tg), mode=1, lam=D(lam),
                              status=status)
    assert int(status.item()) == 1
    with pytest.raises(dtc.NativeError, match="mode"):
        dtc.ops.cifar_augment_mix(D(imgs), D(idx), D(crop), D(flip), MEAN, STD, pad, mode=2, lam=D(lam))


def _loader(dtc, cuda, imgs, tg, seed=3, **kw):
    return dtc.data.DeviceLoader(imgs, tg, 16, device=cuda, seed=seed, **kw)


def test_device_loader_mixed_epoch(dtc, cuda):
    """64 images, batch 16, both alphas 1, mix_prob 0.5: every batch equals the reference built from last_params;
    mode-0 batches are plain tensors bit-equal to today's loader with the same seed; two loaders with one seed
    yield one stream."""
    imgs, tg = _data(64, seed=4)
    kw = dict(mixup_alpha=1.0, cutmix_alpha=1.0, mix_prob=0.5)
    plain = _loader(dtc, cuda, imgs, tg, seed=1)
    streams, modes = [], []
    for rep in range(2):
        mixed = _loader(dtc, cuda, imgs, tg, seed=1, **kw)
        stream = []
        for epoch in (0, 1):
            mixed.set_epoch(epoch)
            plain.set_epoch(epoch)
            expect = dtc.data.mix_params(4, 16, 32, 32, 1.0, 1.0, 0.5, np.random.default_rng(1 + epoch))
            it = iter(plain)
            for k, (x, y) in enumerate(mixed):
                px, py = next(it)
                idx, crop, flip, mix = mixed.last_params
                assert mix["mode"] == int(expect.mode[k])
                assert np.array_equal(mix["lam"].cpu().numpy(), expect.lam[k])
                assert np.array_equal(mix["box"].cpu().numpy(), expect.box[k])
                for a, b in zip((idx, crop, flip), plain.last_params):
                    assert torch.equal(a, b)  # the crop / flip stream is the unmixed loader's
                A, lab = O.cifar_augment(imgs, tg, idx.cpu().numpy(), crop.cpu().numpy(), flip.cpu().numpy(), MEAN,
                                         STD, 4)
                if mix["mode"] == 0:
                    assert isinstance(y, torch.Tensor)
                    assert torch.equal(x, px) and torch.equal(y, py)
                    assert np.array_equal(x.cpu().numpy(), A)
                    stream.append((x.cpu().numpy(), y.cpu().numpy()))
                else:
                    assert isinstance(y, dtc.MixedTarget) and y.to(cuda) is y
                    partner = (np.arange(16) + 15) % 16
                    # Mixup blends with the Beta draw (= the loss's lam); CutMix pastes the box
                    ref = _mix_reference(A, partner, mix["mode"], expect.lam[k], expect.box[k])
                    assert np.array_equal(x.cpu().numpy(), ref)
                    assert np.array_equal(y.labels_a.cpu().numpy(), lab)
                    assert np.array_equal(y.labels_b.cpu().numpy(), lab[partner])
                    assert np.array_equal(y.lam.cpu().numpy(), expect.lam[k])
                    stream.append((x.cpu().numpy(), y.labels_a.cpu().numpy(), y.labels_b.cpu().numpy(),
                                   y.lam.cpu().numpy()))
                if rep == 0:
                    modes.append(mix["mode"])
            assert k == 3
        streams.append(stream)
    assert set(modes) == {0, 1, 2}  # seed 1 draws plain, Mixup and CutMix batches in its first two epochs
    assert len(streams[0]) == len(streams[1]) == 8
    for a, b in zip(streams[0], streams[1]):
        assert len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))
    with pytest.raises(ValueError):
        _loader(dtc, cuda, imgs, tg, train=False, cutmix_alpha=1.0)


def test_mixed_loader_trains_native_resnet(dtc, cuda):
    imgs, tg = dtc.data.synthetic_cifar_u8(n=64, seed=7)
    loader = _loader(dtc, cuda, imgs, tg, mixup_alpha=1.0, cutmix_alpha=1.0, mix_prob=0.5)
    torch.manual_seed(42)
    model = dtc.ResNet18().to(cuda)
    crit = dtc.CrossEntropyLoss(label_smoothing=0.1)
    opt = dtc.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    scaler = dtc.GradScaler()
    losses, kinds = [], []
    for step, (x, y) in enumerate(loader):
        if step == 3:
            break
        y = y.to(cuda)
        opt.zero_grad()
        with dtc.autocast():
            loss = crit(model(x), y)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        losses.append(loss.item())
        kinds.append(type(y).__name__)
    torch.cuda.synchronize()
    assert len(losses) == 3 and all(np.isfinite(losses)), losses
    assert int(loader.status.item()) == 0
    assert torch.isfinite(model.flat.params).all().item()


def test_single_trainer_with_soft_flags(dtc, cuda, tmp_path):
    """`train.py single --amp --device-data --label-smoothing 0.1 --mixup-alpha 1 --cutmix-alpha 1 --mix-prob 0.5`
    through fit -> validate: the train loader mixes, the training criterion smooths, and validate() / test()
    report the plain cross-entropy -- the default and the --fused-eval paths return the same numbers."""
    flags = ["--epoch", "1", "--batch-size", "64", "--max-steps", "4", "--amp", "--synthetic-train", "640",
             "--synthetic-test", "128", "--device-data", "--label-smoothing", "0.1", "--mixup-alpha", "1",
             "--cutmix-alpha", "1", "--mix-prob", "0.5", "--ckpt-path", str(tmp_path)]
    t = dtc.trainer.main(flags, "single")
    assert t.train_loader.mixing and not t.val_loader.mixing and not t.test_loader.mixing
    assert t.criterion.label_smoothing == 0.1 and t.eval_criterion.label_smoothing == 0.0
    assert t.global_step == 4 and int(t.train_loader.status.item()) == 0
    assert len(t.train_loader.last_params) == 4 and len(t.val_loader.last_params) == 3
    with dtc.autocast(enabled=False):
        plain = t.validate(0)
        t.hparams.fused_eval = True
        fused = t.validate(0)
        state = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
        res_fused = t.test(state)
        t.hparams.fused_eval = False
        res_plain = t.test(state)
    assert np.isfinite(plain[0]) and plain == fused
    assert res_plain == res_fused
