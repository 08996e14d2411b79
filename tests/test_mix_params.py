"""data.mix_params: the host-side draw of an epoch's Mixup / CutMix parameters (torchvision.transforms.v2.MixUp /
CutMix's rules, one draw per batch). CPU only; the launch that consumes them is tested in test_gpu_mix_augment.py."""
import numpy as np
import pytest


def _draw(dtc, seed=0, nb=50, batch=6, h=32, w=32, ma=1.0, ca=1.0, prob=1.0):
    return dtc.data.mix_params(nb, batch, h, w, ma, ca, prob, np.random.default_rng(seed))


def test_deterministic_per_seed_and_shapes(dtc):
    a, b, c = _draw(dtc, 3), _draw(dtc, 3), _draw(dtc, 4)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert not all(np.array_equal(u, v) for u, v in zip(a, c))
    assert a.mode.shape == (50,) and a.mode.dtype == np.int32
    assert a.lam.shape == (50, 6) and a.lam.dtype == np.float32
    assert a.box.shape == (50, 6, 4) and a.box.dtype == np.uint8
    assert a.draw.shape == (50,)
    assert set(np.unique(a.mode)) <= {0, 1, 2}
    # one draw per batch, repeated over the rows
    assert (a.lam == a.lam[:, :1]).all() and (a.box == a.box[:, :1]).all()


@pytest.mark.parametrize("h,w", [(32, 32), (8, 12), (1, 255)])
def test_boxes_inside_image_and_adjusted_lam_exact(dtc, h, w):
    p = _draw(dtc, 1, nb=400, h=h, w=w, ma=0.0, ca=0.7)
    assert (p.mode == 2).all()
    y0, y1, x0, x1 = (p.box[:, 0, i].astype(np.int64) for i in range(4))
    assert (y0 <= y1).all() and (y1 <= h).all() and (x0 <= x1).all() and (x1 <= w).all()
    area = (y1 - y0) * (x1 - x0)
    assert np.array_equal(p.lam[:, 0], (1.0 - area / float(h * w)).astype(np.float32))
    assert ((p.lam >= 0) & (p.lam <= 1)).all()
    # torchvision's rule: half sizes int(0.5 * sqrt(1 - lam) * W / H) around a centre inside the image
    r = 0.5 * np.sqrt(1.0 - p.draw)
    assert (y1 - y0 <= 2 * (r * h).astype(np.int64)).all() and (x1 - x0 <= 2 * (r * w).astype(np.int64)).all()
    if h == 32:
        assert (area > 0).any() and (area < h * w).any()


def test_zero_alpha_never_draws_that_kind_and_prob_zero_is_all_plain(dtc):
    assert set(np.unique(_draw(dtc, 2, nb=200, ma=1.0, ca=0.0).mode)) == {1}
    assert set(np.unique(_draw(dtc, 2, nb=200, ma=0.0, ca=1.0).mode)) == {2}
    assert set(np.unique(_draw(dtc, 2, nb=200, ma=1.0, ca=1.0).mode)) == {1, 2}
    p = _draw(dtc, 2, nb=200, prob=0.0)
    assert (p.mode == 0).all() and (p.lam == 1).all() and (p.box == 0).all()
    half = _draw(dtc, 2, nb=2000, prob=0.5)
    assert 0.4 < (half.mode == 0).mean() < 0.6
    assert (half.lam[half.mode == 0] == 1).all() and (half.box[half.mode != 2] == 0).all()
    assert (_draw(dtc, 2, nb=20, ma=0.0, ca=0.0).mode == 0).all()


def test_mixup_lam_is_the_beta_draw_with_mean_one_half(dtc):
    """Beta(1, 1) is uniform: standard deviation 0.29, so over 4,000 batches the mean is within 0.03 of 0.5 at
    about 6 standard errors."""
    p = _draw(dtc, 7, nb=4000, batch=2, ma=1.0, ca=0.0)
    assert np.array_equal(p.lam[:, 0], p.draw.astype(np.float32))
    assert abs(float(p.lam[:, 0].mean()) - 0.5) < 0.03
    assert ((p.lam >= 0) & (p.lam <= 1)).all()


def test_bad_arguments(dtc):
    for kw in (dict(ma=-1.0), dict(ca=-0.5), dict(prob=1.5), dict(h=300)):
        with pytest.raises(ValueError):
            _draw(dtc, **kw)
