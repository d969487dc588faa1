"""Online random augmentation without a GPU: the host generator's known answers, draw() as a pure function of (seed, sample),
the ranges of the drawn parameters, RandomPolicy's argument checks, and warp_items against the numpy restatement of
sg_warp_u8 (tests/_warp_ref.py): the eight symmetries reproduce numpy's own flips / rot90 exactly, the label shares the
image's geometry, an all-off policy is the identity."""
import ctypes
import math

import numpy as np
import pytest

import _dropout_ref as D
import _warp_ref as R
from building_detection_amd import _lib
from building_detection_amd import augment as A

FULL = dict(rotate=180, scale=(0.6, 1.8), shear=12, translate=0.25, flip=True, brightness=0.2, contrast=0.3, saturation=0.4,
            gamma=0.5, hue=20, noise=6.0, swap_rb=0.3, border="reflect", p_geometric=0.9, p_photometric=0.8)


def _hex(ws):
    return " ".join(f"{int(w):08x}" for w in ws)


@pytest.mark.parametrize("counter,key,out", [   # Random123's kat_vectors, philox4x32 10
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_host_philox_known_answers(counter, key, out):
    assert _hex(A.philox4x32_10(counter, key)) == out
    assert _hex(A.philox4x32_10(counter, key)) == _hex(D.philox4x32_10(counter, key))   # and the tests' numpy form agrees


def test_binding_mirrors_the_header():
    assert ctypes.sizeof(_lib.WarpItem) == 112
    assert (_lib.WarpItem.b0.offset, _lib.WarpItem.sample.offset, _lib.WarpItem.fill.offset, _lib.WarpItem.m.offset,
            _lib.WarpItem.off.offset) == (32, 48, 56, 64, 100)
    assert "sg_warp_u8" in _lib.exported_symbols()
    assert (_lib.SG_WARP_NEAREST, _lib.SG_WARP_REFLECT, _lib.SG_WARP_COLOR) == (R.NEAREST, R.REFLECT, R.COLOR)
    assert (_lib.SG_WARP_NOISE_STREAM, _lib.SG_WARP_NOISE_KEY) == (R.NOISE_STREAM, R.NOISE_KEY)
    assert abs(A.NOISE_T_STD - 147.80) < 0.005 and A.NOISE_T_STD == R.T_STD


def test_draw_is_a_pure_function_of_seed_and_sample():
    pol = A.RandomPolicy(**FULL)
    ks = [0, 1, 2, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5]
    first = [A.draw(pol, 9, k) for k in ks]
    assert first == [A.draw(pol, 9, k) for k in ks]
    assert list(reversed(first)) == [A.draw(pol, 9, k) for k in reversed(ks)]      # any order of calls
    assert len({r[1:] for r in first}) == len(ks)                                  # different samples differ
    assert A.draw(pol, 10, 2)[1:] != A.draw(pol, 9, 2)[1:]                         # and so do different seeds
    assert A.draw(pol, 9, 2 ** 32)[1:] != A.draw(pol, 9, 0)[1:]                    # the high word of the sample counts
    assert A.draw(pol, 2 ** 32 + 9, 2)[1:] != A.draw(pol, 9, 2)[1:]                # and the high word of the seed
    assert [r.sample for r in first] == ks
    # switching one option off moves no other parameter
    less = A.RandomPolicy(**dict(FULL, shear=0))
    for k in ks:
        assert A.draw(less, 9, k) == A.draw(pol, 9, k)._replace(shear=0.0)


def test_drawn_parameters_stay_inside_the_policy():
    pol = A.RandomPolicy(**FULL)
    recs = [A.draw(pol, 3, k) for k in range(10000)]
    for r in recs:
        assert -180 <= r.angle <= 180 and 0.6 <= r.scale <= 1.8 and -12 <= r.shear <= 12
        assert -0.25 <= r.tx <= 0.25 and -0.25 <= r.ty <= 0.25 and 0 <= r.sym < 8
        assert -0.2 <= r.brightness <= 0.2 and 0.7 <= r.contrast <= 1.3 and 0.6 <= r.saturation <= 1.4
        assert 1 / 1.5 - 1e-12 <= r.gamma <= 1.5 + 1e-12 and -20 <= r.hue <= 20
        assert r.noise in (0.0, 6.0) and r.border == "reflect" and isinstance(r.swap_rb, bool)
    # the gates and the equiprobable choices, each within five standard errors of its expectation
    n = len(recs)
    def near(count, p, of=n):
        return abs(count - p * of) <= 5 * math.sqrt(of * p * (1 - p))
    geo = [r for r in recs if (r.angle, r.scale, r.tx) != (0.0, 1.0, 0.0)]
    pho = [r for r in recs if r.noise > 0]
    assert near(len(geo), 0.9) and near(len(pho), 0.8)
    for s in range(8):
        assert near(sum(r.sym == s for r in geo), 1 / 8, len(geo))
    assert near(sum(r.swap_rb for r in pho), 0.3, len(pho))
    assert abs(np.mean([r.angle for r in geo])) < 5 * (360 / math.sqrt(12)) / math.sqrt(len(geo))
    assert abs(np.mean([math.log(r.scale) for r in geo]) - (math.log(0.6) + math.log(1.8)) / 2) < \
        5 * (math.log(3) / math.sqrt(12)) / math.sqrt(len(geo))


def test_all_off_policy_is_the_identity_without_a_table():
    pol = A.RandomPolicy()
    for k in (0, 5, 2 ** 40):
        rec = A.draw(pol, 1, k)
        img, lut = A.warp_items(rec, (512, 512), (512, 512), False)
        lab, none = A.warp_items(rec, (512, 512), (512, 512), True)
        assert lut is None and none is None
        assert img["a"] == (65536, 0, 0, 65536) and img["b"] == (0, 0) and img["flags"] == 0 and img["fill"] == 128
        assert "m" not in img and "noise_q12" not in img
        assert lab["a"] == img["a"] and lab["b"] == img["b"] and lab["flags"] == _lib.SG_WARP_NEAREST and lab["fill"] == 0
    # a larger source: the centred crop, still whole pixels
    img, _ = A.warp_items(A.draw(pol, 1, 0), (700, 640), (512, 512), False)
    assert img["a"] == (65536, 0, 0, 65536) and img["b"] == (64 * 65536, 94 * 65536) and (img["sh"], img["sw"]) == (700, 640)


@pytest.mark.parametrize("bad", [
    dict(rotate=-1), dict(rotate=181), dict(rotate="much"), dict(rotate=float("nan")), dict(scale=(0, 1)), dict(scale=(1.5, 1.2)),
    dict(scale=1.0), dict(scale=(1, 17)), dict(shear=61), dict(translate=-0.1), dict(flip=1), dict(brightness=1.5),
    dict(contrast=1.0), dict(saturation=-0.5), dict(gamma=-1), dict(hue=200), dict(noise=-1), dict(noise=65), dict(swap_rb=1.5),
    dict(border="wrap"), dict(p_geometric=-0.1), dict(p_photometric=2)])
def test_bad_policies_raise(bad):
    with pytest.raises(ValueError, match="RandomPolicy"):
        A.RandomPolicy(**bad)


def _restated(src, item, lut=None, out_hw=None, seed=0):
    full = R.item(**{k: v for k, v in item.items()})
    return R.warp(src, [full], None if lut is None else lut[None], seed, out_hw)[0]


@pytest.mark.parametrize("sym", range(8))
def test_symmetries_are_integer_maps_that_equal_numpy(sym):
    name, form, Dm = R.SYMMETRIES[sym]
    rng = np.random.default_rng(sym)
    src = rng.integers(0, 256, size=(1, 40, 40, 3), dtype=np.uint8)
    lab = rng.integers(0, 6, size=(1, 40, 40), dtype=np.uint8)
    rec = A.draw(A.RandomPolicy(), 0, 0)._replace(sym=sym)
    img, lut = A.warp_items(rec, (40, 40), (40, 40), False)
    li, _ = A.warp_items(rec, (40, 40), (40, 40), True)
    assert lut is None and img["flags"] == 0
    assert img["a"] == tuple(65536 * v for v in (Dm[0][0], Dm[0][1], Dm[1][0], Dm[1][1])), name
    assert all(v % 65536 == 0 for v in img["b"]), name
    assert (img["a"], img["b"]) == R.affine((40, 40), (40, 40), D=Dm)               # the tests' own float64 builder agrees
    assert (li["a"], li["b"]) == (img["a"], img["b"])
    assert np.array_equal(_restated(src, img), form(src[0])), name
    assert np.array_equal(_restated(lab, li), form(lab[0])), name


def test_a_quarter_turn_through_the_angle_is_rot90():
    rng = np.random.default_rng(5)
    src = rng.integers(0, 256, size=(1, 32, 32, 3), dtype=np.uint8)
    base = A.draw(A.RandomPolicy(), 0, 0)
    for angle, k in ((90.0, 1), (-90.0, -1), (180.0, 2)):
        img, _ = A.warp_items(base._replace(angle=angle), (32, 32), (32, 32), False)
        assert all(v % 65536 == 0 for v in img["a"] + img["b"])
        assert np.array_equal(_restated(src, img), np.rot90(src[0], k)), angle


def test_image_and_label_items_share_their_geometry():
    pol = A.RandomPolicy(**FULL)
    for k in range(50):
        rec = A.draw(pol, 2, k)
        img, lut = A.warp_items(rec, (300, 420), (512, 512), False)
        lab, none = A.warp_items(rec, (300, 420), (512, 512), True)
        assert none is None and (lab["a"], lab["b"], lab["sh"], lab["sw"]) == (img["a"], img["b"], 300, 420)
        assert lab["flags"] == (_lib.SG_WARP_NEAREST | _lib.SG_WARP_REFLECT) and lab["fill"] == 0 and "m" not in lab
        assert img["flags"] & _lib.SG_WARP_REFLECT and not img["flags"] & _lib.SG_WARP_NEAREST and img["fill"] == 128
        assert all(abs(v) <= R.A_MAX for v in img["a"]) and all(abs(v) < R.B_LIM for v in img["b"])
        if img["flags"] & _lib.SG_WARP_COLOR:
            assert all(abs(v) <= R.M_MAX for v in img["m"]) and 0 <= img["noise_q12"] <= R.NOISE_MAX
            assert lut is None or (lut.shape == (3, 256) and lut.dtype == np.uint8)
        else:
            assert lut is None
        _lib.warp_item(**img), _lib.warp_item(**lab)     # both fit the ABI's struct


def test_colour_items():
    base = A.draw(A.RandomPolicy(), 0, 0)
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, size=(1, 16, 16, 3), dtype=np.uint8)
    swap, lut = A.warp_items(base._replace(swap_rb=True), (16, 16), (16, 16), False)
    assert lut is None and swap["flags"] == _lib.SG_WARP_COLOR and swap["m"] == (0, 0, 4096, 0, 4096, 0, 4096, 0, 0)
    assert np.array_equal(_restated(src, swap), src[0][..., ::-1])
    grey, _ = A.warp_items(base._replace(saturation=0.0), (16, 16), (16, 16), False)
    g = _restated(src, grey)
    assert np.array_equal(g[..., 0], g[..., 1]) and np.array_equal(g[..., 1], g[..., 2])
    luma = src[0].astype(np.float64) @ np.array([0.299, 0.587, 0.114])
    assert np.abs(g[..., 0] - luma).max() <= 1.0            # Q12 rounding of three weights: far below one grey level, + rounding
    hue, _ = A.warp_items(base._replace(hue=120.0), (16, 16), (16, 16), False)   # a third of a turn permutes the channels
    assert np.abs(_restated(src, hue).astype(int) - src[0][..., [2, 0, 1]].astype(int)).max() <= 1
    tone, lut = A.warp_items(base._replace(brightness=0.1, contrast=1.2, gamma=0.8), (16, 16), (16, 16), False)
    assert tone["m"] == R.IDENTITY_M and lut.shape == (3, 256) and (np.diff(lut[0].astype(int)) >= 0).all()
    x = np.arange(256) / 255.0
    assert np.array_equal(lut[1], np.clip(np.rint(255 * ((x ** 0.8 - 0.5) * 1.2 + 0.5 + 0.1)), 0, 255).astype(np.uint8))
    assert np.array_equal(_restated(src, tone, lut), lut[0][src[0]])
    noisy, _ = A.warp_items(base._replace(noise=5.0), (16, 16), (16, 16), False)
    assert noisy["noise_q12"] == round(5.0 / R.T_STD * 4096) and noisy["flags"] == _lib.SG_WARP_COLOR


def test_restated_noise_has_the_derived_moments():
    """The figures the GPU test asserts (mean within 7 of 128, standard deviation within 5 % of 147.80 on 12 288 draws), for
    eight samples of the restatement."""
    src = np.full((1, 64, 64, 3), 128, np.uint8)
    for sample in range(8):
        loud = R.warp(src, [R.item(flags=R.COLOR, noise_q12=4096, sample=sample)], None, 77)[0].astype(np.float64)
        assert abs(loud.mean() - 128) <= 7
        soft = R.warp(src, [R.item(flags=R.COLOR, noise_q12=512, sample=sample)], None, 77)[0].astype(np.float64)
        assert soft.min() > 0 and soft.max() < 255                     # 128 +- 510 / 8: nothing clipped
        assert abs((soft - 128).std() * 8 / R.T_STD - 1) <= 0.05
