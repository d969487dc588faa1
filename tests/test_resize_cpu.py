"""The arbitrary-size resize without a GPU: the numpy restatement of csrc/resize_coords.h (tests/_resize_ref.py) against
torch's float64 interpolate and its autograd, the span of the backward's gather against a brute-force scan, the Resizing
layer's graph node and refusals, builder text on the shim, and the argument checks of multi-scale soft scenes."""
import numpy as np
import pytest
import torch

import _resize_ref as R
from building_detection_amd import layers as L
from building_detection_amd.runtime import Model

F64 = torch.float64
REF_AGREE = 1e-12
SIZES = range(1, 25)


def _torch_axis(x, m):
    """x [n] -> [m] by torch's float64 bilinear interpolate, align_corners=False; also the gradient of sum(y * g)."""
    t = torch.tensor(x, dtype=F64, requires_grad=True)
    y = torch.nn.functional.interpolate(t[None, None, :, None], size=(m, 1), mode="bilinear", align_corners=False)[0, 0, :, 0]
    return t, y


def test_integer_taps_agree_with_torch_float64_interpolate_and_autograd_for_all_sizes_up_to_24():
    rng = np.random.default_rng(7)
    worst_f = worst_b = 0.0
    for n in SIZES:
        for m in SIZES:
            x, g = rng.uniform(-1, 1, n), rng.uniform(-1, 1, m)
            t, y = _torch_axis(x, m)
            y.backward(torch.tensor(g, dtype=F64))
            mine = R.resize_fwd(x.reshape(1, n, 1, 1), m, 1)[0, :, 0, 0]
            back = R.resize_bwd(g.reshape(1, m, 1, 1), n, 1)[0, :, 0, 0]
            worst_f = max(worst_f, np.abs(mine - y.detach().numpy()).max())
            worst_b = max(worst_b, np.abs(back - t.grad.numpy()).max())
    print(f"forward {worst_f:.3e}, backward {worst_b:.3e}")
    assert worst_f <= REF_AGREE and worst_b <= REF_AGREE


def test_two_axes_agree_with_torch_and_the_backward_is_the_transpose():
    rng = np.random.default_rng(11)
    for (h, w, oh, ow) in [(5, 7, 8, 5), (8, 8, 3, 3), (1, 1, 4, 6), (4, 6, 1, 1), (6, 9, 9, 6), (3, 4, 12, 16)]:
        x, dy = rng.uniform(-1, 1, (2, h, w, 3)), rng.uniform(-1, 1, (2, oh, ow, 3))
        t = torch.tensor(x, dtype=F64, requires_grad=True)
        y = torch.nn.functional.interpolate(t.permute(0, 3, 1, 2), size=(oh, ow), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        y.backward(torch.tensor(dy, dtype=F64))
        assert np.abs(R.resize_fwd(x, oh, ow) - y.detach().numpy()).max() <= REF_AGREE
        assert np.abs(R.resize_bwd(dy, h, w) - t.grad.numpy()).max() <= REF_AGREE
        for method in ("bilinear", "nearest"):
            lhs = (R.resize_fwd(x, oh, ow, method) * dy).sum()
            assert abs(lhs - (x * R.resize_bwd(dy, h, w, method)).sum()) <= 1e-10


def test_the_span_never_misses_an_output_and_never_exceeds_its_bound():
    for n in SIZES:
        for m in SIZES:
            for i in range(n):
                o0, o1 = R.span(i, n, m)
                assert 0 <= o0 and o1 <= m and o1 - o0 <= 2 * m // n + 1, (n, m, i, o0, o1)
                hit = R.span_brute(i, n, m)
                if hit is not None:
                    assert o0 <= hit[0] and hit[1] < o1, (n, m, i, o0, o1, hit)


def test_nearest_is_the_integer_rule_and_its_runs_partition_the_outputs():
    for n in SIZES:
        for m in SIZES:
            src = R.nearest_src(n, m)
            assert src.min() >= 0 and src.max() <= n - 1 and (np.diff(src) >= 0).all()
            o = np.arange(m)
            exact = np.floor((2 * o + 1) * n / (2 * m) + 1e-12).astype(np.int64)     # (o + 1/2) n / m with ties resolved upwards
            assert (src == np.minimum(exact, n - 1)).all()
    assert (R.nearest_src(6, 9) == np.array([0, 1, 1, 2, 3, 3, 4, 5, 5])).all()     # the tie pair: (2o + 1) 6 / 18 hits integers
    assert (R.nearest_src(5, 5) == np.arange(5)).all()


def test_equal_sizes_are_the_identity_exactly():
    x = np.random.default_rng(3).uniform(-1, 1, (1, 6, 6, 2))
    lo, hi, r, _ = R.taps(6, 6)
    assert (lo == np.arange(6)).all() and (hi == lo).all() and (r == 0).all()
    assert np.array_equal(R.resize_fwd(x, 6, 6), x) and np.array_equal(R.resize_bwd(x, 6, 6), x)


# ------------------------------------------------------------------------------------------------ the layer
def test_resizing_builds_a_node_of_the_right_shape():
    inp = L.Input(shape=(16, 12, 8))
    y = L.Resizing(11, 9)(inp)
    assert tuple(y.shape) == (None, 11, 9, 8)
    z = L.Resizing(24, 20, interpolation="nearest", name="big")(y)
    assert tuple(z.shape) == (None, 24, 20, 8)
    m = Model(inputs=inp, outputs=z)
    nodes = [n for n in m.nodes if isinstance(n, L._ResizeNode)]
    assert [(n.op, n.height, n.width, n.interpolation) for n in nodes] == [("resizing", 11, 9, "bilinear"), ("resizing", 24, 20, "nearest")]
    assert nodes[1].name == "big" and m.count_params() == 0


def test_resizing_refuses_what_it_must():
    with pytest.raises(ValueError, match="crop_to_aspect_ratio"):
        L.Resizing(8, 8, crop_to_aspect_ratio=True)
    for bad in ("bicubic", "area", "lanczos3"):
        with pytest.raises(ValueError, match="interpolation"):
            L.Resizing(8, 8, interpolation=bad)
    for h, w in [(0, 8), (8, 16385)]:
        with pytest.raises(ValueError, match="16384"):
            L.Resizing(h, w)


def test_no_fusion_mark_touches_a_graph_because_of_a_resizing_node():
    def build(resize):
        inp = L.Input(shape=(16, 16, 8))
        x = L.Conv2D(8, 3, padding="same")(inp)
        x = L.UpSampling2D(size=2)(x)
        if resize:
            x = L.Resizing(32, 32)(x)
        x = L.Conv2D(4, 3, padding="same")(x)
        return Model(inputs=inp, outputs=x)
    with_node, without = build(True), build(False)
    up_w = next(n for n in with_node.nodes if isinstance(n, L._UpNode))
    up_o = next(n for n in without.nodes if isinstance(n, L._UpNode))
    assert up_o.fused_into is not None, "UpSampling2D(2) -> Conv2D 3x3 is the marked pair"
    assert up_w.fused_into is None, "a Resizing node between the two ends the pair, as an _UpNode in that place would"


BUILDER_TEXT = """
import tensorflow as tf
from tensorflow.keras.layers import Input, Conv2D, Resizing

def head(h, w):
    inp = Input(shape=(h, w, 8))
    x = Conv2D(8, 3, padding='same')(inp)
    x = tf.keras.layers.Resizing(11, 9, interpolation='bilinear')(x)
    x = Conv2D(4, 1)(x)
    x = Resizing(height=500, width=375, interpolation='nearest')(x)
    return tf.keras.Model(inputs=inp, outputs=x)
"""


def test_builder_text_with_keras_resizing_runs_on_the_shim_and_image_resize_still_refuses_other_sizes():
    from building_detection_amd import tfshim
    names = tfshim.install("tensorflow")
    try:
        ns = {"__name__": "resizing_builder_text"}
        exec(compile(BUILDER_TEXT, "<builder text>", "exec"), ns)
        m = ns["head"](16, 12)
        nodes = [n for n in m.nodes if isinstance(n, L._ResizeNode)]
        assert [(n.height, n.width, n.interpolation) for n in nodes] == [(11, 9, "bilinear"), (500, 375, "nearest")]
        assert tuple(m.outputs[0].shape) == (None, 500, 375, 4)
        with pytest.raises(ValueError, match="integer"):
            tfshim.image.resize(L.Input(shape=(4, 6, 2)), (33, 48), method="bilinear")
    finally:
        tfshim.uninstall(names)


# ------------------------------------------------------------------------------------------------ multi-scale soft scenes
class _NoModel:
    """Stands where a model would: the argument checks of detection_soft come before anything reads it."""


def test_detection_soft_checks_scales_and_scale_weights_before_it_touches_a_model():
    from building_detection_amd import pipeline
    img = np.zeros((8, 8, 3), np.uint8)
    for bad in [(0.2,), (1.0, 4.5), (float("nan"),), ()]:
        with pytest.raises(ValueError, match="scales"):
            pipeline.detection_soft(img, models=_NoModel(), scales=bad)
    with pytest.raises(ValueError, match="2 scale_weights for 3 scales"):
        pipeline.detection_soft(img, models=_NoModel(), scales=(0.75, 1.0, 1.5), scale_weights=(1.0, 2.0))
    with pytest.raises(ValueError, match="scale_weights"):
        pipeline.detection_soft(img, models=_NoModel(), scales=(1.0,), scale_weights=(0.0,))
    with pytest.raises(ValueError, match="scale_weights without scales"):
        pipeline.detection_soft(img, models=_NoModel(), scale_weights=(1.0,))
    assert pipeline.check_scales((0.25, 1, 4)) == [0.25, 1.0, 4.0]


def test_scaled_size_rounds_half_up_keeps_one_pixel_and_names_its_limits():
    from building_detection_amd.pipeline import scaled_size
    assert scaled_size(37, 45, 0.75) == (28, 34)      # 27.75 -> 28, 33.75 -> 34
    assert scaled_size(37, 45, 1.5) == (56, 68)       # 55.5 -> 56 (half up), 67.5 -> 68
    assert scaled_size(37, 45, 1.0) == (37, 45)
    assert scaled_size(1, 3, 0.25) == (1, 1)          # 0.25 -> max(1, 0), 0.75 -> 1
    assert scaled_size(10, 10, 0.25) == (3, 3)        # 2.5 -> 3
    assert scaled_size(4096, 4096, 4.0) == (16384, 16384)
    with pytest.raises(ValueError, match="16384"):
        scaled_size(4097, 100, 4.0)
    with pytest.raises(ValueError, match="16384"):
        scaled_size(20000, 100, 0.5)
