"""Bilinear UpSampling2D, graph building only (no GPU): the layer, Model._fuse, the DeepLab builders' `upsampling` argument and
the tf.keras / tf.image.resize surface of building_detection_amd.tfshim."""
import pytest

from building_detection_amd import layers as L
from building_detection_amd.runtime import Model


def _up_nodes(model):
    return [n for n in model.nodes if isinstance(n, L._UpNode)]


def test_bilinear_layer_builds_with_the_up_sampled_shape():
    inp = L.Input(shape=(5, 7, 6))
    y = L.UpSampling2D(size=3, interpolation="bilinear")(inp)
    assert tuple(y.shape) == (None, 15, 21, 6)
    node = y.node
    assert isinstance(node, L._UpNode) and node.interpolation == "bilinear" and node.size == 3
    z = L.UpSampling2D(size=(2, 2))(inp)
    assert z.node.interpolation == "nearest" and tuple(z.shape) == (None, 10, 14, 6)


def test_unknown_interpolation_is_a_value_error_that_names_it():
    with pytest.raises(ValueError, match="bicubic"):
        L.UpSampling2D(size=2, interpolation="bicubic")


def _pair_model(interpolation):
    inp = L.Input(shape=(8, 8, 16))
    y = L.UpSampling2D(size=2, interpolation=interpolation)(inp)
    y = L.Conv2D(8, 3, padding="same")(y)
    return Model(inputs=inp, outputs=y)


def test_fuse_leaves_the_bilinear_pair_alone_and_still_fuses_the_nearest_one():
    near, bil = _pair_model("nearest"), _pair_model("bilinear")
    (un,), (ub,) = _up_nodes(near), _up_nodes(bil)
    conv_n = next(n for n in near.nodes if isinstance(n, L._ConvNode))
    conv_b = next(n for n in bil.nodes if isinstance(n, L._ConvNode))
    assert un.fused_into is conv_n and conv_n.up_src is un
    assert ub.fused_into is None and getattr(conv_b, "up_src", None) is None


@pytest.mark.parametrize("name", ["v3plus", "bam"])
def test_default_builders_are_unchanged_and_bilinear_changes_no_parameter(name):
    from building_detection_amd import zoo
    from building_detection_amd import graph

    def build(**kw):   # layer names count up per process: every build starts from the same counters, restored afterwards
        saved = dict(graph.Node._counter)
        graph.reset_names()
        try:
            return zoo.BUILDERS[name]((64, 64, 3), 2, aspp_pool=4, **kw)
        finally:
            graph.Node._counter.clear()
            graph.Node._counter.update(saved)

    default, near, bil = build(), build(upsampling="nearest"), build(upsampling="bilinear")
    assert [n.op for n in default.nodes] == [n.op for n in near.nodes] == [n.op for n in bil.nodes]
    assert default.count_params() == near.count_params() == bil.count_params()
    assert all(n.interpolation == "nearest" for n in _up_nodes(default) + _up_nodes(near))
    assert [n.fused_into is None for n in _up_nodes(default)] == [n.fused_into is None for n in _up_nodes(near)]
    assert [(p.name, p.shape, p.kind) for p in default.params] == [(p.name, p.shape, p.kind) for p in bil.params]
    # every up-sampling of the ASPP and the decoder is bilinear; the SK block's 1x1 broadcast (the first one built) is not switched
    modes = [n.interpolation for n in _up_nodes(bil)]
    assert modes[0] == "nearest" and _up_nodes(bil)[0].inputs[0].shape[1:3] == (1, 1)
    assert modes[1:] == ["bilinear"] * (len(modes) - 1) and len(modes) == {"v3plus": 4, "bam": 5}[name]
    assert all(n.fused_into is None for n in _up_nodes(bil))
    with pytest.raises(ValueError, match="bicubic"):
        build(upsampling="bicubic")


def test_full_size_default_graph_has_the_same_nodes_with_and_without_the_argument():
    from building_detection_amd import zoo
    a, b = zoo.Xception_DeepLabV3_Plus(), zoo.Xception_DeepLabV3_Plus(upsampling="nearest")
    assert [n.op for n in a.nodes] == [n.op for n in b.nodes] and a.count_params() == b.count_params()


BUILDER_TEXT = """
import tensorflow as tf
from tensorflow.keras.layers import Input, Conv2D, UpSampling2D

def head(h, w, out_hw):
    inp = Input(shape=(h, w, 8))
    x = Conv2D(8, 3, padding='same')(inp)
    x = tf.keras.layers.UpSampling2D(size=(4, 4), interpolation='bilinear')(x)
    x = Conv2D(4, 1)(x)
    x = tf.image.resize(x, out_hw, method='bilinear')
    return tf.keras.Model(inputs=inp, outputs=x)

def nearest_head(h, w):
    inp = Input(shape=(h, w, 8))
    return tf.keras.Model(inputs=inp, outputs=tf.image.resize(inp, (3 * h, 3 * w), method='nearest'))
"""


def test_builder_text_with_keras_upsampling_and_image_resize_runs_on_the_shim():
    from building_detection_amd import tfshim
    names = tfshim.install("tensorflow")
    try:
        ns = {"__name__": "bilinear_builder_text"}
        exec(compile(BUILDER_TEXT, "<builder text>", "exec"), ns)
        m = ns["head"](4, 6, (2 * 16, 2 * 24))
        ups = _up_nodes(m)
        assert [(n.size, n.interpolation) for n in ups] == [(4, "bilinear"), (2, "bilinear")]
        assert tuple(m.outputs[0].shape) == (None, 32, 48, 4)
        (n,) = _up_nodes(ns["nearest_head"](4, 6))
        assert (n.size, n.interpolation) == (3, "nearest")
        for bad in [(33, 48), (32, 72), (8, 12), (0, 0)]:   # no multiple, two different multiples, a reduction, nothing
            with pytest.raises(ValueError, match="integer"):
                ns["head"](4, 6, bad)
        with pytest.raises(ValueError, match="bicubic"):
            tfshim.image.resize(L.Input(shape=(4, 4, 2)), (8, 8), method="bicubic")
    finally:
        tfshim.uninstall(names)
