"""Optimizers, host side (no GPU): constructor validation, name resolution in `get` / Model.compile / the tf.keras shim, the
chunk table's properties, and the float64 reference of the GPU tests (tests/_optim_ref.py) against independent restatements."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _optim_ref as R
from _guarded import adam_ref
from building_detection_amd import _lib, optimizers as O, runtime

L = O.CHUNK


# ------------------------------------------------------------------------------------------------ construction
def test_defaults_follow_keras():
    a = O.Adam()
    assert (float(a.lr), a.beta_1, a.beta_2, a.epsilon, a.amsgrad, a.weight_decay, a.use_ema, a.ema_momentum) == \
        (1e-3, 0.9, 0.999, 1e-7, False, None, False, 0.99)
    assert (a.clipnorm, a.clipvalue, a.global_clipnorm) == (None, None, None) and a.iterations == 0
    assert a._plain() and isinstance(a, runtime.Optimizer)
    assert O.AdamW().weight_decay == 0.004 and not O.AdamW()._plain()
    s = O.SGD()
    assert (float(s.lr), s.momentum, s.nesterov) == (0.01, 0.0, False) and not s._plain()
    assert float(O.Adam(lr=3e-4).lr) == 3e-4 and float(O.SGD(lr=0.1).learning_rate) == 0.1
    a.lr = 5e-4                         # what the LR callbacks do
    assert float(a.learning_rate) == 5e-4


def test_runtime_optimizer_keeps_its_surface():
    o = runtime.Optimizer(lr=2e-3, beta_1=0.8, beta_2=0.99, epsilon=1e-6)
    assert (float(o.lr), float(o.learning_rate), o.iterations, o.beta_1, o.beta_2, o.epsilon) == (2e-3, 2e-3, 0, 0.8, 0.99, 1e-6)
    o.iterations = 3
    lr_t, lr = o.step_scalars()
    assert lr == 2e-3 and lr_t == 2e-3 * math.sqrt(1 - 0.99 ** 3) / (1 - 0.8 ** 3)


@pytest.mark.parametrize("kw", [dict(clipnorm=1.0, clipvalue=1.0), dict(clipnorm=1.0, global_clipnorm=1.0),
                                dict(clipvalue=0.5, global_clipnorm=2.0), dict(clipnorm=1.0, clipvalue=1.0, global_clipnorm=1.0)])
@pytest.mark.parametrize("cls", [O.Adam, O.AdamW, O.SGD])
def test_more_than_one_clip_mode_is_refused(cls, kw):
    with pytest.raises(ValueError, match="at most one"):
        cls(**kw)


@pytest.mark.parametrize("kw", [dict(learning_rate=-1e-3), dict(learning_rate=float("nan")), dict(weight_decay=-0.1),
                                dict(weight_decay=float("inf")), dict(clipnorm=-1.0), dict(clipvalue=float("nan")),
                                dict(global_clipnorm=-2.0), dict(ema_momentum=-0.5), dict(ema_momentum=float("inf")),
                                dict(lr=-1.0)])
@pytest.mark.parametrize("cls", [O.Adam, O.AdamW, O.SGD])
def test_negative_or_non_finite_hyperparameters_are_refused(cls, kw):
    with pytest.raises(ValueError):
        cls(**kw)


@pytest.mark.parametrize("cls,kw", [(O.Adam, dict(beta_1=-0.1)), (O.Adam, dict(beta_2=float("nan"))), (O.Adam, dict(epsilon=-1e-7)),
                                    (O.AdamW, dict(epsilon=float("inf"))), (O.SGD, dict(momentum=-0.9)),
                                    (O.SGD, dict(momentum=float("nan")))])
def test_kind_specific_hyperparameters_are_checked(cls, kw):
    with pytest.raises(ValueError):
        cls(**kw)


def test_get_resolves_names_and_instances():
    for name, cls in (("adam", O.Adam), ("Adam", O.Adam), ("ADAMW", O.AdamW), ("adamw", O.AdamW), ("sgd", O.SGD), ("SGD", O.SGD)):
        assert type(O.get(name)) is cls
    inst = O.SGD(momentum=0.9)
    assert O.get(inst) is inst
    old = runtime.Optimizer()
    assert O.get(old) is old
    with pytest.raises(ValueError, match="'adam'.*'adamw'.*'sgd'"):
        O.get("rmsprop")


def _tiny_model():
    from building_detection_amd import layers as KL
    inp = KL.Input(shape=(16, 16, 3))
    x = KL.Conv2D(8, 3, padding="same", name="c1")(inp)
    x = KL.BatchNormalization(name="bn1")(x)
    x = KL.SeparableConv2D(8, 3, name="sep1")(x)
    return runtime.Model(inp, KL.Conv2D(2, 1, activation="softmax", name="head")(x))


def test_compile_resolves_strings_and_keeps_the_value_error():
    from building_detection_amd.losses import focal_loss
    m = _tiny_model()
    for name, cls in (("adam", O.Adam), ("AdamW", O.AdamW), ("sgd", O.SGD)):
        m.compile(optimizer=name, loss=focal_loss)
        assert type(m.optimizer) is cls
    assert m.optimizer is not None and O.get("adam")._plain()
    with pytest.raises(ValueError, match="'adam'.*'adamw'.*'sgd'"):
        m.compile(optimizer="nadam", loss=focal_loss)
    inst = runtime.Optimizer()
    m.compile(optimizer=inst, loss=focal_loss)
    assert m.optimizer is inst


def test_shim_exposes_keras_optimizers():
    import sys
    from building_detection_amd import tfshim
    assert tfshim.keras.optimizers.Adam is O.Adam and tfshim.keras.optimizers.AdamW is O.AdamW
    assert tfshim.keras.optimizers.SGD is O.SGD
    names = tfshim.install("tf_optim_probe")
    try:
        import tf_optim_probe as tf
        from tf_optim_probe.keras.optimizers import SGD
        assert tf.keras.optimizers.Adam is O.Adam and SGD is O.SGD
        assert sys.modules["tf_optim_probe.keras"].optimizers.AdamW is O.AdamW
    finally:
        tfshim.uninstall(names)


# ------------------------------------------------------------------------------------------------ chunk table
def _params(sizes, kinds=None, frozen=()):
    """A parameter list laid out as Model._layout_params does it: trainable and frozen parameters in arenas of their own."""
    kinds = kinds or ["kernel"] * len(sizes)
    out, off_t, off_n = [], 0, 0
    for i, (n, k) in enumerate(zip(sizes, kinds)):
        tr = i not in frozen
        p = SimpleNamespace(name=f"layer{i}/{k}", size=n, kind=k, trainable=tr, offset=off_t if tr else off_n)
        if tr:
            off_t += (n + 3) // 4 * 4
        else:
            off_n += (n + 3) // 4 * 4
        out.append(p)
    return out, off_t


def _check_table(params, n_arena, chunk, chunks, segs, trainable):
    assert [p for p in params if p.trainable] == trainable and len(segs) == len(trainable)
    cover = np.zeros(n_arena, np.int32)
    for c in chunks:
        p = trainable[c["segment"]]
        assert c["start"] % 4 == 0 and 1 <= c["length"] <= chunk
        assert p.offset <= c["start"] and c["start"] + c["length"] <= p.offset + p.size, "a chunk crosses its parameter"
        cover[c["start"]:c["start"] + c["length"]] += 1
    live = np.zeros(n_arena, bool)
    for p in trainable:
        live[p.offset:p.offset + p.size] = True
    assert (cover[live] == 1).all(), "a trainable element is not covered exactly once"
    assert (cover[~live] == 0).all(), "a padding element is covered"
    assert (np.diff(chunks["start"]) > 0).all() and (np.diff(chunks["segment"]) >= 0).all()
    at = 0
    for s, sg in enumerate(segs):
        assert sg["chunk_begin"] == at and sg["chunk_end"] > at
        assert (chunks["segment"][sg["chunk_begin"]:sg["chunk_end"]] == s).all()
        at = sg["chunk_end"]
    assert at == len(chunks)


SIZES = [1, 3, 4, 5, L, L + 1, 2 * L + 3]
KINDS = ["bias", "gamma", "kernel", "beta", "depthwise_kernel", "pointwise_kernel", "kernel"]


def test_chunk_table_of_a_hand_made_parameter_list():
    params, n = _params(SIZES + [7], KINDS + ["moving_mean"], frozen={7})
    chunks, segs, tr = O.chunk_table(params)
    assert chunks.dtype.itemsize == 16 and segs.dtype.itemsize == 16
    _check_table(params, n, L, chunks, segs, tr)
    assert [int(s["chunk_end"] - s["chunk_begin"]) for s in segs] == [1, 1, 1, 1, 1, 2, 3]
    assert [int(c["length"]) for c in chunks[-5:]] == [L, 1, L, L, 3]
    assert [int(s["flags"]) for s in segs] == [0, 0, 1, 0, 1, 1, 1]          # by kind: kernels only
    assert [int(s["flags"]) for s in O.chunk_table(params, decay_kinds=None)[1]] == [1] * 7
    ex = O.chunk_table(params, exclude=("layer6/", "layer4"))[1]
    assert [int(s["flags"]) for s in ex] == [0, 0, 1, 0, 0, 1, 0]            # by substring of the name
    small, segs8, _ = O.chunk_table(params, chunk=8)                        # another bound: same properties
    _check_table(params, n, 8, small, segs8, tr)
    with pytest.raises(ValueError):
        O.chunk_table(params, chunk=6)
    params[2].offset += 1
    with pytest.raises(ValueError):
        O.chunk_table(params)


def test_exclude_from_weight_decay_reaches_the_table():
    opt = O.AdamW()
    opt.exclude_from_weight_decay(var_names=["layer2/"])
    params, _ = _params(SIZES, KINDS)
    segs = O.chunk_table(params, O.CHUNK, opt.decay_kinds, opt._exclude)[1]
    assert [int(s["flags"]) for s in segs] == [0, 0, 0, 0, 1, 1, 1]
    assert O.AdamW(decay_kinds=None).decay_kinds is None


def test_chunk_table_of_a_real_builder():
    from building_detection_amd import zoo
    m = zoo.Xception_DeepLabV3_Plus((64, 64, 3), 2, aspp_pool=4)
    chunks, segs, tr = O.chunk_table(m.params)
    _check_table(m.params, m._n_train, L, chunks, segs, tr)
    assert int(chunks["length"].sum()) == sum(p.size for p in m.trainable_weights)
    for p, s in zip(tr, segs):
        assert bool(s["flags"] & _lib.SG_OPT_SEG_DECAY) == (p.kind in O.DEFAULT_DECAY_KINDS), p.name
    assert any(s["flags"] for s in segs) and not all(s["flags"] for s in segs)


def test_ctypes_mirrors_match_the_table_layouts():
    import ctypes as C
    assert C.sizeof(_lib.OptimChunk) == O.CHUNK_DTYPE.itemsize == 16 and C.sizeof(_lib.OptimSeg) == O.SEG_DTYPE.itemsize == 16
    assert C.sizeof(_lib.OptimDesc) == 11 * 4 and C.sizeof(_lib.OptimTable) == 48
    d = O.SGD(momentum=0.9, nesterov=True, clipnorm=2.0, use_ema=True, weight_decay=0.01).descriptor(0.5)
    assert (d.kind, d.flags, d.clip) == (_lib.SG_OPT_SGD, _lib.SG_OPT_NESTEROV | _lib.SG_OPT_EMA, _lib.SG_OPT_CLIP_NORM)
    assert (d.momentum, d.clip_c, d.grad_scale) == (np.float32(0.9), 2.0, 0.5)
    d = O.Adam(amsgrad=True, global_clipnorm=1.0).descriptor()
    assert (d.kind, d.flags, d.clip) == (_lib.SG_OPT_ADAM, _lib.SG_OPT_AMSGRAD, _lib.SG_OPT_CLIP_GLOBAL)
    assert O.SGD(nesterov=True).descriptor().flags == 0      # no momentum: nothing to look ahead with


# ------------------------------------------------------------------------------------------------ the float64 reference
def _arena(seed, params, n, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo)


def test_reference_without_options_is_the_guarded_adam_reference():
    params, n = _params(SIZES, KINDS)
    segs = [(p.offset, p.size, p.kind in O.DEFAULT_DECAY_KINDS) for p in params]
    w, g = _arena(1, params, n), _arena(2, params, n)
    cfg = R.Cfg(grad_scale=0.5)
    st = R.new_state(cfg, w)
    w1, m1, v1 = w.clone(), st["m"].clone(), st["v"].clone()
    for t in (1, 2, 3):
        lr_t = R.adam_lr_t(1e-3 * t, 0.9, 0.999, t)
        w, st = R.step_ref(cfg, segs, w, g * t, st, 1e-3 * t, lr_t)
        w1n, m1, v1 = adam_ref(w1, m1, v1, g * t, lr_t, 0.9, 0.999, 1e-7, 0.5)
        for p in params:      # (adam_ref walks the flat arena, padding included: compare the parameters)
            sl = slice(p.offset, p.offset + p.size)
            assert torch.equal(w[sl], w1n[sl]) and torch.equal(st["m"][sl], m1[sl]) and torch.equal(st["v"][sl], v1[sl])
        w1 = w1n
    live = torch.zeros(n, dtype=torch.bool)
    for p in params:
        live[p.offset:p.offset + p.size] = True
    assert torch.equal(st["ema"], R.new_state(cfg, _arena(1, params, n))["ema"]), "no average asked for, none kept"
    assert (st["m"][~live] == 0).all(), "padding moved"


@pytest.mark.parametrize("nesterov", [False, True])
def test_reference_sgd_is_torch_sgd_at_a_constant_learning_rate(nesterov):
    """Keras keeps m = momentum m - lr g, torch buf = momentum buf + g: with a constant lr, m = -lr buf and the steps coincide."""
    params, n = _params([5, 64, 3], ["kernel", "kernel", "bias"])
    segs = [(p.offset, p.size, False) for p in params]
    w0 = _arena(3, params, n)
    cfg = R.Cfg(kind="sgd", momentum=0.9, nesterov=nesterov)
    tw = torch.nn.Parameter(w0.clone())
    sgd = torch.optim.SGD([tw], lr=0.05, momentum=0.9, nesterov=nesterov)
    w, st = w0, R.new_state(cfg, w0)
    for t in range(4):
        g = _arena(10 + t, params, n)
        w, st = R.step_ref(cfg, segs, w, g, st, 0.05)
        tw.grad = g.clone()
        sgd.step()
        for p in params:
            sl = slice(p.offset, p.offset + p.size)
            assert (w[sl] - tw.detach()[sl]).abs().max() <= 1e-14, (t, p.name)


def test_reference_clip_decay_and_average_by_hand():
    segs = [(0, 2, True), (4, 2, False)]
    w = torch.tensor([1.0, -2.0, 9.0, 9.0, 0.5, 0.25, 9.0, 9.0], dtype=torch.float64)
    g = torch.tensor([3.0, 4.0, 9.0, 9.0, 0.3, 0.4, 9.0, 9.0], dtype=torch.float64)
    tot, per = R.norms_ref(segs, g)
    assert per.tolist() == pytest.approx([25.0, 0.25]) and float(tot) == pytest.approx(25.25)
    cfg = R.Cfg(kind="sgd", clip="norm", clip_c=1.0, weight_decay=0.1, ema_momentum=0.5)
    w1, st = R.step_ref(cfg, segs, w, g, R.new_state(cfg, w), 0.1)
    want0 = (1.0 - 0.01 * 1.0) - 0.1 * 3.0 / 5.0         # decayed, clipped from norm 5 to 1
    assert float(w1[0]) == pytest.approx(want0) and float(w1[4]) == pytest.approx(0.5 - 0.1 * 0.3)   # norm 0.5 < c: unclipped
    assert float(st["ema"][0]) == pytest.approx(0.5 * 1.0 + 0.5 * want0)
    assert w1[2:4].tolist() == [9.0, 9.0] and w1[6:].tolist() == [9.0, 9.0]
    cfg = R.Cfg(kind="sgd", clip="global", clip_c=1.0)
    w2, _ = R.step_ref(cfg, segs, w, g, R.new_state(cfg, w), 0.1)
    assert float(w2[5]) == pytest.approx(0.25 - 0.1 * 0.4 / math.sqrt(25.25))
    cfg = R.Cfg(kind="sgd", clip="value", clip_c=0.35)
    w3, _ = R.step_ref(cfg, segs, w, g, R.new_state(cfg, w), 0.1)
    assert float(w3[1]) == pytest.approx(-2.0 - 0.035) and float(w3[4]) == pytest.approx(0.5 - 0.03)
    cfg = R.Cfg(amsgrad=True)
    st = R.new_state(cfg, w)
    st["vhat"][:] = 100.0
    w4, st4 = R.step_ref(cfg, segs, w, g, st, 1e-3, 1e-3)
    assert float(st4["vhat"][0]) == 100.0 and float(w4[0]) == pytest.approx(1.0 - 1e-3 * 0.3 / (10.0 + 1e-7))
