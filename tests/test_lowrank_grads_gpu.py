"""Gradients that are low-rank functions of a small tensor, evaluated where they are consumed instead of written out.

Part A: the input gradient of a thin 1x1 convolution (Cout <= 4) in front of which a BatchNormalization sits is
dy[p, c] = sum_o g[p, o] w[c, o]; sg_bn_train_bwd_thin evaluates it inside the BatchNormalization backward's two kernels
(layers.ThinGradDeferred, SG_THIN_GRAD_BN).
Part B: the input gradient of an scSE block is dy (sig s + sig c) plus two rank-one terms, dg[n, c] / HW from the GlobalAveragePooling
and w[c] ds'[p] from the sSE convolution; sg_scse_bwd_sums + sg_scse_bwd_final write it once instead of three times
(layers.ScseGradDeferred, SG_SCSE_LOWRANK).
The expressions are moved, not changed: every comparison here is array_equal against the unfused launches of the same build."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().float().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("co,y_ld", [(1, 1), (2, 2), (3, 3), (4, 4), (2, 4), (1, 3)])
def test_bn_backward_on_an_unexpanded_thin_gradient_has_the_bits_of_dgrad_then_bn(engine, co, y_ld, relu):
    """thin dgrad + bn_train_bwd against bn_train_bwd_thin: dz, dgamma, dbeta.  C = 16 is the thin kernels' minimum, 36 is not a
    multiple of 8; 2 x 5 x 7 rows are odd with a ragged last chunk, 2 x 16 x 16 fill more than one row of lanes; y_ld > CO reads
    the gradient out of a wider tensor."""
    import torch
    e = engine
    gen = torch.Generator(device="cpu").manual_seed(1000 + 10 * co + y_ld + int(relu))
    for c in (16, 32, 36):
        for n, h, w_ in ((2, 5, 7), (2, 16, 16)):
            x = (torch.randn(n, h, w_, c, generator=gen) * 1.5 + 0.3).to(e.device)
            g = torch.randn(n, h, w_, y_ld, generator=gen).to(e.device)
            w = (torch.randn(1, 1, c, co, generator=gen) * 0.4).to(e.device)
            gamma = (torch.rand(c, generator=gen) + 0.5).to(e.device)
            beta = (torch.randn(c, generator=gen) * 0.2).to(e.device)
            xf = x.reshape(-1, c)
            mean = xf.mean(0).contiguous()
            invstd = (1.0 / torch.sqrt(xf.var(0, unbiased=False) + 1e-3)).contiguous()
            d = e.conv_desc((n, h, w_, c), co, 1, 1, y_ld=y_ld)
            assert e.conv2d_caps(d, dgrad=True).thin
            dy = e.conv2d_dgrad(g, w, d)
            dz0, dg0, db0 = e.bn_train_bwd(x, None, dy, gamma, mean, invstd, relu=relu, beta=beta)
            assert e.bn_train_bwd_thin_ok(x, g, w)
            dz1, dg1, db1 = e.bn_train_bwd_thin(x, g, w, gamma, mean, invstd, relu=relu, beta=beta)
            what = (c, n, h, w_, co, y_ld, relu)
            assert np.array_equal(_np(dz0), _np(dz1)), what
            assert np.array_equal(_np(dg0), _np(dg1)), what
            assert np.array_equal(_np(db0), _np(db1)), what
            assert np.abs(_np(dz1)).max() > 0 and np.isfinite(_np(dz1)).all(), what


def test_bn_backward_on_a_thin_gradient_declines_bf16_storage(engine):
    """The thin dgrad rounds dy through bf16 there; these kernels do not: the query says no and the entry point refuses."""
    import torch
    from building_detection_amd import _lib
    e = engine
    x = torch.randn(2, 8, 8, 16, device=e.device).to(torch.bfloat16)
    g = torch.randn(2, 8, 8, 2, device=e.device)
    w = torch.randn(1, 1, 16, 2, device=e.device)
    assert not e.bn_train_bwd_thin_ok(x, g, w)
    assert not e.bn_train_bwd_thin_ok(x, g.to(torch.bfloat16), w)
    assert e.lib.sg_bn_train_bwd_thin_ok(e.h, _lib.SG_BF16, 128, 16, 2, 2) == 0
    assert e.lib.sg_bn_train_bwd_thin_ok(e.h, _lib.SG_F32, 128, 16, 2, 2) == 1
    assert e.lib.sg_bn_train_bwd_thin_ok(e.h, _lib.SG_F32, 128, 16, 5, 5) == 0
    assert e.lib.sg_bn_train_bwd_thin_ok(e.h, _lib.SG_F32, 128, 16, 2, 1) == 0


@pytest.mark.parametrize("gap_first", [True, False])
@pytest.mark.parametrize("c", [16, 64, 20])
def test_scse_backward_in_one_final_pass_has_the_bits_of_the_three_passes(engine, c, gap_first):
    """scse_bwd, avgpool_bwd(accumulate), thin dgrad(res) - in either order of the last two - against scse_bwd_sums +
    scse_bwd_final: dx, ds, dc.  N = 2; 5 x 7 is odd and ragged, 16 x 16 spans several workgroups; C = 16 has C // 16 = 1, 64 fills
    a row of lanes, 20 is no multiple of 8 or 16."""
    import torch
    e = engine
    gen = torch.Generator(device="cpu").manual_seed(2000 + c + int(gap_first))
    n = 2
    for h, w_ in ((5, 7), (16, 16)):
        r = lambda *shape: torch.randn(*shape, generator=gen).to(e.device)
        x, dy, s, cl = r(n, h, w_, c), r(n, h, w_, c), r(n, h, w_, 1), r(n, 1, 1, c)
        dsp, dg, w = r(n, h, w_, 1), r(n, c), r(1, 1, c, 1) * 0.3
        d = e.conv_desc((n, h, w_, c), 1, 1, 1)
        assert e.conv2d_caps(d, dgrad=True).thin
        dx0, ds0, dc0 = e.scse_bwd(x, s, cl, dy)
        if gap_first:
            dx0 = e.avgpool_bwd(dg, (n, h, w_, c), h, w_, out=dx0, accumulate=True)
            dx0 = e.conv2d_dgrad(dsp, w, d, res=dx0)
        else:
            dx0 = e.conv2d_dgrad(dsp, w, d, res=dx0)
            dx0 = e.avgpool_bwd(dg, (n, h, w_, c), h, w_, out=dx0, accumulate=True)
        ds1, dc1 = e.scse_bwd_sums(x, s, cl, dy)
        dx1 = e.scse_bwd_final(dy, s, cl, dsp, w, dg, gap_first=gap_first)
        what = (c, h, w_, gap_first)
        assert np.array_equal(_np(dx0), _np(dx1)), what
        assert np.array_equal(_np(ds0), _np(ds1)), what
        assert np.array_equal(_np(dc0), _np(dc1)), what
        assert np.isfinite(_np(dx1)).all() and np.abs(_np(dx1)).max() > 0, what


def test_scse_final_pass_refuses_bf16_storage(engine):
    import torch
    from building_detection_amd import _lib
    e = engine
    t = torch.zeros(2 * 4 * 4 * 16, device=e.device)
    p = lambda: t.data_ptr()
    import ctypes as C
    v = lambda: C.c_void_p(p())
    rc = e.lib.sg_scse_bwd_final(e.h, e.stream, _lib.SG_BF16, 2, 16, 16, v(), v(), v(), v(), v(), v(), v(), 1)
    assert rc != 0


# --------------------------------------------------------------------------------------------------------- model level
METRICS = ("PA", "IoU", "MIoU", "F1_score")


def _steps(build, monkeypatch, env, steps, jit, dtype=None, spy=None):
    """`steps` training steps of a fresh model under `env`: per step (loss, counts) as arrays, then every gradient."""
    from building_detection_amd import losses
    from building_detection_amd.data import synthetic_batch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = build()
    m.compile(optimizer="adam", loss=losses.edge_focal_loss, metrics=[getattr(losses, k) for k in METRICS], jit_compile=jit)
    _, h, w, _ = m.inputs[0].shape
    x, y = synthetic_batch(2, h, w, seed=91)
    if spy is not None:
        spy(m)
    out = []
    for _ in range(steps):
        loss, counts = m.train_on_batch(x, y, return_device_scalars=True)
        out.append((_np(loss), _np(counts)))
    return m, out, [np.array(g) for g in m.get_gradients()]


def _same_bits(build, monkeypatch, switches, jit, engine, want_calls):
    """the switches off against on: loss, confusion counts, every gradient; want_calls: {engine entry: calls per eager step with the
    switches on}, none of them called with the switches off.  Under jit_compile the third step is the captured one."""
    steps = 3 if jit else 1
    calls = {k: [] for k in want_calls}
    for k in want_calls:
        orig = getattr(engine, k)
        monkeypatch.setattr(engine, k, lambda *a, _o=orig, _k=k, **kw: (calls[_k].append(1), _o(*a, **kw))[1])
    ma, outa, ga = _steps(build, monkeypatch, {k: "0" for k in switches}, steps, jit)
    assert not any(calls.values())
    mb, outb, gb = _steps(build, monkeypatch, {k: "1" for k in switches}, steps, jit)
    for k, want in want_calls.items():
        # (eager steps call it `want` times each; what the capture of the third step adds is the captured sweep's own business)
        got = len(calls[k])
        assert (got >= want * steps if (jit and want) else got == want * steps), (k, got, want, steps)
    for (la, ca), (lb, cb) in zip(outa, outb):
        assert np.array_equal(la, lb) and np.array_equal(ca, cb)
    assert len(ga) == len(gb) > 0
    for a, b in zip(ga, gb):
        assert np.array_equal(a, b)
    assert any(np.abs(a).max() > 0 for a in ga)


BOTH = ("SG_THIN_GRAD_BN", "SG_SCSE_LOWRANK")


def _v3plus():
    from building_detection_amd import zoo
    return zoo.Xception_DeepLabV3_Plus((64, 64, 3), 2, aspp_pool=4)


def _two_consumers():
    """BatchNormalization -> ReLU -> {sSE gate (thin, Cout = 1), GAP, combine}: the gate's input has other consumers, so its gradient
    is a tensor; the head behind the second BatchNormalization is the one pair that stays unexpanded."""
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model
    inp = L.Input(shape=(32, 32, 3))
    t = L.Activation("relu")(L.BatchNormalization()(L.Conv2D(16, 3, padding="same")(inp)))
    t = L.scse_block(t)
    t = L.Activation("relu")(L.BatchNormalization()(L.Conv2D(16, 3, padding="same")(t)))
    out = L.Conv2D(2, 1, padding="same", activation="softmax")(t)
    return Model(inputs=inp, outputs=out, name="two_consumers")


def _scse_unet():
    from building_detection_amd import zoo
    return zoo.UNet(2, (64, 64, 3))


@pytest.mark.parametrize("jit", [False, True])
def test_deeplab_step_with_low_rank_gradients_unexpanded_has_the_same_bits(engine, monkeypatch, jit):
    """The head pair and the four scSE blocks."""
    _same_bits(_v3plus, monkeypatch, BOTH, jit, engine, {"bn_train_bwd_thin": 1, "scse_bwd_final": 4})


@pytest.mark.parametrize("jit", [False, True])
def test_scse_unet_step_with_low_rank_gradients_unexpanded_has_the_same_bits(engine, monkeypatch, jit):
    """An scSE block behind every decoder stage; no BatchNormalization in front of the head."""
    _same_bits(_scse_unet, monkeypatch, BOTH, jit, engine, {"bn_train_bwd_thin": 0, "scse_bwd_final": 4})


def test_hrnet_step_with_the_head_gradient_unexpanded_has_the_same_bits(engine, monkeypatch):
    """No scSE block; the head reads a 64-channel BatchNormalization(+ReLU)."""
    from building_detection_amd import zoo
    _same_bits(lambda: zoo.HRNet((64, 64, 3)), monkeypatch, BOTH, False, engine, {"bn_train_bwd_thin": 1, "scse_bwd_final": 0})


@pytest.mark.parametrize("switch", BOTH)
def test_each_switch_alone_keeps_the_bits(engine, monkeypatch, switch):
    want = {"bn_train_bwd_thin": 1, "scse_bwd_final": 0} if switch == "SG_THIN_GRAD_BN" else {"scse_bwd_final": 4}
    monkeypatch.setenv(BOTH[1 - BOTH.index(switch)], "0")
    _same_bits(_v3plus, monkeypatch, (switch,), False, engine, want)


def test_a_thin_convolution_whose_input_has_other_consumers_takes_the_tensor_path(engine, monkeypatch):
    """The sSE gate reads a BatchNormalization's output that the GAP and the combine node read too: its gradient goes to the block's
    final kernel, never to the BatchNormalization; only the head pair is marked for that."""
    from building_detection_amd import layers as L
    m = _two_consumers()
    marked = [n for n in m.nodes if isinstance(n, L._ConvNode) and n.thin_bn is not None]
    assert len(marked) == 1 and marked[0].activation == "softmax"
    _same_bits(_two_consumers, monkeypatch, BOTH, False, engine, {"bn_train_bwd_thin": 1, "scse_bwd_final": 1})


def test_an_scse_input_with_a_fourth_consumer_takes_the_three_pass_path(engine, monkeypatch):
    """x of the block also feeds a residual add: the block is not marked, the sweep sums tensors as before."""
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model

    def build():
        inp = L.Input(shape=(32, 32, 3))
        t = L.Conv2D(16, 3, padding="same", activation="relu")(inp)
        t = L.add([L.scse_block(t), t])
        out = L.Conv2D(2, 1, padding="same", activation="softmax")(t)
        return Model(inputs=inp, outputs=out, name="fourth_consumer")
    assert not any(n.lowrank for n in build().nodes if isinstance(n, L._ScseCombineNode))
    _same_bits(build, monkeypatch, BOTH, False, engine, {"scse_bwd_final": 0, "scse_bwd_sums": 0})


def test_bf16_storage_keeps_the_materialised_gradients(engine, monkeypatch):
    """Under bf16 storage the query declines and the scSE block takes today's path: the switches change nothing."""
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model

    def build():
        inp = L.Input(shape=(32, 32, 3))
        t = L.Activation("relu")(L.BatchNormalization()(L.Conv2D(16, 3, padding="same")(inp)))
        t = L.scse_block(t)
        t = L.Activation("relu")(L.BatchNormalization()(L.Conv2D(16, 3, padding="same")(t)))
        out = L.Conv2D(2, 1, padding="same", activation="softmax")(t)
        return Model(inputs=inp, outputs=out, name="bf16_head", dtype="mixed_bfloat16")
    _same_bits(build, monkeypatch, BOTH, False, engine, {"bn_train_bwd_thin": 0, "scse_bwd_final": 0})
