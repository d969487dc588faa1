"""layers.Resizing through the runtime on the GPU: the graph
    Conv2D(8, 3) -> Resizing(11, 9) -> Conv2D(4, 1) -> Resizing(24, 20, 'nearest') -> Conv2D(2, 1, softmax)
on 16 x 12 inputs - a bilinear reduction on both axes, then a nearest enlargement by non-integer ratios - against a float64
torch graph of the same nodes (torch's bilinear interpolate with align_corners=False; nearest by the integer rule of
tests/_resize_ref.py, since torch's own nearest rounds ties in floating point), at the tolerances of
tests/test_bilinear_models_gpu.py: 2e-5 of the output's scale forward, _fit_check.compare_gradients for the weight gradients,
bit identity between the eager and the captured train step, and test_bf16_gpu's model bounds under mixed_bfloat16."""
import numpy as np
import pytest
import torch

import _fit_check as FC
import _resize_ref as R
import test_bf16_gpu as B16
from oracle import models as M
from oracle import tfops as T

pytestmark = pytest.mark.gpu

IN_HW, MID_HW, OUT_HW = (16, 12), (11, 9), (24, 20)


def build(**kw):
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model
    inp = L.Input(shape=IN_HW + (3,))
    x = L.Conv2D(8, 3, padding="same")(inp)
    x = L.Resizing(*MID_HW)(x)
    x = L.Conv2D(4, 1)(x)
    x = L.Resizing(*OUT_HW, interpolation="nearest")(x)
    out = L.Conv2D(2, 1, activation="softmax")(x)
    return Model(inputs=inp, outputs=out, **kw)


def batch(seed):
    from building_detection_amd.data import synthetic_batch
    _, y = synthetic_batch(2, *OUT_HW, seed=seed)
    x = np.random.default_rng(seed).uniform(-1, 1, (2,) + IN_HW + (3,)).astype(np.float32)
    return x, y


def random_weights(model, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.normal(0, 0.3, p.shape).astype(np.float32) for p in model.params]


def torch_graph(ws, x, dtype):
    """The same five nodes in torch; returns (probabilities, the leaf tensors of the six weights)."""
    leaves = [torch.from_numpy(w).to(dtype).requires_grad_() for w in ws]
    k1, b1, k2, b2, k3, b3 = leaves
    t = T.conv2d(torch.from_numpy(x).to(dtype), k1, b1, 1, 1, "same")
    t = torch.nn.functional.interpolate(t.permute(0, 3, 1, 2), size=MID_HW, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    t = T.conv2d(t, k2, b2, 1, 1, "same")
    ih = torch.from_numpy(R.nearest_src(MID_HW[0], OUT_HW[0]))
    iw = torch.from_numpy(R.nearest_src(MID_HW[1], OUT_HW[1]))
    t = t[:, ih][:, :, iw]
    return T.softmax(T.conv2d(t, k3, b3, 1, 1, "same")), leaves


def test_forward_and_weight_gradients_against_float64(engine):
    from building_detection_amd import layers as L
    from building_detection_amd.losses import edge_focal_loss
    model = build()
    ws = random_weights(model)
    model.set_weights(ws)
    assert [n.op for n in model.nodes if isinstance(n, L._ResizeNode)] == ["resizing", "resizing"]
    x, y = batch(23)
    with torch.no_grad():
        ref = torch_graph(ws, x, torch.float64)[0].numpy()
    got = model.predict(x)
    assert got.shape == (2,) + OUT_HW + (2,)
    scale, err = float(np.abs(ref).max()), float(np.abs(got - ref).max())
    print(f"resizing graph: max|p - fp64| = {err:.3e} (bound {2e-5 * scale:.3e})")
    assert err <= 2e-5 * scale

    model.compile(optimizer="adam", loss=edge_focal_loss)
    logs = model.train_on_batch(x, y)
    grads = [g.astype(np.float64) for g in model.get_gradients()]
    out = {}
    for dtype in (torch.float32, torch.float64):
        p, leaves = torch_graph(ws, x, dtype)
        loss = M.loss_fn("edge_focal_loss", torch.from_numpy(y).to(dtype), p)
        loss.backward()
        out[dtype] = (loss.item(), [t.grad.double().numpy() for t in leaves])
    (l32, g32), (l64, g64) = out[torch.float32], out[torch.float64]
    print(f"resizing graph: loss gpu {logs['loss']:.7f} cpu32 {l32:.7f} fp64 {l64:.7f}")
    assert abs(logs["loss"] - l64) <= 5 * abs(l32 - l64) + 1e-5 * abs(l64)
    FC.compare_gradients("resizing graph", [p.name for p in model.params if p.trainable], grads, g32, g64)


def test_captured_train_step_is_bit_identical_to_eager(engine):
    from building_detection_amd.losses import edge_focal_loss, PA, IoU
    from building_detection_amd.runtime import GraphedTrainStep
    ma, mb = build(), build()
    ws = random_weights(ma)
    ma.set_weights(ws)
    mb.set_weights(ws)
    ma.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU])
    mb.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU], jit_compile=True)
    for i in range(5):   # two eager warm-up steps of the jit model, then three replayed ones
        x, y = batch(60 + i)
        la, lb = ma.train_on_batch(x, y), mb.train_on_batch(x, y)
        assert la == lb, (i, la, lb)
        for ga, gb in zip(ma.get_gradients(), mb.get_gradients()):
            assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), i
    assert len(mb._train_graphs) == 1 and isinstance(next(iter(mb._train_graphs.values())), GraphedTrainStep)
    for wa, wb in zip(ma.get_weights(), mb.get_weights()):
        assert np.array_equal(wa, wb)


def test_bf16_train_step_against_the_fp32_engine(engine):
    from building_detection_amd import mixed_precision as MP
    from building_detection_amd.losses import edge_focal_loss
    m32 = build()
    MP.set_global_policy("mixed_bfloat16")
    try:
        m16 = build()
    finally:
        MP.set_global_policy("float32")
    assert m16.compute_dtype == "bfloat16" and m32.compute_dtype == "float32"
    ws = random_weights(m32)
    m32.set_weights(ws)
    m16.set_weights(ws)
    x, y = batch(11)
    p32, p16 = m32.predict(x), m16.predict(x)
    dp_mean = float(np.abs(p16 - p32).mean())
    flip = float(((p16[..., 1] > p16[..., 0]) != (p32[..., 1] > p32[..., 0])).mean())
    for m in (m32, m16):
        m.compile(optimizer="adam", loss=edge_focal_loss)
    l32, l16 = m32.train_on_batch(x, y), m16.train_on_batch(x, y)
    rel = []
    for p_, a_, b_ in zip([q for q in m32.params if q.trainable], m32.get_gradients(), m16.get_gradients()):
        n2 = float(np.square(a_.astype(np.float64)).sum())
        if n2 > 0:
            rel.append((p_.name, float(np.sqrt(np.square(b_.astype(np.float64) - a_).sum() / n2))))
    print(f"bf16 resizing graph: mean|dp| {dp_mean:.2e}, argmax flips {flip:.2e}, loss fp32 {l32['loss']:.5f} bf16 {l16['loss']:.5f}, "
          f"gradient rel-L2 {rel}")
    assert dp_mean <= B16.MAX_DP_MEAN and flip <= B16.MAX_FLIP
    assert abs(l16["loss"] - l32["loss"]) <= 3e-2 * abs(l32["loss"])
    assert all(r <= 0.1 for _, r in rel[-2:]), rel
