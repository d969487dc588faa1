"""Bilinear UpSampling2D through layers, runtime and the DeepLab builders on the GPU.

Layer level: Input -> UpSampling2D(2, 'bilinear') -> Conv2D 3x3 'same' against a float64 torch graph of the same three nodes
(and against the nearest model of the same weights: the up-sampling must NOT be folded into the convolution's sub-pixel kernels,
which sum nearest taps).  Model level: both DeepLab builders with upsampling="bilinear" against the CPU oracle's graphs, whose
`oracle.tfops.upsample_nearest` is replaced for the test by a bilinear function (the oracle resolves it through the module at call
time; the SK block's 1x1 broadcast is the same tensor under both modes) - with the bars of tests/test_models_gpu.py's
test_inference_parity and test_train_step_parity unchanged.  Then the hipGraph replays and the bf16 policy (the bounds of
tests/test_bf16_gpu.py's test_model_bf16_against_fp32_engine)."""
import numpy as np
import pytest
import torch

import _fit_check as FC
import test_bf16_gpu as B16
from oracle import models as M
from oracle import tfops as T

pytestmark = pytest.mark.gpu

SIZE, KW = 64, {"aspp_pool": 4}


def bilinear(x, size):
    """tf.image.resize(method='bilinear') by an integer factor on NHWC: half-pixel centres = torch's align_corners=False."""
    y = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), size=(x.shape[1] * size, x.shape[2] * size), mode="bilinear",
                                        align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous()


@pytest.fixture
def bilinear_oracle(monkeypatch):
    monkeypatch.setattr(T, "upsample_nearest", bilinear)


def build(name, **kw):
    from building_detection_amd import zoo
    return zoo.BUILDERS[name]((SIZE, SIZE, 3), 2, upsampling="bilinear", **KW, **kw)


# ------------------------------------------------------------------------------------------------ layer level
def _three_nodes(interpolation, cin=8, cout=4, hw=6):
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model
    inp = L.Input(shape=(hw, hw, cin))
    y = L.Conv2D(cout, 3, padding="same")(L.UpSampling2D(size=2, interpolation=interpolation)(inp))
    return Model(inputs=inp, outputs=y)


def test_three_node_model_against_float64_and_not_fused(engine):
    from building_detection_amd import layers as L
    bil, near = _three_nodes("bilinear"), _three_nodes("nearest")
    rng = np.random.default_rng(7)
    ws = [rng.normal(0, 0.3, p.shape).astype(np.float32) for p in bil.params]
    bil.set_weights(ws)
    near.set_weights(ws)
    up_b = next(n for n in bil.nodes if isinstance(n, L._UpNode))
    up_n = next(n for n in near.nodes if isinstance(n, L._UpNode))
    assert up_b.fused_into is None and up_n.fused_into is not None
    x = rng.uniform(-1, 1, (2, 6, 6, 8)).astype(np.float32)
    dy = rng.uniform(-1, 1, (2, 12, 12, 4)).astype(np.float32)

    kernel, bias = (torch.from_numpy(w).double().requires_grad_() for w in ws)
    ref = T.conv2d(bilinear(torch.from_numpy(x).double(), 2), kernel, bias, 1, 1, "same")
    ref.backward(torch.from_numpy(dy).double())
    k32, b32 = (torch.from_numpy(w).requires_grad_() for w in ws)
    T.conv2d(bilinear(torch.from_numpy(x), 2), k32, b32, 1, 1, "same").backward(torch.from_numpy(dy))

    got = bil.predict(x)
    scale = float(ref.detach().abs().max())
    err = float(np.abs(got - ref.detach().numpy()).max())
    print(f"three nodes: max|y - fp64| = {err:.3e} (bound {2e-5 * scale:.3e})")
    assert err <= 2e-5 * scale
    rt = bil._runtime()
    with rt.eng.lock:
        rt.forward(rt.to_device(x), training=True)
        rt.backward(rt.to_device(dy))
        rt.release()
    grads = [g.astype(np.float64) for g in bil.get_gradients()]
    FC.compare_gradients("three nodes", [p.name for p in bil.params if p.trainable], grads,
                         [k32.grad.double().numpy(), b32.grad.double().numpy()], [kernel.grad.numpy(), bias.grad.numpy()])
    # the nearest model of the same weights computes something else: the bilinear pair did not take its fused kernels
    other = near.predict(x)
    assert float(np.abs(other - got).max()) > 1e-2 * scale


# ------------------------------------------------------------------------------------------------ model level
@pytest.mark.parametrize("name", ["v3plus", "bam"])
def test_bilinear_inference_parity(engine, bilinear_oracle, name):
    """test_models_gpu.py::test_inference_parity for the bilinear builders: the same bars."""
    from building_detection_amd.data import synthetic_batch
    model = build(name)
    x, _ = synthetic_batch(2, SIZE, SIZE, seed=11)
    ws = model.get_weights()
    rng = np.random.default_rng(5)
    for i, p in enumerate(model.params):
        if p.kind == "moving_mean":
            ws[i] = rng.normal(0, 0.1, p.shape).astype(np.float32)
        elif p.kind == "moving_var":
            ws[i] = rng.uniform(0.5, 1.5, p.shape).astype(np.float32)
        elif p.kind in ("bias", "beta"):
            ws[i] = rng.normal(0, 0.05, p.shape).astype(np.float32)
    model.set_weights(ws)
    pg = model.predict(x)
    assert pg.dtype == np.float32 and pg.shape == (2, SIZE, SIZE, 2)
    np.testing.assert_allclose(pg.sum(-1), 1.0, atol=1e-5)

    def infer(dtype):
        P = M.Params(weights=ws, dtype=dtype)
        with torch.no_grad():
            return M.BUILDERS[name](P, torch.from_numpy(x).to(dtype), training=False, **KW).double().numpy()

    p32, p64 = infer(torch.float32), infer(torch.float64)
    err_gpu32, err_gpu64, err_cpu64 = (float(np.abs(a - b).max()) for a, b in ((pg, p32), (pg, p64), (p32, p64)))
    print(f"{name} bilinear: |gpu-cpu32|={err_gpu32:.2e} |gpu-fp64|={err_gpu64:.2e} |cpu32-fp64|={err_cpu64:.2e}")
    assert err_gpu32 <= 1e-3, f"{name}: north_star bar: max |p_gpu - p_cpu| = {err_gpu32:.3e} > 1e-3"
    assert err_gpu64 <= 4 * err_cpu64 + 1e-4, f"{name}: gpu fp32 error {err_gpu64:.3e} vs cpu fp32 error {err_cpu64:.3e}"
    TIE = max(1e-6, 2 * err_cpu64)
    mg, mc = pg[..., 1] > pg[..., 0], p64[..., 1] > p64[..., 0]
    strict = np.abs(p64[..., 1] - p64[..., 0]) > TIE
    bad, excused = int((mg != mc)[strict].sum()), int((mg != mc)[~strict].sum())
    print(f"{name} bilinear: argmax masks: {int((~strict).sum())} of {strict.size} pixels inside the tie margin {TIE:.1e}, "
          f"{excused} of them differ; outside the margin {bad} differ")
    assert bad == 0, f"{name}: {bad} mask pixels differ where the oracle's margin exceeds {TIE:.1e}"
    # the patched oracle is a bilinear one: the nearest builder's probabilities are somewhere else
    from building_detection_amd import zoo
    near = zoo.BUILDERS[name]((SIZE, SIZE, 3), 2, **KW)
    near.set_weights(ws)
    assert float(np.abs(near.predict(x) - p64).max()) > 10 * max(err_gpu64, 1e-4)


@pytest.mark.parametrize("name", ["v3plus", "bam"])
def test_bilinear_train_step_parity(engine, bilinear_oracle, name):
    """test_models_gpu.py::test_train_step_parity for the bilinear builders: loss and whole-model gradients, the same bars."""
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.losses import edge_focal_loss, PA, IoU, MIoU, F1_score
    model = build(name)
    x, y = synthetic_batch(2, SIZE, SIZE, seed=23)
    ws0 = model.get_weights()
    model.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU, MIoU, F1_score])
    model.optimizer.lr = 1e-3
    logs = model.train_on_batch(x, y)
    grads_g = [g.astype(np.float64) for g in model.get_gradients()]
    ws1 = model.get_weights()

    def train(dtype):
        P = M.Params(weights=ws0, dtype=dtype)
        p = M.BUILDERS[name](P, torch.from_numpy(x).to(dtype), training=True, **KW)
        loss = M.loss_fn("edge_focal_loss", torch.from_numpy(y).to(dtype), p)
        loss.backward()
        return P, loss.item(), [t.grad.double().numpy() for t in P.trainable_tensors()]

    P32, loss32, g32 = train(torch.float32)
    _, loss64, g64 = train(torch.float64)
    print(f"{name} bilinear: loss gpu {logs['loss']:.7f} cpu32 {loss32:.7f} fp64 {loss64:.7f}")
    assert abs(logs["loss"] - loss64) <= 5 * abs(loss32 - loss64) + 1e-5 * abs(loss64), (logs["loss"], loss32, loss64)
    FC.compare_gradients(name + " bilinear", [p.name for p in model.params if p.trainable], grads_g, g32, g64)
    for i, p in enumerate(model.params):   # BN moving statistics after the training forward
        if not p.trainable:
            np.testing.assert_allclose(ws1[i], P32.tensors[i].detach().numpy(), rtol=1e-4, atol=1e-5, err_msg=p.name)


# ------------------------------------------------------------------------------------------------ replay
def test_bilinear_captured_train_step_and_predict_are_bit_identical_to_eager(engine):
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.losses import edge_focal_loss, PA, IoU
    from building_detection_amd.runtime import GraphedTrainStep
    ma, mb = build("v3plus"), build("v3plus")
    mb.set_weights(ma.get_weights())
    ma.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU])
    mb.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU], jit_compile=True)
    batches = [synthetic_batch(2, SIZE, SIZE, seed=60 + i) for i in range(5)]
    for i, (x, y) in enumerate(batches):   # two eager warm-up steps of the jit model, then three replayed ones
        la, lb = ma.train_on_batch(x, y), mb.train_on_batch(x, y)
        assert la == lb, (i, la, lb)
        for ga, gb in zip(ma.get_gradients(), mb.get_gradients()):
            assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), i
    assert len(mb._train_graphs) == 1 and isinstance(next(iter(mb._train_graphs.values())), GraphedTrainStep)
    for wa, wb in zip(ma.get_weights(), mb.get_weights()):
        assert np.array_equal(wa, wb)
    g = torch.Generator().manual_seed(9)
    x1 = (torch.rand(2, SIZE, SIZE, 3, generator=g) * 2 - 1).cuda()
    x2 = (torch.rand(2, SIZE, SIZE, 3, generator=g) * 2 - 1).cuda()
    e1, e2 = ma.predict_device(x1).clone(), ma.predict_device(x2).clone()
    gp = ma.capture_predict(2)
    assert torch.equal(gp(x1), e1) and torch.equal(gp(x2), e2) and torch.equal(gp(x1), e1)
    assert not torch.equal(e1, e2)
    assert np.array_equal(ma.predict(x1.cpu().numpy()), e1.cpu().numpy())


# ------------------------------------------------------------------------------------------------ bf16 policy
def test_bilinear_bf16_train_step_against_the_fp32_engine(engine):
    """One train step of the bilinear v3plus under mixed_bfloat16 against the fp32 engine: the bounds that
    test_bf16_gpu.py::test_model_bf16_against_fp32_engine holds the nearest model to (read from that module where it names them)."""
    from building_detection_amd import mixed_precision as MP
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.losses import edge_focal_loss, PA, IoU, MIoU, F1_score
    m32 = build("v3plus")
    MP.set_global_policy("mixed_bfloat16")
    try:
        m16 = build("v3plus")
    finally:
        MP.set_global_policy("float32")
    assert m16.compute_dtype == "bfloat16" and m32.compute_dtype == "float32"
    ws = m32.get_weights()
    rng = np.random.default_rng(5)
    for i, p in enumerate(m32.params):
        if p.kind == "moving_mean":
            ws[i] = rng.normal(0, 0.1, p.shape).astype(np.float32)
        elif p.kind == "moving_var":
            ws[i] = rng.uniform(0.5, 1.5, p.shape).astype(np.float32)
    m32.set_weights(ws)
    m16.set_weights(ws)
    x, y = synthetic_batch(2, SIZE, SIZE, seed=11)
    p32, p16 = m32.predict(x), m16.predict(x)
    dp_mean = float(np.abs(p16 - p32).mean())
    flip = float(((p16[..., 1] > p16[..., 0]) != (p32[..., 1] > p32[..., 0])).mean())
    for m in (m32, m16):
        m.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU, MIoU, F1_score])
    l32, l16 = m32.train_on_batch(x, y), m16.train_on_batch(x, y)
    tail = []
    for p_, a_, b_ in list(zip([q for q in m32.params if q.trainable], m32.get_gradients(), m16.get_gradients()))[-2:]:
        n2 = float(np.square(a_.astype(np.float64)).sum())
        if n2 > 0:
            tail.append((p_.name, float(np.sqrt(np.square(b_.astype(np.float64) - a_).sum() / n2))))
    print(f"bf16 bilinear v3plus: mean|dp| {dp_mean:.2e}, argmax flips {flip:.2e}, loss fp32 {l32['loss']:.5f} bf16 {l16['loss']:.5f}, "
          f"last-layer gradient rel-L2 {tail}")
    assert dp_mean <= B16.MAX_DP_MEAN and flip <= B16.MAX_FLIP
    assert abs(l16["loss"] - l32["loss"]) <= 3e-2 * abs(l32["loss"])
    assert all(r <= 0.1 for _, r in tail), tail
