"""GroupNormalization through layers, fusion, runtime, weights_io and the builders on the GPU, at the smallest shapes.

The small net Input(16,16,3) -> Conv2D(12, 3, same) -> GroupNormalization(3) -> ReLU -> Conv2D(2, 1) -> Softmax is held to the same
net in torch float64 (tests/_groupnorm_ref.py's formulas under autograd): predict within 2e-5 of max|p|, the loss of one plain-SGD
step within 1e-5 relative (the fit-loop test's bound against fp64), every weight's change divided by -lr within 1e-4 of the float64
gradient's largest entry; with bf16 storage all three at 2^-7.  Then what the layer promises: the captured step repeats the eager
bits, an image's prediction does not depend on its batch, weights survive a file, AdamW leaves gamma / beta undecayed."""
import os

import numpy as np
import pytest
import torch

import _groupnorm_ref as R
from oracle import models as M
from oracle import tfops as T

pytestmark = pytest.mark.gpu
LR = 0.5      # plain SGD: w' = w - LR g; a weight of size 1 is stored to 2^-24, so g comes back to 2^-23 / LR


def _small(dtype=None, groups=3):
    from building_detection_amd import layers as L
    from building_detection_amd.graph import reset_names
    from building_detection_amd.runtime import Model
    reset_names()
    inp = L.Input(shape=(16, 16, 3))
    y = L.Conv2D(12, 3, padding="same")(inp)
    y = L.ReLU()(L.GroupNormalization(groups)(y))
    if dtype is None or dtype == "float32":
        out = L.Softmax()(L.Conv2D(2, 1)(y))
    else:   # bf16 storage keeps the head's logits in fp32 only where the convolution owns the softmax (the builders' spelling)
        out = L.Conv2D(2, 1, activation="softmax")(y)
    return Model(inputs=inp, outputs=out, dtype=dtype)


def _batch(n=2, size=16, seed=31):
    from building_detection_amd.data import synthetic_batch
    return synthetic_batch(n, size, size, seed=seed)


def _weights(m, seed=11):
    rng = np.random.default_rng(seed)
    ws = []
    for p in m.params:
        if p.kind == "gamma":
            ws.append(rng.uniform(0.5, 1.5, p.shape).astype(np.float32) * np.where(np.arange(p.shape[0]) % 3 == 1, -1, 1).astype(np.float32))
        elif p.kind in ("beta", "bias"):
            ws.append(rng.uniform(-0.3, 0.3, p.shape).astype(np.float32))
        else:
            ws.append(rng.normal(0, 0.4, p.shape).astype(np.float32))
    return ws


def _float64_net(ws, x, y, groups=3):
    """-> probabilities, loss, gradients of (kernel, bias, gamma, beta, kernel, bias), all float64"""
    k1, b1, gamma, beta, k2, b2 = (torch.from_numpy(w).double().requires_grad_() for w in ws)
    h = T.conv2d(torch.from_numpy(x).double(), k1, b1, 1, 1, "same")
    n, hh, ww, c = h.shape
    h = R.fwd(h.reshape(n, hh * ww, c), gamma, beta, groups, 1e-3, relu=True)[0].reshape(n, hh, ww, c)
    p = T.softmax(T.conv2d(h, k2, b2, 1, 1, "same"))
    loss = M.loss_fn("edge_focal_loss", torch.from_numpy(y).double(), p)
    loss.backward()
    return p.detach().numpy(), float(loss.detach()), [t.grad.numpy() for t in (k1, b1, gamma, beta, k2, b2)]


def _bits_equal(wa, wb):
    return all(np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)) for a, b in zip(wa, wb))


@pytest.mark.parametrize("dtype,bound_p,bound_l,bound_g", [("float32", 2e-5, 1e-5, 1e-4), ("mixed_bfloat16", 2.0 ** -7, 2.0 ** -7, 2.0 ** -7)],
                         ids=["float32", "bf16"])
def test_small_net_against_float64(engine, dtype, bound_p, bound_l, bound_g):
    from building_detection_amd import layers as L, optimizers as O
    from building_detection_amd.losses import edge_focal_loss
    m = _small(dtype)
    act = next(n for n in m.nodes if isinstance(n, L._ActNode) and n.act == "relu")
    gn = next(n for n in m.nodes if isinstance(n, L._GNNode))
    assert act.fused_away and gn.relu
    assert [p.kind for p in m.params] == ["kernel", "bias", "gamma", "beta", "kernel", "bias"]
    ws = _weights(m)
    m.set_weights(ws)
    x, y = _batch()
    p64, l64, g64 = _float64_net(ws, x, y)
    p = m.predict(x)
    err, scale = float(np.abs(p - p64).max()), float(np.abs(p64).max())
    print(f"{dtype}: predict max|p - fp64| = {err:.3e} (bound {bound_p * scale:.3e})")
    assert err <= bound_p * scale
    m.compile(optimizer=O.SGD(learning_rate=LR), loss=edge_focal_loss)
    loss = m.train_on_batch(x, y)["loss"]
    print(f"{dtype}: loss {loss:.8f} fp64 {l64:.8f} rel {abs(loss - l64) / abs(l64):.2e} (bound {bound_l:.1e})")
    assert abs(loss - l64) <= bound_l * abs(l64)
    worst = []
    for spec, w0, w1, g in zip(m.params, ws, m.get_weights(), g64):
        got = (w1.astype(np.float64) - w0.astype(np.float64)) / -LR
        e, s = float(np.abs(got - g).max()), float(np.abs(g).max())
        print(f"{dtype}: {spec.name}: max|dw / -lr - fp64 gradient| = {e:.3e}, largest entry {s:.3e}, rel {e / s:.2e} (bound {bound_g:.1e})")
        worst.append((e <= bound_g * s, spec.name, e, s))
    assert all(ok for ok, *_ in worst), [w for w in worst if not w[0]]


def _steps(m, n, jit, size=16, batch=2):
    from building_detection_amd.losses import edge_focal_loss, PA
    m.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA], jit_compile=jit)
    logs = [m.train_on_batch(*_batch(batch, size, seed=50 + i)) for i in range(n)]
    return logs, m.get_weights()


def test_captured_step_repeats_the_eager_bits(engine):
    eager, jit = _small(), _small()
    ws = _weights(eager)
    eager.set_weights(ws)
    jit.set_weights(ws)
    la, wa = _steps(eager, 3, False)
    lb, wb = _steps(jit, 3, True)
    assert len(jit._train_graphs) == 1      # the third step was a replay
    assert la == lb and _bits_equal(wa, wb)
    assert not _bits_equal(wa, ws)


def _hrnet():
    from building_detection_amd import zoo
    from building_detection_amd.graph import reset_names
    reset_names()
    return zoo.HRNet((64, 64, 3), norm="group"), 64


def _v3plus():
    from building_detection_amd import zoo
    from building_detection_amd.graph import reset_names
    reset_names()
    return zoo.Xception_DeepLabV3_Plus((128, 128, 3), aspp_pool=8, norm="group"), 128


@pytest.mark.parametrize("make", [_hrnet, _v3plus], ids=["hrnet", "v3plus"])
def test_builders_with_group_normalisation(engine, make, tmp_path):
    from building_detection_amd import layers as L
    eager, size = make()
    assert any(isinstance(n, L._GNNode) for n in eager.nodes) and not any(isinstance(n, L._BNNode) for n in eager.nodes)
    jit, _ = make()
    w0 = eager.get_weights()
    jit.set_weights(w0)
    # an image's prediction does not depend on the batch it is in (with BatchNormalization in training mode it would)
    x = _batch(3, size, seed=77)[0]
    p3 = eager.predict(x)
    for i in range(3):
        assert np.array_equal(eager.predict(x[i:i + 1])[0].view(np.uint32), p3[i].view(np.uint32)), i
    # eager and captured steps from equal weights
    la, wa = _steps(eager, 3, False, size)
    lb, wb = _steps(jit, 3, True, size)
    assert len(jit._train_graphs) == 1
    assert all(np.isfinite(l["loss"]) for l in la) and la == lb and _bits_equal(wa, wb)
    # through a Keras-layout file into a fresh model
    path = os.path.join(tmp_path, "gn.h5")
    eager.save_weights(path)
    fresh, _ = make()
    assert not _bits_equal(fresh.get_weights(), wa)
    fresh.load_weights(path)
    assert _bits_equal(fresh.get_weights(), wa)
    assert np.array_equal(fresh.predict(x).view(np.uint32), eager.predict(x).view(np.uint32))
    names = [n.name for n in eager.nodes if isinstance(n, L._GNNode)]
    assert names[:2] == ["group_normalization", "group_normalization_1"]


def test_adamw_leaves_gamma_and_beta_undecayed(engine):
    """One step of AdamW (default options) and of Adam from equal weights see the same gradients; the decoupled decay then moves
    the kernels only."""
    from building_detection_amd import optimizers as O
    from building_detection_amd.losses import edge_focal_loss
    out = []
    for opt in (O.AdamW(), O.Adam()):
        m = _small()
        m.set_weights(_weights(m))
        m.compile(optimizer=opt, loss=edge_focal_loss)
        m.train_on_batch(*_batch())
        out.append((m.params, m.get_weights()))
    (params, wa), (_, wb) = out
    for p, a, b in zip(params, wa, wb):
        same = np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert same == (p.kind in ("gamma", "beta", "bias")), (p.name, p.kind, same)
