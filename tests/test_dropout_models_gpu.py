"""Dropout / SpatialDropout2D through layers, runtime and the builders on the GPU, at the smallest shapes.

Layer level: Input -> Conv2D -> Dropout -> Conv2D against a float64 torch graph that multiplies by the mask of
tests/_dropout_ref.py (the numpy restatement of DESIGN 4.11), with the bars of
tests/test_bilinear_models_gpu.py::test_three_node_model_against_float64_and_not_fused.  Then what the layer promises: inference
does not know it, two nodes and two steps draw different masks, and a run is a function of (model.seed, rank, step) alone - the
captured step, the data-parallel step of world size 1 and a rebuilt model repeat the eager bits."""
import os
import sys

import numpy as np
import pytest
import torch

import _dropout_ref as R
import _fit_check as FC
from oracle import tfops as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1103   # Model's default seed = k0


def _mask(shape, rate, stream=0, step=0, k0=SEED, k1=0, spatial=False):
    """The kept / dropped decisions of an [N,H,W,C] activation as a bool tensor of that shape."""
    n = int(np.prod(shape))
    hwc, c = (int(np.prod(shape[1:])), shape[-1]) if spatial else (0, 0)
    kept = R.keep(R.mask_index(n, 0, hwc, c), k0, k1, stream, step, R.threshold(rate))
    return torch.from_numpy(kept).reshape(shape)


# ------------------------------------------------------------------------------------------------ layer level
def _three_nodes(layer):
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model
    inp = L.Input(shape=(6, 6, 8))
    y = L.Conv2D(8, 3, padding="same")(inp)
    if layer is not None:
        y = layer(y)
    return Model(inputs=inp, outputs=L.Conv2D(4, 3, padding="same")(y))


@pytest.mark.parametrize("spatial", [False, True], ids=["dropout", "spatial"])
def test_three_node_model_against_float64(engine, spatial):
    from building_detection_amd import layers as L
    m = _three_nodes(L.SpatialDropout2D(0.5) if spatial else L.Dropout(0.5))
    rng = np.random.default_rng(7)
    ws = [rng.normal(0, 0.3, p.shape).astype(np.float32) for p in m.params]
    m.set_weights(ws)
    x = rng.uniform(-1, 1, (2, 6, 6, 8)).astype(np.float32)
    dy = rng.uniform(-1, 1, (2, 6, 6, 4)).astype(np.float32)
    kept = _mask((2, 6, 6, 8), 0.5, spatial=spatial)
    assert 0.25 < kept.double().mean() < 0.75
    if spatial:
        assert (kept == kept[:, :1, :1]).all()

    def graph(dtype):
        k1, b1, k2, b2 = (torch.from_numpy(w).to(dtype).requires_grad_() for w in ws)
        h = T.conv2d(torch.from_numpy(x).to(dtype), k1, b1, 1, 1, "same")
        h = h * kept.to(dtype) * R.scale(0.5)
        y = T.conv2d(h, k2, b2, 1, 1, "same")
        y.backward(torch.from_numpy(dy).to(dtype))
        return y.detach(), [t.grad.double().numpy() for t in (k1, b1, k2, b2)]

    ref, g64 = graph(torch.float64)
    _, g32 = graph(torch.float32)
    rt = m._runtime()
    with rt.eng.lock:
        got = rt.forward(rt.to_device(x), training=True).cpu().numpy()   # a fresh runtime: the masks of step 0
        rt.backward(rt.to_device(dy))
        rt.release()
    scale = float(ref.abs().max())
    err = float(np.abs(got - ref.numpy()).max())
    print(f"three nodes ({'spatial' if spatial else 'element'}): max|y - fp64| = {err:.3e} (bound {2e-5 * scale:.3e})")
    assert err <= 2e-5 * scale
    grads = [g.astype(np.float64) for g in m.get_gradients()]
    FC.compare_gradients("three nodes", [p.name for p in m.params if p.trainable], grads, g32, g64)
    # the twin without the node computes something else: the mask was applied
    plain = _three_nodes(None)
    plain.set_weights(ws)
    assert float(np.abs(plain.predict(x) - got).max()) > 1e-2 * scale


# ------------------------------------------------------------------------------------------------ inference
def _head_model(layer):
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model
    inp = L.Input(shape=(8, 8, 8))
    y = L.Conv2D(8, 3, padding="same", activation="relu")(inp)
    if layer is not None:
        y = layer(y)
    return Model(inputs=inp, outputs=L.Conv2D(2, 1, activation="softmax")(y))


def _xy(n, hw, cin, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, hw, hw, cin)).astype(np.float32)
    lab = rng.integers(0, 2, (n, hw, hw))
    y = np.concatenate([np.eye(2, dtype=np.float32)[lab], rng.uniform(0.5, 2, (n, hw, hw, 2)).astype(np.float32)], -1)
    return x, y


def test_inference_does_not_know_the_node(engine):
    from building_detection_amd import layers as L
    from building_detection_amd.losses import edge_focal_loss, PA, IoU
    drop, plain = _head_model(L.Dropout(0.5)), _head_model(None)
    plain.set_weights(drop.get_weights())
    for m in (drop, plain):
        m.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU])
    x, y = _xy(2, 8, 8, 3)
    assert np.array_equal(drop.predict(x).view(np.uint32), plain.predict(x).view(np.uint32))
    assert drop.test_on_batch(x, y) == plain.test_on_batch(x, y)
    rt = drop._runtime()
    xd = rt.to_device(x)
    with rt.eng.lock:
        assert torch.equal(drop.predict_device(xd), plain.predict_device(xd))
        trained = rt.forward(xd, training=True).clone()
        rt.release()
    assert not torch.equal(trained, plain.predict_device(xd))   # ... and the training forward does
    assert plain._runtime().rng is None and rt.rng is not None   # only a model with a dropout node owns the seed words


def test_two_nodes_draw_different_masks(engine):
    """A dropout node as model output exposes its mask: Input -> Dropout -> Dropout keeps x * 2 * 2 where both nodes keep."""
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model
    inp = L.Input(shape=(6, 6, 8))
    m = Model(inputs=inp, outputs=L.Dropout(0.5)(L.Dropout(0.5)(inp)))
    x = torch.from_numpy(_xy(2, 6, 8, 5)[0])
    x = torch.where(x.abs() < 2.0 ** -7, torch.full_like(x, 0.5), x)
    a, b = _mask(x.shape, 0.5, stream=0), _mask(x.shape, 0.5, stream=1)
    assert 0.4 < (a == b).double().mean() < 0.6
    rt = m._runtime()
    with rt.eng.lock:
        got = rt.forward(rt.to_device(x.numpy()), training=True).cpu()
        rt.release()
    want = torch.where(a & b, x * 2 * 2, torch.zeros(()))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert np.array_equal(m.predict(x.numpy()), x.numpy())   # inference: the input itself


def test_two_steps_draw_different_masks(engine):
    """Input [1,4,4,16] -> SpatialDropout2D -> 1x1 softmax head: a dropped channel's row of the head's kernel gradient is exactly
    zero, a kept channel's is not, so the gradient shows which channels each train_on_batch step dropped."""
    from building_detection_amd import layers as L
    from building_detection_amd.losses import edge_focal_loss
    from building_detection_amd.runtime import Model
    inp = L.Input(shape=(4, 4, 16))
    m = Model(inputs=inp, outputs=L.Conv2D(2, 1, activation="softmax")(L.SpatialDropout2D(0.5)(inp)))
    m.compile(optimizer="adam", loss=edge_focal_loss)
    x, y = _xy(1, 4, 16, 9)
    x = np.where(np.abs(x) < 2.0 ** -7, 0.5, x).astype(np.float32)
    seen = []
    for step in range(2):
        m.train_on_batch(x, y)
        dropped = np.all(m.get_gradients()[0].reshape(16, 2) == 0, axis=1)
        want = ~_mask((1, 1, 1, 16), 0.5, step=step, spatial=True).numpy().reshape(16)
        assert np.array_equal(dropped, want), (step, dropped, want)
        seen.append(dropped)
    assert not np.array_equal(seen[0], seen[1]) and 0 < seen[0].sum() < 16


# ------------------------------------------------------------------------------------------------ the same bits on every path
SIZE = 64


def _v3plus(policy="float32", seed=SEED):
    from building_detection_amd import mixed_precision as MP
    from building_detection_amd import zoo
    from building_detection_amd.losses import edge_focal_loss, PA, IoU
    MP.set_global_policy(policy)
    try:
        m = zoo.Xception_DeepLabV3_Plus((SIZE, SIZE, 3), 2, aspp_pool=4, dropout=(0.5, 0.1))
    finally:
        MP.set_global_policy("float32")
    m.seed = seed
    return m


def _compiled(m, jit=False):
    from building_detection_amd.losses import edge_focal_loss, PA, IoU
    m.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU], jit_compile=jit)
    return m


def _steps(m, n=4):
    from building_detection_amd.data import synthetic_batch
    logs = [m.train_on_batch(*synthetic_batch(2, SIZE, SIZE, seed=80 + i)) for i in range(n)]
    return logs, m.get_weights()


def _same(wa, wb):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(wa, wb))


@pytest.mark.parametrize("policy", ["float32", "mixed_bfloat16"])
def test_captured_steps_repeat_the_eager_bits(engine, policy):
    """Four steps with jit_compile=True - two eager ones, the capture and its replay, one more replay - against four eager steps
    of a twin: the masks depend on (seed, rank, step, node, element) and on nothing the capture changes."""
    from building_detection_amd.runtime import GraphedTrainStep
    eager, jit = _v3plus(policy), _v3plus(policy)
    assert eager.compute_dtype == ("bfloat16" if policy != "float32" else "float32")
    jit.set_weights(eager.get_weights())
    la, wa = _steps(_compiled(eager))
    lb, wb = _steps(_compiled(jit, jit=True))
    assert len(jit._train_graphs) == 1 and isinstance(next(iter(jit._train_graphs.values())), GraphedTrainStep)
    assert la == lb, (la, lb)
    assert _same(wa, wb)
    assert eager.optimizer.iterations == jit.optimizer.iterations == 4


def test_a_rebuilt_model_repeats_the_run_and_another_seed_does_not(engine):
    first = _v3plus()
    w0 = first.get_weights()
    la, wa = _steps(_compiled(first), 2)
    again = _v3plus()
    again.set_weights(w0)
    lb, wb = _steps(_compiled(again), 2)
    assert la == lb and _same(wa, wb)
    other = _v3plus(seed=SEED + 1)      # other masks on the same initial weights
    other.set_weights(w0)
    lc, wc = _steps(_compiled(other), 2)
    assert la != lc and not _same(wa, wc)
    # ... and the dropout really acted: the twin without the nodes, same weights, ends elsewhere
    from building_detection_amd import zoo
    plain = zoo.Xception_DeepLabV3_Plus((SIZE, SIZE, 3), 2, aspp_pool=4)
    plain.set_weights(w0)
    ld, wd = _steps(_compiled(plain), 2)
    assert la != ld and not _same(wa, wd)


def _dp_worker(port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    from building_detection_amd.dist import DataParallel
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        single = _v3plus()
        w0 = single.get_weights()
        la, wa = _steps(_compiled(single))
        par = _v3plus()
        par.set_weights(w0)
        _compiled(par, jit=True)
        dp = DataParallel(par, bucket_mb=8.0, comm="sg")
        lb, wb = _steps(par)
        torch.cuda.synchronize()
        q.put(dict(world=dp.world, rank=dp.rank, same=_same(wa, wb), loss_a=[l["loss"] for l in la], loss_b=[l["loss"] for l in lb],
                   graphs=len(par._train_graphs), k1=int(par._runtime().rng[1].item())))
    finally:
        dist.destroy_process_group()


def test_data_parallel_world1_repeats_the_single_process_bits(engine):
    """tests/test_optimizers_gpu.py::test_data_parallel_step_world1's pattern: rank 0 of a world of one draws the single process's
    masks (k1 = 0), through the segmented capture of the data-parallel step."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_worker, args=(37500 + os.getpid() % 2000, q))
    p.start()
    try:
        r = q.get(timeout=180)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.terminate()
    assert p.exitcode == 0, p.exitcode
    assert r["world"] == 1 and r["rank"] == 0 and r["k1"] == 0 and r["graphs"] == 1, r
    assert r["loss_a"] == r["loss_b"] and r["same"], r
