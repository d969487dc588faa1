"""The optimizers at model level: a small layers.py model (Conv2D, BatchNormalization, SeparableConv2D, softmax head) on
2 x 16 x 16 x 3 inputs, four steps.

The float64 reference (tests/_optim_ref.py) is fed the engine's OWN per-step gradients, read back from the gradient arena after
every step: this tests the optimizer, not the convolutions.  Each fp32 step rounds the weight and its update to 2^-24 relative, so
four steps stay far inside the 2e-5 * max|ref| that the kernel tests (and test_adam) use; the same bound is asserted here."""
import os
import sys

import numpy as np
import pytest
import torch

import _optim_ref as R
from _guarded import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_F32 = 2e-5
LRS = (1e-3, 2e-3, 5e-4, 1.5e-3)      # the scheduler: another learning rate at every step
F = lambda v: float(torch.tensor(v, dtype=torch.float32))


def _model(optimizer, jit_compile=False):
    from building_detection_amd import layers as L
    from building_detection_amd.losses import edge_focal_loss, PA
    from building_detection_amd.runtime import Model
    inp = L.Input(shape=(16, 16, 3))
    x = L.Conv2D(8, 3, padding="same")(inp)
    x = L.BatchNormalization()(x)
    x = L.SeparableConv2D(8, 3)(x)
    m = Model(inp, L.Conv2D(2, 1, activation="softmax")(x))
    m.compile(optimizer=optimizer, loss=edge_focal_loss, metrics=[PA], jit_compile=jit_compile)
    return m


def _batch(i):
    from building_detection_amd.data import synthetic_batch
    return synthetic_batch(2, 16, 16, seed=70 + i)


def _train(m, steps=4, schedule=True, grads=None):
    for i in range(steps):
        if schedule:
            m.optimizer.lr = LRS[i]
        m.train_on_batch(*_batch(i))
        if grads is not None:
            grads.append(m._runtime().g_train.detach().cpu().clone())
    torch.cuda.synchronize()
    return m._runtime().w_train.detach().cpu().clone()


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_the_three_spellings_of_plain_adam_give_the_same_bits(engine):
    from building_detection_amd import optimizers as O, runtime
    ws = [_train(_model(opt), schedule=False) for opt in ("adam", runtime.Optimizer(), O.Adam())]
    assert torch.equal(_bits(ws[0]), _bits(ws[1])) and torch.equal(_bits(ws[0]), _bits(ws[2]))
    m = _model(O.Adam())
    _train(m, steps=1)
    assert m.optimizer._state is None, "a default Adam() allocates nothing of its own"


def _cases():
    from building_detection_amd import optimizers as O
    return {
        "adamw": (lambda: O.AdamW(), R.Cfg(weight_decay=0.004)),
        "adam_global_clip_ema": (lambda: O.Adam(global_clipnorm=0.05, use_ema=True),
                                 R.Cfg(clip="global", clip_c=0.05, ema_momentum=0.99)),
        "sgd_nesterov_clipnorm": (lambda: O.SGD(momentum=0.9, nesterov=True, clipnorm=0.02),
                                  R.Cfg(kind="sgd", momentum=0.9, nesterov=True, clip="norm", clip_c=0.02)),
    }


def _reference(m, cfg, w0, grads):
    from building_detection_amd import optimizers as O
    segs = [(p.offset, p.size, p.kind in O.DEFAULT_DECAY_KINDS) for p in m.trainable_weights]
    c = R.Cfg(cfg.kind, F(cfg.beta_1), F(cfg.beta_2), F(cfg.epsilon), cfg.amsgrad, F(cfg.momentum), cfg.nesterov,
              F(cfg.weight_decay), cfg.clip, F(cfg.clip_c), None if cfg.ema_momentum is None else F(cfg.ema_momentum), 1.0)
    w, st = w0.double(), R.new_state(c, w0)
    for t, g in enumerate(grads, 1):
        total, per = R.norms_ref(segs, g)
        print(f"  step {t}: |g| = {float(total.sqrt()):.4f}, per parameter {per.sqrt().min():.4f} .. {per.sqrt().max():.4f}")
        w, st = R.step_ref(c, segs, w, g, st, F(LRS[t - 1]), F(R.adam_lr_t(LRS[t - 1], cfg.beta_1, cfg.beta_2, t)))
    live = torch.zeros(w0.numel(), dtype=torch.bool)
    for o, n, _ in segs:
        live[o:o + n] = True
    return w, st, live


@pytest.mark.parametrize("case", ["adamw", "adam_global_clip_ema", "sgd_nesterov_clipnorm"])
def test_four_scheduled_steps_match_the_reference_and_the_captured_step(engine, case):
    make, cfg = _cases()[case]
    m = _model(make())
    w0 = m._runtime().w_train.detach().cpu().clone()
    grads = []
    w = _train(m, grads=grads)
    ref, st, live = _reference(m, cfg, w0, grads)
    assert not torch.equal(w, w0)
    e = close(w[live], ref[live], TOL_F32, f"{case}: weights after four steps")
    print(f"{case}: weights max err {e:.3e}")
    ema = None
    if cfg.ema_momentum is not None:
        ema = m.optimizer._state[1].ema.detach().cpu().clone()
        close(ema[live], st["ema"][live], TOL_F32, f"{case}: weight average")
        assert not torch.equal(ema, w)
    # the captured step: two eager steps, then the graph is recorded and replayed twice - same kernels, same bits
    j = _model(make(), jit_compile=True)
    wj = _train(j)
    assert len(j._train_graphs) == 1, "the third and fourth step were replays"
    assert torch.equal(_bits(w), _bits(wj)), f"{case}: the captured step differs from the eager one"
    if ema is not None:
        assert torch.equal(_bits(ema), _bits(j.optimizer._state[1].ema.detach().cpu()))


def test_ema_weights_context_and_finalize(engine):
    from building_detection_amd import optimizers as O
    m = _model(O.Adam(global_clipnorm=0.05, use_ema=True))
    w0 = m._runtime().w_train.detach().cpu().clone()
    grads = []
    w = _train(m, grads=grads)
    _, st, live = _reference(m, _cases()["adam_global_clip_ema"][1], w0, grads)
    x, y = _batch(9)
    p_train = m.predict(x)
    # a model loaded with the REFERENCE's average (its frozen statistics are the trained model's)
    other = _model("adam")
    ort = other._runtime()
    avg = torch.where(live, st["ema"].float(), torch.zeros(1))
    ort.w_train.copy_(avg)
    ort.w_frozen.copy_(m._runtime().w_frozen)
    ort.weights_changed()
    p_ref = other.predict(x)
    with m.ema_weights():
        p_ema = m.predict(x)
        logs = m.test_on_batch(x, y)
        inside = m._runtime().w_train.detach().cpu().clone()
    assert np.isfinite(logs["loss"])
    assert not np.array_equal(p_ema, p_train), "the average is not the training weights after four steps"
    err = float(np.abs(p_ema - p_ref).max())
    print(f"predict under ema_weights() against the reference's average: max err {err:.3e}")
    # The two weight sets agree to 2e-5 * max|w| (asserted below).  Four layers, each linear in its weights, move logits of order
    # one by at most about 4 * 2e-5 of their size, and softmax is 1/4-Lipschitz: 1e-4 on a probability covers it.
    assert err <= 1e-4, err
    close(inside[live], st["ema"][live], TOL_F32, "weights inside ema_weights()")
    after = m._runtime().w_train.detach().cpu()
    assert torch.equal(_bits(after), _bits(w)), "ema_weights() did not restore the training weights to the bit"
    assert np.array_equal(m.predict(x), p_train)
    m.optimizer.finalize_variable_values(m)
    st_ema = m.optimizer._state[1].ema.detach().cpu()
    assert torch.equal(_bits(m._runtime().w_train.detach().cpu()), _bits(st_ema)), "finalize_variable_values leaves w == avg"
    assert np.array_equal(m.predict(x), p_ema)
    with pytest.raises(ValueError):
        with _model(O.AdamW()).ema_weights():
            pass


def test_sgd_without_momentum_and_amsgrad_allocate_what_they_need(engine):
    from building_detection_amd import optimizers as O
    m = _model(O.SGD(learning_rate=0.05))
    w0 = m._runtime().w_train.detach().cpu().clone()
    grads = []
    w = _train(m, steps=2, schedule=False, grads=grads)
    st = m.optimizer._state[1]
    assert st.vhat is None and st.ema is None
    assert not m._runtime().adam_m.any() and not m._runtime().adam_v.any(), "plain SGD reads and writes no moment arena"
    live = torch.zeros(w0.numel(), dtype=torch.bool)
    for p in m.trainable_weights:
        live[p.offset:p.offset + p.size] = True
    ref = w0.double() - F(0.05) * (grads[0].double() + grads[1].double())
    close(w[live], ref[live], TOL_F32, "two plain SGD steps")
    a = _model(O.Adam(amsgrad=True))
    _train(a, steps=2)
    sa = a.optimizer._state[1]
    assert sa.vhat is not None and sa.ema is None
    v = a._runtime().adam_v.detach().cpu()
    assert (sa.vhat.detach().cpu()[live] >= v[live]).all() and sa.vhat.any()


# ------------------------------------------------------------------------------------------------ data parallel, world size 1
def _dp_worker(port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from building_detection_amd import optimizers as O
    from building_detection_amd.dist import DataParallel
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        make = lambda: O.AdamW(global_clipnorm=0.05, use_ema=True)
        m = _model(make())
        w0 = m.get_weights()
        dp = DataParallel(m, bucket_mb=8.0, comm="sg")
        before = m._runtime().w_train.clone()
        m.train_on_batch(*_batch(0))
        mrt = m._runtime()
        gsum = mrt.g_train.clone()
        # the step itself: the optimizer on the MEAN gradient == a single process's optimizer fed the summed gradient and 1 / world
        chk = _model(make())
        chk.set_weights(w0)
        crt = chk._runtime()
        crt.g_train.copy_(gsum)
        chk.optimizer.iterations = 1
        chk.optimizer.apply(crt, crt.eng, 1.0 / dp.world)
        torch.cuda.synchronize()
        werr = float((crt.w_train - mrt.w_train).abs().max())
        eerr = float((chk.optimizer._state[1].ema - m.optimizer._state[1].ema).abs().max())
        q.put(dict(werr=werr, eerr=eerr, world=dp.world, moved=not torch.equal(before, mrt.w_train)))
    finally:
        dist.destroy_process_group()


def test_data_parallel_step_world1(engine):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_worker, args=(35500 + os.getpid() % 2000, q))
    p.start()
    try:
        r = q.get(timeout=120)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.terminate()
    assert p.exitcode == 0, p.exitcode
    assert r["world"] == 1 and r["moved"], r
    assert r["werr"] < 1e-7 and r["eerr"] < 1e-7, r      # tests/test_dist_gpu.py's bound on the plain Adam step
