"""Shared pieces of the training-loop checks (tests/test_models_gpu.py, tests/test_fit_check_cpu.py, scripts/fit_envelope_cpu.py).

A training loop is followed as a TRAJECTORY: one `Step` per optimisation step with the complete state before it (every weight,
BatchNorm moving statistics included, Adam's moments, the step counter, the learning rate), the loss and the gradients of the
step, and the complete state after it.  The engine's trajectory is taken by `recorder(model)` (a callback for fit_generator);
`oracle_trajectory` makes one from the fp32 CPU oracle, optionally with an error planted, so the checker itself can be tested
without a GPU.

`check_trajectory` judges every step FROM THE STATE THE STEP STARTED IN: free-running fp32 trajectories of this net leave the fp64
one by several per cent of the loss within three steps whatever the implementation (`loss_envelope` measures that), while one
step from a common state is as tight as the first (loss 6e-6, moving statistics 3e-6: LAB_NOTEBOOK 14).  The bounds are those of
test_train_step_parity (loss, gradients, moving statistics, Adam's weights) and of test_ops_gpu.py::test_adam (moments).
"""
import contextlib
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from oracle import models as M
from oracle import tfops as T

B1, B2, EPS = 0.9, 0.999, 1e-7
RTOL_MOMENTS = 2e-5    # tests/test_ops_gpu.py RTOL, the bound of test_adam
ATOL_WEIGHTS = 2e-6    # test_train_step_parity's Adam block (same base rate 1e-3)
SCHEDULE = dict(learning_rate_base=1e-3, total_steps=40, warmup_learning_rate=1e-5, warmup_steps=2)


def schedule_lr(s: int) -> float:
    """The rate WarmUpCosineDecayScheduler(**SCHEDULE) sets before step s (its global_step is 0 at the first batch)."""
    return float(M.cosine_decay_with_warmup(s, SCHEDULE["learning_rate_base"], SCHEDULE["total_steps"],
                                            warmup_learning_rate=SCHEDULE["warmup_learning_rate"],
                                            warmup_steps=SCHEDULE["warmup_steps"]))


@dataclass
class State:
    weights: List[np.ndarray]            # every parameter in creation order (model.params / Params.tensors), fp32
    m: List[np.ndarray]                  # Adam's first moments, trainable parameters in order
    v: List[np.ndarray]                  # second moments
    iterations: int
    lr: float
    pad: Dict[str, np.ndarray] = field(default_factory=dict)   # arena elements that belong to no parameter (engine only)


@dataclass
class Step:
    pre: State
    post: State
    loss: float
    grads: List[np.ndarray]              # trainable parameters in order


# ---- recording the engine ---------------------------------------------------------------------------------------------------------
def _slices(arena, specs):
    host = arena.detach().cpu().numpy()   # ONE device read per arena; parameters are cut out on the host
    out = [host[p.offset:p.offset + p.size].reshape(p.shape).copy() for p in specs]
    used = np.zeros(host.shape[0], bool)
    for p in specs:
        used[p.offset:p.offset + p.size] = True
    return out, host[~used].copy()        # the rest: alignment gaps between parameters and the tail beyond the last one


def engine_state(model) -> State:
    rt = model._runtime()
    train = [p for p in model.params if p.trainable]
    frozen = [p for p in model.params if not p.trainable]
    wt, pad_w = _slices(rt.w_train, train)
    wf, _ = _slices(rt.w_frozen, frozen)
    m, pad_m = _slices(rt.adam_m, train)
    v, pad_v = _slices(rt.adam_v, train)
    it_t, it_f = iter(wt), iter(wf)
    weights = [next(it_t) if p.trainable else next(it_f) for p in model.params]
    return State(weights, m, v, int(model.optimizer.iterations), float(model.optimizer.lr),
                 {"w": pad_w, "m": pad_m, "v": pad_v})


def recorder(model):
    """A callback that records the trajectory of fit_generator into `.steps`.  Place it AFTER the learning-rate scheduler in the
    callback list: on_batch_begin then sees the rate the scheduler has just set for this step."""
    from building_detection_amd.callbacks import Callback

    class Recorder(Callback):
        def __init__(self):
            super().__init__()
            self.steps: List[Step] = []
            self._pre = None

        def on_batch_begin(self, batch, logs=None):
            self._pre = engine_state(model)

        def on_batch_end(self, batch, logs=None):
            # a captured step replays its backward into the same gradient arena the eager step writes (GraphedTrainStep.run
            # hands rt.g_train to run_segments), so get_gradients() is the step's own gradient in both modes
            grads = [g.astype(np.float64) for g in model.get_gradients()]
            self.steps.append(Step(self._pre, engine_state(model), float(logs["loss"]), grads))

    return Recorder()


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def oracle_step(weights, x, y, dtype):
    """HRNet forward (training mode) + edge_focal_loss + backward from `weights`: loss, gradients (fp64 numpy), the Params
    afterwards (its moving statistics are those after the step)."""
    P = M.Params(weights=weights, dtype=dtype)
    p = M.hrnet(P, torch.from_numpy(x).to(dtype), training=True)
    loss = M.loss_fn("edge_focal_loss", torch.from_numpy(y).to(dtype), p)
    loss.backward()
    return loss.item(), [t.grad.double().numpy() for t in P.trainable_tensors()], P


def oracle_initial_weights(size=32, seed=1103):
    P = M.Params(seed=seed, dtype=torch.float32)
    with torch.no_grad():
        M.hrnet(P, torch.zeros(1, size, size, 3), training=False)
    return P.numpy_weights(), list(P.trainable), list(P.kinds)


FAULTS = ("step_counter", "bias_correction_one_step_ahead", "lr_one_step_late", "lr_one_step_late_unreported",
          "moving_statistics_swapped", "first_moment_not_carried")


def swappable_bn_pair(weights, kinds):
    """Two BatchNorm layers of the same width (indices of their moving_mean; moving_var follows at + 1)."""
    idx = [i for i, k in enumerate(kinds) if k == "moving_mean"]
    for a in idx:
        for b in idx:
            if b > a and weights[a].shape == weights[b].shape:
                return a, b
    raise AssertionError("no two BatchNorm layers of one width")


def oracle_trajectory(ws0, batches, fault: Optional[str] = None) -> List[Step]:
    """The fp32 oracle driven like the engine (Keras-2 Adam, the rates of SCHEDULE), recorded like the engine.  `fault` plants
    one of FAULTS into this host arithmetic - what a broken engine would hand to the recorder."""
    assert fault is None or fault in FAULTS, fault
    dtype = torch.float32
    ws = [np.asarray(w, np.float32) for w in ws0]
    m = v = None
    iterations = 1 if fault == "step_counter" else 0
    steps = []
    for s, (x, y) in enumerate(batches):
        lr_used = schedule_lr(max(s - 1, 0) if fault in ("lr_one_step_late", "lr_one_step_late_unreported") else s)
        lr_seen = schedule_lr(s) if fault == "lr_one_step_late_unreported" else lr_used
        loss, grads, P = oracle_step(ws, x, y, dtype)
        tr = P.trainable_tensors()
        if m is None:
            m, v = [torch.zeros_like(t) for t in tr], [torch.zeros_like(t) for t in tr]
        pre = State([w.copy() for w in ws], [t.numpy().copy() for t in m], [t.numpy().copy() for t in v], iterations, lr_seen)
        if fault == "first_moment_not_carried":
            for t in m:
                t.zero_()
        iterations += 1
        M.adam_step(tr, [t.grad for t in tr], m, v, iterations + (fault == "bias_correction_one_step_ahead"), lr_used)
        ws = P.numpy_weights()
        if fault == "moving_statistics_swapped":
            a, b = swappable_bn_pair(ws, P.kinds)
            for k in (0, 1):
                ws[a + k], ws[b + k] = ws[b + k], ws[a + k]
        post = State([w.copy() for w in ws], [t.numpy().copy() for t in m], [t.numpy().copy() for t in v], iterations, lr_seen)
        steps.append(Step(pre, post, loss, grads))
    return steps


# ---- the checks ---------------------------------------------------------------------------------------------------------------------
def compare_gradients(tag, names, grads_g, g32, g64):
    """Whole-model gradients of the engine (grads_g) against the fp64 oracle's (g64), judged by the fp32 oracle's own distance
    from fp64 (g32).  A ReLU whose pre-activation lies within fp32 rounding of zero takes a different branch in two correct
    implementations (and in fp32 vs fp64); one such flip near the output moves every upstream gradient by O(1e-3..1e-2) of its
    scale (signature: BN dbeta off, dgamma exact, since x_hat ~ 0 there).  So whole-model fp32 gradients are held to L2 bounds
    that catch real bugs (a missing or mis-scaled term is O(1)), while exactness is carried by the per-op tests (2e-5) and
    test_backward_chain_exact.  Returns (global relative L2 of the engine, of the fp32 oracle, the worst tensor's excess)."""
    assert len(g64) == len(grads_g) == len(g32) == len(names)
    num = den = num_c = 0.0
    per = []
    for nm, gg, gc, gt in zip(names, grads_g, g32, g64):
        n2 = float(np.square(gt).sum())
        e2, c2 = float(np.square(gg - gt).sum()), float(np.square(gc - gt).sum())
        num, den, num_c = num + e2, den + n2, num_c + c2
        per.append((nm, n2, e2, c2))
    worst = (0.0, None, 0.0, 0.0, 0.0)
    for nm, n2, e2, c2 in per:
        # skip structurally-zero gradients (conv bias feeding BatchNorm) and tensors that carry under a millionth
        # of the gradient energy (a gate bias on a 2-sample batch: its relative error is flip noise by itself)
        if n2 > 1e-6 * den:
            r, rc = (e2 / n2) ** 0.5, (c2 / n2) ** 0.5
            # a tensor is judged against the fp32 CPU oracle's own distance from fp64 on that tensor: where the
            # oracle itself is several per cent off (a flip right at that layer) the GPU may be, too
            excess = r / max(0.1, 4.0 * rc)
            if excess > worst[0]:
                worst = (excess, nm, r, rc, n2 / den)
    g_rel, c_rel = (num / den) ** 0.5, (num_c / den) ** 0.5
    print(f"{tag}: global rel-L2 grad error gpu {g_rel:.2e} (cpu-fp32 oracle {c_rel:.2e}); worst tensor {worst[1]}: "
          f"gpu {worst[2]:.2e}, cpu-fp32 oracle {worst[3]:.2e}, share of gradient energy {worst[4]:.1e}")
    # ... and the whole gradient against the fp32 CPU oracle's own distance from fp64 (Res34: 1.6e-2 by itself)
    assert g_rel <= max(2e-2, 2.5 * c_rel), f"{tag}: global gradient error {g_rel:.3e} (fp32 oracle {c_rel:.3e})"
    assert worst[0] <= 1.0, f"{tag}: gradient of {worst[1]} off by {worst[2]:.3e} (relative L2; fp32 oracle {worst[3]:.3e})"
    return g_rel, c_rel, worst[0]


def check_step(s: int, step: Step, x, y, names, trainable) -> dict:
    """One step of a trajectory, from its own pre-state.  `names`: every parameter's name, `trainable`: its flag (creation
    order).  Returns the figures it asserted on."""
    tag = f"step {s}"
    pre, post = step.pre, step.post
    tnames = [n for n, t in zip(names, trainable) if t]

    # 1. forward / backward from the pre-state, fp64 (the yardstick) and fp32 (what a correct fp32 implementation does)
    l64, g64, _ = oracle_step(pre.weights, x, y, torch.float64)
    l32, g32, P32 = oracle_step(pre.weights, x, y, torch.float32)
    loss_dev, loss_bound = abs(step.loss - l64), 5 * abs(l32 - l64) + 1e-5 * abs(l64)
    print(f"{tag}: loss {step.loss:.7f} fp32 oracle {l32:.7f} fp64 {l64:.7f}: |loss - fp64| / fp64 = {loss_dev / abs(l64):.2e} "
          f"(bound {loss_bound / abs(l64):.2e})")
    assert loss_dev <= loss_bound, f"{tag}: loss {step.loss} leaves the fp64 oracle's {l64} from the same state (fp32 oracle {l32})"
    g_rel, c_rel, excess = compare_gradients(tag, tnames, step.grads, g32, g64)
    stat_dev = 0.0
    for i, (nm, tr) in enumerate(zip(names, trainable)):
        if not tr:
            want = P32.tensors[i].detach().numpy()
            stat_dev = max(stat_dev, float(np.abs(post.weights[i].astype(np.float64) - want).max()))
            np.testing.assert_allclose(post.weights[i], want, rtol=1e-4, atol=1e-5,
                                       err_msg=f"{tag}: moving statistics {nm} after the step")

    # 2. the optimiser, exactly, from the step's own gradients: Keras-2 Adam in fp64 with the step number and the rate of the
    # schedule as THIS function computes them (nothing read from the model)
    t, lr = s + 1, schedule_lr(s)
    assert post.iterations == t, f"{tag}: step counter {post.iterations} after the step, expected {t}"
    assert pre.iterations == s, f"{tag}: step counter {pre.iterations} before the step, expected {s}"
    assert abs(pre.lr - lr) <= 2.0 ** -23 * lr, f"{tag}: learning rate {pre.lr!r}, the schedule gives {lr!r}"
    lr_t = lr * math.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)
    w_pre = [w for w, tr in zip(pre.weights, trainable) if tr]
    w_post = [w for w, tr in zip(post.weights, trainable) if tr]
    worst_m = worst_v = worst_w = 0.0
    for nm, w0, w1, m0, m1, v0, v1, g in zip(tnames, w_pre, w_post, pre.m, post.m, pre.v, post.v, step.grads):
        g = g.astype(np.float64)
        m_want = B1 * m0.astype(np.float64) + (1 - B1) * g
        v_want = B2 * v0.astype(np.float64) + (1 - B2) * g * g
        w_want = w0.astype(np.float64) - lr_t * m_want / (np.sqrt(v_want) + EPS)
        em, ev, ew = (float(np.abs(a.astype(np.float64) - b).max()) for a, b in ((m1, m_want), (v1, v_want), (w1, w_want)))
        sm, sv = float(np.abs(m_want).max()), float(np.abs(v_want).max())
        worst_m, worst_v, worst_w = max(worst_m, em / sm if sm else em), max(worst_v, ev / sv if sv else ev), max(worst_w, ew)
        assert em <= RTOL_MOMENTS * sm, f"{tag}: Adam first moment of {nm} off by {em:.3e} (largest entry {sm:.3e})"
        assert ev <= RTOL_MOMENTS * sv, f"{tag}: Adam second moment of {nm} off by {ev:.3e} (largest entry {sv:.3e})"
        assert ew <= ATOL_WEIGHTS, f"{tag}: Adam weights of {nm} off by {ew:.3e} (t = {t}, lr = {lr:.6g})"
    for k, a in post.pad.items():
        assert not a.any(), f"{tag}: padding of the {k} arena is no longer zero"
    print(f"{tag}: t {t} lr {lr:.6g}; moving statistics off by {stat_dev:.2e}; Adam m {worst_m:.2e} v {worst_v:.2e} (relative to "
          f"the tensor's largest entry), |w' - w| {worst_w:.2e}")
    return {"loss_rel": loss_dev / abs(l64), "loss32_rel": abs(l32 - l64) / abs(l64), "g_rel": g_rel, "c_rel": c_rel,
            "excess": excess, "stat_dev": stat_dev, "m_rel": worst_m, "v_rel": worst_v, "w_abs": worst_w}


def check_carry_over(s: int, a: State, b: State, names):
    """3. nothing moves between steps: the state before step s + 1 (b) is the state after step s (a), bit for bit."""
    tag = f"between steps {s} and {s + 1}"
    for nm, wa, wb in zip(names, a.weights, b.weights):
        assert np.array_equal(wa.view(np.uint32), wb.view(np.uint32)), f"{tag}: {nm} changed"
    for what, la, lb in (("first", a.m, b.m), ("second", a.v, b.v)):
        for k, (ma, mb) in enumerate(zip(la, lb)):
            assert np.array_equal(ma.view(np.uint32), mb.view(np.uint32)), f"{tag}: Adam {what} moment {k} changed"
    assert a.iterations == b.iterations, f"{tag}: step counter went from {a.iterations} to {b.iterations}"
    for k, p in b.pad.items():
        assert not p.any(), f"{tag}: padding of the {k} arena is no longer zero"


def check_trajectory(steps: List[Step], batches, names, trainable) -> List[dict]:
    assert len(steps) == len(batches)
    figures = []
    for s, (step, (x, y)) in enumerate(zip(steps, batches)):
        if s:
            check_carry_over(s - 1, steps[s - 1].post, step.pre, names)
        figures.append(check_step(s, step, x, y, names, trainable))
    return figures


# ---- the free-running yardstick -------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def permuted_convolutions(seed: Optional[int]):
    """Inside, every oracle conv2d sums its input channels in a random order (x and w permuted alike: mathematically neutral,
    in fp32 another order of summation - what separates two correct implementations)."""
    if seed is None:
        yield
        return
    orig = T.conv2d
    gen = torch.Generator().manual_seed(seed)

    def conv2d(x, w, b=None, *a, **k):
        if x.shape[-1] > 1:
            p = torch.randperm(x.shape[-1], generator=gen)
            x, w = x[..., p], w[:, :, p, :]
        return orig(x, w, b, *a, **k)

    T.conv2d = conv2d
    try:
        yield
    finally:
        T.conv2d = orig


def oracle_run(ws0, batches, dtype, perm: Optional[int] = None):
    """Free-running oracle: len(batches) steps of HRNet + edge_focal_loss + Keras-Adam at the rates of SCHEDULE.  Returns the
    losses and the trainable weights afterwards (fp64 numpy)."""
    with permuted_convolutions(perm):
        P = M.Params(weights=ws0, dtype=dtype)
        tr = m = v = None
        losses = []
        for s, (x, y) in enumerate(batches):
            p = M.hrnet(P, torch.from_numpy(x).to(dtype), training=True)
            loss = M.loss_fn("edge_focal_loss", torch.from_numpy(y).to(dtype), p)
            tr = P.trainable_tensors()
            for t in tr:
                t.grad = None
            loss.backward()
            losses.append(loss.item())
            if m is None:
                m, v = [torch.zeros_like(t) for t in tr], [torch.zeros_like(t) for t in tr]
            M.adam_step(tr, [t.grad for t in tr], m, v, s + 1, schedule_lr(s))
        return losses, [t.detach().double().numpy() for t in tr]


PERTURBATION_SEED0 = 1000


def loss_envelope(ws0, batches, l64, k=8):
    """Per step: max over k perturbed fp32 oracle runs of |loss - fp64 loss|, and the runs' losses."""
    runs = [oracle_run(ws0, batches, torch.float32, perm=PERTURBATION_SEED0 + i)[0] for i in range(k)]
    env = np.abs(np.array(runs) - np.array(l64)[None, :]).max(0)
    return env, runs
