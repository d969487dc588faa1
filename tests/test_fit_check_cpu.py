"""The training-loop checker (tests/_fit_check.py) tested without a GPU: a trajectory recorded from the fp32 CPU oracle must pass
every per-step check - which also shows that the reference alone stays inside every bound the engine is held to - and the same
trajectory with one error planted in the host arithmetic must fail the assertion that error belongs to."""
import copy

import numpy as np
import pytest
import torch

import _fit_check as FC

SIZE = 32


def _batches(seed, steps):
    from building_detection_amd.data import synthetic_batch
    return [synthetic_batch(2, SIZE, SIZE, seed=seed + i) for i in range(steps)]


@pytest.fixture(scope="module")
def net():
    ws0, trainable, kinds = FC.oracle_initial_weights(SIZE)
    names = [f"{k}_{i}" for i, k in enumerate(kinds)]
    return ws0, trainable, kinds, names


def test_schedule_matches_the_scheduler_callback():
    """schedule_lr(s) is what WarmUpCosineDecayScheduler sets before its batch s."""
    from building_detection_amd.callbacks import WarmUpCosineDecayScheduler
    from building_detection_amd.runtime import Optimizer

    class _M:
        optimizer = Optimizer()

    sched = WarmUpCosineDecayScheduler(**FC.SCHEDULE)
    sched.set_model(_M())
    for s in range(6):
        sched.on_batch_begin(s)
        assert float(_M.optimizer.lr) == FC.schedule_lr(s)
        sched.on_batch_end(s)
    assert FC.schedule_lr(0) == 1e-5 and FC.schedule_lr(2) == 1e-3 and FC.schedule_lr(1) == pytest.approx(5.05e-4, rel=1e-12)


def test_the_fp32_oracle_passes_every_step_from_its_own_state(net):
    """Six steps of the fp32 oracle, each judged from the state it started in: all inside the engine's bounds, and as tight
    at step 5 as at step 0 (the free-running loss is several per cent from fp64 by then)."""
    ws0, trainable, kinds, names = net
    batches = _batches(100, 6)
    steps = FC.oracle_trajectory(ws0, batches)
    figures = FC.check_trajectory(steps, batches, names, trainable)
    assert len(figures) == 6
    for f in figures:
        assert f["loss_rel"] <= 1e-4 and f["stat_dev"] <= 1e-5 and f["w_abs"] <= FC.ATOL_WEIGHTS
    assert steps[-1].post.iterations == 6


@pytest.mark.parametrize("fault,match", [
    ("step_counter", "step counter"),
    ("bias_correction_one_step_ahead", "Adam weights"),
    ("lr_one_step_late", "learning rate"),
    ("lr_one_step_late_unreported", "Adam weights"),
    ("moving_statistics_swapped", "moving statistics"),
    ("first_moment_not_carried", "Adam first moment"),
])
def test_a_planted_error_fails_its_assertion(net, fault, match):
    """t off by one (reported, or only used in the bias correction), the learning rate of step s - 1 (reported, or only used: a
    captured step whose device-side rate is not refreshed), the moving statistics of two BatchNorm layers swapped, Adam's first
    moment not carried over.  All of them leave step 0's LOSS untouched; two steps are enough for each to show."""
    ws0, trainable, kinds, names = net
    batches = _batches(200, 2)
    steps = FC.oracle_trajectory(ws0, batches, fault=fault)
    with pytest.raises(AssertionError, match=match):
        FC.check_trajectory(steps, batches, names, trainable)


def test_the_swapped_layers_have_different_statistics(net):
    ws0, trainable, kinds, names = net
    batches = _batches(200, 1)
    post = FC.oracle_trajectory(ws0, batches)[0].post.weights
    a, b = FC.swappable_bn_pair(post, kinds)
    assert kinds[a] == kinds[b] == "moving_mean" and kinds[a + 1] == kinds[b + 1] == "moving_var"
    assert float(np.abs(post[a] - post[b]).max()) > 1e-3   # two orders above the check's atol 1e-5 + rtol 1e-4


def test_state_that_moves_between_steps_is_caught(net):
    ws0, trainable, kinds, names = net
    batches = _batches(300, 2)
    clean = FC.oracle_trajectory(ws0, batches)
    for what, match in (("weight", "changed"), ("moment", "Adam second moment"), ("padding", "padding of the m arena")):
        steps = copy.deepcopy(clean)
        if what == "weight":    # one ulp in one moving variance
            i = kinds.index("moving_var")
            w = steps[1].pre.weights[i]
            w[0] = np.nextafter(w[0], np.float32(2))
        elif what == "moment":
            v = steps[1].pre.v[3].reshape(-1)
            v[0] = np.nextafter(v[0], np.float32(2))
        else:
            steps[1].pre.pad = {"m": np.array([0, 1e-30], np.float32)}
        with pytest.raises(AssertionError, match=match):
            FC.check_carry_over(0, steps[0].post, steps[1].pre, names)
    FC.check_carry_over(0, clean[0].post, clean[1].pre, names)


def test_permuted_convolutions_are_neutral_in_fp64_and_not_in_fp32(net):
    """The perturbation of the free-running yardstick: the same mathematics (fp64 agrees to rounding), another order of
    summation (fp32 differs in the last bits), and the oracle's conv2d is restored afterwards."""
    from oracle import tfops as T
    ws0, trainable, kinds, names = net
    (x, y), = _batches(100, 1)
    orig = T.conv2d
    l64, g64, _ = FC.oracle_step(ws0, x, y, torch.float64)
    l32, _, _ = FC.oracle_step(ws0, x, y, torch.float32)
    with FC.permuted_convolutions(1000):
        p64, q64, _ = FC.oracle_step(ws0, x, y, torch.float64)
        p32, _, _ = FC.oracle_step(ws0, x, y, torch.float32)
    assert T.conv2d is orig
    assert abs(p64 - l64) <= 1e-12 * abs(l64)
    num = sum(float(np.square(a - b).sum()) for a, b in zip(q64, g64))
    den = sum(float(np.square(b).sum()) for b in g64)
    assert (num / den) ** 0.5 <= 1e-9
    assert p32 != l32 and abs(p32 - l64) <= 1e-4 * abs(l64)
