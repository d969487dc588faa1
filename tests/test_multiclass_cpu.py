"""The C-class segmentation head without a GPU: the builders take num_classes, the matrix metrics reduce to the reference's
2-class formulas, the synthetic batch and its edge-weight rule, what compile() refuses, and the binary-only tail."""
import numpy as np
import pytest

from _multiclass_ref import metrics_ref64


def _head_cin(model):
    return [p for p in model.params if p.trainable][-2].shape[-2]   # kernel [1][1][Cin][C] of the softmax head


@pytest.mark.parametrize("name", ["hrnet", "scse", "v3plus"])
def test_builders_take_num_classes(name):
    from building_detection_amd import zoo
    build = {"hrnet": lambda C: zoo.HRNet((32, 32, 3), num_classes=C),
             "scse": lambda C: zoo.UNet(C, (32, 32, 3)),
             "v3plus": lambda C: zoo.Xception_DeepLabV3_Plus((64, 64, 3), C, aspp_pool=4)}[name]
    C = {"hrnet": 5, "scse": 3, "v3plus": 4}[name]
    m2, mc = build(2), build(C)
    assert tuple(mc.outputs[0].shape)[-1] == C and mc.num_classes == C and m2.num_classes == 2
    assert tuple(mc.outputs[0].shape)[:-1] == tuple(m2.outputs[0].shape)[:-1]
    assert mc.count_params() == m2.count_params() + (C - 2) * (_head_cin(m2) + 1)


def test_softmax_heads_refuse_class_counts_outside_the_range():
    from building_detection_amd import zoo
    for C in (1, 33):
        with pytest.raises(ValueError, match=rf"2 \.\.\. 32 classes, not {C}"):
            zoo.HRNet((32, 32, 3), num_classes=C)


def test_matrix_metrics_equal_the_count_metrics_at_two_classes():
    from building_detection_amd.losses import metrics_from_counts, metrics_from_matrix
    rng = np.random.default_rng(7)
    quads = [(0, 0, 0, 0), (5, 0, 0, 0), (0, 9, 0, 0), (0, 0, 3, 0), (0, 0, 0, 4)]
    for i in range(400):
        q = [int(v) for v in rng.integers(0, (6, 1 << 20, (1 << 31) - 1)[i % 3], 4)]
        if i % 5 == 0:
            q[int(rng.integers(0, 4))] = 0
        quads.append(tuple(q))
    for tp, tn, fp, fn in quads:
        a, b = metrics_from_counts(tp, tn, fp, fn), metrics_from_matrix([[tn, fp], [fn, tp]])
        for k in ("PA", "IoU", "MIoU", "F1_score"):
            assert a[k] == b[k], (k, (tp, tn, fp, fn), a[k], b[k])     # the same float32 bits
        assert b["IoU_per_class"][1] == a["IoU"] and b["F1_per_class"][1] == a["F1_score"]


def test_matrix_metrics_at_four_classes_against_float64():
    from building_detection_amd.losses import metrics_from_matrix
    rng = np.random.default_rng(8)
    for i in range(50):
        M = rng.integers(0, 5000, (4, 4))
        if i % 4 == 0:
            M[:, int(rng.integers(0, 4))] = 0       # a class that is never predicted
        if i % 6 == 0:
            M[int(rng.integers(0, 4)), :] = 0       # ... and one that never occurs
        got, ref = metrics_from_matrix(M), metrics_ref64(M)
        for k in ("PA", "IoU", "MIoU", "F1_score"):
            assert abs(got[k] - ref[k]) <= 1e-6, (k, got[k], ref[k], M)
        assert np.allclose(got["IoU_per_class"], ref["IoU_per_class"], rtol=0, atol=1e-6)
        assert np.allclose(got["F1_per_class"], ref["F1_per_class"], rtol=0, atol=1e-6)
    with pytest.raises(ValueError):
        metrics_from_matrix(np.zeros((3, 4), np.int64))


def test_synthetic_batch_default_is_unchanged_and_the_edge_rule_is_the_binary_one():
    from building_detection_amd.data import class_edge_weights, edge_weight_channels, synthetic_batch
    x, y = synthetic_batch(2, 64, 48, seed=31)
    x2, y2 = synthetic_batch(2, 64, 48, seed=31, num_classes=2)
    assert x.tobytes() == x2.tobytes() and y.tobytes() == y2.tobytes() and y.shape == (2, 64, 48, 4)
    # the default path restated draw by draw, as it stood before num_classes: nothing was inserted into the random stream
    rng = np.random.default_rng(31)
    xr = rng.integers(0, 256, size=(2, 64, 48, 3), dtype=np.uint8).astype(np.float32) / 127.5 - 1.0
    assert xr.astype(np.float32).tobytes() == x.tobytes()
    yr = np.empty((2, 64, 48, 4), np.float32)
    for i in range(2):
        mask = np.zeros((64, 48), np.float32)
        for _ in range(int(rng.integers(3, 13))):
            rh, rw = int(rng.integers(max(64 // 32, 2), max(64 // 4, 3))), int(rng.integers(max(48 // 32, 2), max(48 // 4, 3)))
            r0, c0 = int(rng.integers(0, 64 - rh)), int(rng.integers(0, 48 - rw))
            mask[r0:r0 + rh, c0:c0 + rw] = 1.0
        f_edge, p_edge = edge_weight_channels(mask)
        yr[i, ..., 0], yr[i, ..., 1], yr[i, ..., 2], yr[i, ..., 3] = 1.0 - mask, mask, f_edge, p_edge
    assert yr.tobytes() == y.tobytes()
    for i in range(2):   # C = 2: w_0 is f_edge (dilate(fg) - fg), w_1 is p_edge (fg - erode(fg))
        fg = y[i, ..., 1]
        w = class_edge_weights(fg.astype(np.int64), 2)
        f_edge, p_edge = edge_weight_channels(fg)
        assert np.array_equal(w[..., 0], f_edge) and np.array_equal(w[..., 1], p_edge)
        assert np.array_equal(w[..., 0], y[i, ..., 2]) and np.array_equal(w[..., 1], y[i, ..., 3])
        assert (w == 2).any()


def test_synthetic_batch_of_four_classes():
    from building_detection_amd.data import synthetic_batch
    x, y = synthetic_batch(3, 64, 64, seed=5, num_classes=4)
    assert x.shape == (3, 64, 64, 3) and y.shape == (3, 64, 64, 8) and y.dtype == np.float32
    onehot, w = y[..., :4], y[..., 4:]
    assert set(np.unique(onehot)) <= {0.0, 1.0} and np.array_equal(onehot.sum(-1), np.ones((3, 64, 64), np.float32))
    assert set(np.unique(w)) == {1.0, 2.0}
    assert (w[onehot == 0] == 1.0).all()          # a weight of 2 sits on the pixel's own class only
    cls = onehot.argmax(-1)
    assert set(np.unique(cls)) <= {0, 1, 2, 3} and len(np.unique(cls)) >= 3
    # a pixel deep inside one class (its 11 x 11 window uniform) keeps weight 1; one next to another class has 2
    i, r, c = np.argwhere(w.max(-1) == 2)[0]
    win = cls[i, max(r - 5, 0):r + 6, max(c - 5, 0):c + 6]
    assert len(np.unique(win)) > 1
    x2, y2 = synthetic_batch(3, 64, 64, seed=5, num_classes=4)
    assert y.tobytes() == y2.tobytes() and x.tobytes() == x2.tobytes()


def test_compile_checks_the_class_weights():
    from building_detection_amd import zoo
    from building_detection_amd.losses import binary_crossentropy, edge_focal_loss, focal_loss, resolve_loss
    m = zoo.HRNet((32, 32, 3), num_classes=5)
    with pytest.raises(ValueError, match="with_alpha"):
        m.compile(loss=edge_focal_loss)
    with pytest.raises(ValueError, match="class weights"):
        m.compile(loss=edge_focal_loss.with_alpha([0.35, 0.65]))
    with pytest.raises(ValueError, match="class weights"):
        m.compile(loss=focal_loss.with_alpha([1.0] * 6))
    w = edge_focal_loss.with_alpha([0.2, 0.4, 0.6, 0.8, 1.0])
    assert w.__name__ == "edge_focal_loss" and resolve_loss(w) == resolve_loss(edge_focal_loss)
    assert edge_focal_loss.alpha is None                       # with_alpha returns a new object
    m.compile(loss=w)
    assert m.loss_alpha == (0.2, 0.4, 0.6, 0.8, 1.0)
    m.compile(loss=focal_loss)
    assert m.loss_alpha == (0.5,) * 5
    m.compile(loss=binary_crossentropy)
    assert m.loss_alpha is None
    m2 = zoo.HRNet((32, 32, 3))
    m2.compile(loss=edge_focal_loss)
    assert m2.loss_alpha is None and m2._two_class()           # the 2-class kernels with their built-in (.35, .65)
    m2.compile(loss=edge_focal_loss.with_alpha([0.35, 0.65, 0.5]).with_alpha([0.3, 0.7]))
    assert m2.loss_alpha == (0.3, 0.7) and not m2._two_class()


def test_binary_tail_refuses_a_class_map():
    from building_detection_amd import cleanup, pipeline
    cm = np.zeros((40, 50), np.uint8)
    cm[5:20, 5:20], cm[25:35, 10:40] = 1, 3
    for fn in (lambda: pipeline.vote([cm] * 5), lambda: pipeline.model_confuse([cm] * 5), lambda: cleanup.clean(cm),
               lambda: cleanup.model_confuse([cm] * 5), lambda: cleanup.fill_and_delete(cm)):
        with pytest.raises(ValueError, match="class map"):
            fn()
    for ok in (np.zeros((4, 4), np.uint8), np.full((4, 4), 255, np.uint8)):
        cleanup.require_binary(ok, "mask")
