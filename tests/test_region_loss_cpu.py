"""The region-overlap losses without a GPU: the float64 reference (tests/_region_loss_ref.py) against central differences and
the textbook Dice / Jaccard expressions, the public loss objects and what they refuse, and what compile() stores."""
import ctypes

import pytest
import torch

import _multiclass_ref as MR
import _region_loss_ref as RR

F64 = torch.float64
FD_BOUND = 1e-7   # of max |grad|; central differences with h = 1e-6 in float64 sit at about 1e-9 (truncation h^2, rounding eps / h)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def inputs(seed, rows, C, y_cols, absent=None, span=4.0):
    g = gen(seed)
    p, yt = MR.class_probs(g, rows, C, -span, span).double(), MR.class_labels(g, rows, C, y_cols).double()
    if absent is not None:                          # no pixel of this class: Y = I = 0
        hit = yt[:, absent] == 1
        yt[hit, absent] = 0
        yt[hit, (absent + 1) % C] = 1
        assert yt[:, absent].sum() == 0
    return p, yt


CONFIGS = [
    dict(C=2, rows=24, images=1, y_cols=4, kw=dict(a=0.5, b=0.5, gamma=1.0, point_kind=2, point_alpha=(0.35, 0.65))),
    dict(C=3, rows=30, images=3, y_cols=3, kw=dict(a=1.0, b=1.0, gamma=2.0, smooth=0.5, class_w=(1.0, 0.0, 2.0))),
    dict(C=5, rows=40, images=2, y_cols=10, absent=3,
         kw=dict(a=0.3, b=0.7, gamma=1.5, class_w=(0.5, 1.0, 0.0, 2.0, 1.5), point_kind=1, point_alpha=(0.2, 0.4, 0.6, 0.8, 1.0),
                 point_weight=0.5, region_weight=2.0)),
    dict(C=3, rows=18, images=1, y_cols=3, kw=dict(a=0.3, b=0.7, gamma=1.0, point_kind=0, region_weight=0.25)),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=[f"C{c['C']}-g{c['images']}" for c in CONFIGS])
def test_reference_gradient_against_central_differences(cfg):
    C, rows = cfg["C"], cfg["rows"]
    d = RR.desc(C, images=cfg["images"], **cfg["kw"])
    # logits within +-1.5, so p >= 0.012: the central difference of the pointwise terms' log(p) is off by about h^2 / (3 p^2)
    # of the derivative itself (their third derivative grows as 1 / p^3), 2e-9 here and 3e-6 at the p = 3e-4 of logits +-4
    p, yt = inputs(100 + C, rows, C, cfg["y_cols"], cfg.get("absent"), span=1.5)
    g = RR.grad_ref(d, p, yt)
    h = 1e-6
    fd = torch.zeros_like(p)
    for r in range(rows):
        for c in range(C):
            hi, lo = p.clone(), p.clone()
            hi[r, c] += h
            lo[r, c] -= h
            fd[r, c] = (RR.loss_ref(d, hi, yt)[0] - RR.loss_ref(d, lo, yt)[0]) / (2 * h)
    err, scale = (g - fd).abs().max().item(), g.abs().max().item()
    print(f"C={C} images={cfg['images']}: max |grad - fd| = {err:.3e} = {err / scale:.2e} of max |grad| {scale:.3e}")
    assert err <= FD_BOUND * scale
    assert torch.allclose(RR.grad_ref(d, p, yt, 0.25), 0.25 * g, rtol=1e-15, atol=0)


def test_presets_are_the_textbook_dice_and_jaccard():
    C, rows, s = 4, 50, 1.0
    p, yt = inputs(7, rows, C, C)
    I, P, Y = (p * yt).sum(0), p.sum(0), yt.sum(0)
    dice = (1 - (2 * I + 2 * s) / (P + Y + 2 * s)).mean()          # the usual notation with the smoothing constant 2 s
    jacc = (1 - (I + s) / (P + Y - I + s)).mean()
    assert abs(RR.loss_ref(RR.desc(C, a=0.5, b=0.5, smooth=s), p, yt)[0] - dice) <= 1e-15
    assert abs(RR.loss_ref(RR.desc(C, a=1.0, b=1.0, smooth=s), p, yt)[0] - jacc) <= 1e-15
    # per image: the mean of the images' own losses
    per = torch.stack([RR.loss_ref(RR.desc(C), p[g * 25:(g + 1) * 25], yt[g * 25:(g + 1) * 25])[0] for g in range(2)]).mean()
    assert abs(RR.loss_ref(RR.desc(C, images=2), p, yt)[0] - per) <= 1e-15
    # a perfect prediction: T = 1, the loss 0, and (1 - T)^0 = 1 keeps the gamma = 1 gradient finite
    d = RR.desc(C)
    L = RR.loss_ref(d, yt.clone(), yt)
    assert L[0].abs() <= 1e-15 and torch.isfinite(RR.grad_ref(d, yt.clone(), yt)).all()
    assert torch.isfinite(RR.grad_ref(RR.desc(C, gamma=2.0), yt.clone(), yt)).all()


def test_compound_without_region_weight_is_the_pointwise_reference():
    C, rows = 3, 40
    p, yt = inputs(9, rows, C, 2 * C)
    alpha = (0.3, 0.5, 0.7)
    for kind in (0, 1, 2):
        d = RR.desc(C, point_kind=kind, point_alpha=alpha, region_weight=0.0)
        L = RR.loss_ref(d, p, yt)
        assert L[0] == L[1] == MR.loss_ref(kind, p, yt, alpha)
        assert torch.allclose(RR.grad_ref(d, p, yt, 0.5), MR.loss_bwd_ref(kind, p, yt, alpha, 0.5), rtol=1e-14, atol=0)
        assert torch.equal(RR.coef_ref(d, p, yt), torch.zeros(1, 2 * C, dtype=F64))
    d = RR.desc(C, gamma=2.0)
    L = RR.loss_ref(d, p, yt)
    assert L[1] == 0 and L[0] == L[2] > 0


def test_loss_objects_and_what_they_refuse():
    from building_detection_amd import losses as LS
    from building_detection_amd._lib import SG_LOSS_CE2, SG_LOSS_EDGE_FOCAL, SG_LOSS_FOCAL
    assert (LS.dice_loss.alpha, LS.dice_loss.beta) == (0.5, 0.5) and (LS.jaccard_loss.alpha, LS.jaccard_loss.beta) == (1.0, 1.0)
    t = LS.tversky_loss(0.3, 0.7)
    assert (t.alpha, t.beta, t.smooth, t.gamma, t.class_weights, t.per_image) == (0.3, 0.7, 1.0, 1.0, None, False)
    o = LS.dice_loss.with_options(smooth=0.5, gamma=2, class_weights=[1, 0, 3], per_image=True)
    assert (o.alpha, o.beta, o.smooth, o.gamma, o.class_weights, o.per_image) == (0.5, 0.5, 0.5, 2.0, (1.0, 0.0, 3.0), True)
    assert o.__name__ == "dice_loss" and LS.dice_loss.smooth == 1.0 and LS.dice_loss.class_weights is None      # a new object
    with pytest.raises(RuntimeError, match="compile"):
        o(None, None)
    # the three existing names resolve as ever; region losses have no pointwise kind
    assert [LS.resolve_loss(n) for n in (LS.binary_crossentropy, LS.focal_loss, LS.edge_focal_loss)] == [0, 1, 2]
    assert LS.resolve_loss(o) == LS.NO_POINTWISE == -1
    for l in (LS.binary_crossentropy, LS.focal_loss, LS.edge_focal_loss, "focal_loss"):
        assert LS.resolve_region(l, 2) is None
    r = LS.resolve_region(o, 3)
    assert r == dict(a=0.5, b=0.5, smooth=0.5, gamma=2.0, class_w=(1.0, 0.0, 3.0), per_image=True, point_kind=-1, point_alpha=None,
                     point_weight=0.0, region_weight=1.0)
    assert LS.resolve_region(LS.jaccard_loss, 4)["class_w"] == (1.0,) * 4
    # compounds: the pointwise kind, its weights (the reference's own, explicitly, at two classes)
    c = LS.compound(LS.edge_focal_loss, LS.dice_loss)
    assert LS.resolve_loss(c) == SG_LOSS_EDGE_FOCAL
    r = LS.resolve_region(c, 2)
    assert (r["point_kind"], r["point_alpha"], r["point_weight"], r["region_weight"]) == (SG_LOSS_EDGE_FOCAL, (0.35, 0.65), 1.0, 1.0)
    r = LS.resolve_region(LS.compound(LS.focal_loss, t, region_weight=2, pointwise_weight=0.5), 2)
    assert (r["point_kind"], r["point_alpha"], r["point_weight"], r["region_weight"]) == (SG_LOSS_FOCAL, (0.5, 0.5), 0.5, 2.0)
    assert (r["a"], r["b"]) == (0.3, 0.7)
    assert LS.resolve_region(LS.compound(LS.focal_loss, t), 5)["point_alpha"] == (0.5,) * 5
    r = LS.resolve_region(LS.compound(LS.binary_crossentropy, LS.jaccard_loss, region_weight=0), 3)
    assert (r["point_kind"], r["point_alpha"], r["region_weight"]) == (SG_LOSS_CE2, None, 0.0)
    w5 = [0.2, 0.4, 0.6, 0.8, 1.0]
    assert LS.resolve_region(LS.compound(LS.edge_focal_loss.with_alpha(w5), LS.dice_loss), 5)["point_alpha"] == tuple(w5)
    # refusals
    for kw in (dict(smooth=0), dict(smooth=-1.0), dict(smooth=float("nan")), dict(gamma=0.5), dict(gamma=float("inf")),
               dict(class_weights=[]), dict(class_weights=[0, 0]), dict(class_weights=[1, -1]), dict(class_weights=[1, float("nan")])):
        with pytest.raises(ValueError, match="with_options"):
            LS.dice_loss.with_options(**kw)
    for a, b in ((-0.1, 0.5), (0.5, float("inf")), ("x", 1)):
        with pytest.raises(ValueError, match="tversky_loss"):
            LS.tversky_loss(a, b)
    for args, kw in (((LS.dice_loss, LS.dice_loss), {}), ((LS.focal_loss, LS.focal_loss), {}), (("focal_loss", LS.dice_loss), {}),
                     ((LS.PA, LS.dice_loss), {}), ((LS.focal_loss, LS.dice_loss), dict(region_weight=-1)),
                     ((LS.focal_loss, LS.dice_loss), dict(region_weight=0, pointwise_weight=0)),
                     ((LS.focal_loss, LS.dice_loss), dict(pointwise_weight=float("nan")))):
        with pytest.raises(ValueError, match="compound"):
            LS.compound(*args, **kw)
    with pytest.raises(ValueError, match="class weights"):
        LS.resolve_region(LS.dice_loss.with_options(class_weights=[1, 2, 3]), 2)
    with pytest.raises(ValueError, match="class weights"):
        LS.resolve_region(LS.compound(LS.focal_loss.with_alpha([0.5, 0.5]), LS.dice_loss), 3)
    with pytest.raises(ValueError, match="with_alpha"):
        LS.resolve_region(LS.compound(LS.edge_focal_loss, LS.dice_loss), 3)
    with pytest.raises(ValueError, match="the engine implements"):
        LS.resolve_loss("dice")


def test_compile_stores_the_descriptor():
    from building_detection_amd import losses as LS, zoo
    m = zoo.HRNet((32, 32, 3), num_classes=3)
    w3 = [0.35, 0.5, 0.65]
    loss = LS.compound(LS.edge_focal_loss.with_alpha(w3), LS.dice_loss.with_options(gamma=2, per_image=True), region_weight=0.5)
    m.compile(loss=loss, metrics=[LS.MIoU])
    assert m.loss_kind == 2 and m.loss_alpha == tuple(w3)
    assert m.loss_region == dict(a=0.5, b=0.5, smooth=1.0, gamma=2.0, class_w=(1.0, 1.0, 1.0), per_image=True, point_kind=2,
                                 point_alpha=tuple(w3), point_weight=1.0, region_weight=0.5)
    m.compile(loss=LS.tversky_loss(0.3, 0.7))
    assert m.loss_kind == -1 and m.loss_alpha is None and m.loss_region["point_kind"] == -1
    m.compile(loss=LS.focal_loss)                                          # back to a pointwise loss: no descriptor
    assert m.loss_region is None and m.loss_kind == 1
    with pytest.raises(ValueError, match="with_alpha"):
        m.compile(loss=LS.compound(LS.edge_focal_loss, LS.dice_loss))
    with pytest.raises(ValueError, match="class weights"):
        m.compile(loss=LS.jaccard_loss.with_options(class_weights=[1, 1]))
    m2 = zoo.HRNet((32, 32, 3))
    m2.compile(loss=LS.compound(LS.edge_focal_loss, LS.dice_loss))
    assert m2.loss_region["point_alpha"] == (0.35, 0.65) and m2.loss_alpha is None


def test_descriptor_binding_and_what_the_engine_wrapper_refuses():
    """Engine.region_desc needs no device: the struct it fills, the groups it forms, and the label widths it refuses."""
    from building_detection_amd import losses as LS
    from building_detection_amd._lib import RegionDesc, SG_MAX_CLASSES
    from building_detection_amd.ops import Engine
    assert ctypes.sizeof(RegionDesc) == 4 * 4 + 8 + 6 * 4 + 2 * 4 * SG_MAX_CLASSES
    p, y6, y3 = torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 6), torch.zeros(2, 8, 8, 3)
    r = LS.resolve_region(LS.compound(LS.edge_focal_loss.with_alpha([0.2, 0.3, 0.5]), LS.tversky_loss(0.3, 0.7)), 3)
    d = Engine.region_desc(r, p, y6)
    assert (d.C, d.y_cols, d.images, d.rows_per_image, d.point_kind) == (3, 6, 1, 128, 2)
    assert abs(d.a - 0.3) < 1e-7 and abs(d.b - 0.7) < 1e-7 and list(d.class_w)[:4] == [1.0, 1.0, 1.0, 0.0]
    assert [round(v, 6) for v in list(d.point_alpha)[:3]] == [0.2, 0.3, 0.5]
    with pytest.raises(ValueError, match="edge_focal_loss needs"):
        Engine.region_desc(r, p, y3)
    r = LS.resolve_region(LS.dice_loss.with_options(per_image=True), 3)
    d = Engine.region_desc(r, p, y3)
    assert (d.images, d.rows_per_image, d.y_cols, d.point_kind) == (2, 64, 3, -1)
    with pytest.raises(ValueError, match="columns"):
        Engine.region_desc(r, p, torch.zeros(2, 8, 8, 4))
    with pytest.raises(ValueError, match="class"):
        Engine.region_desc(LS.resolve_region(LS.dice_loss, 2), p, y3)
