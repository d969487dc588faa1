"""Lovasz-Softmax without a GPU: what losses.lovasz_loss and compound take and refuse, what the resolve_* functions and
compile() make of it, the binding's table, and the numpy reference (tests/_lovasz_ref.py) against known answers, against the
difference form of g_k in exact arithmetic, under permutations of tied pixels and against central differences."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import _lovasz_ref as LR
import _multiclass_ref as MR

FD_BOUND = 1e-7   # of max |grad|: the loss is linear in p between rank changes, so central differences with h = 1e-6 in
                  # float64 err by rounding alone, 2^-53 |L| / h = 1e-10 against gradients of 1 / (rows * C) = 1e-2 and more


def gen(seed):
    return torch.Generator().manual_seed(seed)


def test_lovasz_options_and_compound():
    from building_detection_amd import losses as LS
    l = LS.lovasz_loss
    assert isinstance(l, LS._Named) and l.__name__ == "lovasz_loss" and (l.classes, l.per_image) == ("present", False)
    o = l.with_options(classes="all", per_image=True)
    assert (o.classes, o.per_image, o.__name__) == ("all", True, "lovasz_loss") and (l.classes, l.per_image) == ("present", False)
    assert l.with_options().classes == "present" and "classes='all'" in repr(o)
    with pytest.raises(RuntimeError, match="compile"):
        l(None, None)
    for bad in ("some", None, 1, True):
        with pytest.raises(ValueError, match="classes"):
            l.with_options(classes=bad)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="per_image"):
            l.with_options(per_image=bad)
    c = LS.compound(LS.edge_focal_loss, l, 0.5, 2.0)
    assert c.__name__ == "edge_focal_loss+lovasz_loss" and (c.region, c.region_weight, c.pointwise_weight) == (l, 0.5, 2.0)
    assert LS.compound(LS.focal_loss.with_alpha([1, 2, 3]), o).__name__ == "focal_loss+lovasz_loss"
    for bad in ((LS.dice_loss, l), (l, l), (l, LS.focal_loss), ("focal_loss", l), (LS.focal_loss, "lovasz_loss")):
        with pytest.raises(ValueError, match="compound"):
            LS.compound(*bad)
    for w in ((0.0, 0.0), (-1.0, 1.0), (1.0, float("nan")), (float("inf"), 1.0)):
        with pytest.raises(ValueError, match="compound"):
            LS.compound(LS.focal_loss, l, *w)
    with pytest.raises(ValueError, match="mined pointwise term inside a compound is not implemented"):
        LS.compound(LS.hard_mining(LS.focal_loss), l)
    for bad in (l, LS.compound(LS.focal_loss, l)):
        with pytest.raises(ValueError, match="pointwise"):
            LS.hard_mining(bad)


def test_resolve_functions():
    from building_detection_amd import losses as LS
    from building_detection_amd._lib import SG_LOSS_CE2, SG_LOSS_FOCAL, SG_LOSS_EDGE_FOCAL
    l = LS.lovasz_loss
    for other in (LS.binary_crossentropy, LS.focal_loss, "edge_focal_loss", LS.dice_loss, LS.compound(LS.focal_loss, LS.dice_loss),
                  LS.hard_mining(LS.focal_loss)):
        assert LS.resolve_lovasz(other, 2) is None
    assert LS.resolve_loss(l) == LS.NO_POINTWISE and LS.resolve_region(l, 3) is None and LS.resolve_mining(l, 3) is None
    assert LS.resolve_alpha(l, 3) is None
    assert LS.resolve_lovasz(l, 3) == dict(classes_all=False, per_image=False, point_kind=-1, point_alpha=None, point_weight=0.0,
                                           lovasz_weight=1.0)
    assert LS.resolve_lovasz(l.with_options("all", True), 2)["classes_all"] is True
    assert LS.resolve_lovasz(l.with_options("all", True), 2)["per_image"] is True
    c = LS.compound(LS.edge_focal_loss, l, 0.5, 2.0)
    assert LS.resolve_loss(c) == SG_LOSS_EDGE_FOCAL and LS.resolve_region(c, 2) is None and LS.resolve_mining(c, 2) is None
    assert LS.resolve_alpha(c, 2) is None
    assert LS.resolve_lovasz(c, 2) == dict(classes_all=False, per_image=False, point_kind=SG_LOSS_EDGE_FOCAL, point_alpha=(0.35, 0.65),
                                           point_weight=2.0, lovasz_weight=0.5)
    with pytest.raises(ValueError, match="with_alpha"):
        LS.resolve_lovasz(c, 3)                                   # edge_focal_loss has weights for two classes only
    w3 = (0.2, 0.3, 0.5)
    c = LS.compound(LS.focal_loss.with_alpha(w3), l.with_options(per_image=True))
    assert LS.resolve_lovasz(c, 3)["point_alpha"] == w3 == LS.resolve_alpha(c, 3) and LS.resolve_loss(c) == SG_LOSS_FOCAL
    with pytest.raises(ValueError, match="class weights"):
        LS.resolve_lovasz(c, 2)
    with pytest.raises(ValueError, match="class weights"):
        LS.resolve_lovasz(c, 4)
    c = LS.compound(LS.binary_crossentropy, l)
    assert LS.resolve_lovasz(c, 5)["point_alpha"] is None and LS.resolve_lovasz(c, 5)["point_kind"] == SG_LOSS_CE2
    assert LS.resolve_lovasz(LS.compound(LS.focal_loss, l), 4)["point_alpha"] == (0.5,) * 4
    for C in (1, 33):
        with pytest.raises(ValueError, match="classes"):
            LS.resolve_lovasz(l, C)
    # the region compound answers as before
    r = LS.compound(LS.focal_loss, LS.dice_loss)
    assert LS.resolve_region(r, 2) is not None and LS.resolve_lovasz(r, 2) is None
    with pytest.raises(ValueError, match="the engine implements") as e:
        LS.resolve_loss("lovasz")
    assert "lovasz_loss" in str(e.value)


def test_compile_stores_the_lovasz_fields():
    from building_detection_amd import losses as LS, zoo
    m = zoo.HRNet((32, 32, 3), num_classes=3)
    m.compile(loss=LS.compound(LS.focal_loss, LS.lovasz_loss.with_options("all"), 0.25), metrics=[LS.MIoU])
    assert m.loss_kind == 1 and m.loss_region is None and m.loss_mining is None and m.last_loss_terms() is None
    assert m.loss_lovasz == dict(classes_all=True, per_image=False, point_kind=1, point_alpha=(0.5,) * 3, point_weight=1.0,
                                 lovasz_weight=0.25)
    m.compile(loss=LS.focal_loss)
    assert m.loss_lovasz is None and m.last_loss_terms() is None
    m.compile(loss=LS.lovasz_loss)
    assert m.loss_kind == LS.NO_POINTWISE and m.loss_lovasz["point_kind"] == -1 and m.loss_alpha is None


def test_descriptor_binding():
    from building_detection_amd import losses as LS
    from building_detection_amd import _lib
    from building_detection_amd.ops import Engine
    assert ctypes.sizeof(_lib.LovaszDesc) == 4 * 4 + 8 + 2 * 4 + 2 * 4 + 4 * _lib.SG_MAX_CLASSES
    assert _lib.LovaszDesc.rows_per_image.offset == 16 and _lib.LovaszDesc.point_alpha.offset == 40
    names = _lib.exported_symbols()
    for s in ("sg_sort_pairs_ws_bytes", "sg_sort_pairs_u32", "sg_loss_lovasz_ws_bytes", "sg_loss_lovasz_fwd", "sg_loss_lovasz_bwd"):
        assert s in names
    p, y6, y3 = torch.zeros(2, 8, 8, 3), torch.zeros(2, 8, 8, 6), torch.zeros(2, 8, 8, 3)
    r = LS.resolve_lovasz(LS.compound(LS.edge_focal_loss.with_alpha([0.2, 0.3, 0.5]), LS.lovasz_loss.with_options("all", True), 0.5), 3)
    d = Engine.lovasz_desc(r, p, y6)
    assert (d.C, d.y_cols, d.images, d.classes_all, d.rows_per_image, d.point_kind, d.reserved) == (3, 6, 2, 1, 64, 2, 0)
    assert (d.point_weight, d.lovasz_weight) == (1.0, 0.5) and [round(v, 6) for v in list(d.point_alpha)[:4]] == [0.2, 0.3, 0.5, 0.0]
    with pytest.raises(ValueError, match="edge_focal_loss needs"):
        Engine.lovasz_desc(r, p, y3)
    r = LS.resolve_lovasz(LS.lovasz_loss, 3)
    d = Engine.lovasz_desc(r, p, y3)
    assert (d.images, d.rows_per_image, d.classes_all, d.point_kind) == (1, 128, 0, -1)
    with pytest.raises(ValueError, match="does not go with"):
        Engine.lovasz_desc(r, p, torch.zeros(2, 8, 8, 4))
    assert Engine.lovasz_desc(r, p.reshape(-1, 3), y3.reshape(-1, 3)).images == 1          # flat rows: one group
    rp = LS.resolve_lovasz(LS.lovasz_loss.with_options(per_image=True), 3)
    assert Engine.lovasz_desc(rp, p, y3).images == 2
    with pytest.raises(ValueError, match="per_image"):                                     # ... and no image axis to split
        Engine.lovasz_desc(rp, p.reshape(-1, 3), y3.reshape(-1, 3))
    with pytest.raises(ValueError, match="class"):
        Engine.lovasz_desc(LS.resolve_lovasz(LS.compound(LS.focal_loss, LS.lovasz_loss), 4), p, y3)


def one_hot(t, C):
    return np.eye(C, dtype=np.float32)[t]


@pytest.mark.parametrize("images", (1, 3))
@pytest.mark.parametrize("C", (2, 3, 5))
def test_known_answers(C, images):
    rows = 60
    t = np.random.default_rng(C).integers(0, C, rows)
    t[:C] = np.arange(C)
    yt = one_hot(t, C)
    for all_ in (False, True):
        r = LR.lovasz_ref(yt.copy(), yt, images, all_)              # the one-hot truth: every error is 0
        assert r["loss"] == 0.0
        wrong = one_hot((t + 1) % C, C)                             # certain and wrong everywhere
        r = LR.lovasz_ref(wrong, yt, images, all_)
        assert abs(r["loss"] - 1.0) < 1e-12, r["loss"]
    # an absent class: skipped under "present", its l = max p under "all" (G = 0: g_1 = 1)
    t2 = np.where(t == C - 1, 0, t)
    p = MR.class_probs(gen(3), rows, C).numpy()
    r0, r1 = LR.lovasz_ref(p, one_hot(t2, C), 1, False), LR.lovasz_ref(p, one_hot(t2, C), 1, True)
    assert not r0["used"][0, C - 1] and r0["n_c"][0] == C - 1 and (r0["g"][:, C - 1] == 0).all()
    assert r1["used"].all() and abs(r1["l"][0, C - 1] - float(p[:, C - 1].max())) < 1e-15
    assert abs(r1["loss"] - (r0["loss"] * (C - 1) + r1["l"][0, C - 1]) / C) < 1e-15
    assert np.count_nonzero(r1["g"][:, C - 1]) == 1


def test_closed_form_equals_the_difference_form():
    rng = np.random.default_rng(11)
    for n, frac in ((1, 1.0), (2, 0.5), (7, 0.3), (64, 0.5), (257, 0.05), (300, 0.95), (40, 0.0)):
        f = rng.random(n) < frac
        if frac == 1.0:
            f[:] = True
        exact_d, exact_c = LR.gk_diff(f, exact=True), LR.gk_closed_exact(f)
        assert exact_d == exact_c, (n, frac)                       # the same rational number at every rank
        assert sum(exact_c) == (Fraction(1) if n else 0)           # J_n = 1: every pixel counted wrong
        c64 = LR.gk_closed(f)
        for k in range(n):
            assert abs(c64[k] - float(exact_c[k])) <= 2.0 ** -51 * float(exact_c[k])
        d64 = LR.gk_diff(f)
        assert np.abs(d64 - c64).max() <= 2.0 ** -51               # absolute: the difference cancels
    assert LR.gk_closed(np.zeros(5, bool)).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]


def test_keys_order_as_a_descending_stable_sort_of_the_errors():
    rows, C = 400, 3
    g = gen(5)
    p = (torch.round(MR.class_probs(g, rows, C) * 8) / 8).numpy()   # heavy ties
    p[7] = [np.nan, 0.5, 0.5]
    p[8] = [-0.0, 1.5, -0.25]
    yt = MR.class_labels(g, rows, C, C).numpy()
    t = LR.truth(yt, C)
    for c in range(C):
        f, m, key = LR.errors_and_keys(p, t, c)
        assert (m >= 0).all() and (m <= 1).all() and not np.isnan(m).any()
        assert np.array_equal(np.argsort(key, kind="stable"), np.argsort(-m, kind="stable"))
    assert LR.clamp_bits(np.float32([np.nan, -0.0, -1.0, 1.5, 1e-40, 1.0])).tolist() == [0, 0, 0, 0x3F800000, 71362, 0x3F800000]


def test_loss_is_unchanged_under_a_permutation_of_tied_pixels():
    rows, C = 300, 3
    g = gen(9)
    p = (torch.round(MR.class_probs(g, rows, C) * 8) / 8).numpy()
    yt = MR.class_labels(g, rows, C, C).numpy()
    base = LR.lovasz_ref(p, yt)
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(rows)       # moves tied pixels (and all others) about
        r = LR.lovasz_ref(p[perm], yt[perm])
        assert abs(r["loss"] - base["loss"]) <= 1e-13 * base["loss"]
    # ... while the gradient of a tied pixel does depend on its place: the stable order decides it
    assert len(np.unique(p[:, 0])) < 12


@pytest.mark.parametrize("images,all_", ((1, False), (2, True)))
def test_reference_gradient_against_central_differences(images, all_):
    rows, C = 24, 3
    g = gen(21 + images)
    p32 = MR.class_probs(g, rows, C).numpy()
    yt = MR.class_labels(g, rows, C, C).numpy()
    t = LR.truth(yt, C)
    for c in range(C):                                             # tie-free, and no error within 2h of another
        _, m, _ = LR.errors_and_keys(p32, t, c)
        assert np.diff(np.sort(m.astype(np.float64))).min() > 1e-5
    r = LR.lovasz_ref(p32, yt, images, all_)
    p, h = p32.astype(np.float64), 1e-6
    fd = np.zeros((rows, C))
    for i in range(rows):
        for c in range(C):
            hi, lo = p.copy(), p.copy()
            hi[i, c] += h
            lo[i, c] -= h
            fd[i, c] = (LR.lovasz_ref(p32, yt, images, all_, p64=hi)["loss"] - LR.lovasz_ref(p32, yt, images, all_, p64=lo)["loss"]) / (2 * h)
    err, scale = np.abs(r["g"] - fd).max(), np.abs(r["g"]).max()
    print(f"max |g - fd| = {err:.3e} = {err / scale:.2e} of max |g| {scale:.3e}")
    assert err <= FD_BOUND * scale
    assert abs(LR.lovasz_ref(p32, yt, images, all_, p64=p)["loss"] - r["loss"]) < 1e-6
