"""Losses and metrics of train_model/DeepLabv3plus.py:490-623 as the engine sees them.

`model.compile(loss=edge_focal_loss, metrics=[PA, IoU, MIoU, F1_score])` (DeepLabv3plus.py:834-837) passes
Python callables.  The engine does not trace tf ops: it recognises the three losses and four metrics of the
reference by name (these objects, or any callable with the same `__name__`, e.g. the reference's own
functions) and runs the fused HIP kernels `sg_loss_fwd/bwd` and `sg_confusion_counts` instead.

A model of C > 2 classes runs `sg_lossn_fwd/bwd` and `sg_confusion_matrix`: the focal losses then carry one weight per
class (`focal_loss.with_alpha([...])`, `edge_focal_loss.with_alpha([...])`), and the four metrics come from the C x C
matrix (`metrics_from_matrix`).

Beyond the reference: the region-overlap losses `dice_loss`, `jaccard_loss`, `tversky_loss(alpha, beta)` and
`compound(pointwise, region)`, which adds one of them to one of the three losses above (`sg_loss_region_fwd/bwd`, at 2 ... 32
classes), and `hard_mining(pointwise, thresh, min_kept)`, one of the three averaged over the batch's hard pixels
only (`sg_loss_mined_fwd/bwd`), and `lovasz_loss`, the Lovasz-Softmax surrogate of the Jaccard index, alone or
as the second term of `compound` (`sg_loss_lovasz_fwd/bwd` on a stable segmented radix sort).
"""
from __future__ import annotations

import warnings

import numpy as np

from ._lib import SG_LOSS_CE2, SG_LOSS_FOCAL, SG_LOSS_EDGE_FOCAL, SG_MAX_CLASSES

K_EPSILON = 1e-7

_LOSS_KINDS = {
    "binary_crossentropy": SG_LOSS_CE2,   # 2-class categorical CE on softmax outputs, eps inside the log (:490-499)
    "focal_loss": SG_LOSS_FOCAL,          # alpha = (.5,.5), gamma = 2 (:502-512)
    "edge_focal_loss": SG_LOSS_EDGE_FOCAL,  # alpha = (.35,.65), gamma = 2, edge weights y_true[...,2:4] (:515-527)
}
_METRICS = ("PA", "IoU", "MIoU", "F1_score")


class _Named:
    def __init__(self, name, doc):
        self.__name__ = name
        self.__doc__ = doc

    def __call__(self, y_true, y_pred):
        raise RuntimeError(
            f"{self.__name__} is evaluated by the engine's fused kernel inside Model.train_on_batch/test_on_batch; "
            "pass it to model.compile(...) rather than calling it")

    def __repr__(self):
        return f"<building_detection_amd {self.__name__}>"


class _FocalLoss(_Named):
    """A focal loss that may carry its per-class weights: `with_alpha(seq)` returns an object of the same `__name__`
    (compile() selects the kernel by it, as ever) whose `alpha` the model reads - nothing global changes."""

    alpha = None

    def with_alpha(self, alpha):
        a = tuple(float(v) for v in alpha)
        if not a or any(not np.isfinite(v) for v in a):
            raise ValueError(f"{self.__name__}.with_alpha: {alpha!r} is not a list of finite class weights")
        out = _FocalLoss(self.__name__, self.__doc__)
        out.alpha = a
        return out

    def __repr__(self):
        return f"<building_detection_amd {self.__name__}{'' if self.alpha is None else ' alpha=' + repr(self.alpha)}>"


binary_crossentropy = _Named("binary_crossentropy", "CE on softmax probabilities (DeepLabv3plus.py:490-499)")
focal_loss = _FocalLoss("focal_loss", "focal loss, alpha = .5 for every class, gamma=2 (DeepLabv3plus.py:502-512)")
edge_focal_loss = _FocalLoss("edge_focal_loss", "edge-weighted focal loss, alpha=(.35,.65) at 2 classes (DeepLabv3plus.py:515-527)")


def _finite(v):
    try:
        v = float(v)
    except (TypeError, ValueError):
        return None
    return v if np.isfinite(v) else None


class _RegionLoss(_Named):
    """A region-overlap loss (no counterpart in the reference).  Per group g - the batch, or one image with
    `per_image` - and class c, with I = sum p y, P = sum p, Y = sum y over the group's pixels:

        T = (I + smooth) / (I + alpha (P - I) + beta (Y - I) + smooth),   l[g,c] = (1 - T)^gamma,
        L = sum_g sum_c w_c l[g,c] / (G * sum_c w_c).

    alpha = beta = .5 is Dice, T = (2 I + 2 smooth) / (P + Y + 2 smooth): `smooth` here is HALF the smoothing constant of the
    usual Dice notation.  alpha = beta = 1 is Jaccard (soft IoU); gamma > 1 is the focal-Tversky form."""

    smooth, gamma, class_weights, per_image = 1.0, 1.0, None, False

    def __init__(self, name, doc, alpha, beta):
        super().__init__(name, doc)
        a, b = _finite(alpha), _finite(beta)
        if a is None or b is None or a < 0 or b < 0:
            raise ValueError(f"{name}: alpha = {alpha!r}, beta = {beta!r} must be finite and >= 0")
        self.alpha, self.beta = a, b

    def with_options(self, smooth=1.0, gamma=1.0, class_weights=None, per_image=False):
        s, g = _finite(smooth), _finite(gamma)
        if s is None or s <= 0:
            raise ValueError(f"{self.__name__}.with_options: smooth = {smooth!r} must be finite and > 0")
        if g is None or g < 1:
            raise ValueError(f"{self.__name__}.with_options: gamma = {gamma!r} must be finite and >= 1")
        w = None
        if class_weights is not None:
            w = tuple(_finite(v) for v in class_weights)
            if not w or any(v is None or v < 0 for v in w) or not sum(w) > 0:
                raise ValueError(f"{self.__name__}.with_options: class_weights = {class_weights!r} must be finite, >= 0 and "
                                 "have a positive sum")
        out = _RegionLoss(self.__name__, self.__doc__, self.alpha, self.beta)
        out.smooth, out.gamma, out.class_weights, out.per_image = s, g, w, bool(per_image)
        return out

    def __repr__(self):
        return (f"<building_detection_amd {self.__name__} alpha={self.alpha} beta={self.beta} smooth={self.smooth} "
                f"gamma={self.gamma} class_weights={self.class_weights} per_image={self.per_image}>")


dice_loss = _RegionLoss("dice_loss", "soft Dice loss: 1 - (2 I + 2 smooth) / (P + Y + 2 smooth) per class", 0.5, 0.5)
jaccard_loss = _RegionLoss("jaccard_loss", "soft Jaccard (IoU) loss: 1 - (I + smooth) / (P + Y - I + smooth) per class", 1.0, 1.0)


def tversky_loss(alpha, beta):
    """Tversky loss: alpha weighs the false positives P - I, beta the false negatives Y - I."""
    return _RegionLoss("tversky_loss", "Tversky loss: 1 - (I + smooth) / (I + alpha (P - I) + beta (Y - I) + smooth) per class",
                       alpha, beta)


class _LovaszLoss(_Named):
    """Lovasz-Softmax (Berman, Triggs, Blaschko, CVPR 2018), the tight convex surrogate of the Jaccard index.
    Per group g - the batch, or one image with `per_image` - and class c: the pixels' errors m = 1 - p (a pixel of class c) or
    p (any other) are ranked in descending order, ties by ascending pixel index, and

        l[g,c] = sum_k m_(k) (J_k - J_(k-1)),   J_k = the Jaccard loss of calling the first k ranked pixels wrong,
        L = mean over the groups of the mean of l[g,c] over the classes.

    classes="present" averages over the classes that occur in the group, "all" over every class."""

    classes, per_image = "present", False

    def with_options(self, classes="present", per_image=False):
        if classes not in ("present", "all"):
            raise ValueError(f"{self.__name__}.with_options: classes = {classes!r} is not 'present' or 'all'")
        if not isinstance(per_image, (bool, np.bool_)):
            raise ValueError(f"{self.__name__}.with_options: per_image = {per_image!r} is not a bool")
        out = _LovaszLoss(self.__name__, self.__doc__)
        out.classes, out.per_image = classes, bool(per_image)
        return out

    def __repr__(self):
        return f"<building_detection_amd {self.__name__} classes={self.classes!r} per_image={self.per_image}>"


lovasz_loss = _LovaszLoss("lovasz_loss", _LovaszLoss.__doc__)


class _MinedLoss(_Named):
    """A pointwise loss averaged over the hard pixels of the batch only (online hard example mining)."""

    def __init__(self, pointwise, thresh, min_kept):
        super().__init__(f"hard_mining({pointwise.__name__})", self.__doc__)
        self.pointwise, self.thresh, self.min_kept = pointwise, thresh, min_kept

    def __repr__(self):
        return f"<building_detection_amd hard_mining({self.pointwise!r}, thresh={self.thresh}, min_kept={self.min_kept})>"


def hard_mining(pointwise, thresh=0.7, min_kept=0.1):
    """`pointwise` (binary_crossentropy, focal_loss or edge_focal_loss, with or without with_alpha) averaged over the hard
    pixels only.  A pixel's key q is the probability the network gives its TRUE class; with q_(k) the k-th smallest key of the
    batch,

        T = max(thresh, q_(k)),   a pixel is kept iff q <= T,   L = sum of the kept pixels' terms / number of kept pixels.

    Every tie at T is kept, so at least k pixels always are and the set depends on no order.  (The published
    OhemCrossEntropy / OHEMPixelSampler compare with `<` and can drop the k-th pixel itself: a deliberate difference.)
    thresh in [0, 1]: 1 keeps every pixel (the plain loss), 0 is pure top-k.  min_kept: a float in (0, 1] is a fraction of the
    batch's pixels, k = min(rows, max(1, ceil(f * rows))); an int >= 1 is a pixel count, k = min(rows, n)."""
    if isinstance(pointwise, _MinedLoss) or not isinstance(pointwise, _Named) or pointwise.__name__ not in _LOSS_KINDS:
        raise ValueError(f"hard_mining: pointwise = {pointwise!r} is not one of {sorted(_LOSS_KINDS)}")
    t = None if isinstance(thresh, bool) else _finite(thresh)
    if t is None or not 0.0 <= t <= 1.0:
        raise ValueError(f"hard_mining: thresh = {thresh!r} must be finite and in [0, 1]")
    if isinstance(min_kept, (bool, np.bool_)):
        k = None
    elif isinstance(min_kept, (int, np.integer)):
        k = int(min_kept) if min_kept >= 1 else None
    elif isinstance(min_kept, (float, np.floating)):
        k = float(min_kept) if 0.0 < min_kept <= 1.0 else None      # a NaN fails both
    else:
        k = None
    if k is None:
        raise ValueError(f"hard_mining: min_kept = {min_kept!r} must be a float in (0, 1] (a fraction of the batch's pixels) or "
                         "an int >= 1 (a pixel count)")
    return _MinedLoss(pointwise, t, k)


def mined_rows(min_kept, rows: int) -> int:
    """k of a batch of `rows` pixels: a float is a fraction, k = min(rows, max(1, ceil(f * rows))); an int a count, min(rows, n)."""
    if isinstance(min_kept, float):
        return min(rows, max(1, int(np.ceil(min_kept * rows))))
    return min(rows, int(min_kept))


class _CompoundLoss(_Named):
    """pointwise_weight * pointwise + region_weight * region, evaluated by ONE forward and ONE backward pass."""

    def __init__(self, pointwise, region, region_weight, pointwise_weight):
        super().__init__(f"{pointwise.__name__}+{region.__name__}", self.__doc__)
        self.pointwise, self.region, self.region_weight, self.pointwise_weight = pointwise, region, region_weight, pointwise_weight

    def __repr__(self):
        return f"<building_detection_amd {self.pointwise_weight} * {self.pointwise!r} + {self.region_weight} * {self.region!r}>"


def compound(pointwise, region, region_weight=1.0, pointwise_weight=1.0):
    """`pointwise` is binary_crossentropy, focal_loss or edge_focal_loss (with or without with_alpha), `region` one of
    dice_loss / jaccard_loss / tversky_loss(...) or lovasz_loss.  The weights are >= 0 and not both 0."""
    if isinstance(pointwise, _MinedLoss):
        raise ValueError(f"compound: pointwise = {pointwise!r}: a mined pointwise term inside a compound is not implemented")
    if not isinstance(pointwise, _Named) or pointwise.__name__ not in _LOSS_KINDS:
        raise ValueError(f"compound: pointwise = {pointwise!r} is not one of {sorted(_LOSS_KINDS)}")
    if not isinstance(region, (_RegionLoss, _LovaszLoss)):
        raise ValueError(f"compound: region = {region!r} is not dice_loss, jaccard_loss, a tversky_loss(...) or lovasz_loss")
    wr, wp = _finite(region_weight), _finite(pointwise_weight)
    if wr is None or wp is None or wr < 0 or wp < 0 or wr + wp == 0:
        raise ValueError(f"compound: region_weight = {region_weight!r}, pointwise_weight = {pointwise_weight!r} must be finite, "
                         ">= 0 and not both 0")
    return _CompoundLoss(pointwise, region, wr, wp)


NO_POINTWISE = -1   # sg_region_desc.point_kind of a region loss on its own

PA = _Named("PA", "pixel accuracy (DeepLabv3plus.py:530-553)")
IoU = _Named("IoU", "foreground IoU (DeepLabv3plus.py:556-575)")
MIoU = _Named("MIoU", "mean of foreground / background IoU (DeepLabv3plus.py:578-598)")
F1_score = _Named("F1_score", "F1 (DeepLabv3plus.py:601-623)")


class ForeignCallableWarning(UserWarning):
    """A loss / metric callable that is not the engine's own object was selected BY NAME."""


def _warn_foreign(fn, what, lines):
    """The reference's training scripts hand their own Python functions to compile() (DeepLabv3plus.py:834-837).  The engine
    never runs their bodies: it picks its fused kernel by `__name__`.  An EDITED edge_focal_loss would therefore train with
    the stock formula - say so, once per compile, instead of doing it silently."""
    if isinstance(fn, (str, _Named)):
        return
    warnings.warn(
        f"{what} {getattr(fn, '__name__', fn)!r} is a foreign callable ({getattr(fn, '__module__', '?')}): the engine selects its "
        f"fused kernel by NAME and evaluates the stock formula of train_model/DeepLabv3plus.py:{lines}; the body of the "
        "callable is never executed, so any edit to it has no effect", ForeignCallableWarning, stacklevel=4)


def resolve_loss(loss) -> int:
    """The pointwise kind of `loss`: SG_LOSS_* for the reference's three names (and for the pointwise part of a compound),
    NO_POINTWISE for a region loss or lovasz_loss on its own; for hard_mining(pointwise) the kind of `pointwise`."""
    if isinstance(loss, (_CompoundLoss, _MinedLoss)):
        return _LOSS_KINDS[loss.pointwise.__name__]
    if isinstance(loss, (_RegionLoss, _LovaszLoss)):
        return NO_POINTWISE
    name = loss if isinstance(loss, str) else getattr(loss, "__name__", None)
    if name not in _LOSS_KINDS:
        raise ValueError(f"loss {loss!r}: the engine implements {sorted(_LOSS_KINDS)} (train_model/DeepLabv3plus.py:490-527), "
                         "dice_loss, jaccard_loss, tversky_loss(alpha, beta), lovasz_loss, compound(pointwise, region) and "
                         "hard_mining(pointwise)")
    _warn_foreign(loss, "loss", "490-527")
    return _LOSS_KINDS[name]


_TWO_CLASS_ALPHA = {SG_LOSS_FOCAL: (0.5, 0.5), SG_LOSS_EDGE_FOCAL: (0.35, 0.65)}   # what the 2-class kernels have built in


def _pointwise(pointwise, num_classes: int):
    """(kind, alpha) of a compound's or mined loss's pointwise term; alpha: None (cross-entropy) or `num_classes` weights."""
    kind = _LOSS_KINDS[pointwise.__name__]
    alpha = resolve_alpha(pointwise, num_classes)
    if alpha is None and kind != SG_LOSS_CE2:
        alpha = _TWO_CLASS_ALPHA[kind]
    return kind, alpha


def resolve_region(loss, num_classes: int):
    """The fields of `sg_region_desc` that `loss` fixes for a `num_classes` model, or None for a loss without a region term:
    dict(a, b, smooth, gamma, class_w, per_image, point_kind, point_alpha, point_weight, region_weight).  class_w has
    `num_classes` entries (ones when none were given); point_alpha is None (no pointwise term, or cross-entropy) or
    `num_classes` weights - at two classes without with_alpha the reference's own, passed explicitly."""
    if isinstance(loss, _CompoundLoss) and isinstance(loss.region, _LovaszLoss):
        return None                                               # resolve_lovasz answers for it
    if isinstance(loss, _CompoundLoss):
        region, (kind, alpha) = loss.region, _pointwise(loss.pointwise, num_classes)
        wp, wr = loss.pointwise_weight, loss.region_weight
    elif isinstance(loss, _RegionLoss):
        region, kind, alpha, wp, wr = loss, NO_POINTWISE, None, 0.0, 1.0
    else:
        return None
    w = region.class_weights
    if w is None:
        w = (1.0,) * num_classes
    elif len(w) != num_classes:
        raise ValueError(f"the loss carries {len(w)} class weights, the model has {num_classes} classes")
    return dict(a=region.alpha, b=region.beta, smooth=region.smooth, gamma=region.gamma, class_w=tuple(w),
                per_image=region.per_image, point_kind=kind, point_alpha=alpha, point_weight=wp, region_weight=wr)


def resolve_lovasz(loss, num_classes: int):
    """The fields of `sg_lovasz_desc` that `loss` fixes for a `num_classes` model, or None for a loss without a Lovasz term:
    dict(classes_all, per_image, point_kind, point_alpha, point_weight, lovasz_weight).  point_alpha is None (no pointwise
    term, or cross-entropy) or `num_classes` weights - at two classes without with_alpha the reference's own, passed
    explicitly."""
    if isinstance(loss, _CompoundLoss) and isinstance(loss.region, _LovaszLoss):
        lov, (kind, alpha) = loss.region, _pointwise(loss.pointwise, num_classes)
        wp, wl = loss.pointwise_weight, loss.region_weight
    elif isinstance(loss, _LovaszLoss):
        lov, kind, alpha, wp, wl = loss, NO_POINTWISE, None, 0.0, 1.0
    else:
        return None
    if not 2 <= int(num_classes) <= SG_MAX_CLASSES:
        raise ValueError(f"lovasz_loss: the model has {num_classes} classes, the engine takes 2 ... {SG_MAX_CLASSES}")
    return dict(classes_all=lov.classes == "all", per_image=lov.per_image, point_kind=kind, point_alpha=alpha, point_weight=wp,
                lovasz_weight=wl)


def resolve_mining(loss, num_classes: int):
    """The fields of `sg_mine_desc` that `loss` fixes for a `num_classes` model, or None for a loss that is not mined:
    dict(kind, alpha, thresh, min_kept).  alpha is None (cross-entropy) or `num_classes` weights - at two classes without
    with_alpha the reference's own, passed explicitly; min_kept is the fraction (float) or the count (int) as given:
    `mined_rows` turns it into the k of a batch."""
    if not isinstance(loss, _MinedLoss):
        return None
    kind, alpha = _pointwise(loss.pointwise, num_classes)
    return dict(kind=kind, alpha=alpha, thresh=loss.thresh, min_kept=loss.min_kept)


def resolve_alpha(loss, num_classes: int):
    """The per-class weights `loss` trains a `num_classes` model with: None = what the 2-class kernels have built in
    (no weights given, 2 classes; cross-entropy has none at all), else a tuple of `num_classes` floats."""
    if isinstance(loss, (_CompoundLoss, _MinedLoss)):
        return resolve_alpha(loss.pointwise, num_classes)
    if isinstance(loss, (_RegionLoss, _LovaszLoss)):
        return None
    kind = _LOSS_KINDS[loss if isinstance(loss, str) else getattr(loss, "__name__", None)]
    alpha = getattr(loss, "alpha", None)
    if kind == SG_LOSS_CE2:
        return None
    if alpha is None:
        if num_classes == 2:
            return None
        if kind == SG_LOSS_EDGE_FOCAL:
            raise ValueError(f"edge_focal_loss has class weights for 2 classes only ((.35, .65), DeepLabv3plus.py:515-527): "
                             f"compile a {num_classes}-class model with loss=edge_focal_loss.with_alpha([...{num_classes} weights])")
        return (0.5,) * num_classes
    alpha = tuple(float(a) for a in alpha)
    if len(alpha) != num_classes:
        raise ValueError(f"the loss carries {len(alpha)} class weights, the model has {num_classes} classes")
    return alpha


def resolve_metric(metric) -> str:
    name = metric if isinstance(metric, str) else getattr(metric, "__name__", None)
    if name not in _METRICS:
        raise ValueError(f"metric {metric!r}: the engine implements {_METRICS} (train_model/DeepLabv3plus.py:530-623)")
    _warn_foreign(metric, "metric", "530-623")
    return name


def metrics_from_counts(tp: int, tn: int, fp: int, fn: int) -> dict:
    """The reference casts the int32 counts to float32 and divides with +epsilon (DeepLabv3plus.py:547-598,
    614-623); the same float32 arithmetic is done here on the host from the exact device counts."""
    f = np.float32
    tp, tn, fp, fn, e = f(tp), f(tn), f(fp), f(fn), f(K_EPSILON)
    pa = (tp + tn) / (tp + tn + fp + fn + e)
    iou = tp / (tp + fp + fn + e)
    miou = (tp / (tp + fp + fn + e) + tn / (tn + fp + fn + e)) / f(2)
    recall, precision = tp / (tp + fn + e), tp / (tp + fp + e)
    f1 = (f(2.0) * precision * recall) / (precision + recall + e)
    return {"PA": float(pa), "IoU": float(iou), "MIoU": float(miou), "F1_score": float(f1)}


def metrics_from_matrix(M) -> dict:
    """The four metrics from the C x C count matrix M[truth][prediction], in the float32 arithmetic with +epsilon of
    metrics_from_counts (to which every one of them reduces bit for bit at C = 2, where M = [[TN, FP], [FN, TP]]):

        PA = trace / total;  per class  IoU_c = M_cc / (row_c + col_c - M_cc + e),  recall_c = M_cc / (row_c + e),
        precision_c = M_cc / (col_c + e),  F1_c = 2 precision_c recall_c / (precision_c + recall_c + e);
        IoU = mean of IoU_c over the foreground classes 1 ... C-1,  F1_score = mean of F1_c over the same,
        MIoU = mean of IoU_c over all classes.  `IoU_per_class` and `F1_per_class` hold the lists.

    Sums run diagonal first, then the cells above it, then those below it (each in row-major order): the order in which
    the reference adds TP, TN, FP, FN."""
    f = np.float32
    M = np.asarray(M)
    if M.ndim != 2 or M.shape[0] != M.shape[1] or M.shape[0] < 2:
        raise ValueError(f"metrics_from_matrix: a C x C matrix with C >= 2, not {M.shape}")
    C = M.shape[0]
    m = [[f(int(M[t][q])) for q in range(C)] for t in range(C)]
    e = f(K_EPSILON)

    def fsum(vals):
        s = f(0.0)
        for v in vals:
            s = s + v
        return s

    trace = fsum([m[c][c] for c in reversed(range(C))])      # TP + TN at two classes
    upper = [m[t][q] for t in range(C) for q in range(t + 1, C)]
    lower = [m[t][q] for t in range(C) for q in range(t)]
    total = trace
    for v in upper + lower:
        total = total + v
    pa = trace / (total + e)
    iou, f1 = [], []
    for c in range(C):
        up = [m[t][c] for t in range(c)] + [m[c][q] for q in range(c + 1, C)]        # cells above the diagonal that involve c
        lo = [m[c][q] for q in range(c)] + [m[t][c] for t in range(c + 1, C)]        # ... and below it
        den = m[c][c]
        for v in up + lo:
            den = den + v
        iou.append(m[c][c] / (den + e))
        row = m[c][c]
        for q in range(C):
            if q != c:
                row = row + m[c][q]
        col = m[c][c]
        for t in range(C):
            if t != c:
                col = col + m[t][c]
        recall, precision = m[c][c] / (row + e), m[c][c] / (col + e)
        f1.append((f(2.0) * precision * recall) / (precision + recall + e))
    fg = list(reversed(range(1, C)))
    miou = fsum([iou[c] for c in reversed(range(C))]) / f(C)
    return {"PA": float(pa), "IoU": float(fsum([iou[c] for c in fg]) / f(len(fg))), "MIoU": float(miou),
            "F1_score": float(fsum([f1[c] for c in fg]) / f(len(fg))),
            "IoU_per_class": [float(v) for v in iou], "F1_per_class": [float(v) for v in f1]}
