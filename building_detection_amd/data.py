"""Seeded synthetic tiles shaped like the reference's generator output (train_model/DeepLabv3plus.py:32-107).

x: uint8 RGB noise -> `/127.5 - 1` float32 [N,H,W,3] (decode_img, :36-37).
y: [N,H,W,4] = one-hot(background, building), f_edge weight, p_edge weight, built like train_data_gen
(:70-100): the binary mask comes from random filled rectangles; `erode`/`dilate` with a 3x3 kernel, 5
iterations, restated with scipy min/max filters (OpenCV is not available): cv.erode pads with +inf, cv.dilate
with -inf; p_edge = 2 where mask - erode == 1 (inner building rim), f_edge = 2 where dilate - mask == 1 (outer
rim), else 1; channel order (one_hot, f_edge, p_edge) as in `np.concatenate` at :100.

`num_classes=C` > 2: every rectangle gets a class in 1 ... C-1 and y is [N,H,W,2C] = one-hot C, then one edge weight per class
(class_edge_weights: 2 on a pixel of class c whose 11 x 11 window holds another class - the same rule, said per class).
"""
from __future__ import annotations

import numpy as np


def edge_weight_channels(mask: np.ndarray):
    from scipy import ndimage
    m = mask.astype(np.float32)
    er, di = m, m
    for _ in range(5):
        er = ndimage.minimum_filter(er, size=3, mode="constant", cval=np.inf)
        di = ndimage.maximum_filter(di, size=3, mode="constant", cval=-np.inf)
    p_edge = np.where((m - er) == 1, 2.0, 1.0)
    f_edge = np.where((di - m) == 1, 2.0, 1.0)
    return f_edge, p_edge


def check_separation(separation):
    """`separation=(w0, sigma)` of the generators and Engine.edge_labels -> (float w0, float sigma); w0 >= 0, sigma > 0, finite."""
    try:
        w0, sigma = (float(v) for v in separation)
    except (TypeError, ValueError):
        raise ValueError(f"separation = {separation!r}: expected (w0, sigma)") from None
    if not (np.isfinite(w0) and np.isfinite(sigma) and w0 >= 0.0 and sigma > 0.0):
        raise ValueError(f"separation = ({w0}, {sigma}): w0 >= 0 and sigma > 0, both finite")
    return w0, sigma


def separation_term(mask: np.ndarray, w0: float = 10.0, sigma: float = 5.0) -> np.ndarray:
    """The U-Net border weight (Ronneberger et al. 2015) of a binary building mask [H,W] (non-zero = building), float64:
    w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) on background pixels, d1 / d2 the Euclidean distances in pixels to the nearest and the
    second-nearest distinct building (8-connected, as findContours and the clean-up count buildings); 0 on buildings and
    where the tile holds fewer than two.  The term is large only in narrow gaps between two buildings.  It is ADDED to
    f_edge (channel 2 of y), which edge_focal_loss multiplies into its background term.  One distance_transform_edt per
    building: the host definition of sg_object_distances + sg_separation_weights (Engine.edge_labels(separation=...))."""
    from scipy import ndimage
    w0, sigma = check_separation((w0, sigma))
    m = np.asarray(mask) != 0
    if m.ndim != 2:
        raise ValueError(f"separation_term: a mask is [H, W], got {m.shape}")
    lab, n = ndimage.label(m, structure=np.ones((3, 3), np.int8))
    out = np.zeros(m.shape, np.float64)
    if n < 2:
        return out
    d1 = np.full(m.shape, np.inf)
    d2 = np.full(m.shape, np.inf)
    for k in range(1, n + 1):
        d = ndimage.distance_transform_edt(lab != k)
        d2 = np.minimum(d2, np.maximum(d1, d))
        d1 = np.minimum(d1, d)
    bg = ~m
    out[bg] = w0 * np.exp(-((d1[bg] + d2[bg]) ** 2) / (2.0 * sigma * sigma))
    return out


def class_edge_weights(class_map: np.ndarray, num_classes: int) -> np.ndarray:
    """[H,W] integer class map -> [H,W,C] edge weights: w_c = 2 where the pixel is of class c and its 11 x 11 in-image window
    (five 3 x 3 iterations) holds a pixel of another class, else 1.  At C = 2 this is (f_edge, p_edge) of
    edge_weight_channels: `dilate(fg) - fg == 1` says the same of class 0 as `fg - erode(fg) == 1` says of class 1."""
    from scipy import ndimage
    cm = np.asarray(class_map)
    w = np.ones(cm.shape + (num_classes,), np.float32)
    for c in range(num_classes):
        other = ndimage.maximum_filter((cm != c).astype(np.uint8), size=11, mode="constant", cval=0)
        w[..., c] = np.where((cm == c) & (other == 1), 2.0, 1.0)
    return w


def _synthetic_multiclass(n, h, w, seed, num_classes):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8).astype(np.float32) / 127.5 - 1.0
    y = np.empty((n, h, w, 2 * num_classes), np.float32)
    for i in range(n):
        cm = np.zeros((h, w), np.int64)
        for _ in range(int(rng.integers(3, 13))):
            rh = int(rng.integers(max(h // 32, 2), max(h // 4, 3)))
            rw = int(rng.integers(max(w // 32, 2), max(w // 4, 3)))
            r0, c0 = int(rng.integers(0, h - rh)), int(rng.integers(0, w - rw))
            cm[r0:r0 + rh, c0:c0 + rw] = int(rng.integers(1, num_classes))   # a later rectangle covers an earlier one
        y[i, ..., :num_classes] = np.eye(num_classes, dtype=np.float32)[cm]
        y[i, ..., num_classes:] = class_edge_weights(cm, num_classes)
    return x.astype(np.float32), y


def synthetic_batch(n: int, h: int = 512, w: int = 512, seed: int = 1103, num_classes: int = 2):
    """num_classes > 2: every rectangle gets a class in 1 ... C-1 and y is [N,H,W,2C] = one-hot C, then the per-class edge
    weights of class_edge_weights.  The default draws exactly what it always drew."""
    if num_classes != 2:
        if num_classes < 2:
            raise ValueError(f"num_classes = {num_classes}")
        return _synthetic_multiclass(n, h, w, seed, num_classes)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8).astype(np.float32) / 127.5 - 1.0
    y = np.empty((n, h, w, 4), np.float32)
    for i in range(n):
        mask = np.zeros((h, w), np.float32)
        for _ in range(int(rng.integers(3, 13))):
            rh = int(rng.integers(max(h // 32, 2), max(h // 4, 3)))
            rw = int(rng.integers(max(w // 32, 2), max(w // 4, 3)))
            r0, c0 = int(rng.integers(0, h - rh)), int(rng.integers(0, w - rw))
            mask[r0:r0 + rh, c0:c0 + rw] = 1.0
        f_edge, p_edge = edge_weight_channels(mask)
        y[i, ..., 0], y[i, ..., 1], y[i, ..., 2], y[i, ..., 3] = 1.0 - mask, mask, f_edge, p_edge
    return x.astype(np.float32), y
