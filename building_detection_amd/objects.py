"""Per-building evaluation of a scene: how many true buildings were found, how many predicted ones are real, by size.

    label(map, connectivity=8)         -> (labels i32 device tensor, object table numpy [n, 8])      sg_objects_label
    distances(map, connectivity=8)     -> (d1sq, d2sq) i32 device tensors: squared distance to the two nearest objects  sg_object_distances
    overlaps(labels_a, labels_b)       -> numpy [n_pairs, 3] = (a, b, intersection px), sorted         sg_objects_overlap
    match(pairs, table_pred, table_truth, iou=0.5, ...)   greedy IoU matching, exact integers (host)
    ObjectScores(iou=0.5, bins=...)    accumulator over scenes: .update(pred, truth), .result()
    pipeline.evaluate_objects(pred, truth)   the one-call form

An object is a connected set of pixels of equal non-zero value: a building of a 0/255 mask, a building of one class of a class
map (what pipeline.detection / detection_soft return for a model of more than two classes).  Objects are numbered by their
first pixel in raster order, so the table of a scene is the same in every run.  Table row: first pixel, area in pixels, x0, y0,
x1, y1 (inclusive), value, 0.

The image-wide work (labelling, intersection counts) runs on the GPU (csrc/objects.hip); the matching works on the few
thousand rows that come back and never compares floats: an IoU is the pair of integers (I, U), the threshold a fraction, every
comparison a cross-multiplication.  There is no CPU path for the image-wide part.
"""
from __future__ import annotations

import ctypes as C
from fractions import Fraction
from functools import cmp_to_key

import numpy as np

from . import _lib

AREA_BINS = (150, 300, 3000, 8000, 15000)  # the area tiers by which edge_3.py:364-376 picks a building's outline treatment


def _dev_map(m, eng):
    """uint8 [H, W] device tensor of a mask / class map: uint8 is taken as it is (class indices or 0/255), any other dtype
    counts as binary; [H, W, 3] -> channel 0 (as cleanup._dev)."""
    import torch
    t = m.to(eng.device) if isinstance(m, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(m)).to(eng.device)
    if t.dim() == 3:
        t = t[..., 0]
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"objects: a map is [H, W] or [H, W, 3] and not empty, got {tuple(t.shape)}")
    if t.dtype != torch.uint8:
        t = (t != 0).to(torch.uint8) * 255
    return t.contiguous()


def _pow2_at_least(n: int) -> int:
    return 1 << max(0, int(n) - 1).bit_length()


def label(map, connectivity: int = 8, engine=None, max_objs: int = 1 << 14):
    """-> (labels int32 device tensor [H, W]: object number or -1, object table as a numpy array [n, 8]).
    `max_objs` only sizes the first attempt: a scene with more objects is labelled again with a table that holds them."""
    import torch
    from .ops import get_engine
    if connectivity not in (4, 8):
        raise ValueError(f"objects.label: connectivity {connectivity} (4 or 8)")
    eng = engine or get_engine(0)
    m = _dev_map(map, eng)
    h, w = m.shape
    lib = eng.lib
    max_objs = max(1, int(max_objs))
    with eng.lock:
        ws = torch.empty(lib.sg_objects_label_ws_bytes(h, w), dtype=torch.uint8, device=eng.device)
        labels = torch.empty(h, w, dtype=torch.int32, device=eng.device)
        count = torch.zeros(1, dtype=torch.int32, device=eng.device)
        while True:
            table = torch.empty(max_objs, 8, dtype=torch.int32, device=eng.device)
            _lib.check(lib.sg_objects_label(eng.h, eng.stream, h, w, C.c_void_p(m.data_ptr()), 1 if connectivity == 8 else 0,
                                            C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(labels.data_ptr()),
                                            C.c_void_p(table.data_ptr()), max_objs, C.c_void_p(count.data_ptr())),
                       "sg_objects_label")
            n = int(count.item())
            if n <= max_objs:
                break
            max_objs = _pow2_at_least(n)
        return labels, table[:n].cpu().numpy()


def distances(map, connectivity: int = 8, second: bool = True, engine=None):
    """label(map, connectivity), then the exact squared Euclidean distance of every pixel to the nearest object (d1sq, 0 on an
    object) and to the nearest object other than that one (d2sq): int32 device tensors [H, W], 0x7fffffff where there is no
    such object.  second=False -> (d1sq, None): the plain exact distance transform of the map's background.  On a class map
    the objects are the regions of equal value, as for label."""
    import torch
    from .ops import get_engine
    if connectivity not in (4, 8):
        raise ValueError(f"objects.distances: connectivity {connectivity} (4 or 8)")
    eng = engine or get_engine(0)
    m = _dev_map(map, eng)
    h, w = m.shape
    lib = eng.lib
    with eng.lock:
        ws = torch.empty(lib.sg_objects_label_ws_bytes(h, w), dtype=torch.uint8, device=eng.device)
        labels = torch.empty(h, w, dtype=torch.int32, device=eng.device)
        row = torch.empty(1, 8, dtype=torch.int32, device=eng.device)   # labels are written whatever max_objs is: the table
        count = torch.empty(1, dtype=torch.int32, device=eng.device)    # and the count are never read
        _lib.check(lib.sg_objects_label(eng.h, eng.stream, h, w, C.c_void_p(m.data_ptr()), 1 if connectivity == 8 else 0,
                                        C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(labels.data_ptr()),
                                        C.c_void_p(row.data_ptr()), 1, C.c_void_p(count.data_ptr())), "sg_objects_label")
        return eng.object_distances(labels, second=second)


def overlaps(labels_a, labels_b, engine=None, slots: int = 1 << 12):
    """Every pair (a, b) of objects of two label maps that share pixels, with the number of shared pixels: numpy int32
    [n_pairs, 3], sorted by (a, b).  `slots` sizes the first attempt of the device hash table (rounded up to a power of two); it is
    doubled until no pixel is lost."""
    import torch
    from .ops import get_engine
    eng = engine or get_engine(0)
    la = labels_a.to(eng.device).contiguous()
    lb = labels_b.to(eng.device).contiguous()
    if la.dtype != torch.int32 or lb.dtype != torch.int32 or la.dim() != 2 or la.shape != lb.shape or la.numel() == 0:
        raise ValueError(f"objects.overlaps: two int32 label maps of one shape, got {la.dtype} {tuple(la.shape)} and "
                         f"{lb.dtype} {tuple(lb.shape)}")
    h, w = la.shape
    lib = eng.lib
    slots = _pow2_at_least(max(1, int(slots)))
    with eng.lock:
        stat = torch.zeros(2, dtype=torch.int32, device=eng.device)
        while True:
            ws = torch.empty(lib.sg_objects_overlap_ws_bytes(slots), dtype=torch.uint8, device=eng.device)
            pairs = torch.empty(slots, 3, dtype=torch.int32, device=eng.device)
            _lib.check(lib.sg_objects_overlap(eng.h, eng.stream, h, w, C.c_void_p(la.data_ptr()), C.c_void_p(lb.data_ptr()), slots,
                                              C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(pairs.data_ptr()),
                                              C.c_void_p(stat.data_ptr())), "sg_objects_overlap")
            n_pairs, lost = (int(v) for v in stat.cpu().numpy())
            if lost == 0:
                break
            slots *= 2
        out = pairs[:n_pairs].cpu().numpy()
    return out[np.lexsort((out[:, 1], out[:, 0]))]


def _threshold(iou):
    f = iou if isinstance(iou, Fraction) else Fraction(str(iou))
    if not 0 < f <= 1:
        raise ValueError(f"objects: IoU threshold {iou} outside (0, 1]")
    return f.numerator, f.denominator


def _zero_counts():
    return {"tp": 0, "fp": 0, "fn": 0}


def match(pairs, table_pred, table_truth, iou=0.5, min_area_pred: int = 0, min_area_truth: int = 0):
    """Greedy one-to-one matching of predicted and true objects of equal value, in exact integers.

    A pair (p, t) with I shared pixels has IoU I / U, U = area_p + area_t - I.  Pairs with I / U >= iou (the threshold read as
    Fraction(str(iou)), compared by cross-multiplication) are taken in descending IoU, ties by ascending (p, t), while both
    sides are still free.  Objects below their side's minimum area take part in the matching; afterwards a truth below
    min_area_truth and whatever is matched to it are ignored, and so is an unmatched prediction below min_area_pred.

    -> (matches int64 [m, 4] = (p, t, I, U) in the order taken, ignored ones included,
        {"tp", "fp", "fn", "per_class": {value: {"tp", "fp", "fn"}}})"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 3)
    tp_ = np.asarray(table_pred, np.int64).reshape(-1, 8)
    tt_ = np.asarray(table_truth, np.int64).reshape(-1, 8)
    num, den = _threshold(iou)
    area_p, area_t, val_p, val_t = tp_[:, 1], tt_[:, 1], tp_[:, 6], tt_[:, 6]
    cand = []
    for p, t, i in pairs.tolist():
        if val_p[p] != val_t[t]:
            continue
        u = int(area_p[p] + area_t[t]) - i
        if i * den >= num * u:
            cand.append((p, t, i, u))

    def order(x, y):  # descending I / U: x before y when Ix * Uy > Iy * Ux; then ascending (p, t)
        d = y[2] * x[3] - x[2] * y[3]
        if d:
            return -1 if d < 0 else 1
        return -1 if x[:2] < y[:2] else (1 if x[:2] > y[:2] else 0)

    cand.sort(key=cmp_to_key(order))
    of_p, of_t, taken = {}, {}, []
    for p, t, i, u in cand:
        if p in of_p or t in of_t:
            continue
        of_p[p], of_t[t] = t, p
        taken.append((p, t, i, u))
    per = {}
    for v in sorted(set(val_p.tolist()) | set(val_t.tolist())):
        per[int(v)] = _zero_counts()
    for p, t, _, _ in taken:
        if area_t[t] >= min_area_truth:
            per[int(val_t[t])]["tp"] += 1
    for p in range(len(tp_)):
        if p not in of_p and area_p[p] >= min_area_pred:
            per[int(val_p[p])]["fp"] += 1
    for t in range(len(tt_)):
        if t not in of_t and area_t[t] >= min_area_truth:
            per[int(val_t[t])]["fn"] += 1
    counts = {k: sum(c[k] for c in per.values()) for k in ("tp", "fp", "fn")}
    counts["per_class"] = per
    return np.asarray(taken, np.int64).reshape(-1, 4), counts


def _ratio(a: int, b: int) -> float:
    return a / b if b else float("nan")


def _scores(c):
    tp, fp, fn = c["tp"], c["fp"], c["fn"]
    return {"tp": tp, "fp": fp, "fn": fn, "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn),
            "f1": _ratio(2 * tp, 2 * tp + fp + fn)}


class ObjectScores:
    """Object-level precision / recall / F1 summed over scenes.

        s = ObjectScores(iou=0.5)
        for pred, truth in scenes: s.update(pred, truth)
        s.result() -> {"tp", "fp", "fn", "precision", "recall", "f1", "mean_iou", "bins": [{"lo", "hi", "tp", "fn", "recall"}, ...],
                       "per_class": {value: {...}} when the maps held more than one value}

    `bins` are ascending truth-area edges: bin k holds the counted truths with edges[k-1] <= area < edges[k] (the first bin
    starts at 0, the last has no upper edge).  Only integers are added up; every ratio is one division in result(), and a
    ratio with a zero denominator is nan."""

    def __init__(self, iou=0.5, bins=AREA_BINS, connectivity: int = 8, min_area_pred: int = 0, min_area_truth: int = 0, engine=None):
        self.iou, self.connectivity, self.engine = iou, connectivity, engine
        _threshold(iou)
        self.bins = tuple(int(b) for b in bins)
        if list(self.bins) != sorted(set(self.bins)):
            raise ValueError(f"ObjectScores: bins {bins} are not strictly ascending")
        self.min_area_pred, self.min_area_truth = int(min_area_pred), int(min_area_truth)
        self.reset()

    def reset(self):
        self.total = _zero_counts()
        self.per_class = {}
        self.bin_tp = [0] * (len(self.bins) + 1)
        self.bin_fn = [0] * (len(self.bins) + 1)
        self.iou_sums = {}   # union size -> sum of the intersections of the counted matches with that union
        self.scenes = 0

    def add(self, matches, counts, table_truth):
        """Adds what `match` returned for one scene."""
        table_truth = np.asarray(table_truth, np.int64).reshape(-1, 8)
        for k in ("tp", "fp", "fn"):
            self.total[k] += counts[k]
        for v, c in counts["per_class"].items():
            acc = self.per_class.setdefault(v, _zero_counts())
            for k in ("tp", "fp", "fn"):
                acc[k] += c[k]
        area = table_truth[:, 1]
        matched = np.zeros(len(table_truth), bool)
        for p, t, i, u in np.asarray(matches, np.int64).reshape(-1, 4).tolist():
            matched[t] = True
            if area[t] >= self.min_area_truth:
                self.iou_sums[u] = self.iou_sums.get(u, 0) + i
        which = np.searchsorted(np.asarray(self.bins, np.int64), area, side="right")
        counted = area >= self.min_area_truth
        for k in range(len(self.bins) + 1):
            self.bin_tp[k] += int((counted & matched & (which == k)).sum())
            self.bin_fn[k] += int((counted & ~matched & (which == k)).sum())
        self.scenes += 1

    def update(self, pred, truth):
        """Labels both maps, counts their overlaps, matches; -> (matches, counts) of this scene."""
        lp, tab_p = label(pred, self.connectivity, self.engine)
        lt, tab_t = label(truth, self.connectivity, self.engine)
        if lp.shape != lt.shape:
            raise ValueError(f"ObjectScores: prediction {tuple(lp.shape)} and truth {tuple(lt.shape)} differ in shape")
        pairs = overlaps(lp, lt, self.engine, slots=4 * (len(tab_p) + len(tab_t)) + 1024)
        matches, counts = match(pairs, tab_p, tab_t, self.iou, self.min_area_pred, self.min_area_truth)
        self.add(matches, counts, tab_t)
        return matches, counts

    def result(self):
        out = _scores(self.total)
        s = sum((Fraction(i, u) for u, i in self.iou_sums.items()), Fraction(0))
        tp = self.total["tp"]
        out["mean_iou"] = float(s / tp) if tp else float("nan")
        edges = (0,) + self.bins + (None,)
        out["bins"] = [{"lo": edges[k], "hi": edges[k + 1], "tp": self.bin_tp[k], "fn": self.bin_fn[k],
                        "recall": _ratio(self.bin_tp[k], self.bin_tp[k] + self.bin_fn[k])} for k in range(len(self.bins) + 1)]
        if len(self.per_class) > 1:
            out["per_class"] = {v: _scores(c) for v, c in sorted(self.per_class.items())}
        out["scenes"] = self.scenes
        return out
