"""Host restatement of building_detection_amd/objects.py for tests/test_objects_cpu.py and tests/test_objects_gpu.py: numpy + scipy,
written without looking at the product's code paths (scipy labelling instead of union-find, np.unique instead of a hash table,
plain loops over Fraction keys instead of a cross-multiplying comparator)."""
from fractions import Fraction

import numpy as np
from scipy import ndimage as ndi

STRUCT8 = np.ones((3, 3), int)
STRUCT4 = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])


def as_map(m):
    """What the product takes a map for: channel 0 of [H, W, 3]; uint8 as it is; any other dtype as binary 0 / 255."""
    m = np.asarray(m)
    if m.ndim == 3:
        m = m[..., 0]
    if m.dtype != np.uint8:
        m = np.where(m != 0, 255, 0).astype(np.uint8)
    return m


def label_ref(m, connectivity=8):
    """-> (labels int32 [H, W]: object number or -1, table int32 [n, 8] = first pixel, area, x0, y0, x1, y1, value, 0).
    Objects: per distinct non-zero value the connected components; numbered by first raster pixel across all values."""
    m = as_map(m)
    h, w = m.shape
    struct = STRUCT8 if connectivity == 8 else STRUCT4
    labels = np.full(h * w, -1, np.int64)
    rows = []
    base = 0
    for v in np.unique(m):
        if v == 0:
            continue
        lab, n = ndi.label(m == v, structure=struct)
        flat = lab.ravel()
        idx = np.nonzero(flat)[0]
        comp = flat[idx] - 1
        ys, xs = idx // w, idx % w
        big = np.iinfo(np.int64).max
        first, x0, y0 = np.full(n, big), np.full(n, big), np.full(n, big)
        x1, y1 = np.full(n, -1), np.full(n, -1)
        np.minimum.at(first, comp, idx)
        np.minimum.at(x0, comp, xs)
        np.minimum.at(y0, comp, ys)
        np.maximum.at(x1, comp, xs)
        np.maximum.at(y1, comp, ys)
        area = np.bincount(comp, minlength=n)
        rows.append(np.stack([first, area, x0, y0, x1, y1, np.full(n, int(v)), np.zeros(n, np.int64)], 1))
        labels[idx] = base + comp          # provisional numbers: per value, in scipy's order
        base += n
    if not rows:
        return labels.reshape(h, w).astype(np.int32), np.zeros((0, 8), np.int32)
    table = np.concatenate(rows)
    order = np.argsort(table[:, 0], kind="stable")   # by first raster pixel, across all values
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    fg = labels >= 0
    labels[fg] = rank[labels[fg]]
    return labels.reshape(h, w).astype(np.int32), table[order].astype(np.int32)


def overlaps_ref(la, lb):
    """-> int32 [n_pairs, 3] = (a, b, shared pixels), sorted by (a, b)."""
    la, lb = np.asarray(la).ravel().astype(np.int64), np.asarray(lb).ravel().astype(np.int64)
    both = (la >= 0) & (lb >= 0)
    nb = int(lb.max()) + 2
    key, cnt = np.unique(la[both] * nb + lb[both], return_counts=True)
    return np.stack([key // nb, key % nb, cnt], 1).astype(np.int32).reshape(-1, 3)


def match_ref(pairs, table_pred, table_truth, iou=0.5, min_area_pred=0, min_area_truth=0):
    """-> (matches [(p, t, I, U), ...] in the order taken, {"tp", "fp", "fn", "per_class": {value: {...}}})."""
    thr = Fraction(str(iou))
    cand = []
    for row in pairs:
        p, t, i = int(row[0]), int(row[1]), int(row[2])
        if int(table_pred[p][6]) != int(table_truth[t][6]):
            continue
        u = int(table_pred[p][1]) + int(table_truth[t][1]) - i
        q = Fraction(i, u)
        if q >= thr:
            cand.append((-q, p, t, i, u))
    cand.sort()
    used_p, used_t, matches = set(), set(), []
    for _, p, t, i, u in cand:
        if p in used_p or t in used_t:
            continue
        used_p.add(p)
        used_t.add(t)
        matches.append((p, t, i, u))
    per = {}
    for row in list(table_pred) + list(table_truth):
        per.setdefault(int(row[6]), {"tp": 0, "fp": 0, "fn": 0})
    for p, t, i, u in matches:
        if int(table_truth[t][1]) >= min_area_truth:
            per[int(table_truth[t][6])]["tp"] += 1
    for p, row in enumerate(table_pred):
        if p not in used_p and int(row[1]) >= min_area_pred:
            per[int(row[6])]["fp"] += 1
    for t, row in enumerate(table_truth):
        if t not in used_t and int(row[1]) >= min_area_truth:
            per[int(row[6])]["fn"] += 1
    counts = {k: sum(c[k] for c in per.values()) for k in ("tp", "fp", "fn")}
    counts["per_class"] = per
    return matches, counts


def evaluate_ref(pred, truth, iou=0.5, connectivity=8, min_area_pred=0, min_area_truth=0):
    lp, tp = label_ref(pred, connectivity)
    lt, tt = label_ref(truth, connectivity)
    matches, counts = match_ref(overlaps_ref(lp, lt), tp, tt, iou, min_area_pred, min_area_truth)
    return matches, counts, tp, tt


def scores_ref(scenes, iou=0.5, bins=(150, 300, 3000, 8000, 15000), min_area_truth=0):
    """What ObjectScores.result() must say after the scenes [(matches, counts, table_truth), ...]."""
    tp = sum(c["tp"] for _, c, _ in scenes)
    fp = sum(c["fp"] for _, c, _ in scenes)
    fn = sum(c["fn"] for _, c, _ in scenes)
    nan = float("nan")
    s = Fraction(0)
    btp, bfn = [0] * (len(bins) + 1), [0] * (len(bins) + 1)
    for matches, _, tt in scenes:
        hit = set()
        for p, t, i, u in matches:
            hit.add(int(t))
            if int(tt[int(t)][1]) >= min_area_truth:
                s += Fraction(int(i), int(u))
        for t, row in enumerate(tt):
            a = int(row[1])
            if a < min_area_truth:
                continue
            k = sum(1 for e in bins if a >= e)
            if t in hit:
                btp[k] += 1
            else:
                bfn[k] += 1
    return {"tp": tp, "fp": fp, "fn": fn,
            "precision": tp / (tp + fp) if tp + fp else nan, "recall": tp / (tp + fn) if tp + fn else nan,
            "f1": 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else nan,
            "mean_iou": float(s / tp) if tp else nan,
            "bin_tp": btp, "bin_fn": bfn}
