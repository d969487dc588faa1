#!/usr/bin/env python
"""Times the per-building evaluation (building_detection_amd/objects.py, csrc/objects.hip) on synthetic towns of 2048^2 and
4096^2 pixels against the same work done with scipy on the host.

The prediction is the town of tests/test_cleanup_gpu.py::test_many_separate_buildings scaled to the scene size (one rectangle /
L-shape / dumbbell / courtyard house per 100-px cell); the truth is a perturbed copy: moved by a few pixels, some houses
missing, some added, some grown together.

Per scene size it first ASSERTS that the engine and scipy count the same things - objects of both maps, their areas, the
overlapping pairs and their pixel counts - and then reports, as host clocks around the calls (synchronised before and after; the
engine's calls end in the read-back of their small tables), median / minimum / maximum of --reps calls after one warm-up:
  * label:             objects.label(prediction)                 | ndimage.label + per-object area (np.bincount)
  * overlaps:          objects.overlaps(labels_p, labels_t)      | np.unique over a * nb + b where both labels are >= 0
  * evaluate_objects:  pipeline.evaluate_objects(pred, truth)    | two labellings + pair keys on the host + objects.match
once with the maps as numpy arrays (what pipeline.detection returns; the upload is inside the time) and once as device tensors.
Needs the GPU (no time is reported without one).  One JSON line per row, then the file.

    python scripts/bench_objects.py [--sizes 2048 4096] [--reps 5] [--out profiles/objects_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from building_detection_amd import objects as OB, pipeline as PL   # noqa: E402
from building_detection_amd.ops import get_engine                  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def stats(ms):
    return {"ms": round(statistics.median(ms), 2), "ms_min": round(min(ms), 2), "ms_max": round(max(ms), 2), "reps": len(ms)}


def town(size, seed=42):
    rng = np.random.default_rng(seed)
    g = np.zeros((size, size), np.uint8)
    for gy in range(0, size - 99, 100):
        for gx in range(0, size - 99, 100):
            y, x = gy + rng.integers(2, 12), gx + rng.integers(2, 12)
            hh, ww = rng.integers(20, 86), rng.integers(20, 86)
            g[y:y + hh, x:x + ww] = 255
            kind = rng.integers(0, 4)
            if kind == 0:    # L-shape
                g[y:y + hh // 2, x + ww // 2:x + ww] = 0
            elif kind == 1:  # dumbbell: a neck cut into the middle
                n0 = rng.integers(3, 12)
                g[y + hh // 2 - 4:y + hh // 2 + 4, x:x + ww // 2 - n0 // 2] = 0
                g[y + hh // 2 - 4:y + hh // 2 + 4, x + ww // 2 + n0 // 2:x + ww] = 0
            elif kind == 2:  # courtyard
                g[y + hh // 3:y + 2 * hh // 3, x + ww // 3:x + 2 * ww // 3] = 0
    return g


def perturbed(g, seed=7):
    rng = np.random.default_rng(seed)
    size = g.shape[0]
    t = np.roll(g, (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))), (0, 1)).copy()
    cells = [(gy, gx) for gy in range(0, size - 99, 100) for gx in range(0, size - 99, 100)]
    for k in rng.permutation(len(cells))[:len(cells) // 10]:      # a tenth of the houses is missing
        gy, gx = cells[k]
        t[gy:gy + 100, gx:gx + 100] = 0
    for k in rng.permutation(len(cells))[:len(cells) // 20]:      # some have grown together with their right-hand neighbour
        gy, gx = cells[k]
        t[gy + 40:gy + 46, gx:min(size, gx + 160)] = 255
    for _ in range(len(cells) // 10):                              # sheds nobody predicted
        y, x = int(rng.integers(0, size - 12)), int(rng.integers(0, size - 12))
        t[y:y + int(rng.integers(3, 12)), x:x + int(rng.integers(3, 12))] = 255
    return t


S8 = np.ones((3, 3), int)


def host_label(m):
    lab, n = ndi.label(m > 0, structure=S8)
    return lab, n, np.bincount(lab.ravel(), minlength=n + 1)[1:]


def host_pairs(la, lb, nb):
    a, b = la.ravel().astype(np.int64), lb.ravel().astype(np.int64)
    both = (a > 0) & (b > 0)
    key, cnt = np.unique((a[both] - 1) * nb + (b[both] - 1), return_counts=True)
    return np.stack([key // nb, key % nb, cnt], 1)


def host_table(lab, n, area):
    """Area and value are all the matching reads; scipy numbers a binary map's objects in raster order of their first pixel."""
    t = np.zeros((n, 8), np.int64)
    t[:, 1], t[:, 6] = area, 255
    return t


def host_evaluate(pred, truth, iou):
    lp, n_p, ap = host_label(pred)
    lt, n_t, at = host_label(truth)
    return OB.match(host_pairs(lp, lt, n_t), host_table(lp, n_p, ap), host_table(lt, n_t, at), iou)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iou", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_objects: no GPU - times are measured on the device or not at all")
    eng = get_engine(0)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn):
        fn()
        return stats([wall(fn) for _ in range(a.reps)])

    for size in a.sizes:
        pred = town(size)
        truth = perturbed(pred)
        pred_d, truth_d = torch.from_numpy(pred).to(eng.device), torch.from_numpy(truth).to(eng.device)
        # ---- both sides count the same things, or no time is reported
        lp, tab_p = OB.label(pred_d, 8, eng)
        lt, tab_t = OB.label(truth_d, 8, eng)
        pairs = OB.overlaps(lp, lt, eng)
        hp, n_p, area_p = host_label(pred)
        ht, n_t, area_t = host_label(truth)
        hpairs = host_pairs(hp, ht, n_t)
        assert len(tab_p) == n_p and len(tab_t) == n_t, (len(tab_p), n_p, len(tab_t), n_t)
        assert np.array_equal(tab_p[:, 1], area_p) and np.array_equal(tab_t[:, 1], area_t)
        assert np.array_equal(lp.cpu().numpy(), hp - 1) and np.array_equal(lt.cpu().numpy(), ht - 1)
        assert np.array_equal(pairs, hpairs), (pairs.shape, hpairs.shape)
        res = PL.evaluate_objects(pred, truth, iou=a.iou, engine=eng)
        hres = host_evaluate(pred, truth, a.iou)
        assert (res["tp"], res["fp"], res["fn"]) == (hres["tp"], hres["fp"], hres["fn"])
        emit({"scene": size, "what": "counts (engine == scipy)", "objects_pred": n_p, "objects_truth": n_t, "pairs": len(pairs),
              "tp": res["tp"], "fp": res["fp"], "fn": res["fn"], "f1": round(res["f1"], 4), "mean_iou": round(res["mean_iou"], 4)})
        # ---- times
        emit({"scene": size, "what": "label: engine, device tensor in", **timed(lambda: OB.label(pred_d, 8, eng))})
        emit({"scene": size, "what": "label: engine, numpy in", **timed(lambda: OB.label(pred, 8, eng))})
        emit({"scene": size, "what": "label: scipy", **timed(lambda: host_label(pred))})
        emit({"scene": size, "what": "overlaps: engine", **timed(lambda: OB.overlaps(lp, lt, eng))})
        emit({"scene": size, "what": "overlaps: numpy unique", **timed(lambda: host_pairs(hp, ht, n_t))})
        emit({"scene": size, "what": "evaluate_objects: engine, device tensors in",
              **timed(lambda: PL.evaluate_objects(pred_d, truth_d, iou=a.iou, engine=eng))})
        emit({"scene": size, "what": "evaluate_objects: engine, numpy in",
              **timed(lambda: PL.evaluate_objects(pred, truth, iou=a.iou, engine=eng))})
        emit({"scene": size, "what": "evaluate_objects: scipy + numpy + objects.match", **timed(lambda: host_evaluate(pred, truth, a.iou))})
        del pred_d, truth_d, lp, lt
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
