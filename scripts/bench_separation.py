#!/usr/bin/env python
"""Times the separation weights (Engine.edge_labels(separation=...), csrc/separation.hip) on a training batch of 16 x 512^2
synthetic towns against the label channels alone (sg_edge_labels, what the generator did before) and against the host
definition (data.separation_term: one scipy distance transform per building).

Two towns: "rectangles" = the masks of data.synthetic_batch (3 to 12 large rectangles per tile), "houses" = 40 to 60 small
houses per tile on a jittered 8 x 8 grid, 2 to 6 pixels apart - the case the weight exists for.

Per town it first ASSERTS that the device result equals the host definition within 5e-7 * (1 + w0) (the bound of
tests/test_separation_gpu.py), then reports device-event times per call - median / minimum / maximum of --reps samples of
--inner back-to-back calls each, after --warmup calls - of
  * edge_labels alone                         (the parent's work)
  * labelling                                 (one sg_objects_label per image)
  * sg_object_distances with and without d2sq
  * sg_separation_weights
  * edge_labels(separation=(w0, sigma))       (all of the above, as the generators call it)
and the host clock around data.separation_term for the same batch.  The two ratios the feature is held against:
whole / edge_labels alone, and whole / the 69 ms training step the prefetching generator hides behind (README).
Needs the GPU (no time is reported without one).  One JSON line per row, then the file.

    python scripts/bench_separation.py [--batch 16] [--size 512] [--reps 7] [--out profiles/separation_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from building_detection_amd import _lib                               # noqa: E402
from building_detection_amd.data import edge_weight_channels, separation_term, synthetic_batch   # noqa: E402
from building_detection_amd.ops import get_engine                    # noqa: E402

STEP_MS = 69.0   # the fp32 DeepLabv3+ training step at batch 16 x 512^2 (README: 68 - 70 ms)


def houses(n, size, seed=5):
    """[n, size, size] float32 0 / 1: 40 to 60 houses per tile in the cells of an 8 x 8 grid, neighbours 2 to 6 pixels apart."""
    rng = np.random.default_rng(seed)
    cell = size // 8
    out = np.zeros((n, size, size), np.float32)
    for i in range(n):
        cells = rng.permutation(64)[:int(rng.integers(40, 61))]
        for k in cells:
            r, c = divmod(int(k), 8)
            gy, gx = int(rng.integers(2, 7)), int(rng.integers(2, 7))
            out[i, r * cell + gy // 2:(r + 1) * cell - (gy - gy // 2), c * cell + gx // 2:(c + 1) * cell - (gx - gx // 2)] = 1.0
    return out


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--w0", type=float, default=10.0)
    ap.add_argument("--sigma", type=float, default=5.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_separation: no GPU - times are measured on the device or not at all")
    eng = get_engine(0)
    lib = eng.lib
    n, s = a.batch, a.size
    sep = (a.w0, a.sigma)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.inner)
        return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "reps": len(ms),
                "inner": a.inner}

    towns = {"rectangles": np.ascontiguousarray(synthetic_batch(n, s, s)[1][..., 1]), "houses": houses(n, s)}
    for town, lab in towns.items():
        ld = torch.from_numpy(lab).to(eng.device)
        # ---- the device result is the host definition, or no time is reported
        t0 = time.perf_counter()
        terms = [separation_term(m, *sep) for m in lab]
        host_ms = [(time.perf_counter() - t0) * 1e3]
        for _ in range(a.host_reps - 1):
            t0 = time.perf_counter()
            for m in lab:
                separation_term(m, *sep)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        ref = np.stack([edge_weight_channels(m)[0] + t for m, t in zip(lab, terms)])
        got = eng.edge_labels(ld, separation=sep)[..., 2].cpu().numpy().astype(np.float64)
        err = float(np.abs(got - ref).max())
        assert err <= 5e-7 * (1.0 + a.w0), err
        emit({"town": town, "what": "device == host definition", "max_abs_err": err, "largest_weight": float(ref.max()),
              "pixels_with_term": int((np.stack(terms) > 1e-6).sum()), "batch": n, "size": s, "w0": a.w0, "sigma": a.sigma})
        # ---- the parts, on operands made once
        y = eng.edge_labels(ld)
        fg = y[..., 1].to(torch.uint8).contiguous()
        labels = torch.empty((n, s, s), dtype=torch.int32, device=eng.device)
        lws = torch.empty(lib.sg_objects_label_ws_bytes(s, s), dtype=torch.uint8, device=eng.device)
        row = torch.empty((1, 8), dtype=torch.int32, device=eng.device)
        count = torch.empty(1, dtype=torch.int32, device=eng.device)
        dws = torch.empty(lib.sg_object_distances_ws_bytes(n, s, s), dtype=torch.uint8, device=eng.device)
        d1, d2 = torch.empty_like(labels), torch.empty_like(labels)

        def label_all():
            for i in range(n):
                _lib.check(lib.sg_objects_label(eng.h, eng.stream, s, s, vp(fg[i]), 1, vp(lws), lws.numel(), vp(labels[i]), vp(row), 1,
                                                vp(count)), "sg_objects_label")

        def distances(second):
            _lib.check(lib.sg_object_distances(eng.h, eng.stream, n, s, s, vp(labels), vp(dws), dws.numel(), vp(d1),
                                               vp(d2) if second else None), "sg_object_distances")

        def weights():
            _lib.check(lib.sg_separation_weights(eng.h, eng.stream, n, s, s, vp(d1), vp(d2), a.w0, a.sigma, vp(y)),
                       "sg_separation_weights")

        base = timed(lambda: eng.edge_labels(ld))
        emit({"town": town, "what": "edge_labels alone", **base})
        emit({"town": town, "what": "labelling: sg_objects_label per image", **timed(label_all)})
        emit({"town": town, "what": "sg_object_distances, d1sq and d2sq", **timed(lambda: distances(True))})
        emit({"town": town, "what": "sg_object_distances, d2sq == NULL (distance transform)", **timed(lambda: distances(False))})
        distances(True)
        emit({"town": town, "what": "sg_separation_weights", **timed(weights)})
        whole = timed(lambda: eng.edge_labels(ld, separation=sep))
        emit({"town": town, "what": "edge_labels(separation=(w0, sigma))", **whole,
              "over_edge_labels_alone": round(whole["ms"] / base["ms"], 2), "over_training_step": round(whole["ms"] / STEP_MS, 4),
              "training_step_ms": STEP_MS})
        emit({"town": town, "what": "data.separation_term on the host, whole batch", "ms": round(statistics.median(host_ms), 1),
              "ms_min": round(min(host_ms), 1), "ms_max": round(max(host_ms), 1), "reps": len(host_ms),
              "over_device": round(statistics.median(host_ms) / whole["ms"], 1)})
        del ld, y, fg, labels, lws, dws, d1, d2
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
