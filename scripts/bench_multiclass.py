#!/usr/bin/env python
"""Times the five head-side launches of a training step - softmax forward / backward, loss forward / backward, confusion
counts - at the flagship workload's row count (512 x 512 x 16 = 4.19 M rows): C = 2 through the 2-class entry points, and
C = 2, 3, 8, 21 through the C-class ones (sg_softmax_*, sg_lossn_*, sg_confusion_matrix).

Device events around REPS back-to-back launches after a warm-up, the median of RUNS such windows; GB/s are the bytes the
algorithm has to move (each operand once) over that time, printed beside a device-to-device copy of one rows x C tensor
timed the same way.  Imports the engine only.  One JSON line per row of the table, then the table.

    python scripts/bench_multiclass.py [--rows 4194304] [--runs 9] [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from building_detection_amd._lib import SG_LOSS_EDGE_FOCAL   # noqa: E402
from building_detection_amd.ops import get_engine            # noqa: E402


def timed(fn, runs, reps, warmup=5):
    """Median over `runs` windows of (device time of `reps` launches) / reps, in microseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=512 * 512 * 16)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multiclass: no GPU - times are measured on the device or not at all")
    eng = get_engine(0)
    rows, kind = a.rows, SG_LOSS_EDGE_FOCAL
    g = torch.Generator().manual_seed(7)
    table = []
    for path, C in (("2-class", 2), ("C-class", 2), ("C-class", 3), ("C-class", 8), ("C-class", 21)):
        z = (torch.rand(rows, C, generator=g) * 8 - 4).to(eng.device)
        p = torch.softmax(z, 1).contiguous()
        dp = (torch.rand(rows, C, generator=g) * 2 - 1).to(eng.device)
        t = torch.randint(0, C, (rows,), generator=g)
        y = torch.cat([torch.nn.functional.one_hot(t, C).float(), 1 + (torch.rand(rows, C, generator=g) > 0.7).float()], 1).to(eng.device)
        out, dst = torch.empty_like(z), torch.empty_like(z)
        alpha = [0.35 + 0.3 * c / (C - 1) for c in range(C)]
        counts = torch.zeros(4 if path == "2-class" else C * C, dtype=torch.int64, device=eng.device)
        if path == "2-class":
            ops = {"softmax_fwd": lambda: eng.softmax2_fwd(z, out=out), "softmax_bwd": lambda: eng.softmax2_bwd(p, dp, out=out),
                   "loss_fwd": lambda: eng.loss_fwd(kind, p, y), "loss_bwd": lambda: eng.loss_bwd(kind, p, y, 1.0, out=out),
                   "confusion": lambda: eng.confusion_counts(p, y, out=counts)}
        else:
            ops = {"softmax_fwd": lambda: eng.softmax_fwd(z, out=out), "softmax_bwd": lambda: eng.softmax_bwd(p, dp, out=out),
                   "loss_fwd": lambda: eng.lossn_fwd(kind, p, y, alpha), "loss_bwd": lambda: eng.lossn_bwd(kind, p, y, alpha, 1.0, out=out),
                   "confusion": lambda: eng.confusion_matrix(p, y, out=counts)}
        ops["copy"] = lambda: dst.copy_(z)
        # bytes each launch has to move: every operand once (y_true has 2C columns; the confusion count reads C of them)
        T = rows * C * 4
        need = {"softmax_fwd": 2 * T, "softmax_bwd": 3 * T, "loss_fwd": 3 * T, "loss_bwd": 4 * T, "confusion": 2 * T, "copy": 2 * T}
        for name, fn in ops.items():
            with eng.lock:
                med, lo, hi = timed(fn, a.runs, a.reps)
            row = {"path": path, "C": C, "op": name, "rows": rows, "us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2),
                   "bytes": need[name], "GBps": round(need[name] / med / 1e3, 1)}
            table.append(row)
            print(json.dumps(row), flush=True)
        del z, p, dp, y, out, dst
        torch.cuda.empty_cache()
    print(f"\n{'path':8} {'C':>3} " + " ".join(f"{n:>22}" for n in ("softmax_fwd", "softmax_bwd", "loss_fwd", "loss_bwd", "confusion", "copy")))
    for path, C in sorted({(r["path"], r["C"]) for r in table}, key=lambda k: (k[0] != "2-class", k[1])):
        cells = {r["op"]: r for r in table if (r["path"], r["C"]) == (path, C)}
        print(f"{path:8} {C:>3} " + " ".join(f"{cells[n]['us']:>9.1f} us {cells[n]['GBps']:>6.0f} GB/s"
                                              for n in ("softmax_fwd", "softmax_bwd", "loss_fwd", "loss_bwd", "confusion", "copy")))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
