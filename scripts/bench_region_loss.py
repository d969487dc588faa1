#!/usr/bin/env python
"""Does fusing the region term into the pointwise loss pay?  At the flagship workload's head (16 x 512 x 512 rows) this times,
in one process and with one method, for C = 2 (y_true 4 wide) and C = 6 (12 wide), batch-wide and per image (16 images):

    pointwise   sg_lossn_fwd + sg_lossn_bwd, edge focal            (what a step pays today)
    compound    sg_loss_region_fwd + _bwd, edge focal + Dice       (the fused pair)
    region      sg_loss_region_fwd + _bwd with point_kind = -1     (what an unfused design would ADD to `pointwise`)
    final       region_final_kernel (+ region_total_kernel per image) alone, from the profiler's kernel records of the
                compound forward calls (null where the profiler gives none)

Device events around REPS back-to-back forward + backward pairs after a warm-up, the median of RUNS such windows.  The fusion
has done its job if compound < pointwise + region; compound / pointwise says what the region term costs a step.  One JSON line
per measurement, then the table; --out writes the list.

    python scripts/bench_region_loss.py [--rows-per-image 262144] [--images 16] [--runs 9] [--reps 20] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from building_detection_amd import losses as LS               # noqa: E402
from building_detection_amd._lib import SG_LOSS_EDGE_FOCAL    # noqa: E402
from building_detection_amd.ops import get_engine             # noqa: E402


def timed(fn, runs, reps, warmup=5):
    """Median over `runs` windows of (device time of `reps` calls) / reps, in microseconds."""
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


def final_kernels_us(fn, reps):
    """Median device time of the final kernel(s) of one forward call, from the profiler's kernel records; None without them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        per = {}
        for e in prof.events():
            for name in ("region_final_kernel", "region_total_kernel"):
                if name in e.name:
                    t = getattr(e, "device_time", None) or getattr(e, "cuda_time", None) or 0.0
                    if t > 0:
                        per.setdefault(name, []).append(float(t))
        if "region_final_kernel" not in per:
            return None
        return sum(statistics.median(v) for v in per.values())
    except Exception as exc:   # no kernel records on this build of the profiler: the row says so
        print(f"bench_region_loss: the profiler gave no kernel records ({exc!r})", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-per-image", type=int, default=512 * 512)
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_region_loss: no GPU - times are measured on the device or not at all")
    eng = get_engine(0)
    n, rpi = a.images, a.rows_per_image
    rows = n * rpi
    g = torch.Generator().manual_seed(7)
    table = []
    for C in (2, 6):
        p = torch.softmax(torch.rand(rows, C, generator=g) * 8 - 4, 1).reshape(n, rpi, C).contiguous().to(eng.device)
        t = torch.randint(0, C, (rows,), generator=g)
        y = torch.cat([torch.nn.functional.one_hot(t, C).float(), 1 + (torch.rand(rows, C, generator=g) > 0.7).float()], 1)
        y = y.reshape(n, rpi, 2 * C).contiguous().to(eng.device)
        dp = torch.empty_like(p)
        alpha = [0.35 + 0.3 * c / (C - 1) for c in range(C)]
        point = LS.edge_focal_loss.with_alpha(alpha)
        T = rows * C * 4                     # bytes of p; y_true is twice that, its weight half read by the edge term only

        def pointwise():
            eng.lossn_fwd(SG_LOSS_EDGE_FOCAL, p, y, alpha)
            eng.lossn_bwd(SG_LOSS_EDGE_FOCAL, p, y, alpha, 1.0, out=dp)

        for groups in ("batch", "image"):
            dice = LS.dice_loss.with_options(per_image=groups == "image")
            rc, rr = LS.resolve_region(LS.compound(point, dice), C), LS.resolve_region(dice, C)

            def pair(r):
                def fn():
                    _, coef = eng.loss_region_fwd(r, p, y)
                    eng.loss_region_bwd(r, p, y, coef, 1.0, out=dp)
                return fn

            ops = {"pointwise": (pointwise, 3 * T + 4 * T), "compound": (pair(rc), 3 * T + 4 * T), "region": (pair(rr), 2 * T + 3 * T)}
            cell = {}
            for name, (fn, need) in ops.items():
                with eng.lock:
                    med, lo, hi = timed(fn, a.runs, a.reps)
                cell[name] = med
                row = {"C": C, "y_cols": 2 * C, "groups": groups, "images": n if groups == "image" else 1, "op": name, "rows": rows,
                       "us": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2), "bytes": need,
                       "GBps": round(need / med / 1e3, 1)}
                table.append(row)
                print(json.dumps(row), flush=True)
            with eng.lock:
                fin = final_kernels_us(lambda: eng.loss_region_fwd(rc, p, y), a.reps)
            row = {"C": C, "y_cols": 2 * C, "groups": groups, "images": n if groups == "image" else 1, "op": "final", "rows": rows,
                   "us": None if fin is None else round(fin, 2)}
            table.append(row)
            print(json.dumps(row), flush=True)
            unfused = cell["pointwise"] + cell["region"]
            row = {"C": C, "groups": groups, "op": "verdict", "compound_us": round(cell["compound"], 2), "unfused_us": round(unfused, 2),
                   "fusion_pays": bool(cell["compound"] < unfused), "compound_over_pointwise": round(cell["compound"] / cell["pointwise"], 3)}
            table.append(row)
            print(json.dumps(row), flush=True)
        del p, y, dp
        torch.cuda.empty_cache()
    print(f"\n{'C':>3} {'groups':>6} {'pointwise':>12} {'compound':>12} {'region':>12} {'final':>10} {'unfused':>12} {'compound/pointwise':>19}  fusion pays")
    for v in (r for r in table if r["op"] == "verdict"):
        cells = {r["op"]: r for r in table if (r["C"], r["groups"]) == (v["C"], v["groups"])}
        fin = cells["final"]["us"]
        print(f"{v['C']:>3} {v['groups']:>6} {cells['pointwise']['us']:>9.1f} us {cells['compound']['us']:>9.1f} us "
              f"{cells['region']['us']:>9.1f} us {'-' if fin is None else format(fin, '.1f'):>7} us {v['unfused_us']:>9.1f} us "
              f"{v['compound_over_pointwise']:>19.3f}  {'yes' if v['fusion_pays'] else 'NO'}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
