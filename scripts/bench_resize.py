#!/usr/bin/env python3
"""sg_resize_fwd / _bwd and sg_prob_resize_accumulate on the device.

  * resize, batch 16, 256 channels, fp32 and bf16: 128^2 -> 200^2 (no integer factor) against the byte floor, and 128^2 -> 256^2
    against sg_upsample_bilinear_fwd / _bwd (and nearest against sg_upsample_nearest_*) on the same tensors: the yardstick is the
    existing integer-factor pair, launches alternating;
  * the fold of a 0.75-scale scene into 2048^2 and 4096^2 two-class canvases against a device copy of the canvases' bytes.
Per launch one pair of device events; 5 warm-ups, then 20 timed launches; the median is reported with the bytes the algorithm
needs (source read once, result written once; the fold reads and writes acc and wsum and reads the scaled canvases once) over
that time, and that rate over the HBM peak.
Use: python scripts/bench_resize.py [--batch 16] [--out profiles/resize_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_detection_amd.ops import get_engine  # noqa: E402

WARMUP, REPS = 5, 20
HBM_PEAK_GBPS = 8000.0   # MI355X, HBM3E


def timed(*fns):
    """Median and minimum device time (us) of every fn, launches alternating."""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(REPS):
        for fn, acc in zip(fns, ts):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            acc.append(a.elapsed_time(z) * 1e3)
    return [(statistics.median(t), min(t)) for t in ts]


def row(what, us, us_min, nbytes, **kw):
    r = dict(what=what, us=round(us, 2), us_min=round(us_min, 2), bytes=nbytes, GBps=round(nbytes / us * 1e-3, 1),
             share_of_hbm_peak=round(nbytes / us * 1e-3 / HBM_PEAK_GBPS, 3), **kw)
    print(json.dumps(r), flush=True)
    return r


def resize_rows(e, batch, c=256):
    rows = []
    for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for oh, factor in ((200, None), (256, 2)):
            g = torch.Generator().manual_seed(1)
            x = torch.randn(batch, 128, 128, c, generator=g).to(dtype).cuda()
            dy = torch.randn(batch, oh, oh, c, generator=g).to(dtype).cuda()
            y, dx = torch.empty_like(dy), torch.empty_like(x)
            nbytes = (x.numel() + dy.numel()) * x.element_size()
            tag = f"{batch}x128x128x{c} -> {oh}x{oh} {dname}"
            for method, up_f, up_b in (("bilinear", e.upsample_bilinear_fwd, e.upsample_bilinear_bwd), ("nearest", e.upsample_fwd, e.upsample_bwd)):
                fwd = lambda: e.resize_fwd(x, oh, oh, method, out=y)                                   # noqa: E731
                bwd = lambda: e.resize_bwd(dy, tuple(x.shape), method, out=dx)                         # noqa: E731
                if factor is None:
                    (tf, mf), (tb, mb) = timed(fwd, bwd)
                    rows.append(row(f"sg_resize_fwd {method} {tag}", tf, mf, nbytes))
                    rows.append(row(f"sg_resize_bwd {method} {tag}", tb, mb, nbytes))
                else:
                    ofwd = lambda: up_f(x, factor, out=y)                                              # noqa: E731
                    obwd = lambda: up_b(dy, tuple(x.shape), factor, out=dx)                            # noqa: E731
                    (tf, mf), (to, mo) = timed(fwd, ofwd)
                    rows.append(row(f"sg_resize_fwd {method} {tag}", tf, mf, nbytes, integer_factor_us=round(to, 2),
                                    integer_factor_us_min=round(mo, 2), ratio=round(tf / to, 3)))
                    (tb, mb), (to, mo) = timed(bwd, obwd)
                    rows.append(row(f"sg_resize_bwd {method} {tag}", tb, mb, nbytes, integer_factor_us=round(to, 2),
                                    integer_factor_us_min=round(mo, 2), ratio=round(tb / to, 3)))
            del x, dy, y, dx
            torch.cuda.empty_cache()
    return rows


def fold_rows(e, classes=2, scale=0.75):
    rows = []
    for size in (2048, 4096):
        hs = int(size * scale + 0.5)
        acc_s = torch.rand(hs, hs, classes, device="cuda")
        wsum_s = torch.rand(hs, hs, device="cuda") + 0.5
        acc, wsum = torch.zeros(size, size, classes, device="cuda"), torch.zeros(size, size, device="cuda")
        acc2, wsum2 = torch.empty_like(acc), torch.empty_like(wsum)
        canvas = (acc.numel() + wsum.numel()) * 4
        nbytes = 2 * canvas + (acc_s.numel() + wsum_s.numel()) * 4

        def copy():
            acc2.copy_(acc)
            wsum2.copy_(wsum)
        (tf, mf), (tc, mc) = timed(lambda: e.prob_resize_accumulate(acc_s, wsum_s, acc, wsum, 1.0), copy)
        rows.append(row(f"sg_prob_resize_accumulate {hs}^2 -> {size}^2 x {classes}", tf, mf, nbytes, canvas_copy_us=round(tc, 2),
                        canvas_copy_us_min=round(mc, 2), canvas_copy_bytes=2 * canvas, ratio_to_copy=round(tf / tc, 3)))
        del acc_s, wsum_s, acc, wsum, acc2, wsum2
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_resize.py needs the GPU: a CPU run gives no time")
    e = get_engine(0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, hbm_peak_GBps=HBM_PEAK_GBPS, resize=resize_rows(e, a.batch),
               fold=fold_rows(e))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
