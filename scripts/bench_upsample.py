#!/usr/bin/env python3
"""sg_upsample_bilinear_fwd / _bwd against sg_upsample_nearest_fwd / _bwd of the same build (the nearest pair is the fixed
yardstick), at DeepLabv3+'s batch-16 up-samplings and the BAM head's x4, both dtypes.  Per launch one pair of device events;
5 warm-ups, then 20 timed launches alternating the two modes; the median is reported, with the bytes the algorithm needs
(source read once, result written once; backward: dy read once, dx written once) over that time.
With --step: additionally the training step time of the bilinear DeepLabv3+ next to the nearest one (512 x 512, batch 16).
Use: python scripts/bench_upsample.py [--batch 16] [--step] [--out profiles/upsample_bilinear.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_detection_amd.ops import get_engine  # noqa: E402

# (label, source H, source W, C, factor)
SHAPES = [("x2 64x64x256", 64, 64, 256, 2), ("x2 128x128x64", 128, 128, 64, 2), ("x32 1x1x256 (ASPP image pooling)", 1, 1, 256, 32),
          ("x4 128x128x64 (BAM head)", 128, 128, 64, 4),
          # the same layers at the sizes the 512 x 512 builders give them
          ("x2 32x32x256 (decoder, 512 input)", 32, 32, 256, 2), ("x2 256x256x64 (decoder, 512 input)", 256, 256, 64, 2)]
WARMUP, REPS = 5, 20


def timed_pair(fa, fb):
    """Median device time (us) of fa and of fb, launches alternating."""
    for _ in range(WARMUP):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(REPS):
        for fn, acc in ((fa, ta), (fb, tb)):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            z.record()
            z.synchronize()
            acc.append(a.elapsed_time(z) * 1e3)
    return statistics.median(ta), statistics.median(tb), min(ta), min(tb)


def kernels(e, batch):
    rows = []
    for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for label, h, w, c, s in SHAPES:
            g = torch.Generator().manual_seed(1)
            x = torch.randn(batch, h, w, c, generator=g).to(dtype).cuda()
            dy = torch.randn(batch, h * s, w * s, c, generator=g).to(dtype).cuda()
            y, dx = torch.empty_like(dy), torch.empty_like(x)
            nbytes = (x.numel() + dy.numel()) * x.element_size()
            for name, near, bil in (("fwd", lambda: e.upsample_fwd(x, s, out=y), lambda: e.upsample_bilinear_fwd(x, s, out=y)),
                                    ("bwd", lambda: e.upsample_bwd(dy, tuple(x.shape), s, out=dx),
                                     lambda: e.upsample_bilinear_bwd(dy, tuple(x.shape), s, out=dx))):
                tn, tb, mn, mb = timed_pair(near, bil)
                rows.append(dict(shape=label, batch=batch, dtype=dname, op=name, bytes=nbytes, nearest_us=round(tn, 2),
                                 bilinear_us=round(tb, 2), nearest_min_us=round(mn, 2), bilinear_min_us=round(mb, 2),
                                 ratio=round(tb / tn, 3), nearest_GBps=round(nbytes / tn * 1e-3, 1), bilinear_GBps=round(nbytes / tb * 1e-3, 1)))
                print(f"{dname} {label:36s} {name}: nearest {tn:8.1f} us  bilinear {tb:8.1f} us  ratio {tb / tn:5.2f}  "
                      f"({nbytes / tb * 1e-3:7.1f} GB/s)", flush=True)
    return rows


def step_times(batch, steps=10, warmup=3):
    from building_detection_amd import zoo
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.losses import edge_focal_loss
    out = {}
    x, y = synthetic_batch(batch, 512, 512, seed=1)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for mode in ("nearest", "bilinear"):
        m = zoo.Xception_DeepLabV3_Plus((512, 512, 3), 2, upsampling=mode)
        m.compile(optimizer="adam", loss=edge_focal_loss, metrics=[])
        for _ in range(warmup):
            m.train_on_batch(xd, yd, return_device_scalars=True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(steps):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            m.train_on_batch(xd, yd, return_device_scalars=True)
            z.record()
            z.synchronize()
            ts.append(a.elapsed_time(z))
        out[mode] = dict(step_ms_median=round(statistics.median(ts), 3), step_ms_min=round(min(ts), 3))
        print(f"DeepLabv3+ 512x512 batch {batch} fp32 eager train step, {mode}: median {statistics.median(ts):.2f} ms", flush=True)
        del m
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_upsample.py needs the GPU: a CPU run gives no time")
    e = get_engine(0)
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, kernels=kernels(e, a.batch))
    if a.step:
        res["train_step"] = step_times(a.batch)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
