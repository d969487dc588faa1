#!/usr/bin/env python3
"""data_enhancement.py on the device (building_detection_amd/augment.py): what it costs.

  --kernel   sg_augment_u8 for one batch of 16 512 x 512 tiles of a mixed plan (every 4th entry of plan() over 20 sources,
             originals, flips, rescales 0.6 ... 2.0, R-B swaps), images (C = 3) and labels (C = 1), timed with
             device events over --reps launches; bytes moved = the tiles written + the source pixels each item samples
             (its covered canvas mapped back through the rescale), against the HBM bound (--hbm, bytes/s)
  --feed     tiles per second yielded by device_augment_gen and by device_data_gen over the same --sources PNG files
             (random pixels, written to a temporary folder), the two alternated --trials times in one process

Use: python scripts/augment_bench.py --kernel [--reps 200]   |   python scripts/augment_bench.py --feed [--batch 8]
Each measurement prints one JSON line (and appends it to --out when given).  Under rocprofv3 --kernel-trace --stats run
--kernel alone: the launches are augment_u8_kernel<3> / <1>, one pair per repetition."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_detection_amd import augment as A  # noqa: E402
from building_detection_amd import input_pipeline as IP  # noqa: E402
from building_detection_amd.ops import get_engine  # noqa: E402

SIZE = 512


def emit(rec, out):
    line = json.dumps(rec, sort_keys=True)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def footprint(it, c):
    """Bytes of source pixels an item samples: the canvas it covers (min(n, 512) per side) mapped back by 512 / n."""
    _, n, _, _ = it
    side = min(n, SIZE) * SIZE / n
    return side * side * c


def kernel(args, e):
    names = [f"{i:04d}.png" for i in range(20)]
    entries = A.plan(names, args.seed)[::4][:16]       # every 4th virtual file: all five kinds, up to 16 sources
    srcs = sorted({x.source for x in entries})
    slot = {s: k for k, s in enumerate(srcs)}
    xi = [A.item(x.variant, False, slot[x.source]) for x in entries]
    li = [A.item(x.variant, True, slot[x.source]) for x in entries]
    g = torch.Generator().manual_seed(args.seed)
    rgb = torch.randint(0, 256, (len(srcs), SIZE, SIZE, 3), dtype=torch.uint8, generator=g).cuda()
    gray = torch.randint(0, 256, (len(srcs), SIZE, SIZE), dtype=torch.uint8, generator=g).cuda()
    ox = e.augment_u8(rgb, xi, A.IMAGE_FILL)
    oy = e.augment_u8(gray, li, A.LABEL_FILL)
    launches = {"image": lambda: e.augment_u8(rgb, xi, A.IMAGE_FILL), "label": lambda: e.augment_u8(gray, li, A.LABEL_FILL)}
    launches["both"] = lambda: (launches["image"](), launches["label"]())
    for _ in range(20):
        launches["both"]()
    torch.cuda.synchronize()
    written = {"image": ox.numel(), "label": oy.numel()}
    read = {"image": sum(footprint(it, 3) for it in xi), "label": sum(footprint(it, 1) for it in li)}
    written["both"] = written["image"] + written["label"]
    read["both"] = read["image"] + read["label"]
    for what in ("image", "label", "both"):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            launches[what]()
        z.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(z) / args.reps * 1e3
        moved = written[what] + read[what]
        emit({"measure": "augment_u8_kernel", "launches": what, "tiles": len(xi), "sources": len(srcs),
              "variants": "".join(sorted({x.variant.suffix or "0" for x in entries})),
              "scales": sorted({x.variant.scale for x in entries if x.variant.scale is not None}),
              "us_per_batch": round(us, 2), "reps": args.reps, "bytes_written": int(written[what]), "bytes_read_est": int(read[what]),
              "bytes_per_s": moved / (us * 1e-6), "frac_of_hbm": moved / (us * 1e-6) / args.hbm,
              "note": "device events around --reps back-to-back launches (Engine.augment_u8, host table build included)"},
             args.out)


def feed(args, e):
    from PIL import Image
    rng = np.random.default_rng(args.seed)
    tmp = tempfile.mkdtemp(prefix="augbench_")
    idir, ldir = os.path.join(tmp, "img"), os.path.join(tmp, "lab")
    os.makedirs(idir)
    os.makedirs(ldir)
    for i in range(args.sources):
        Image.fromarray(rng.integers(0, 256, (SIZE, SIZE, 3), dtype=np.uint8)).save(os.path.join(idir, f"{i:04d}.png"))
        lab = np.zeros((SIZE, SIZE), np.uint8)
        lab[rng.integers(0, 256):rng.integers(256, 512), rng.integers(0, 256):rng.integers(256, 512)] = 255
        Image.fromarray(lab).save(os.path.join(ldir, f"{i:04d}.png"))
    imgs = sorted(os.path.join(idir, n) for n in os.listdir(idir))
    labs = sorted(os.path.join(ldir, n) for n in os.listdir(ldir))
    gens = {"device_augment_gen": lambda: A.device_augment_gen(list(imgs), list(labs), args.batch, e, seed=args.seed,
                                                               depth=args.depth, workers=args.workers),
            "device_data_gen": lambda: IP.device_data_gen(list(imgs), list(labs), args.batch, e, depth=args.depth,
                                                          workers=args.workers)}
    for trial in range(args.trials):
        for name, make in gens.items():
            g = make()
            for _ in range(args.warm):
                next(g)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.batches):
                x, y = next(g)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            g.close()
            emit({"measure": "feed", "generator": name, "trial": trial, "batch": args.batch, "batches": args.batches,
                  "sources": args.sources, "workers": args.workers, "depth": args.depth,
                  "tiles_per_s": round(args.batch * args.batches / dt, 1), "ms_per_batch": round(dt / args.batches * 1e3, 2),
                  "note": "consumer does nothing but next(); host decode in worker threads is the bound"}, args.out)
    shutil.rmtree(tmp, ignore_errors=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--kernel", action="store_true")
    p.add_argument("--feed", action="store_true")
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--hbm", type=float, default=8.0e12, help="HBM bound in bytes/s (MI355X: 8 TB/s)")
    p.add_argument("--sources", type=int, default=32)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--batches", type=int, default=24)
    p.add_argument("--warm", type=int, default=3)
    p.add_argument("--trials", type=int, default=3)
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--depth", type=int, default=2)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    e = get_engine(0)
    if args.kernel or not args.feed:
        kernel(args, e)
    if args.feed:
        feed(args, e)


if __name__ == "__main__":
    main()
