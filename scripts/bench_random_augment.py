#!/usr/bin/env python3
"""Online random augmentation (building_detection_amd/augment.py, sg_warp_u8): what it costs on the device.

One batch = 16 tiles of 512 x 512 cut from 4 sources of 1024 x 1024 (random pixels, seeded).  Every figure is a device-event
time over --reps repetitions after a warm-up, each repetition the image warp (C = 3) followed by the label warp (C = 1):

  warp            sg_warp_u8 (raw ABI calls, table and output built once; `through_engine` adds Engine.warp_u8's per-call host
                  work, which at these sizes is longer than the kernels) under three policies: identity (all off: the centred
                  crop), rotate + scale, and the full policy with tone tables and noise; beside it the byte floor = (bytes written + distinct source bytes read) at the copy
                  bandwidth measured here (a device-to-device copy of 256 MiB, read + write counted), the source bytes of an
                  item being its output area times |det| of its map, capped at the whole source per source
  augment_u8      sg_augment_u8 writing the same number of output bytes (16 tiles from 16 sources of 512 x 512: originals and
                  flips), the offline augmentation's kernel, for scale
  device stage    the device half of one device_random_gen batch (upload of the pinned uint8 sources, two warps, the two
                  normalisations, sg_edge_labels) against device_data_gen's (upload, normalisations, sg_edge_labels)
  step            with --step: `bench.py --gpus 1` in a child process; the device stage is reported as a fraction of its
                  ms_per_step (the feed runs ahead of the step on its own thread: it hides as long as the fraction is below 1)

Use: python scripts/bench_random_augment.py [--reps 100] [--step] [--out profiles/random_augment_bench.json]
Writes one JSON document; needs the GPU (there is no CPU path)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from building_detection_amd import augment as A  # noqa: E402
from building_detection_amd import _lib  # noqa: E402
from building_detection_amd.ops import get_engine  # noqa: E402

CROP, SRC, TILES, SOURCES = 512, 1024, 16, 4
POLICIES = {
    "identity": A.RandomPolicy(),
    "rotate_scale": A.RandomPolicy(rotate=180, scale=(0.6, 1.8)),
    "full": A.RandomPolicy(rotate=180, scale=(0.6, 1.8), shear=10, translate=0.25, flip=True, brightness=0.2, contrast=0.3,
                           saturation=0.4, gamma=0.4, hue=15, noise=5.0, swap_rb=0.3, border="reflect"),
}


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) / reps * 1e3   # us


def items_of(policy, seed):
    xi, li, luts = [], [], []
    for k in range(TILES):
        rec = A.draw(policy, seed, k)
        it, lut = A.warp_items(rec, (SRC, SRC), (CROP, CROP), False)
        xi.append(dict(it, src=k % SOURCES))
        li.append(dict(A.warp_items(rec, (SRC, SRC), (CROP, CROP), True)[0], src=k % SOURCES))
        luts.append(lut)
    lt = None
    if any(l is not None for l in luts):
        ident = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
        lt = torch.from_numpy(np.stack([ident if l is None else l for l in luts]))
    return xi, li, lt


def raw_call(e, src, items, luts, seed):
    """A closure that issues sg_warp_u8 with a table built once and an output allocated once: the kernel without the
    per-call host work of Engine.warp_u8 (the feed pays that work once per batch, on the consumer's thread)."""
    import ctypes as C
    s, h, w = src.shape[:3]
    c = src.shape[3] if src.dim() == 4 else 1
    table = (_lib.WarpItem * len(items))(*[_lib.warp_item(**it) for it in items])
    dst = torch.empty((len(items), CROP, CROP) + tuple(src.shape[3:]), dtype=torch.uint8, device=e.device)
    args = (e.h, e.stream, s, h, w, c, C.c_void_p(src.data_ptr()), len(items), table,
            None if luts is None else C.c_void_p(luts.data_ptr()), seed, CROP, CROP, C.c_void_p(dst.data_ptr()))
    fn = e.lib.sg_warp_u8

    def call():
        rc = fn(*args)
        assert rc == 0, e.lib.sg_last_error().decode()
    call.keep = (table, dst, src, luts)
    return call


def source_bytes(items, c):
    """Distinct source bytes the items can touch: per source min(whole source, sum of output area x |det|) x channels."""
    per = {}
    for src, a, _ in {(it["src"], it["a"], it["b"]) for it in items}:     # items with one map read the same window
        a = [v / 65536.0 for v in a]
        per[src] = per.get(src, 0.0) + CROP * CROP * abs(a[0] * a[3] - a[1] * a[2])
    return int(sum(min(v, SRC * SRC) for v in per.values()) * c)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--step", action="store_true", help="also run bench.py in a child process for the step time")
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_augment_bench.json"))
    args = p.parse_args()
    assert torch.cuda.is_available(), "bench_random_augment.py measures on the GPU; there is nothing to measure without one"
    e = get_engine(0)
    g = torch.Generator().manual_seed(args.seed)
    rgb_h = torch.randint(0, 256, (SOURCES, SRC, SRC, 3), dtype=torch.uint8, generator=g).pin_memory()
    lab_h = ((torch.randint(0, 256, (SOURCES, SRC, SRC), dtype=torch.uint8, generator=g) > 127).to(torch.uint8) * 255).pin_memory()
    rgb, lab = rgb_h.to(e.device), lab_h.to(e.device)
    doc = {"tiles": TILES, "crop": CROP, "sources": SOURCES, "source_size": SRC, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "timing": "device events around --reps repetitions after 10 warm-up calls"}

    big = torch.empty(256 << 20, dtype=torch.uint8, device=e.device)
    dst = torch.empty_like(big)
    us = timed(lambda: dst.copy_(big), 20, 5)
    copy_bw = 2 * big.numel() / (us * 1e-6)
    doc["copy_bandwidth_bytes_per_s"] = copy_bw
    del big, dst

    doc["warp"] = {}
    for name, pol in POLICIES.items():
        xi, li, lt = items_of(pol, args.seed)
        ltd = None if lt is None else lt.to(e.device)
        us_engine = timed(lambda: (e.warp_u8(rgb, xi, ltd, args.seed, out_hw=(CROP, CROP)),
                                   e.warp_u8(lab, li, None, args.seed, out_hw=(CROP, CROP))), args.reps)
        img, lbl = raw_call(e, rgb, xi, ltd, args.seed), raw_call(e, lab, li, None, args.seed)
        us_img, us_lbl = timed(img, args.reps), timed(lbl, args.reps)
        us = timed(lambda: (img(), lbl()), args.reps)
        written = TILES * CROP * CROP * 4
        read = source_bytes(xi, 3) + source_bytes(li, 1)
        floor_us = (written + read) / copy_bw * 1e6
        doc["warp"][name] = {"us_per_batch": round(us, 2), "us_image": round(us_img, 2), "us_label": round(us_lbl, 2),
                             "us_per_batch_through_engine": round(us_engine, 2), "bytes_written": written, "distinct_source_bytes": read,
                             "byte_floor_us": round(floor_us, 2), "times_the_floor": round(us / floor_us, 2),
                             "colour_items": sum(1 for it in xi if it["flags"] & _lib.SG_WARP_COLOR), "tone_tables": lt is not None}

    s512 = torch.randint(0, 256, (TILES, CROP, CROP, 3), dtype=torch.uint8, generator=g).to(e.device)
    l512 = torch.randint(0, 256, (TILES, CROP, CROP), dtype=torch.uint8, generator=g).to(e.device)
    old = [(k, CROP, 0, (0, _lib.SG_AUG_FLIP_UD, _lib.SG_AUG_FLIP_LR)[k % 3]) for k in range(TILES)]
    us = timed(lambda: (e.augment_u8(s512, old, A.IMAGE_FILL), e.augment_u8(l512, old, A.LABEL_FILL)), args.reps)
    doc["augment_u8_same_output_bytes"] = {"us_per_batch_through_engine": round(us, 2),
                                           "items": "originals and flips of 16 sources of 512 x 512",
                                           "note": "Engine.augment_u8 builds its table per call, as Engine.warp_u8 does: compare with "
                                                   "us_per_batch_through_engine; the kernels alone are in the rocprofv3 summary"}

    xi, li, lt = items_of(POLICIES["full"], args.seed)
    lt = lt.pin_memory() if lt is not None else None

    def random_stage():
        xd, ld = rgb_h.to(e.device, non_blocking=True), lab_h.to(e.device, non_blocking=True)
        ltd = lt.to(e.device, non_blocking=True) if lt is not None else None
        xa = e.warp_u8(xd, xi, ltd, args.seed, out_hw=(CROP, CROP))
        la = e.warp_u8(ld, li, None, args.seed, out_hw=(CROP, CROP))
        return e.u8_to_f32(xa, 127.5, 1.0), e.edge_labels(e.u8_to_f32(la, 255.0, 0.0))

    x_h, l_h = s512.cpu().pin_memory(), ((l512 > 127).to(torch.uint8) * 255).cpu().pin_memory()

    def data_stage():
        xd, ld = x_h.to(e.device, non_blocking=True), l_h.to(e.device, non_blocking=True)
        return e.u8_to_f32(xd, 127.5, 1.0), e.edge_labels(e.u8_to_f32(ld, 255.0, 0.0))

    stage = {"device_random_gen": [], "device_data_gen": []}
    for _ in range(3):                       # alternated
        stage["device_random_gen"].append(round(timed(random_stage, max(args.reps // 4, 5), 3), 1))
        stage["device_data_gen"].append(round(timed(data_stage, max(args.reps // 4, 5), 3), 1))
    doc["device_stage_us_per_batch"] = dict(stage, note="upload of pinned uint8 + device work of one batch of 16, three alternated "
                                            "trials; device_random_gen uploads 4 sources of 1024 x 1024, device_data_gen 16 tiles of 512 x 512")

    if args.step:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.steps), "--warmup",
                            str(args.warmup)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT)
        lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            doc["step"] = {"error": f"exit {r.returncode}: {r.stderr.decode()[-300:]}"}
        else:
            j = json.loads(lines[-1])
            ms = j["ms_per_step"]
            worst = max(stage["device_random_gen"]) / 1e3
            doc["step"] = {"ms_per_step": ms, "tiles_per_s": j.get("value"), "feed_device_ms_per_batch": round(worst, 3),
                           "feed_fraction_of_step": round(worst / ms, 4),
                           "note": "bench.py --gpus 1 in a child process of this run; the slowest of the three feed trials over its ms_per_step"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
