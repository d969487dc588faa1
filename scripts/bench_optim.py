#!/usr/bin/env python
"""What do the optimizer options cost?  On the DeepLabv3+ (Xception) trainable arena this times, in one process:

  alone     one optimizer.apply() - sg_optim_grad_norms where the configuration clips by a norm, then sg_optim_step - for
            plain Adam (sg_adam_step, the reference's kernel), AdamW, + global_clipnorm, + amsgrad, + EMA, and SGD-Nesterov.
            Device events around REPS back-to-back calls after a warm-up, the median of RUNS such windows; plain Adam is timed
            again before every other configuration, and the spread of those repeats (max - min over their median) is what a
            difference has to exceed.  Reported as achieved GB/s over the configuration's ALGORITHMIC bytes per element:
            28 for Adam (read w, g, m, v; write w, m, v), + 4 for the norm pass's second read of g, + 8 for amsgrad (vhat),
            + 8 for the average; SGD with momentum is 20.
  in_step   the same configurations inside the batch-16 512 x 512 training step (eager): median step time.

One JSON line per measurement; --out writes the list (profiles/optim_bench.json).

    python scripts/bench_optim.py [--size 512] [--batch 16] [--runs 9] [--reps 20] [--steps 7] [--no-step] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from building_detection_amd import optimizers as O, zoo               # noqa: E402
from building_detection_amd.losses import edge_focal_loss              # noqa: E402


def configs():
    return [("adam", lambda: O.Adam(), 28),
            ("adamw", lambda: O.AdamW(), 28),
            ("adamw+global_clip", lambda: O.AdamW(global_clipnorm=1.0), 32),
            ("adamw+global_clip+amsgrad", lambda: O.AdamW(global_clipnorm=1.0, amsgrad=True), 40),
            ("adamw+global_clip+amsgrad+ema", lambda: O.AdamW(global_clipnorm=1.0, amsgrad=True, use_ema=True), 48),
            ("sgd_nesterov", lambda: O.SGD(momentum=0.9, nesterov=True), 20)]


def timed(fn, runs, reps, warmup=5):
    """Median, min, max over `runs` windows of (device time of `reps` calls) / reps, in microseconds."""
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
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim: no GPU - times are measured on the device or not at all")
    model = zoo.Xception_DeepLabV3_Plus((a.size, a.size, 3), 2)
    rt = model._runtime()
    eng = rt.eng
    elems = sum(p.size for p in model.trainable_weights)
    rt.g_train.copy_((torch.rand(rt.g_train.numel(), generator=torch.Generator().manual_seed(5)) * 2e-2 - 1e-2).to(eng.device))
    table = []

    def emit(row):
        table.append(row)
        print(json.dumps(row), flush=True)

    def alone(make):
        opt = make()
        opt.iterations = 10
        opt.prepare(rt)
        with eng.lock:
            return timed(lambda: opt.apply(rt, eng, 1.0), a.runs, a.reps)

    plain = []
    for name, make, bpe in configs():
        pm, plo, phi = alone(configs()[0][1])          # plain Adam again, right before this configuration
        plain.append(pm)
        if name == "adam":
            med, lo, hi = pm, plo, phi
        else:
            med, lo, hi = alone(make)
        emit({"where": "alone", "config": name, "elements": elems, "bytes_per_element": bpe, "us": round(med, 2),
              "us_min": round(lo, 2), "us_max": round(hi, 2), "GBps": round(elems * bpe / med / 1e3, 1),
              "plain_adam_us": round(pm, 2), "plain_adam_GBps": round(elems * 28 / pm / 1e3, 1)})
        torch.cuda.empty_cache()
    spread = (max(plain) - min(plain)) / statistics.median(plain)
    emit({"where": "alone", "config": "plain_adam_repeats", "us": [round(v, 2) for v in plain], "spread": round(spread, 4),
          "GBps_min": round(elems * 28 / max(plain) / 1e3, 1), "GBps_max": round(elems * 28 / min(plain) / 1e3, 1)})

    if not a.no_step:
        from building_detection_amd.data import synthetic_batch
        x, y = synthetic_batch(a.batch, a.size, a.size, seed=3)
        xd, yd = rt.to_device(x), rt.to_device(y)
        w0 = rt.w_train.clone()

        def step_ms(make):
            rt.w_train.copy_(w0)
            rt.adam_m.zero_()
            rt.adam_v.zero_()
            rt.weights_changed()
            model.compile(optimizer=make(), loss=edge_focal_loss, metrics=[])
            for _ in range(3):
                model.train_on_batch(xd, yd, return_device_scalars=True)
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                model.train_on_batch(xd, yd, return_device_scalars=True)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts), min(ts), max(ts)

        plain = []
        for name, make, _ in configs():
            pm, _, _ = step_ms(configs()[0][1])
            plain.append(pm)
            med, lo, hi = (pm, pm, pm) if name == "adam" else step_ms(make)
            emit({"where": "in_step", "config": name, "batch": a.batch, "size": a.size, "step_ms": round(med, 3),
                  "step_ms_min": round(lo, 3), "step_ms_max": round(hi, 3), "plain_adam_step_ms": round(pm, 3)})
            torch.cuda.empty_cache()
        emit({"where": "in_step", "config": "plain_adam_repeats", "step_ms": [round(v, 3) for v in plain],
              "spread": round((max(plain) - min(plain)) / statistics.median(plain), 4)})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
