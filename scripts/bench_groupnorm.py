#!/usr/bin/env python3
"""sg_gn_fwd / sg_gn_bwd against sg_bn_train_fwd / sg_bn_train_bwd of the same build on the same tensor (BatchNormalization's pair has
the same pass structure and moves the same bytes: it is the yardstick), fp32 and bf16, fused ReLU on in both.
Per launch one pair of device events; 5 warm-ups, then 20 timed calls alternating the two layers; the median is reported with the
bytes the algorithm needs over that time (forward: 2 reads + 1 write of the tensor, backward: 4 reads + 1 write).  The whole
measurement is repeated --runs times in the process: the spread of the ratio over the runs is what a difference is judged by.
With --step: the captured DeepLabv3+ training step (512 x 512, batch 16, fp32) with norm="group" next to norm="batch".
With --profile: no timing, a few calls of every kernel for a kernel trace taken from outside.
Use: python scripts/bench_groupnorm.py [--runs 3] [--step] [--out profiles/groupnorm_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from building_detection_amd.ops import get_engine  # noqa: E402

# (label, N, H, W, C, G)
SHAPES = [("16x128x128x256 G=32", 16, 128, 128, 256, 32), ("16x32x32x728 G=8", 16, 32, 32, 728, 8)]
WARMUP, REPS = 5, 20


def timed_pair(fa, fb):
    """Median device time (us) of fa and of fb, calls alternating."""
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
    return statistics.median(ta), statistics.median(tb)


def calls(e, dtype, n, h, w, c, groups):
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(n, h, w, c, generator=g) * 1.5 + 0.3).to(dtype).cuda()
    dy = torch.randn(n, h, w, c, generator=g).to(dtype).cuda()
    gamma, beta = (torch.rand(c, generator=g) + 0.5).cuda(), (torch.randn(c, generator=g) * 0.1).cuda()
    mm, mv = torch.zeros(c).cuda(), torch.ones(c).cuda()
    y, dx, dgm, dbt = torch.empty_like(x), torch.empty_like(x), torch.empty(c).cuda(), torch.empty(c).cuda()
    _, bmean, binv = e.bn_train_fwd(x, gamma, beta, mm, mv, relu=True, out=y)
    _, gmean, ginv = e.gn_fwd(x, gamma, beta, groups, relu=True, out=y)
    return dict(
        bn_fwd=lambda: e.bn_train_fwd(x, gamma, beta, mm, mv, relu=True, out=y),
        gn_fwd=lambda: e.gn_fwd(x, gamma, beta, groups, relu=True, out=y),
        bn_bwd=lambda: e.bn_train_bwd(x, None, dy, gamma, bmean, binv, relu=True, out=dx, dgamma=dgm, dbeta=dbt, beta=beta),
        gn_bwd=lambda: e.gn_bwd(x, dy, gamma, beta, gmean, ginv, groups, relu=True, out=dx, dgamma=dgm, dbeta=dbt)), x


def kernels(e, runs):
    rows = []
    for dtype, dname in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for label, n, h, w, c, groups in SHAPES:
            fn, x = calls(e, dtype, n, h, w, c, groups)
            tensor = x.numel() * x.element_size()
            for op, passes in (("fwd", 3), ("bwd", 5)):
                nbytes = passes * tensor
                per_run = [timed_pair(fn["bn_" + op], fn["gn_" + op]) for _ in range(runs)]
                ratios = [tg / tb for tb, tg in per_run]
                tb, tg = statistics.median(t[0] for t in per_run), statistics.median(t[1] for t in per_run)
                rows.append(dict(shape=label, dtype=dname, op=op, needed_bytes=nbytes, bn_us=[round(t[0], 2) for t in per_run],
                                 gn_us=[round(t[1], 2) for t in per_run], ratio=[round(r, 4) for r in ratios],
                                 ratio_median=round(statistics.median(ratios), 4), ratio_spread=round(max(ratios) - min(ratios), 4),
                                 bn_GBps=round(nbytes / tb * 1e-3, 1), gn_GBps=round(nbytes / tg * 1e-3, 1)))
                print(f"{dname} {label:22s} {op}: BN {tb:8.1f} us  GN {tg:8.1f} us  ratio {statistics.median(ratios):5.3f} "
                      f"(spread {max(ratios) - min(ratios):.3f} over {runs} runs)  GN {nbytes / tg * 1e-3:7.1f} GB/s of needed bytes", flush=True)
            del fn, x
            torch.cuda.empty_cache()
    return rows


def profile_calls(e):
    for dtype in (torch.float32, torch.bfloat16):
        for _, n, h, w, c, groups in SHAPES:
            fn, _x = calls(e, dtype, n, h, w, c, groups)
            for _ in range(5):
                for f in fn.values():
                    f()
            torch.cuda.synchronize()


def step_times(batch=16, steps=12, warmup=5):
    from building_detection_amd import zoo
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.losses import edge_focal_loss
    out = {}
    x, y = synthetic_batch(batch, 512, 512, seed=1)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for norm in ("batch", "group"):
        m = zoo.Xception_DeepLabV3_Plus((512, 512, 3), 2, norm=norm)
        m.compile(optimizer="adam", loss=edge_focal_loss, metrics=[], jit_compile=True)
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
        out[norm] = dict(step_ms_median=round(statistics.median(ts), 3), step_ms_min=round(min(ts), 3), step_ms_max=round(max(ts), 3),
                         captured=len(m._train_graphs) == 1)
        print(f"DeepLabv3+ 512x512 batch {batch} fp32 captured train step, norm={norm}: median {statistics.median(ts):.2f} ms "
              f"(min {min(ts):.2f}, max {max(ts):.2f})", flush=True)
        del m
        torch.cuda.empty_cache()
    out["group_over_batch"] = round(out["group"]["step_ms_median"] / out["batch"]["step_ms_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_groupnorm.py needs the GPU: a CPU run gives no time")
    e = get_engine(0)
    if a.profile:
        profile_calls(e)
        return
    res = dict(device=torch.cuda.get_device_name(0), warmup=WARMUP, reps=REPS, runs=a.runs, kernels=kernels(e, a.runs))
    if a.step:
        res["train_step"] = step_times()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w", encoding="utf-8") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
