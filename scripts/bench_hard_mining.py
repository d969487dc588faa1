#!/usr/bin/env python
"""What does hard-pixel mining cost?  Two measurements, in one process and with one method.

head    At the flagship workload's head (16 x 512 x 512 rows, C = 2, y_true 4 wide, edge focal), forward + backward pairs:
            plain       sg_lossn_fwd + sg_lossn_bwd                         (what an unmined step pays)
            mined 0.7   sg_loss_mined_fwd + _bwd, thresh 0.7, min_kept 0.1  (#{key <= thresh} >= k after the first digit:
                        the two narrowing passes return at once)
            mined 0     the same at thresh 0                                (the full three-digit select)
        and the forward and the backward call of each on their own.  Device events around REPS back-to-back calls after a
        warm-up, the median of RUNS windows.  Bytes are the algorithm's: per row, with P = 4 C bytes of p and Y = 4 y_cols of
        y_true, the key pass reads P + Y (it touches one p of the row: the line is fetched whole) and writes 4, a narrowing
        pass reads 4, the sum pass reads P + Y, the backward pass reads P + Y and writes P.  GB/s = those bytes / time.
        Then every kernel of a pair on its own, from the profiler's kernel records (null where it gives none).
step    The batch-16 512 x 512 DeepLabv3+ training step (captured, as bench.py runs it) with hard_mining(edge_focal_loss)
        against the same step with edge_focal_loss, alternating windows of STEPS steps.  (No file on the unmined step's path
        differs from the commit before this feature, so its time is that commit's; run the script there for a second box.)

One JSON line per measurement; --out writes the list.  Without a GPU the script stops: nothing here is measured on a CPU.

    python scripts/bench_hard_mining.py [--images 16] [--size 512] [--runs 9] [--reps 20] [--steps 10] [--no-step] [--out F.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from building_detection_amd import losses as LS               # noqa: E402
from building_detection_amd._lib import SG_LOSS_EDGE_FOCAL    # noqa: E402
from building_detection_amd.ops import get_engine             # noqa: E402


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


KERNELS = ("mine_zero_kernel", "mine_key_kernel", "mine_pick_kernel", "mine_narrow_kernel", "mine_sum_kernel", "mine_final_kernel",
           "mine_bwd_kernel")


def kernel_us(fn, reps):
    """{kernel: (median device time in us, launches per call)} from the profiler's kernel records; None without them."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        per = {}
        for e in prof.events():
            for name in KERNELS:
                if name in e.name:
                    t = getattr(e, "device_time", None) or getattr(e, "cuda_time", None) or 0.0
                    if t > 0:
                        per.setdefault(name, []).append(float(t))
        return {k: (statistics.median(v), len(v) / reps) for k, v in per.items()} or None
    except Exception as exc:   # no kernel records on this build of the profiler: the rows say so
        print(f"bench_hard_mining: the profiler gave no kernel records ({exc!r})", file=sys.stderr)
        return None


def head(eng, a, table):
    C, y_cols = 2, 4
    rows = a.images * a.size * a.size
    g = torch.Generator().manual_seed(7)
    p = torch.softmax(torch.rand(rows, C, generator=g) * 8 - 4, 1).contiguous().to(eng.device)
    t = torch.randint(0, C, (rows,), generator=g)
    y = torch.cat([torch.nn.functional.one_hot(t, C).float(), 1 + (torch.rand(rows, C, generator=g) > 0.7).float()], 1)
    y = y.contiguous().to(eng.device)
    dp = torch.empty_like(p)
    alpha = (0.35, 0.65)
    P, Y = 4 * C * rows, 4 * y_cols * rows
    K = 4 * rows

    def emit(op, fn, need, **extra):
        with eng.lock:
            med, lo, hi = timed(fn, a.runs, a.reps)
        row = dict(part="head", op=op, rows=rows, C=C, y_cols=y_cols, us=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2),
                   bytes=need, GBps=round(need / med / 1e3, 1), **extra)
        table.append(row)
        print(json.dumps(row), flush=True)
        return med

    def plain_fwd():
        eng.lossn_fwd(SG_LOSS_EDGE_FOCAL, p, y, alpha)

    def plain_bwd():
        eng.lossn_bwd(SG_LOSS_EDGE_FOCAL, p, y, alpha, 1.0, out=dp)

    emit("plain fwd", plain_fwd, P + Y)
    emit("plain bwd", plain_bwd, 2 * P + Y)
    base = emit("plain fwd+bwd", lambda: (plain_fwd(), plain_bwd()), 3 * P + 2 * Y)
    for thresh in (0.7, 0.0):
        r = LS.resolve_mining(LS.hard_mining(LS.edge_focal_loss, thresh, 0.1), C)
        _, sel = eng.loss_mined_fwd(r, p, y)
        w = sel.cpu().numpy().view("uint32")
        kept = int(w[2]) | (int(w[3]) << 32)
        narrow = 0 if thresh > 0 else 2            # passes over the stored keys that do work
        info = dict(thresh=thresh, min_kept=0.1, kept=kept, kept_share=round(kept / rows, 4), narrowing_passes=narrow)
        fwd_bytes = (P + Y + K) + narrow * K + (P + Y)

        def mined_fwd():
            return eng.loss_mined_fwd(r, p, y)

        def mined_bwd():
            eng.loss_mined_bwd(r, p, y, sel, 1.0, out=dp)

        def mined_pair():
            _, s = eng.loss_mined_fwd(r, p, y)
            eng.loss_mined_bwd(r, p, y, s, 1.0, out=dp)

        emit(f"mined {thresh} fwd", mined_fwd, fwd_bytes, **info)
        emit(f"mined {thresh} bwd", mined_bwd, 2 * P + Y, **info)
        med = emit(f"mined {thresh} fwd+bwd", mined_pair, fwd_bytes + 2 * P + Y, **info)
        row = dict(part="head", op=f"mined {thresh} over plain", ratio=round(med / base, 3), extra_us=round(med - base, 2))
        table.append(row)
        print(json.dumps(row), flush=True)
        # the passes one by one: bytes of ONE launch over its median device time (the narrowing kernel returns at once when
        # the threshold decided after the first digit: its GB/s then says nothing)
        with eng.lock:
            per = kernel_us(mined_pair, a.reps)
        pass_bytes = {"mine_key_kernel": P + Y + K, "mine_narrow_kernel": K if narrow else 0, "mine_sum_kernel": P + Y,
                      "mine_bwd_kernel": 2 * P + Y}
        for name in KERNELS:
            t = None if per is None or name not in per else per[name]
            need = pass_bytes.get(name)
            row = dict(part="head", op=f"mined {thresh} kernel", kernel=name, us=None if t is None else round(t[0], 2),
                       launches_per_call=None if t is None else round(t[1], 2), bytes=need,
                       GBps=None if t is None or not need else round(need / t[0] / 1e3, 1))
            table.append(row)
            print(json.dumps(row), flush=True)


def step(eng, a, table):
    from building_detection_amd import zoo
    from building_detection_amd.data import synthetic_batch
    x, y = synthetic_batch(a.images, a.size, a.size, seed=1103)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    metrics = [LS.PA, LS.IoU, LS.MIoU, LS.F1_score]
    models = {}
    for name, loss in (("edge_focal_loss", LS.edge_focal_loss), ("hard_mining(edge_focal_loss)", LS.hard_mining(LS.edge_focal_loss))):
        m = zoo.BUILDERS["v3plus"]((a.size, a.size, 3), 2, aspp_pool=a.size // 16)
        m.compile(optimizer="adam", loss=loss, metrics=metrics, jit_compile=True)
        for _ in range(4):                         # two eager steps, the capture, one replay
            m.train_on_batch(xd, yd, return_device_scalars=True)
        torch.cuda.synchronize()
        models[name] = m
    times = {n: [] for n in models}
    for _ in range(a.runs):                        # alternating windows: a busy neighbour meets both alike
        for n, m in models.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                m.train_on_batch(xd, yd, return_device_scalars=True)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) * 1e3 / a.steps)
    for n, m in models.items():
        row = dict(part="step", loss=n, model="v3plus", batch=a.images, size=a.size, ms_per_step=round(statistics.median(times[n]), 3),
                   ms_min=round(min(times[n]), 3), ms_max=round(max(times[n]), 3), windows=a.runs, steps_per_window=a.steps,
                   last_hard_mining=m.last_hard_mining())
        table.append(row)
        print(json.dumps(row), flush=True)
    b, h = (statistics.median(times[n]) for n in models)
    row = dict(part="step", op="mined over plain", ratio=round(h / b, 4), extra_ms=round(h - b, 3))
    table.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hard_mining: no GPU - times are measured on the device or not at all")
    eng = get_engine(0)
    table = []
    head(eng, a, table)
    torch.cuda.empty_cache()
    if not a.no_step:
        step(eng, a, table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
