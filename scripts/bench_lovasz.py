#!/usr/bin/env python
"""What does the Lovasz-Softmax loss cost?  Three measurements, in one process and with one method.

sort    sg_sort_pairs_u32 alone on 2 segments of 2^22 pairs, 30 key bits (the keys of the head below), and every kernel of a
        pass on its own from the profiler's kernel records.  Bytes are the algorithm's: per pass and pair the histogram reads 4,
        the scatter reads 8 and writes 8.  GB/s = those bytes / time, to be read beside the dropout kernel's 5570 GB/s copy.
head    At the flagship workload's head (16 x 512 x 512 rows, C = 2, y_true 4 wide), forward + backward pairs:
            plain     sg_lossn_fwd + sg_lossn_bwd with edge focal                    (what a step without the loss pays)
            lovasz    sg_loss_lovasz_fwd + _bwd for compound(edge_focal_loss, lovasz_loss)
        and the two calls of each on their own, then every kernel of the pair.  Device events around REPS back-to-back calls
        after a warm-up, the median of RUNS windows.
step    The batch-16 512 x 512 DeepLabv3+ training step (captured, as bench.py runs it) with compound(edge_focal_loss,
        lovasz_loss) against the same step with edge_focal_loss, alternating windows of STEPS steps.

One JSON line per measurement; --out writes the list.  Without a GPU the script stops: nothing here is measured on a CPU.

    python scripts/bench_lovasz.py [--images 16] [--size 512] [--runs 9] [--reps 10] [--steps 10] [--no-step] [--out F.json]
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

KERNELS = ("sort_hist_kernel", "sort_scan_kernel", "sort_scatter_kernel", "lv_key_kernel", "lv_count_kernel", "lv_scan_kernel",
           "lv_grad_kernel", "lv_seg_kernel", "lv_final_kernel", "lv_bwd_kernel")


def timed(fn, runs, reps, warmup=3):
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
        print(f"bench_lovasz: the profiler gave no kernel records ({exc!r})", file=sys.stderr)
        return None


def emit(table, **row):
    table.append(row)
    print(json.dumps(row), flush=True)


def kernel_rows(eng, a, table, part, fn, pass_bytes):
    with eng.lock:
        per = kernel_us(fn, max(2, a.reps // 2))
    for name in KERNELS:
        if per is None or name not in per:
            continue
        us, n = per[name]
        need = pass_bytes.get(name)
        emit(table, part=part, op="kernel", kernel=name, us=round(us, 2), launches_per_call=round(n, 2), bytes=need,
             GBps=None if not need else round(need / us / 1e3, 1))


def sort(eng, a, table):
    segments, n, bits = 2, 1 << 22, 30
    g = torch.Generator().manual_seed(11)
    for name, keys in (("random 30-bit", torch.randint(0, 1 << 30, (segments, n), generator=g, dtype=torch.int64)),
                       ("softmax errors", (0x3F800000 - torch.softmax(torch.rand(segments * n, 2, generator=g) * 8 - 4, 1)[:, 0]
                                           .contiguous().view(torch.int32).long()).reshape(segments, n))):
        kd = keys.to(torch.int32).contiguous().to(eng.device)
        vd = torch.arange(segments * n, dtype=torch.int32).reshape(segments, n).to(eng.device)
        passes = -(-bits // 8)
        need = passes * segments * n * (4 + 16)
        with eng.lock:
            med, lo, hi = timed(lambda: eng.sort_pairs(kd, vd, bits), a.runs, a.reps)
        emit(table, part="sort", op="sort_pairs", keys=name, segments=segments, len=n, key_bits=bits, passes=passes, us=round(med, 2),
             us_min=round(lo, 2), us_max=round(hi, 2), bytes=need, GBps=round(need / med / 1e3, 1),
             Mpairs_per_s=round(segments * n / med, 1))
        kernel_rows(eng, a, table, f"sort ({name})", lambda: eng.sort_pairs(kd, vd, bits),
                    {"sort_hist_kernel": 4 * segments * n, "sort_scatter_kernel": 16 * segments * n})
        del kd, vd


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
    P, Y, N = 4 * C * rows, 4 * y_cols * rows, rows * C

    def row(op, fn, need, **extra):
        with eng.lock:
            med, lo, hi = timed(fn, a.runs, a.reps)
        emit(table, part="head", op=op, rows=rows, C=C, y_cols=y_cols, us=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2),
             bytes=need, GBps=round(need / med / 1e3, 1), **extra)
        return med

    row("plain fwd", lambda: eng.lossn_fwd(SG_LOSS_EDGE_FOCAL, p, y, alpha), P + Y)
    row("plain bwd", lambda: eng.lossn_bwd(SG_LOSS_EDGE_FOCAL, p, y, alpha, 1.0, out=dp), 2 * P + Y)
    base = row("plain fwd+bwd", lambda: (eng.lossn_fwd(SG_LOSS_EDGE_FOCAL, p, y, alpha),
                                         eng.lossn_bwd(SG_LOSS_EDGE_FOCAL, p, y, alpha, 1.0, out=dp)), 3 * P + 2 * Y)
    r = LS.resolve_lovasz(LS.compound(LS.edge_focal_loss, LS.lovasz_loss), C)
    out, gl = eng.loss_lovasz_fwd(r, p, y)
    terms = [round(float(v), 6) for v in out.cpu()]
    # key pass: reads p and y, writes a pair; four sort passes; count reads 4; grad reads 4, gathers p, scatters g
    fwd_bytes = (P + Y + 8 * N) + 4 * 20 * N + 4 * N + (4 * N + 2 * P)
    bwd_bytes = 3 * P + Y

    def pair():
        _, gg = eng.loss_lovasz_fwd(r, p, y)
        eng.loss_lovasz_bwd(r, p, y, gg, 1.0, out=dp)

    row("lovasz fwd", lambda: eng.loss_lovasz_fwd(r, p, y), fwd_bytes, terms=terms)
    row("lovasz bwd", lambda: eng.loss_lovasz_bwd(r, p, y, gl, 1.0, out=dp), bwd_bytes)
    med = row("lovasz fwd+bwd", pair, fwd_bytes + bwd_bytes)
    emit(table, part="head", op="lovasz over plain", ratio=round(med / base, 3), extra_us=round(med - base, 2))
    kernel_rows(eng, a, table, "head", pair,
                {"sort_hist_kernel": 4 * N, "sort_scatter_kernel": 16 * N, "lv_key_kernel": P + Y + 8 * N, "lv_count_kernel": 4 * N,
                 "lv_grad_kernel": 4 * N + 2 * P, "lv_bwd_kernel": bwd_bytes})


def step(eng, a, table):
    from building_detection_amd import zoo
    from building_detection_amd.data import synthetic_batch
    x, y = synthetic_batch(a.images, a.size, a.size, seed=1103)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    metrics = [LS.PA, LS.IoU, LS.MIoU, LS.F1_score]
    models = {}
    for name, loss in (("edge_focal_loss", LS.edge_focal_loss), ("edge_focal_loss+lovasz_loss", LS.compound(LS.edge_focal_loss, LS.lovasz_loss))):
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
        emit(table, part="step", loss=n, model="v3plus", batch=a.images, size=a.size, ms_per_step=round(statistics.median(times[n]), 3),
             ms_min=round(min(times[n]), 3), ms_max=round(max(times[n]), 3), windows=a.runs, steps_per_window=a.steps,
             last_loss_terms=m.last_loss_terms())
    b, h = (statistics.median(times[n]) for n in models)
    emit(table, part="step", op="with lovasz over without", ratio=round(h / b, 4), extra_ms=round(h - b, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lovasz: no GPU - times are measured on the device or not at all")
    eng = get_engine(0)
    table = []
    sort(eng, a, table)
    torch.cuda.empty_cache()
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
