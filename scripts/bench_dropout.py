#!/usr/bin/env python
"""What does dropout cost?  Two measurements, in one process and with one method.

kernel  sg_dropout on a 16 x 128 x 128 x 256 activation (67 M elements: 268 MB in fp32, read once and written once), element
        and spatial form, fp32 and bf16 storage, against sg_act_fwd ReLU on the same tensor: both read the tensor once and write it
        once, so the ratio says what the hundred-odd integer operations of a Philox4x32-10 call (one per 4 elements) cost beside the
        memory traffic.  Also the scalar form (operands one element off 16-byte alignment: one call per element), and the in-place
        call.  Device events around REPS back-to-back calls after a warm-up, the median of RUNS windows; GB/s = 2 x tensor bytes /
        time.
step    The batch-16 512 x 512 DeepLabv3+ training step (captured, as bench.py runs it) with dropout=(0.5, 0.1) against the same step
        with dropout=None, alternating windows of STEPS steps.  (No launch of the dropout=None step differs from the commit before
        this feature; run bench.py there for a second box.)

One JSON line per measurement; --out writes the list.  Without a GPU the script stops: nothing here is measured on a CPU.

    python scripts/bench_dropout.py [--images 16] [--size 128] [--channels 256] [--runs 9] [--reps 20] [--steps 10] [--no-step]
                                    [--step-size 512] [--out F.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from building_detection_amd import layers as L                # noqa: E402
from building_detection_amd import losses as LS               # noqa: E402
from building_detection_amd._lib import SG_ACT_RELU           # noqa: E402
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


def kernel(eng, a, table):
    N, HW, C = a.images, a.size * a.size, a.channels
    n = N * HW * C
    rng = torch.tensor([1103, 0, 0, 0], dtype=torch.int32, device=eng.device)
    thr, scale = L.dropout_threshold(0.5), L.dropout_scale(0.5)
    for dtype in (torch.float32, torch.bfloat16):
        g = torch.Generator().manual_seed(7)
        # one spare vector behind the tensor: the "offset" rows start one element further
        buf_x = (torch.rand(n + 8, generator=g) * 2 - 1).to(dtype).to(eng.device)
        buf_y = torch.empty_like(buf_x)
        x, y = buf_x[:n].view(N, a.size, a.size, C), buf_y[:n].view(N, a.size, a.size, C)
        xo, yo = buf_x[1:n + 1].view(N, a.size, a.size, C), buf_y[1:n + 1].view(N, a.size, a.size, C)
        need = 2 * n * x.element_size()
        name = "f32" if dtype == torch.float32 else "bf16"
        base = {}

        def emit(op, fn, ref=None):
            with eng.lock:
                med, lo, hi = timed(fn, a.runs, a.reps)
            row = dict(part="kernel", op=op, dtype=name, elements=n, us=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2),
                       bytes=need, GBps=round(need / med / 1e3, 1))
            if ref is not None:
                row["over_relu"] = round(med / base[ref], 3)
            table.append(row)
            print(json.dumps(row), flush=True)
            return med

        base["v"] = emit("relu (sg_act_fwd)", lambda: eng.act_fwd(x, SG_ACT_RELU, out=y))
        base["s"] = emit("relu (sg_act_fwd), offset operands", lambda: eng.act_fwd(xo, SG_ACT_RELU, out=yo))
        emit("dropout element", lambda: eng.dropout(x, thr, scale, rng, 0, out=y), "v")
        emit("dropout spatial", lambda: eng.dropout(x, thr, scale, rng, 0, hwc=HW * C, c=C, out=y), "v")
        emit("dropout element, in place", lambda: eng.dropout(y, thr, scale, rng, 0, out=y), "v")
        emit("dropout element, offset operands (scalar form)", lambda: eng.dropout(xo, thr, scale, rng, 0, out=yo), "s")
        emit("dropout spatial, offset operands (scalar form)", lambda: eng.dropout(xo, thr, scale, rng, 0, hwc=HW * C, c=C, out=yo), "s")
        del buf_x, buf_y, x, y, xo, yo
        torch.cuda.empty_cache()


def step(eng, a, table):
    from building_detection_amd import zoo
    from building_detection_amd.data import synthetic_batch
    size = a.step_size
    x, y = synthetic_batch(a.images, size, size, seed=1103)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    metrics = [LS.PA, LS.IoU, LS.MIoU, LS.F1_score]
    models = {}
    for name, drop in (("dropout=None", None), ("dropout=(0.5, 0.1)", (0.5, 0.1))):
        m = zoo.BUILDERS["v3plus"]((size, size, 3), 2, aspp_pool=size // 16, dropout=drop)
        m.compile(optimizer="adam", loss=LS.edge_focal_loss, metrics=metrics, jit_compile=True)
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
        row = dict(part="step", model="v3plus", config=n, batch=a.images, size=size, ms_per_step=round(statistics.median(times[n]), 3),
                   ms_min=round(min(times[n]), 3), ms_max=round(max(times[n]), 3), windows=a.runs, steps_per_window=a.steps,
                   dropout_nodes=sum(isinstance(q, L._DropoutNode) for q in m.nodes))
        table.append(row)
        print(json.dumps(row), flush=True)
    b, h = (statistics.median(times[n]) for n in models)
    row = dict(part="step", op="dropout over none", ratio=round(h / b, 4), extra_ms=round(h - b, 3))
    table.append(row)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--step-size", type=int, default=512)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dropout: no GPU - times are measured on the device or not at all")
    eng = get_engine(0)
    table = []
    kernel(eng, a, table)
    torch.cuda.empty_cache()
    if not a.no_step:
        step(eng, a, table)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(table, f, indent=1)


if __name__ == "__main__":
    main()
