#!/usr/bin/env python3
"""Hardware counters of the sort's and the Lovasz loss's kernels.  Counters are collected in runs of their own (no tracing
beside them), one small set per run:

    rocprofv3 --pmc WRITE_SIZE --output-format csv -d OUT/write -- python3 scripts/pmc_sort.py
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT/fetch -- python3 scripts/pmc_sort.py
    rocprofv3 --pmc SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA --output-format csv -d OUT/sq1 -- python3 scripts/pmc_sort.py
    rocprofv3 --pmc SQ_BUSY_CYCLES SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM --output-format csv -d OUT/sq2 -- python3 scripts/pmc_sort.py
    python3 scripts/pmc_sort.py --parse OUT profiles/lovasz_pmc.json

Without arguments: one sg_sort_pairs_u32 of 2 x 2^22 pairs at 30 bits (random keys) and one sg_loss_lovasz_fwd + _bwd at
16 x 512 x 512 rows, C = 2, each once after one warm-up call.  --parse: per kernel and counter the median over its dispatches
(the warm-up's included: the counters do not depend on it), WRITE_SIZE and FETCH_SIZE in bytes (KiB x 1024; FETCH_SIZE doubled,
gfx950 tallies 128-byte requests at 64), beside the algorithm's bytes of one launch."""
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEGMENTS, LEN, ROWS, C = 2, 1 << 22, 16 * 512 * 512, 2
N = SEGMENTS * LEN
ALGORITHM = {   # bytes one launch has to move: (read, written)
    "sort_hist_kernel": (4 * N, 0), "sort_scatter_kernel": (8 * N, 8 * N), "lv_key_kernel": (4 * 6 * ROWS, 8 * ROWS * C),
    "lv_count_kernel": (4 * ROWS * C, 0), "lv_grad_kernel": (8 * ROWS * C, 4 * ROWS * C), "lv_bwd_kernel": (4 * 8 * ROWS, 4 * 2 * ROWS)}
KERNELS = ("sort_hist_kernel", "sort_scan_kernel", "sort_scatter_kernel", "lv_key_kernel", "lv_count_kernel", "lv_scan_kernel",
           "lv_grad_kernel", "lv_seg_kernel", "lv_final_kernel", "lv_bwd_kernel")


def workload():
    import torch
    from building_detection_amd import losses as LS
    from building_detection_amd.ops import get_engine
    eng = get_engine(0)
    g = torch.Generator().manual_seed(11)
    kd = torch.randint(0, 1 << 30, (SEGMENTS, LEN), generator=g, dtype=torch.int64).to(torch.int32).to(eng.device)
    vd = torch.arange(N, dtype=torch.int32).reshape(SEGMENTS, LEN).to(eng.device)
    for _ in range(2):
        eng.sort_pairs(kd, vd, 30)
    torch.cuda.synchronize()
    del kd, vd
    p = torch.softmax(torch.rand(ROWS, C, generator=g) * 8 - 4, 1).contiguous().to(eng.device)
    t = torch.randint(0, C, (ROWS,), generator=g)
    y = torch.cat([torch.nn.functional.one_hot(t, C).float(), 1 + (torch.rand(ROWS, C, generator=g) > 0.7).float()], 1).contiguous().to(eng.device)
    r = LS.resolve_lovasz(LS.compound(LS.edge_focal_loss, LS.lovasz_loss), C)
    for _ in range(2):
        _, gl = eng.loss_lovasz_fwd(r, p, y)
        eng.loss_lovasz_bwd(r, p, y, gl, 1.0)
    torch.cuda.synchronize()


def parse(src, dst):
    scale = {"WRITE_SIZE": 1024.0, "FETCH_SIZE": 2048.0}
    per = {}
    for f in glob.glob(f"{src}/*/*/*counter_collection.csv") + glob.glob(f"{src}/*/*counter_collection.csv"):
        for r in csv.DictReader(open(f)):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    per.setdefault(k, {}).setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]) * scale.get(r["Counter_Name"], 1.0))
    out = {"workload": f"sort {SEGMENTS} x {LEN} pairs, 30 bits; lovasz fwd + bwd {ROWS} rows, C = {C}",
           "note": "median per launch; WRITE_SIZE / FETCH_SIZE in bytes on the fabric side of L2; SQ counters are sums over the shader engines",
           "kernels": {}}
    for k in KERNELS:
        if k in per:
            row = {c: statistics.median(v) for c, v in sorted(per[k].items())}
            row["dispatches_seen"] = max(len(v) for v in per[k].values())
            if k in ALGORITHM:
                row["algorithm_read_bytes"], row["algorithm_written_bytes"] = ALGORITHM[k]
            out["kernels"][k] = row
            print(k, json.dumps(row))
    json.dump(out, open(dst, "w"), indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--parse":
        parse(sys.argv[2], sys.argv[3])
    else:
        workload()
