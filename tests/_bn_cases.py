"""The cases of tests/test_batchnorm_variants_gpu.py: one function per entry point of csrc/norm.hip and of the column sums built
on csrc/sg_reduce.h in csrc/conv_thin.hip (sg_bias_grad, sg_bn_train_fwd_tiles), each against plain float64 (tests/_guarded.py).

A case states which kernels its launch takes - the reduction's V / TX / gx / row-split regime / finalize lanes and the apply
pass's form - from the ENGINE's plan (sg_bn_plan; sg_seg_plan for the column sums), after checked_plan() has asserted that
plan equal in every field to plan_mirror() (the mirrors of plan_bn, seg_plan and bn_cols_grid) for this device's CU count,
and its name equal to the one at the 256 CUs the shapes were chosen at.

Run as a program (`python tests/_bn_cases.py`, SG_BN_COLS=0 SG_FINALIZE_LANES=4 in the environment: the switches are read once
per process) it runs child_cases() - the aligned, vectorisable subset - asserts on the engine's plans that the switches took
effect, and prints one line per case."""
import ctypes as CT
import functools
import os
import sys

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from _guarded import (Guarded, add2_bn_ref, assert_written, bn_apply_ref, bn_bwd_ref, bn_cols_grid, bn_fwd_ref, bn_stats_ref,
                      check_all, close_cols, colsum_ref, regime, seg_plan, short_last_slab, tile_stats_ref, ulp32)
from building_detection_amd._lib import BnPlan, SegPlan
from test_bandwidth_variants_gpu import BF16, DEV, F32, G, GO, call, done, gen, rnd, sgdt, tol

REF_CUS = 256            # the CU count the shapes below were chosen at (MI355X)
SG_EINVAL, SG_EUNSUPPORTED = -1, -3
MOMENTUM, EPS = 0.5, 1e-3
BM = 128                 # rows per statistics tile of the producing convolution (csrc/conv_common.h)
COLS_ON = os.environ.get("SG_BN_COLS", "1") != "0"
LANES16 = os.environ.get("SG_FINALIZE_LANES", "16") == "16"
QUIET = False            # the child process prints its one line per case and nothing else
RECORDS = {}             # (entry point, kind of input, storage) -> largest observed error / scale (a record, not a threshold)


def dname(dtype):
    return "bf16" if dtype == BF16 else "f32"


def record(entry, kind, dtype):
    def put(rel):
        key = (entry, kind, dname(dtype))
        RECORDS[key] = max(RECORDS.get(key, 0.0), rel)
        if not QUIET:
            print(f"REC {entry} {kind} {dname(dtype)} rel={rel:.3e}")
    return put


# ================================================================================================ which kernels a launch takes
def apply_v(C, dtype, vec):
    return 8 if (vec and dtype == BF16 and C % 8 == 0) else (4 if vec else 1)


FWD, APPLY, BWD, BWD_APPLY, ADD2 = range(5)                     # SG_BN_FWD .. SG_BN_ADD2
PERIODS = {FWD: 4, APPLY: 4, BWD: 1, BWD_APPLY: 1, ADD2: 2}     # BN_APPLY_PERIODS / BN_BWD_PERIODS / BN_ADD2_PERIODS (csrc/norm.hip)
EW_CAP = 8192
BN_FIELDS = tuple(n for n, _ in BnPlan._fields_)
SEG_FIELDS = tuple(n for n, _ in SegPlan._fields_)
PLANS = []               # every engine plan checked_plan() has handed out, in order (the child looks at its cases')


def fin_lanes(S):
    """(fused, lanes of the separate finalize launch) of a reduction with S row slabs, SG_SEG_FUSED at its default 1."""
    return (1, 0) if S == 1 else (0, 16 if (S >= 32 and LANES16) else 4)


def plan_mirror(cus, rows, C, dtype, pass_, aligned):
    """plan_bn: every field of sg_bn_plan_t; None where sg_add2_bn refuses."""
    z = dict.fromkeys(BN_FIELDS, 0)
    vec = bool(aligned) and C % 4 == 0
    V = z["V"] = apply_v(C, dtype, vec)
    grid = bn_cols_grid(cus, rows, C // V, PERIODS[pass_]) if (vec and (COLS_ON or pass_ == ADD2)) else None
    if grid:
        z.update(cols=1, prow=grid[0], gx=grid[1], gy=grid[2])
    elif pass_ == ADD2:
        return None
    else:
        z.update(gx=max(1, min(-(-(rows * (C // V)) // 256), EW_CAP)), gy=1)
    if pass_ in (FWD, BWD):
        p = seg_plan(cus, rows, C, vec, wide8=(dtype == BF16), nout=2)
        fused, lanes = fin_lanes(p["S"])
        z.update(seg_V=p["V"], seg_TX=p["TX"], seg_TY=p["TY"], seg_gx=p["gx"], seg_S=p["S"], fused=fused, fin_lanes=lanes,
                 ws_bytes=p["part_bytes"])
    return z


def reduce_name(V, TX, gx, S, rows, fused, lanes):
    return f"V{V}tx{TX}gx{gx}.{regime(S)}{'+short' if short_last_slab(rows, S) else ''}.{'fused' if fused else f'fin{lanes}'}"


def name_of(z, rows, pass_=FWD):
    """The kernels of one call, from the fields of a plan (the engine's or the mirror's)."""
    if pass_ == ADD2:
        return f"add2.V{z['V']}p{z['prow']}b{z['gx']}k{z['gy']}"
    form = f"cols{z['V']}p{z['prow']}b{z['gx']}k{z['gy']}" if z["cols"] else f"flat{z['V']}"
    if not z["seg_V"]:
        return "apply." + form
    return reduce_name(z["seg_V"], z["seg_TX"], z["seg_gx"], z["seg_S"], rows, z["fused"], z["fin_lanes"]) + "." + form


def plan(cus, rows, C, dtype, off, pass_=FWD):
    """The names of the kernels one call takes, from the mirror.  off: some tensor operand is not 16-byte aligned."""
    return name_of(plan_mirror(cus, rows, C, dtype, pass_, not off), rows, pass_)


def seg_name(p, rows):
    return reduce_name(p["V"], p["TX"], p["gx"], p["S"], rows, *fin_lanes(p["S"]))


def num_cus(engine):
    return engine.lib.sg_num_cus(engine.h)


def plan_query(engine, rows, C, dtype, pass_, aligned):
    """(return code, fields) of sg_bn_plan."""
    p = BnPlan()
    rc = engine.lib.sg_bn_plan(engine.h, sgdt(dtype), rows, C, pass_, int(bool(aligned)), CT.byref(p))
    return rc, {n: getattr(p, n) for n in BN_FIELDS}


def seg_query(engine, nout, rows, C, vec, wide8=False, nseg=1):
    """(return code, fields) of sg_seg_plan."""
    p = SegPlan()
    rc = engine.lib.sg_seg_plan(engine.h, nout, nseg, rows, C, int(bool(vec)), int(bool(wide8)), CT.byref(p))
    return rc, {n: getattr(p, n) for n in SEG_FIELDS}


def _same(what, got, want):
    diff = {n: (got[n], want[n]) for n in want if got[n] != want[n]}
    assert not diff, f"{what}: (engine, mirror) differ in {diff}"


def checked_plan(engine, rows, C, dtype, pass_, aligned):
    """The predicate of a case, asserted before it launches: the engine's plan equals plan_mirror in every field for this device's
    CU count, and names the kernels the case was written for (at REF_CUS).  Returns that name, built from the engine's fields."""
    what = f"sg_bn_plan rows={rows} C={C} {dname(dtype)} pass={pass_} aligned={int(bool(aligned))}"
    rc, got = plan_query(engine, rows, C, dtype, pass_, aligned)
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    _same(what, got, plan_mirror(num_cus(engine), rows, C, dtype, pass_, aligned))
    here, ref = name_of(got, rows, pass_), plan(REF_CUS, rows, C, dtype, not aligned, pass_)
    assert here == ref, f"{what}: {num_cus(engine)} CUs take {here}, the case was chosen for {ref}"
    PLANS.append(got)
    return here


def checked_seg_plan(engine, nout, rows, C, vec):
    """The same for a column sum on the segment reducer alone (sg_bias_grad, sg_bn_train_fwd_tiles: fp32 sums, never V = 8)."""
    what = f"sg_seg_plan nout={nout} rows={rows} C={C} vec={int(bool(vec))}"
    rc, got = seg_query(engine, nout, rows, C, vec)
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    _same(what, got, seg_plan(num_cus(engine), rows, C, vec, nout=nout))
    here, ref = seg_name(got, rows), seg_name(seg_plan(REF_CUS, rows, C, vec, nout=nout), rows)
    assert here == ref, f"{what}: {num_cus(engine)} CUs take {here}, the case was chosen for {ref}"
    return here


def rows_for(C, want, vec=None, wide8=False, nout=2):
    """The smallest rows (of a ladder that is no multiple of anything) whose reduction at REF_CUS runs in regime `want`, with a
    short last slab when the rows are split."""
    vec = (C % 4 == 0) if vec is None else vec
    ty = seg_plan(REF_CUS, 1, C, vec, wide8, nout)["TY"]
    if want == "one":
        return 67
    for j in range(1 << 14):
        r = ty * 16 + 8 + 64 * j
        assert r * C <= (1 << 21), f"C={C}: regime '{want}' needs more than 2 M elements at {REF_CUS} CUs"
        S = seg_plan(REF_CUS, r, C, vec, wide8, nout)["S"]
        if regime(S) == want and short_last_slab(r, S):
            return r
    raise AssertionError((C, want))


C64_ROWS = (1, 3, 17, 130, 256, 520, 4100)
OTHER_CS = ((1, "one"), (1, "few"), (1, "many"), (4, "one"), (4, "few"), (8, "one"), (8, "many"), (20, "one"), (20, "few"), (20, "many"),
            (45, "one"), (45, "few"), (45, "many"), (68, "one"), (68, "few"), (72, "one"), (72, "few"), (72, "many"),
            (728, "one"), (728, "few"), (728, "many"))
SHAPES = [(64, r) for r in C64_ROWS] + [(c, rows_for(c, w)) for c, w in OTHER_CS]
# through offset pointers every C takes the scalar plan (TX = 16 from C = 16 on): a few shapes, every regime
OFF_SHAPES = [(64, 3), (64, 130), (64, 520), (64, 4100), (1, 67), (4, rows_for(4, "few", vec=False)), (20, 67),
              (72, rows_for(72, "few", vec=False))]
# sg_add2_bn: C % 4 == 0 only; rows around the two-period unroll of its grid (prow = 256 / gcd(256, C / V))
ADD2_SHAPES = [(4, 1), (4, 515), (8, 67), (20, 67), (20, 777), (64, 3), (64, 130), (64, 520), (72, 520), (728, 67), (728, 300)]
# sg_bias_grad: C, rows (seg_plan<1>: no V = 8)
BIAS_SHAPES = [(1, 67), (4, 67), (4, rows_for(4, "few", nout=1)), (45, 67), (45, rows_for(45, "few", nout=1)),
               (45, rows_for(45, "many", nout=1)), (64, 1), (64, 130), (64, 520), (64, 4100), (68, 300), (728, 300)]
# sg_bn_train_fwd_tiles: C, rows; the reducer's rows are the tiles (C = 64: S = 1 up to 256 tiles, S = ceil(tiles / 64) after)
TILE_SHAPES = [(64, 100), (64, 128), (64, 7 * BM - 91), (64, 260 * BM - 5), (64, 2100 * BM - 77), (45, 3 * BM + 1),
               (45, 300 * BM - 64), (4, 40 * BM + 17), (728, 5 * BM - 1)]


def kinds_for(C, dtype):
    """x = 1000 + N(0, 1) in bf16 is a handful of distinct numbers: there the ordinary input is the better test of most shapes."""
    return ("plain", "mean1000") if (dtype == F32 or C == 64) else ("plain",)


# ================================================================================================ inputs
def const_channel(C):
    return C // 2 if C >= 2 else None     # (C = 1 has no channel to spare)


def gap_beta(v, target, need):
    """The middle of the widest gap between sorted values v within reach of `target`: the window doubles until it holds a gap
    whose half is 1.25 x `need`; beyond the extremes everything is gap."""
    s = torch.sort(v).values
    pad = max(1.0, 8.0 * need)
    e = torch.cat([s[:1] - pad, s, s[-1:] + pad])
    gaps, mids = e[1:] - e[:-1], (e[1:] + e[:-1]) / 2
    ok = gaps >= 2.5 * need
    w = 0.25
    while True:
        sel = ok & (mids >= target - w) & (mids <= target + w)
        if sel.any():
            i = torch.argmax(torch.where(sel, gaps, torch.zeros_like(gaps)))
            return float(mids[i])
        w *= 2


class Inputs:
    pass


@functools.lru_cache(maxsize=None)
def inputs(C, rows, dtype, kind):
    """x (storage type), dy, fp32 parameters and moving values, and the float64 statistics of the STORED x.  kind: "plain" (per
    channel mean in [-1, 1], sigma in [0.5, 2]), "mean1000" (1000 + N(0, 1)), "pivot4" / "pivot16" (N(0, 1) with row 0 - the
    kernels' pivot - at +-k sigma).  One channel is constant.  beta: gap_beta, so that no gamma * xhat + beta is within
    1e-4 max|y| of the fused ReLU's boundary (asserted here, from the reference alone)."""
    g = gen(f"bn{C}.{rows}.{dtype}.{kind}")
    z = torch.randn(rows, C, generator=g, dtype=torch.float64)
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0).double()
    if kind == "plain":
        x = z * (0.5 + 1.5 * torch.rand(C, generator=g).double()) + (2 * torch.rand(C, generator=g).double() - 1)
    elif kind == "mean1000":
        x = 1000.0 + z
    else:
        x = z
        x[0] = float(kind[5:]) * sign
    cc = const_channel(C)
    if cc is not None:
        x[:, cc] = 1000.25 if kind == "mean1000" else 0.75
    I = Inputs()
    I.C, I.rows, I.dtype, I.kind, I.cc = C, rows, dtype, kind, cc
    I.apart = () if cc is None else (cc,)
    I.x = x.float().to(dtype)
    I.x64 = I.x.double()
    I.dy = rnd(g, rows, C, dtype=dtype)
    gamma = (rnd(g, C) + 1.5).double() * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0).double()
    I.gamma = gamma.float()
    I.mm, I.mv = rnd(g, C) + (1000.0 if kind == "mean1000" else 0.0), rnd(g, C, lo=0.5, hi=2.0)
    I.mean, I.var = bn_stats_ref(I.x64)
    I.invstd = 1.0 / torch.sqrt(I.var + EPS)
    I.mean32, I.invstd32 = I.mean.float(), I.invstd.float()
    v = -(I.gamma.double() * ((I.x64 - I.mean) * I.invstd))       # beta = v[r] puts row r on the ReLU's boundary
    target = (3 * torch.rand(C, generator=g).double() - 1.5) * I.gamma.double().abs()
    need = 1e-4 * (float(v.abs().max()) + float(target.abs().max()) + 0.5)
    beta = torch.tensor([gap_beta(v[:, c], float(target[c]), need) for c in range(C)], dtype=torch.float64)
    if cc is not None:
        beta[cc] = 0.375 * float(sign[cc])                        # xhat = 0 there: gamma * xhat + beta = beta, |beta| >= 2^-7
    I.beta = beta.float()
    t = I.beta.double() - v
    I.ymax = float(t.abs().max())
    I.margin = float(t.abs().min())
    assert I.margin >= 1e-4 * I.ymax, f"C={C} rows={rows} {kind}: {I.margin:.3e} from the ReLU boundary, max|y| = {I.ymax:.3e}"
    I.mask = t > 0
    # the same mask from the fp32-rounded statistics the backward is handed, and from the stored y
    t32 = I.gamma.double() * ((I.x64 - I.mean32.double()) * I.invstd32.double()) + I.beta.double()
    assert torch.equal(t32 > 0, I.mask) and float(t32.abs().min()) >= 0.5e-4 * I.ymax
    I.y_relu = torch.relu(t32).to(dtype)
    assert torch.equal(I.y_relu.float() > 0, I.mask)
    return I


def stat_tol(kind):
    """fp32 statistics: the element-wise tolerance; the k = 16 pivot outlier is held at the reduced one."""
    return 1e-4 if kind == "pivot16" else 2e-5


def y_tol(dtype, kind):
    return 2.0 ** -7 if dtype == BF16 else stat_tol(kind)


def compare_forward(I, y, mean, invstd, mm, mv, relu, unb, what, entry="bn_train_fwd"):
    """The whole forward comparison, on tensors (the CPU self-check hands it statistics with a planted error)."""
    g64, b64 = I.gamma.double(), I.beta.double()
    yr, mr, ir, nmm, nmv = bn_fwd_ref(I.x64, g64, b64, I.mm.double(), I.mv.double(), MOMENTUM, EPS, relu, unb)
    st, rec = stat_tol(I.kind), lambda n: record(f"{entry}.{n}", I.kind, I.dtype)
    close_cols(mean, mr, st, what + " mean", report=rec("mean"))
    close_cols(invstd, ir, st, what + " invstd", apart=I.apart, report=rec("invstd"))
    close_cols(mm, nmm, st, what + " moving mean", report=rec("moving_mean"))
    close_cols(mv, nmv, st, what + " moving var", report=rec("moving_var"))
    # save_mean is an fp32 number: y may be off by |gamma| invstd ulp32(mean) / 2 on top of the tolerance
    extra = g64.abs() * ir * ulp32(mr) / 2
    close_cols(y, yr, y_tol(I.dtype, I.kind), what + " y", extra=extra, report=rec("y"))


# ================================================================================================ the cases
def bn_ws(engine, rows, C):
    """The workspace query, checked against the three plans it has to cover."""
    nws = engine.lib.sg_bn_ws_bytes(engine.h, rows, C)
    cus = num_cus(engine)
    want = max(seg_plan(cus, rows, C, True, nout=2)["part_bytes"], seg_plan(cus, rows, C, False, nout=2)["part_bytes"],
               seg_plan(cus, rows, C, True, True, 2)["part_bytes"]) + 256
    assert nws == want, (rows, C, nws, want)
    return nws


def fwd_case(engine, C, rows, dtype, off, kind, off_only=None):
    """sg_bn_train_fwd: (relu, unbiased_update) = (0, 1) and (1, 0).  off_only: only that operand ("x" or "y") is offset."""
    I, dt = inputs(C, rows, dtype, kind), sgdt(dtype)
    name = checked_plan(engine, rows, C, dtype, FWD, not (off or off_only))
    nws = bn_ws(engine, rows, C)
    po = off and not off_only           # the fp32 vectors move with the tensors
    for relu, unb in ((0, 1), (1, 0)):
        what = f"bn_train_fwd C={C} rows={rows} {dname(dtype)} off={off_only or off} {kind} relu={relu} unbiased={unb} [{name}]"
        X, Gm, Bt = G(I.x, off and off_only in (None, "x")), G(I.gamma, po), G(I.beta, po)
        MM, MV = G(I.mm, po, role="out"), G(I.mv, po, role="out")
        Y, SM, SI = GO((rows, C), dtype, off and off_only in (None, "y")), GO((C,), F32, po), GO((C,), F32, po)
        W = Guarded.ws(nws, DEV)
        rc = call(engine, "sg_bn_train_fwd", dt, rows, C, X.ptr(), Gm.ptr(), Bt.ptr(), MM.ptr(), MV.ptr(), Y.ptr(), SM.ptr(),
                  SI.ptr(), MOMENTUM, EPS, relu, unb, W.ptr(), nws)
        done(engine, rc, what, X, Gm, Bt, MM, MV, Y, SM, SI, W)
        for o in (Y, SM, SI):
            assert_written(o.read(), what)
        compare_forward(I, Y.read(), SM.read(), SI.read(), MM.read(), MV.read(), relu, unb, what)
    return name


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def bwd_case(engine, C, rows, dtype, off, kind, off_only=None):
    """sg_bn_train_bwd in its three mask modes; mean / invstd / y are the float64 reference's, rounded to their storage."""
    I, dt = inputs(C, rows, dtype, kind), sgdt(dtype)
    name = checked_plan(engine, rows, C, dtype, BWD, not (off or off_only))
    nws = bn_ws(engine, rows, C)
    po = off and not off_only
    g64, m64, i64 = I.gamma.double(), I.mean32.double(), I.invstd32.double()
    got = {}
    for mode in (0, 1, 2):
        if off_only == "y" and mode != 1:
            continue
        what = f"bn_train_bwd mode={mode} C={C} rows={rows} {dname(dtype)} off={off_only or off} {kind} [{name}]"
        isoff = lambda n: off and off_only in (None, n)
        X, DY, Gm, SM, SI = G(I.x, isoff("x")), G(I.dy, isoff("dy")), G(I.gamma, po), G(I.mean32, po), G(I.invstd32, po)
        Yi = G(I.y_relu, isoff("y")) if mode == 1 else None
        Bt = G(I.beta, po) if mode == 2 else None
        DX, DG, DB, W = GO((rows, C), dtype, isoff("dx")), GO((C,), F32, po), GO((C,), F32, po), Guarded.ws(nws, DEV)
        rc = call(engine, "sg_bn_train_bwd", dt, rows, C, X.ptr(), Yi.ptr() if Yi else None, DY.ptr(), Gm.ptr(),
                  Bt.ptr() if Bt else None, SM.ptr(), SI.ptr(), DX.ptr(), DG.ptr(), DB.ptr(), int(mode != 0), W.ptr(), nws)
        done(engine, rc, what, X, DY, Gm, SM, SI, DX, DG, DB, W, *[o for o in (Yi, Bt) if o])
        for o in (DX, DG, DB):
            assert_written(o.read(), what)
        dxr, dgr, dbr = bn_bwd_ref(I.x64, I.dy.double(), g64, m64, i64, I.mask.double() if mode else None)
        rec = lambda n: record(f"bn_train_bwd.{n}", kind, dtype)
        close_cols(DG.read(), dgr, 1e-4, what + " dgamma", report=rec("dgamma"))
        close_cols(DB.read(), dbr, 1e-4, what + " dbeta", report=rec("dbeta"))
        close_cols(DX.read(), dxr, tol(dtype, True), what + " dx", apart=I.apart, report=rec("dx"))
        got[mode] = (DX.read(), DG.read(), DB.read())
    if 1 in got and 2 in got:
        for a, b, n in zip(got[1], got[2], ("dx", "dgamma", "dbeta")):
            assert _bits_equal(a, b), f"{name}: {n} with the mask recomputed from x is not bit-identical to the mask read from y"
    return name


def bwd_apply_case(engine, C, rows, dtype, off, kind):
    """sg_bn_train_bwd_apply: dgamma / dbeta are the reference's column sums (fp32); relu = 1 recomputes the mask from x."""
    I, dt = inputs(C, rows, dtype, kind), sgdt(dtype)
    name = checked_plan(engine, rows, C, dtype, BWD_APPLY, not off)
    g64, m64, i64 = I.gamma.double(), I.mean32.double(), I.invstd32.double()
    for relu in (0, 1):
        what = f"bn_train_bwd_apply relu={relu} C={C} rows={rows} {dname(dtype)} off={off} {kind} [{name}]"
        mask = I.mask.double() if relu else None
        _, dg, db = bn_bwd_ref(I.x64, I.dy.double(), g64, m64, i64, mask)
        dg, db = dg.float(), db.float()
        X, DY, Gm, Bt, SM, SI = G(I.x, off), G(I.dy, off), G(I.gamma, off), G(I.beta, off), G(I.mean32, off), G(I.invstd32, off)
        DG, DB, DX = G(dg, off), G(db, off), GO((rows, C), dtype, off)
        rc = call(engine, "sg_bn_train_bwd_apply", dt, rows, C, X.ptr(), DY.ptr(), Gm.ptr(), Bt.ptr() if relu else None, SM.ptr(),
                  SI.ptr(), DG.ptr(), DB.ptr(), DX.ptr(), relu)
        done(engine, rc, what, X, DY, Gm, Bt, SM, SI, DG, DB, DX)
        assert_written(DX.read(), what)
        dxr, _, _ = bn_bwd_ref(I.x64, I.dy.double(), g64, m64, i64, mask, dg.double(), db.double())
        close_cols(DX.read(), dxr, tol(dtype, True), what, apart=I.apart, report=record("bn_train_bwd_apply.dx", kind, dtype))
    return name


def apply_case(engine, C, rows, dtype, off, kind):
    """sg_bn_apply (given mean / invstd) and sg_bn_infer (moving mean / variance, eps inside the kernel), relu 0 and 1."""
    I, dt = inputs(C, rows, dtype, kind), sgdt(dtype)
    name = checked_plan(engine, rows, C, dtype, APPLY, not off)
    g64, b64 = I.gamma.double(), I.beta.double()
    g = gen(f"infer{C}.{rows}.{kind}")
    mm = (I.mean + 0.1 * (2 * torch.rand(C, generator=g).double() - 1)).float()     # moving values near, not at, the batch's
    mv = (I.var * (0.5 + 1.5 * torch.rand(C, generator=g).double())).float()
    for relu in (0, 1):
        what = f"C={C} rows={rows} {dname(dtype)} off={off} {kind} relu={relu} [{name}]"
        X, Gm, Bt, SM, SI, Y = G(I.x, off), G(I.gamma, off), G(I.beta, off), G(I.mean32, off), G(I.invstd32, off), GO((rows, C), dtype, off)
        rc = call(engine, "sg_bn_apply", dt, rows, C, X.ptr(), Gm.ptr(), Bt.ptr(), SM.ptr(), SI.ptr(), Y.ptr(), relu)
        done(engine, rc, "bn_apply " + what, X, Gm, Bt, SM, SI, Y)
        assert_written(Y.read(), what)
        close_cols(Y.read(), bn_apply_ref(I.x64, g64, b64, I.mean32.double(), I.invstd32.double(), relu), tol(dtype),
                   "bn_apply " + what, report=record("bn_apply.y", kind, dtype))
        X, Gm, Bt, MM, MV, Y = G(I.x, off), G(I.gamma, off), G(I.beta, off), G(mm, off), G(mv, off), GO((rows, C), dtype, off)
        rc = call(engine, "sg_bn_infer", dt, rows, C, X.ptr(), Gm.ptr(), Bt.ptr(), MM.ptr(), MV.ptr(), Y.ptr(), EPS, relu)
        done(engine, rc, "bn_infer " + what, X, Gm, Bt, MM, MV, Y)
        assert_written(Y.read(), what)
        ref = bn_apply_ref(I.x64, g64, b64, mm.double(), 1.0 / torch.sqrt(mv.double() + float(torch.tensor(EPS))), relu)
        close_cols(Y.read(), ref, tol(dtype), "bn_infer " + what, report=record("bn_infer.y", kind, dtype))
    return name


def add2_plan(cus, rows, C, dtype):
    return plan(cus, rows, C, dtype, False, ADD2)


ADD2_COMBOS = [(na, nb, infer, rl) for na in (0, 1) for nb in (0, 1) for infer in (0, 1) for rl in ((1, 0, 1), (0, 1, 0))]


def add2_case(engine, C, rows, dtype, kind):
    """sg_add2_bn: normalise a, b, both or neither; operand ReLUs and the outer one; training and inference parameters."""
    I, dt = inputs(C, rows, dtype, kind), sgdt(dtype)
    name = checked_plan(engine, rows, C, dtype, ADD2, True)
    g = gen(f"add2{C}.{rows}.{dtype}")
    b = rnd(g, rows, C, dtype=dtype, lo=-2, hi=2)
    pb32 = (rnd(g, C), rnd(g, C, lo=0.5, hi=2.0), rnd(g, C) + 1.5, rnd(g, C))       # mean, invstd | variance, gamma, beta
    for na, nb, infer, (a_relu, b_relu, relu) in ADD2_COMBOS:
        pa32 = (I.mean32, (I.var.float() if infer else I.invstd32), I.gamma, I.beta)
        what = f"add2_bn a={na} b={nb} infer={infer} relus={a_relu}{b_relu}{relu} C={C} rows={rows} {dname(dtype)} {kind} [{name}]"
        A, B, Y = G(I.x), G(b), GO((rows, C), dtype)
        PA, PB = [G(t) for t in pa32] if na else [], [G(t) for t in pb32] if nb else []
        rc = call(engine, "sg_add2_bn", dt, rows, C, A.ptr(), B.ptr(), *([p.ptr() for p in PA] or [None] * 4),
                  *([p.ptr() for p in PB] or [None] * 4), Y.ptr(), relu, infer, EPS, a_relu, b_relu)
        done(engine, rc, what, A, B, Y, *PA, *PB)
        assert_written(Y.read(), what)
        eps64 = float(torch.tensor(EPS))
        ref = add2_bn_ref(I.x64, b.double(), [t.double() for t in pa32] if na else None, [t.double() for t in pb32] if nb else None,
                          relu, infer, eps64, a_relu, b_relu)
        close_cols(Y.read(), ref, tol(dtype), what, report=record("add2_bn.y", kind, dtype))
    return name


def add2_refusal_case(engine, dtype):
    """SG_EUNSUPPORTED for C % 4 != 0 and for any operand that is not 16-byte aligned; the output keeps its prefill."""
    dt = sgdt(dtype)
    for C, offs in ((45, (False, False, False)), (64, (True, False, False)), (64, (False, True, False)), (64, (False, False, True))):
        I = inputs(C, 67, dtype, "plain")
        A, B, Y = G(I.x, offs[0]), G(I.dy, offs[1]), GO((67, C), dtype, offs[2])
        P = [G(t) for t in (I.mean32, I.invstd32, I.gamma, I.beta)]
        rc = call(engine, "sg_add2_bn", dt, 67, C, A.ptr(), B.ptr(), *[p.ptr() for p in P], *[None] * 4, Y.ptr(), 1, 0, EPS, 0, 0)
        assert rc == SG_EUNSUPPORTED, (C, offs, rc)
        check_all([A, B, Y] + P, f"add2_bn refusal C={C} offs={offs}")
        assert torch.isnan(Y.read().float()).all(), f"add2_bn refused C={C} offs={offs} and still wrote its output"


def bias_case(engine, C, rows, dtype, form):
    """sg_bias_grad.  form: "dense" (ld == C), "slice" (ld = C + 16, the channels [8, 8 + C) of a wider buffer), "odd" (ld = C + 3,
    channels [1, 1 + C): the scalar plan), "offset" (dense, one element past 16-byte alignment)."""
    dt, g = sgdt(dtype), gen(f"bias{C}.{rows}.{dtype}.{form}")
    ld, mid = {"dense": (C, 0), "slice": (C + 16, 8), "odd": (C + 3, 1), "offset": (C, 0)}[form]
    off = form == "offset"
    vec = C % 4 == 0 and ld % 4 == 0 and not off
    name = checked_seg_plan(engine, 1, rows, C, vec)
    cus = num_cus(engine)
    nws = engine.lib.sg_bias_grad_ws_bytes(engine.h, rows, C)
    assert nws == max(seg_plan(cus, rows, C, True)["part_bytes"], seg_plan(cus, rows, C, False)["part_bytes"]) + 256
    wide = (rnd(g, rows, ld, dtype=dtype).float() + 0.25).to(dtype)
    what = f"bias_grad {form} C={C} rows={rows} ld={ld} {dname(dtype)} [{name}]"
    DY, DB, W = G(wide, off), GO((C,), F32, off), Guarded.ws(nws, DEV)
    rc = call(engine, "sg_bias_grad", dt, rows, C, 0 if form == "dense" else ld, DY.ptr(mid), DB.ptr(), W.ptr(), nws)
    done(engine, rc, what, DY, DB, W)
    assert_written(DB.read(), what)
    close_cols(DB.read(), colsum_ref(wide[:, mid:mid + C].double()), 1e-4, what, report=record("bias_grad", "plain", dtype))
    return name


@functools.lru_cache(maxsize=None)
def tile_inputs(C, rows, kind):
    """stats[tiles][2][C] in fp32 from float64 rows drawn 64 tiles at a time, and the float64 (mean, variance) of all rows: the
    sums are taken about the generator's own centre K, so nothing cancels in float64 either."""
    g = gen(f"tiles{C}.{rows}.{kind}")
    mu = torch.full((C,), 1000.0, dtype=torch.float64) if kind == "mean1000" else 2 * torch.rand(C, generator=g).double() - 1
    sg = torch.ones(C, dtype=torch.float64) if kind == "mean1000" else 0.5 + 1.5 * torch.rand(C, generator=g).double()
    cc = const_channel(C)
    stats, s1, s2 = [], torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for r0 in range(0, rows, 64 * BM):
        n = min(64 * BM, rows - r0)
        x = (torch.randn(n, C, generator=g, dtype=torch.float64) * sg + mu).float().double()   # fp32 activations
        if cc is not None:
            x[:, cc] = float(mu[cc].float())
        stats.append(tile_stats_ref(x, BM))
        s1 += (x - mu).sum(0)
        s2 += ((x - mu) ** 2).sum(0)
    m1 = s1 / rows
    return torch.cat(stats).float(), mu + m1, s2 / rows - m1 * m1


def tiles_case(engine, C, rows, dtype, off, kind):
    """sg_bn_train_fwd_tiles against the float64 statistics of the whole tensor; unbiased_update 0 and 1."""
    dt = sgdt(dtype)
    tiles = -(-rows // BM)
    stats, mean, var = tile_inputs(C, rows, kind)
    assert stats.shape == (tiles, 2, C)
    name = checked_seg_plan(engine, 2, tiles, C, C % 4 == 0 and not off) + (".ragged" if rows % BM else "")
    cus = num_cus(engine)
    nws = engine.lib.sg_bn_tiles_ws_bytes(engine.h, tiles, C)
    assert nws == seg_plan(cus, tiles, C, True, nout=2)["part_bytes"] + seg_plan(cus, tiles, C, False, nout=2)["part_bytes"]
    g = gen(f"tilesmv{C}.{rows}")
    mm, mv = rnd(g, C) + (1000.0 if kind == "mean1000" else 0.0), rnd(g, C, lo=0.5, hi=2.0)
    invstd = 1.0 / torch.sqrt(var + EPS)
    apart = () if const_channel(C) is None else (const_channel(C),)
    for unb in (0, 1):
        what = f"bn_train_fwd_tiles C={C} rows={rows} tiles={tiles} {dname(dtype)} off={off} {kind} unbiased={unb} [{name}]"
        ST, MM, MV = G(stats, off), G(mm, off, role="out"), G(mv, off, role="out")
        SM, SI, W = GO((C,), F32, off), GO((C,), F32, off), Guarded.ws(nws, DEV)
        rc = call(engine, "sg_bn_train_fwd_tiles", dt, rows, C, ST.ptr(), tiles, MM.ptr(), MV.ptr(), SM.ptr(), SI.ptr(), MOMENTUM,
                  EPS, unb, W.ptr(), nws)
        done(engine, rc, what, ST, MM, MV, SM, SI, W)
        for o in (SM, SI):
            assert_written(o.read(), what)
        var_u = var * (rows / (rows - 1.0)) if (unb and rows > 1) else var
        rec = lambda n: record(f"bn_train_fwd_tiles.{n}", kind, dtype)
        close_cols(SM.read(), mean, 1e-4, what + " mean", report=rec("mean"))
        close_cols(SI.read(), invstd, 1e-4, what + " invstd", apart=apart, report=rec("invstd"))
        close_cols(MM.read(), mm.double() * MOMENTUM + mean * (1 - MOMENTUM), 1e-4, what + " moving mean", report=rec("moving_mean"))
        close_cols(MV.read(), mv.double() * MOMENTUM + var_u * (1 - MOMENTUM), 1e-4, what + " moving var", report=rec("moving_var"))
    return name


# ================================================================================================ the forms behind switches
CHILD_ENV = {"SG_BN_COLS": "0", "SG_FINALIZE_LANES": "4"}
CHILD_SHAPES = [(64, 130), (64, 4100), (20, 67), (72, rows_for(72, "many"))]


def child_cases():
    """(label, function, arguments): the aligned, vectorisable subset - with SG_BN_COLS=0 the flat V = 4 / V = 8 apply and
    backward-apply kernels, with SG_FINALIZE_LANES=4 the 4-lane finalize behind S >= 32."""
    out = []
    for C, rows in CHILD_SHAPES:
        for dtype in (F32, BF16):
            for fn in (fwd_case, bwd_case, bwd_apply_case, apply_case):
                out.append((f"{fn.__name__} C={C} rows={rows} {dname(dtype)}", fn, (C, rows, dtype, False, "plain")))
    return out


def main():
    global QUIET
    QUIET = True
    assert not COLS_ON and not LANES16, "run with SG_BN_COLS=0 SG_FINALIZE_LANES=4"
    from building_detection_amd.ops import get_engine
    engine = get_engine(0)
    lines = []
    for label, fn, args in child_cases():
        seen = len(PLANS)
        name = fn(engine, *args)
        # the ENGINE's plan of this case: the switches took effect in the library, not only in this file's reading of them
        mine = PLANS[seen:]
        assert mine and all(p["cols"] == 0 and p["fin_lanes"] in (0, 4) for p in mine), (label, mine)
        assert all(p["fin_lanes"] == 4 for p in mine if p["seg_S"] >= 32), (label, mine)
        assert ".flat" in name and "fin16" not in name, name
        lines.append(f"CASE ok {label} [{name}]")
    many = [ln for ln in lines if ".many" in ln]
    assert many and all(".fin4" in ln for ln in many), "no case reached the 4-lane finalize behind S >= 32"
    sys.stdout.flush()
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()
