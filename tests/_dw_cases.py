"""The cases of tests/test_depthwise_variants_gpu.py: the depthwise convolution entry points of csrc/spatial.hip (sg_dwconv2d_fwd,
sg_dwconv2d_dgrad, sg_dwconv2d_wgrad) through the C ABI on tests/_guarded.py arenas, each launch against plain float64
(F.conv2d(groups = C) on the explicitly padded tensor, autograd for dx and dw).

A case states which kernel its launch takes - from the mirrors below of the parts of plan_dw (csrc/spatial.hip): dw_run_ok,
dw_stencil_strips_ok, dw_wgrad_strips_ok, dw_rows_per_run, plan_dw_stencil_run, plan_dw_stencil_strip, plan_dw_wgrad_strip and
(tests/_guarded.py) seg_plan - and asserts before launching that the mirrors say the same for this device's CU count as for the 256
CUs the shapes were chosen at, and that the engine's own plan (sg_dwconv2d_plan) equals plan_mirror field by field.

Run as a program (`python tests/_dw_cases.py` with one of CHILD_ENVS in the environment: the switches are read once per process)
it runs child_cases() of that environment and prints one `CASE ok|FAIL ...` line per case, then its records."""
import ctypes as CT
import functools
import os
import sys
import traceback

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from _bn_cases import gap_beta
from _guarded import (Guarded, assert_written, bn_sums_ref, check_all, dw_conv_ref, dw_geom, dw_grads_ref, gaps_keep_prefill,
                      regime, seg_plan, untouched, widen)
from building_detection_amd._lib import BnIn, ConvDesc, DwBnSums, DwPlan
from test_bandwidth_variants_gpu import BF16, DEV, F32, G, GO, SP_CAP, call, gen, rnd, sgdt

REF_CUS = 256
SG_EINVAL, SG_EWORKSPACE, SG_EUNSUPPORTED = -1, -2, -3
DW_SUMS_MAX_ROWS = 1024
SWITCH_NAMES = ("SG_DW_FSTRIP", "SG_DW_FSTRIP_HS", "SG_DW_STRIP", "SG_DW_RR")
QUIET = False
RECORDS = {}             # (kernel form, result, storage) -> largest observed error / scale (a record, not a threshold)
COUNTS = {}              # the same key -> comparisons made


def _atoll(v):
    try:
        return int(v.strip())
    except ValueError:
        return 0


def switches_of(env):
    """The four switches as csrc/sg_switch.h reads them (INT: atoll of the value, the default when unset)."""
    d = dict(SG_DW_FSTRIP=1, SG_DW_FSTRIP_HS=0, SG_DW_STRIP=1, SG_DW_RR=0)
    return {k: (_atoll(env[k]) if k in env else v) for k, v in d.items()}


SW = switches_of(os.environ)


class switched:
    """The mirrors as a process with `env` sees them (the parent lists a child's cases)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = dict(SW)
        SW.update(switches_of(self.env))

    def __exit__(self, *a):
        SW.update(self.old)


def dname(dtype):
    return "bf16" if dtype == BF16 else "f32"


def esize(dtype):
    return 2 if dtype == BF16 else 4


def record(form, qty, dtype, rel):
    if form == "selfcheck":      # the CPU self-checks compare planted errors: not a kernel's figure
        return
    key = (form, qty, dname(dtype))
    RECORDS[key] = max(RECORDS.get(key, 0.0), rel)
    COUNTS[key] = COUNTS.get(key, 0) + 1
    if not QUIET:
        print(f"REC {form} {qty} {dname(dtype)} rel={rel:.3e}")


def records_table():
    return "\n".join(f"REC {f} {q} {d} rel={RECORDS[(f, q, d)]:.3e} n={COUNTS.get((f, q, d), 0)}" for f, q, d in sorted(RECORDS))


def cmp(got, ref, t, what, form, qty, dtype):
    """max|got - ref| <= t * max|ref| over the whole tensor; the figure is recorded before anything is asserted."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    scale = ref.abs().max().item()
    diff = (got - ref).abs()
    err = float("inf") if not torch.isfinite(got).all() else diff.max().item()
    record(form, qty, dtype, err / scale if scale > 0 else (0.0 if err == 0 else float("inf")))
    assert torch.isfinite(got).all(), f"{what} {qty}: non-finite values in the result"
    assert err <= t * scale, f"{what} {qty}: max err {err:.3e} > {t:.3e} * {scale:.3e} (rel {err / max(scale, 1e-300):.2e})"


def etol(dtype):
    return 2.0 ** -7 if dtype == BF16 else 2e-5


RTOL = 1e-4      # fp32 reduced results (dw, dgamma, dbeta are fp32 whatever the activations' storage)


# ================================================================================================ geometry
class Geom:
    def __init__(self, N, H, W, C, KH=3, KW=3, s=1, d=1, same=True):
        self.N, self.H, self.W, self.C, self.KH, self.KW, self.s, self.d, self.same = N, H, W, C, KH, KW, s, d, same
        self.geom = dw_geom(H, W, KH, KW, s, d, same)
        self.Ho, self.Wo, self.pt, self.pb, self.pl, self.pr = self.geom
        self.key = (N, H, W, C, KH, KW, s, d, same)

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, o):
        return self.key == o.key

    @property
    def tag(self):
        t = f"n{self.N}h{self.H}w{self.W}c{self.C}"
        if (self.KH, self.KW) != (3, 3):
            t += f"k{self.KH}x{self.KW}"
        if self.s != 1:
            t += f"s{self.s}"
        if self.d != 1:
            t += f"d{self.d}"
        return t + ("" if self.same else "valid")

    def desc(self, xgap=0, ygap=0):
        return ConvDesc(self.N, self.H, self.W, self.C, self.C, self.KH, self.KW, self.s, self.d, self.pt, self.pl, self.Ho, self.Wo,
                        self.C + xgap if xgap else 0, self.C + ygap if ygap else 0)


# ================================================================================================ mirrors of the dispatch code
def cdiv(a, b):
    return -(-a // b)


def dw_run_ok(g):
    return (g.KH == 3 and g.KW == 3 and g.s == 1 and g.d == 1 and g.pt == 1 and g.pl == 1 and g.Ho == g.H and g.Wo == g.W
            and g.W % 4 == 0 and g.C % 4 == 0)


def dw_wgrad_strips_ok(g, xl, yl):
    return bool(SW["SG_DW_STRIP"]) and dw_run_ok(g) and g.H % 4 == 0 and g.N * g.H * g.W * max(xl, yl) * 4 < (1 << 30)


def dw_rows_per_run(H, pixels, wgrad):
    force = SW["SG_DW_RR"]
    want = force if force else ((1 if pixels <= 32768 else 2) if wgrad else 2)
    return 2 if (want >= 2 and H % 2 == 0) else 1


def dw_stencil_strips_ok(g, in_ld, es):
    on = SW["SG_DW_FSTRIP"]
    if not on or (on == 1 and g.H < 64):
        return False
    return g.H % 4 == 0 and g.W % 4 == 0 and g.N * g.H * g.W * in_ld * es < (1 << 30)


def plan_dw_stencil_strip(g, sums):
    """(HS, nstrips, gx, gy) of plan_dw_stencil_strip (with plan_dw_stencil_grid)."""
    hs_force = SW["SG_DW_FSTRIP_HS"]
    HS = hs_force if hs_force > 0 else (16 if g.H >= 64 else (8 if g.H >= 16 else g.H))
    if HS % 4 != 0 or HS > g.H:
        HS = 4
    nstrips = g.N * cdiv(g.H, HS) * (g.W // 4)
    gx = cdiv(g.C // 4, 16)
    gy = max(1, min(cdiv(nstrips, 16), cdiv(16384, gx)))
    if sums:
        gy = min(gy, DW_SUMS_MAX_ROWS)
    return HS, nstrips, gx, gy


def plan_dw_stencil_run(g, sums):
    """(rr, lc, gx, gy, nruns) of plan_dw_stencil_run (with plan_dw_stencil_grid)."""
    rr = dw_rows_per_run(g.H, g.N * g.H * g.W, False)
    nruns = g.N * (g.H // rr) * (g.W // 4)
    lc = 1
    while lc < g.C // 4 and lc < 64:
        lc <<= 1
    gx = cdiv(g.C // 4, lc)
    gy = max(1, min(cdiv(nruns, 256 // lc), cdiv(16384, gx)))
    if sums:
        gy = min(gy, DW_SUMS_MAX_ROWS)
    return rr, lc, gx, gy, nruns


def plan_dw_wgrad_strip(cus, g):
    """(HS, nhs, nstrips, gx, S) of plan_dw_wgrad_strip (the filter gradient's strips)."""
    HS = 16 if g.H >= 128 else (8 if g.H >= 16 else g.H)
    nhs = cdiv(g.H, HS)
    nstrips = g.N * nhs * (g.W // 4)
    gx = cdiv(g.C // 4, 16)
    S = max(1, min(cdiv(nstrips, 16), cdiv(4 * cus, gx), 256))
    return HS, nhs, nstrips, gx, S


def stencil_name(g, es, in_ld, sums):
    """The stencil kernel (forward, or dgrad of a stride-1 3x3 'same' layer) of one launch:
    run.RR<rows per run>lc<lanes per run>gx<column blocks>gy<rows of workgroups>.dead<lanes past the last chunk>[.trip2]
    strip.HS<strip height>[+short last band]r<remainder of the three-step unroll in the last band>gx..gy...dead..[.trip2]"""
    chunks = g.C // 4
    if dw_stencil_strips_ok(g, in_ld, es):
        HS, nstrips, gx, gy = plan_dw_stencil_strip(g, sums)
        last = g.H - (cdiv(g.H, HS) - 1) * HS
        name = f"strip.HS{HS}{'+short' if last != HS else ''}r{last % 3}gx{gx}gy{gy}.dead{gx * 16 - chunks}"
        return name + (".trip2" if nstrips > gy * 16 else "")
    rr, lc, gx, gy, nruns = plan_dw_stencil_run(g, sums)
    return f"run.RR{rr}lc{lc}gx{gx}gy{gy}.dead{gx * lc - chunks}" + (".trip2" if nruns > gy * (256 // lc) else "")


def fwd_name(g, dtype, vec, xl, form=""):
    """dw_fwd_kernel<V> (".cap": past ew_blocks' 16384 workgroups) or the stencil with its <RELU, -, BN, -> form."""
    if vec and dw_run_ok(g):
        return "fwd." + stencil_name(g, esize(dtype), xl, False) + (f".{form}" if form else "")
    V = 4 if vec else 1
    return f"fwd.V{V}" + (".cap" if g.N * g.Ho * g.Wo * (g.C // V) > SP_CAP else "")


def dgrad_name(g, dtype, vec, yl, form="", sums=False):
    if vec and dw_run_ok(g):
        return "dgrad." + stencil_name(g, esize(dtype), yl, sums) + (f".{form}" if form else "")
    V = 4 if vec else 1
    return f"dgrad.V{V}" + (".cap" if g.N * g.H * g.W * (g.C // V) > SP_CAP else "")


def wgrad_name(cus, g, vec, xl, yl, form=""):
    """strip.HS<band>[+short last band]gx<column blocks>.<one|few|many partial rows>[.capped: a slot walks a second strip]
    run.RR<rows per run>.V4tx<TX>gx<gx>.<regime> / seg.V<V>tx<TX>gx<gx>.<regime> (the segment reducer, tests/_guarded.seg_plan)"""
    rows = g.N * g.Ho * g.Wo
    tail = f".{form}" if form else ""
    if vec and dw_wgrad_strips_ok(g, xl, yl):
        HS, nhs, nstrips, gx, S = plan_dw_wgrad_strip(cus, g)
        return (f"wgrad.strip.HS{HS}{'+short' if g.H % HS else ''}gx{gx}.{regime(S)}{'.capped' if nstrips > S * 16 else ''}" + tail)
    if vec and dw_run_ok(g):
        rr = dw_rows_per_run(g.H, rows, True)
        p = seg_plan(cus, rows // (4 * rr), g.C, True, nout=9)
        return f"wgrad.run.RR{rr}.V{p['V']}tx{p['TX']}gx{p['gx']}.{regime(p['S'])}" + tail
    p = seg_plan(cus, rows, g.C, vec, nout=9)
    return f"wgrad.seg.V{p['V']}tx{p['TX']}gx{p['gx']}.{regime(p['S'])}" + tail


def wgrad_need(cus, g, vec, xl, yl):
    """The bytes of workspace the launch itself asks for."""
    rows = g.N * g.Ho * g.Wo
    if vec and dw_wgrad_strips_ok(g, xl, yl):
        return plan_dw_wgrad_strip(cus, g)[4] * 9 * g.C * 4
    if vec and dw_run_ok(g):
        return seg_plan(cus, rows // (4 * dw_rows_per_run(g.H, rows, True)), g.C, True, nout=9)["part_bytes"]
    return seg_plan(cus, rows, g.C, vec, nout=9)["part_bytes"]


def wgrad_ws_query(cus, g):
    """sg_dwconv2d_wgrad_ws_bytes."""
    rows = g.N * g.Ho * g.Wo
    m = max(seg_plan(cus, rows, g.C, True, nout=9)["part_bytes"], seg_plan(cus, rows, g.C, False, nout=9)["part_bytes"],
            seg_plan(cus, cdiv(rows, 4), g.C, True, nout=9)["part_bytes"])
    if dw_run_ok(g):
        m = max(m, plan_dw_wgrad_strip(cus, g)[4] * 9 * g.C * 4)
    return m + 256


def num_cus(engine):
    return engine.lib.sg_num_cus(engine.h)


def pinned(engine, fn, *a, **kw):
    """The predicate of a case, asserted: this device takes the kernel the case was written for."""
    here, ref = fn(num_cus(engine), *a, **kw), fn(REF_CUS, *a, **kw)
    assert here == ref, f"{num_cus(engine)} CUs take {here}, the case was chosen for {ref}"
    return here


FWD, DGRAD, WGRAD = 0, 1, 2                      # SG_DW_FWD, SG_DW_DGRAD, SG_DW_WGRAD
K_GENERIC, K_RUN, K_STRIP = 0, 1, 2              # SG_DWK_GENERIC, SG_DWK_RUN, SG_DWK_STRIP
PLAN_FIELDS = tuple(n for n, _ in DwPlan._fields_)


def plan_mirror(cus, g, dtype, direction, vec, xl, yl, sums=False):
    """plan_dw: every field of sg_dw_plan, from the mirrors above."""
    z = dict.fromkeys(PLAN_FIELDS, 0)
    fast = bool(vec and dw_run_ok(g))
    V = z["V"] = 4 if vec else 1
    if direction == WGRAD:
        rows = g.N * g.Ho * g.Wo
        z["bn"] = int(fast)
        z["ws_bytes"] = wgrad_need(cus, g, vec, xl, yl)
        if vec and dw_wgrad_strips_ok(g, xl, yl):
            HS, nhs, nstrips, gx, S = plan_dw_wgrad_strip(cus, g)
            z.update(family=K_STRIP, HS=HS, nhs=nhs, count=nstrips, gx=gx, S=S)
            return z
        if fast:
            z.update(family=K_RUN, RR=dw_rows_per_run(g.H, rows, True))
            rows = z["count"] = rows // (4 * z["RR"])
        p = seg_plan(cus, rows, g.C, vec, nout=9)
        z.update(seg_V=p["V"], seg_TX=p["TX"], seg_gx=p["gx"], seg_S=p["S"], S=p["S"])
        return z
    z.update({"bn": int(fast)} if direction == FWD else {"res": int(fast), "sums": int(fast)})
    if not fast:
        items = g.N * (g.Ho * g.Wo if direction == FWD else g.H * g.W) * (g.C // V)
        z.update(family=K_GENERIC, gx=max(1, min(cdiv(items, 256), 16384)), gy=1)
    elif dw_stencil_strips_ok(g, xl if direction == FWD else yl, esize(dtype)):
        HS, nstrips, gx, gy = plan_dw_stencil_strip(g, sums)
        z.update(family=K_STRIP, HS=HS, nhs=cdiv(g.H, HS), count=nstrips, gx=gx, gy=gy)
    else:
        rr, lc, gx, gy, nruns = plan_dw_stencil_run(g, sums)
        z.update(family=K_RUN, RR=rr, lc=lc, count=nruns, gx=gx, gy=gy)
    if direction == DGRAD and sums:
        z.update(S=z["gy"] if fast else 0, ws_bytes=DW_SUMS_MAX_ROWS * 2 * g.C * 4)
    return z


def plan_query(engine, g, dtype, direction, aligned, sums=False, xgap=0, ygap=0):
    """(return code, fields) of sg_dwconv2d_plan."""
    d, p = g.desc(xgap, ygap), DwPlan()
    rc = engine.lib.sg_dwconv2d_plan(engine.h, sgdt(dtype), CT.byref(d), direction, int(bool(aligned)), int(bool(sums)), CT.byref(p))
    return rc, {n: getattr(p, n) for n in PLAN_FIELDS}


def checked_plan(engine, g, dtype, direction, aligned, sums=False, xgap=0, ygap=0):
    """The engine's plan of one launch, asserted equal to plan_mirror in every field for this device's CU count.  aligned: every
    pointer of the call is 16-byte aligned (channel count and pixel strides are the plan's own business)."""
    rc, got = plan_query(engine, g, dtype, direction, aligned, sums, xgap, ygap)
    what = f"sg_dwconv2d_plan {g.tag} {dname(dtype)} dir={direction} aligned={int(bool(aligned))} sums={int(bool(sums))} gaps={xgap},{ygap}"
    if direction == WGRAD and (g.KH, g.KW) != (3, 3):      # sg_dwconv2d_wgrad refuses the descriptor: all-zero with its code
        assert rc == SG_EINVAL and not any(got.values()), (what, rc, got)
        return got
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    want = plan_mirror(num_cus(engine), g, dtype, direction, is_vec(g, xgap, ygap, not aligned), g.C + xgap, g.C + ygap, sums)
    diff = {n: (got[n], want[n]) for n in PLAN_FIELDS if got[n] != want[n]}
    assert not diff, f"{what}: (engine, mirror) differ in {diff}"
    return got


FAMILY_IN_NAME = {K_GENERIC: (".V", ".seg."), K_RUN: (".run.",), K_STRIP: (".strip.",)}


def plan_names(plan, name):
    """The case's kernel name speaks of the family the engine planned."""
    assert any(t in name for t in FAMILY_IN_NAME[plan["family"]]), (name, plan)


# ================================================================================================ inputs
@functools.lru_cache(maxsize=24)
def tensor(g, dtype, which):
    """x, res, bsx: [N][H][W][C]; dy: [N][Ho][Wo][C]; uniform in [-1, 1], different in every channel, non-zero on every border."""
    shape = (g.N, g.Ho, g.Wo, g.C) if which == "dy" else (g.N, g.H, g.W, g.C)
    return rnd(gen(f"dw.{g.key}.{which}"), *shape, dtype=dtype)


@functools.lru_cache(maxsize=None)
def taps(g):
    """w[KH][KW][C]: fp32 master weights, KH x KW distinct random taps per channel."""
    return rnd(gen(f"dw.taps.{g.C}.{g.KH}.{g.KW}"), g.KH, g.KW, g.C)


@functools.lru_cache(maxsize=None)
def bn_params(C, tag="gather"):
    """(mean, invstd, gamma, beta) in fp32: |mean| <= 0.3, invstd in [0.7, 1.5], gamma in +-[0.5, 1.5], beta in [-0.5, 0.5]."""
    gg = gen(f"dw.bn.{C}.{tag}")
    gamma = rnd(gg, C, lo=0.5, hi=1.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
    return rnd(gg, C, lo=-0.3, hi=0.3), rnd(gg, C, lo=0.7, hi=1.5), gamma, rnd(gg, C, lo=-0.5, hi=0.5)


class Sums:
    pass


@functools.lru_cache(maxsize=8)
def sums_inputs(g, dtype):
    """The BatchNormalization whose sums the dgrad also forms: its raw input bsx (storage type, dense), mean / invstd / gamma, and
    beta from _bn_cases.gap_beta so that no gamma * xhat + beta is within 1e-4 max|z| of the fused ReLU's boundary (asserted here
    from the reference alone).  With many rows uniform data leaves no such gap inside its range, so one is made: an xhat within
    0.06 of a per-channel target in [-0.3, 0.3] moves 0.12 / invstd away from it, and gap_beta is asked to look there."""
    C = g.C
    gg = gen(f"dw.sums.{g.key}.{dtype}")
    mean, invstd, gamma, _ = bn_params(C, "sums")
    m64, i64, g64 = mean.double(), invstd.double(), gamma.double()
    raw = rnd(gg, g.N, g.H, g.W, C).double()
    t = (0.6 * torch.rand(C, generator=gg) - 0.3).double()
    dlt = (raw - m64) * i64 - t
    raw = torch.where(dlt.abs() < 0.06, raw + torch.where(dlt >= 0, 0.12, -0.12) / i64, raw)
    S = Sums()
    S.bsx = raw.float().to(dtype)
    S.mean, S.invstd, S.gamma = mean, invstd, gamma
    xhat = ((S.bsx.double() - m64) * i64).reshape(-1, C)
    v = -(g64 * xhat)
    target = -(g64 * t)
    need = 1e-4 * (float(v.abs().max()) + float(target.abs().max()) + 0.5)
    beta = torch.tensor([gap_beta(v[:, c], float(target[c]), need) for c in range(C)], dtype=torch.float64)
    S.beta = beta.float()
    z = S.beta.double() - v
    S.zmax, S.margin = float(z.abs().max()), float(z.abs().min())
    assert S.margin >= 1e-4 * S.zmax, f"{g.tag}: {S.margin:.3e} from the ReLU boundary, max|z| = {S.zmax:.3e}"
    # the kernel's own fp32 expression decides the same mask
    z32 = torch.addcmul(S.beta, (S.bsx.float() - mean) * invstd, gamma)
    assert torch.equal(z32.reshape(-1, C) > 0, z > 0)
    S.on = (z > 0).double().mean().item()
    return S


# ================================================================================================ operands
def vin(t, gap=0, off=False, device=None):
    """An input [..][C], dense or as the first C columns of a [pixels][C + gap] tensor whose gap columns hold NaN."""
    o = Guarded(widen(t, t.shape[-1] + gap) if gap else t, device or DEV, off=off)
    o.C, o.mid, o.nhwc, o.gap = t.shape[-1], 0, tuple(t.shape), gap
    return o


def vout(shape, dtype, gap=0, off=False, prior=None, device=None):
    """An output: NaN-prefilled (dense, or C columns of a NaN-prefilled [pixels][C + gap] tensor - at its end where that keeps the
    16-byte alignment), or starting from `prior` (dense: the collected gradient of an in-place `res`)."""
    C = shape[-1]
    if prior is not None:
        assert not gap
        o = Guarded(prior, device or DEV, off=off, role="out")
        mid = 0
    else:
        mid = gap if (gap * esize(dtype)) % 16 == 0 else 0
        pix = 1
        for s in shape[:-1]:
            pix *= s
        o = Guarded.out((pix, C + gap) if gap else shape, dtype, device or DEV, off=off)
    o.C, o.mid, o.nhwc, o.gap = C, mid, tuple(shape), gap
    return o


def vptr(o):
    return o.ptr(o.mid) if o is not None else None


def vread(o, what):
    """The written tensor; every element written, every gap byte still the prefill."""
    wide = o.read()
    if o.gap:
        gaps_keep_prefill(wide, o.C, o.mid, what)
        wide = wide[:, o.mid:o.mid + o.C].reshape(o.nhwc)
    assert_written(wide, what)
    return wide


def stop_on_device_error(rc, what, err=""):
    """A HIP error (a positive return code, or one that surfaces in the copy back) ends the whole session: nothing more is launched
    on a device that has faulted."""
    if rc > 0 or "HIP error" in err:
        import pytest
        pytest.exit(f"{what}: HIP error (rc={rc}) {err[:500]}: ending the session", returncode=3)


def ok(engine, rc, what, ops):
    stop_on_device_error(rc, what, engine.lib.sg_last_error().decode("utf-8", "replace") if rc > 0 else "")
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    try:
        check_all([o for o in ops if o is not None], what)
    except RuntimeError as e:
        stop_on_device_error(0, what, str(e))
        raise


def refused(rc, code, what, ops, outs):
    stop_on_device_error(rc, what)
    assert rc == code, f"{what}: rc={rc}, expected {code}"
    check_all([o for o in ops if o is not None], what)
    for o in outs:
        untouched(o, what)


def is_vec(g, xgap, ygap, off):
    return g.C % 4 == 0 and xgap % 4 == 0 and ygap % 4 == 0 and not off


def bn_ops(C, off=None):
    mean, invstd, gamma, beta = bn_params(C)
    return [G(mean, off == "bn"), G(invstd), G(gamma), G(beta)]


def bn_struct(ops, relu):
    return BnIn(ops[0].ptr(), ops[1].ptr(), ops[2].ptr(), ops[3].ptr(), int(relu), 0, 0.0)


def bn_ref(C, relu):
    return tuple(t.double() for t in bn_params(C)) + (bool(relu),)


def form_of(name):
    """The key of RECORDS: entry point, kernel family (V, RR), template form."""
    p = name.split(".")
    if p[1][0] == "V":
        return f"{p[0]}.{p[1]}"
    key = f"{p[0]}.{p[1]}"
    if p[2].startswith("RR"):
        key += "." + p[2][:3]
    elif p[1] == "seg":
        key += "." + p[2][:2]
    return key + (f".{p[-1]}" if p[-1].startswith(("plain", "RELU", "BN", "MASK", "PRE")) else "")


# ================================================================================================ the launches
FWD_FORMS = (("plain", 0, None), ("RELU", 1, None), ("BN", 0, 0), ("BN+RELU", 0, 1))      # name, pre_relu, bn's relu (None: no bn)


def fwd_launch(engine, g, dtype, pre=0, bn=None, xgap=0, ygap=0, off=None, expect=0):
    """One sg_dwconv2d_fwd.  bn: None or the BatchNormalization's relu flag.  off: the one operand ("x", "w", "y", "bn") that is not
    16-byte aligned.  expect: the return code; non-zero: the output must keep its prefill."""
    x, w = tensor(g, dtype, "x"), taps(g)
    X, W, Y = vin(x, xgap, off == "x"), G(w, off == "w"), vout((g.N, g.Ho, g.Wo, g.C), dtype, ygap, off == "y")
    B = bn_ops(g.C, off) if bn is not None else []
    st = bn_struct(B, bn) if bn is not None else None
    d = g.desc(xgap, ygap)
    fname = ("BN+RELU" if bn else "BN") if bn is not None else ("RELU" if pre else "plain")
    vec = is_vec(g, xgap, ygap, off)
    name = fwd_name(g, dtype, vec, g.C + xgap, fname if (vec and dw_run_ok(g)) else "")
    what = f"dwconv2d_fwd {g.tag} {dname(dtype)} pre={pre} bn={bn} gaps={xgap},{ygap} off={off} [{name}]"
    plan = checked_plan(engine, g, dtype, FWD, not off, False, xgap, ygap)
    rc = call(engine, "sg_dwconv2d_fwd", sgdt(dtype), CT.byref(d), vptr(X), W.ptr(), vptr(Y), pre, CT.byref(st) if st else None)
    ops = [X, W, Y] + B
    if expect:
        refused(rc, expect, what, ops, [Y])
        return name
    ok(engine, rc, what, ops)
    plan_names(plan, name)
    ref = dw_conv_ref(x.double(), w.double(), g.geom, g.s, g.d, bool(pre), bn_ref(g.C, bn) if bn is not None else None)
    cmp(vread(Y, what), ref, etol(dtype), what, form_of(name), "y", dtype)
    return name


@functools.lru_cache(maxsize=8)
def dx_ref(g, dtype, mask):
    return dw_grads_ref(tensor(g, dtype, "x").double(), taps(g).double(), tensor(g, dtype, "dy").double(), g.geom, g.s, g.d,
                        bool(mask), None, "dx")


# mask (pre_relu), res (0, 1, "inplace": res == dx), sums, the summed layer's fused ReLU
DGRAD_FORMS = ((0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, "inplace", 0, 0), (0, 0, 1, 0), (1, 0, 1, 0), (0, 1, 1, 0),
               (0, 0, 1, 1), (1, "inplace", 1, 1))


def dgrad_form(mask, res, sums, relu):
    return ("MASK" if mask else "plain") + ("+res" if res == 1 else ("+res=dx" if res else "")) + \
        (("+SUMS" + ("relu" if relu else "")) if sums else "")


def dgrad_launch(engine, g, dtype, mask=0, res=0, sums=0, relu=0, xgap=0, ygap=0, off=None, expect=0, ws_short=0, no_x=False):
    """One sg_dwconv2d_dgrad.  off: "dy", "w", "dx", "x", "res" or "bsx".  ws_short: bytes taken off the sums workspace."""
    x, dy, w = tensor(g, dtype, "x"), tensor(g, dtype, "dy"), taps(g)
    DY, W = vin(dy, ygap, off == "dy"), G(w, off == "w")
    Xm = vin(x, xgap, off == "x") if (mask and not no_x) else None
    rt = tensor(g, dtype, "res") if res else None
    if res == "inplace":
        DX = vout((g.N, g.H, g.W, g.C), dtype, 0, off == "dx", prior=rt)
        R, rptr = None, vptr(DX)
    else:
        DX = vout((g.N, g.H, g.W, g.C), dtype, xgap, off == "dx")
        R = vin(rt, xgap, off == "res") if res else None       # read with dx's ld, from its own pointer
        rptr = vptr(R)
    ops, outs, q = [DY, W, Xm, R, DX], [DX], None
    if sums:
        S = sums_inputs(g, dtype)
        BX, SM, SI, SG_, SB = G(S.bsx, off == "bsx"), G(S.mean), G(S.invstd), G(S.gamma), G(S.beta)
        DG, DB = GO((g.C,), F32), GO((g.C,), F32)
        d0 = g.desc()
        nws = engine.lib.sg_dwconv2d_dgrad_bnsums_ws_bytes(engine.h, CT.byref(d0))
        assert nws == DW_SUMS_MAX_ROWS * 2 * g.C * 4 + 256, nws
        WS = Guarded.ws(nws - ws_short, DEV)
        q = DwBnSums(BX.ptr(), SM.ptr(), SI.ptr(), SG_.ptr(), SB.ptr(), int(relu), DG.ptr(), DB.ptr(), WS.ptr(), nws - ws_short)
        ops += [BX, SM, SI, SG_, SB, DG, DB, WS]
        outs += [DG, DB]
    d = g.desc(xgap, ygap)
    vec = is_vec(g, xgap, ygap, off)
    stencil = vec and dw_run_ok(g)
    name = dgrad_name(g, dtype, vec, g.C + ygap, dgrad_form(mask, res, sums, relu) if stencil else "", bool(sums))
    what = f"dwconv2d_dgrad {g.tag} {dname(dtype)} {dgrad_form(mask, res, sums, relu)} gaps={xgap},{ygap} off={off} [{name}]"
    plan = checked_plan(engine, g, dtype, DGRAD, not off, bool(sums), xgap, ygap)
    if sums:
        assert nws == plan["ws_bytes"] + 256, (what, nws, plan)
    rc = call(engine, "sg_dwconv2d_dgrad", sgdt(dtype), CT.byref(d), vptr(DY), W.ptr(), vptr(Xm), vptr(DX), int(mask), rptr,
              CT.byref(q) if q else None)
    if expect:
        refused(rc, expect, what, ops, outs)
        return name
    ok(engine, rc, what, ops)
    plan_names(plan, name)
    ref = dx_ref(g, dtype, bool(mask))
    if res:
        ref = ref + rt.double()
    cmp(vread(DX, what), ref, etol(dtype), what, form_of(name), "dx", dtype)
    if sums:
        dgr, dbr = bn_sums_ref(ref, S.bsx.double(), S.mean.double(), S.invstd.double(), S.gamma.double(), S.beta.double(), relu)
        for o, r, n in ((DG, dgr, "dgamma"), (DB, dbr, "dbeta")):
            got = o.read()
            assert_written(got, what + " " + n)
            cmp(got, r, RTOL, what, form_of(name), n, dtype)
    return name


WGRAD_FORMS = (("PRE0BN0", 0, None), ("PRE1BN0", 1, None), ("PRE0BN1", 0, 0), ("PRE1BN1", 0, 1))


def wgrad_launch(engine, g, dtype, pre=0, bn=None, xgap=0, ygap=0, off=None, expect=0, ws_bytes=None):
    """One sg_dwconv2d_wgrad on a workspace of exactly the queried size (or ws_bytes)."""
    x, dy = tensor(g, dtype, "x"), tensor(g, dtype, "dy")
    X, DY, DWo = vin(x, xgap, off == "x"), vin(dy, ygap, off == "dy"), GO((g.KH, g.KW, g.C), F32, off == "dw")
    B = bn_ops(g.C, off) if bn is not None else []
    st = bn_struct(B, bn) if bn is not None else None
    d, d0 = g.desc(xgap, ygap), g.desc()
    vec = is_vec(g, xgap, ygap, off in ("x", "dy"))
    fname = f"PRE{int(bool(bn)) if bn is not None else int(pre)}BN{int(bn is not None)}"
    plan = checked_plan(engine, g, dtype, WGRAD, off not in ("x", "dy", "bn"), False, xgap, ygap)
    if g.KH == 3 and g.KW == 3:
        name = pinned(engine, wgrad_name, g, vec, g.C + xgap, g.C + ygap, fname)
        cus = num_cus(engine)
        nws = engine.lib.sg_dwconv2d_wgrad_ws_bytes(engine.h, CT.byref(d0))
        assert nws == wgrad_ws_query(cus, g), (g.tag, nws, wgrad_ws_query(cus, g))
        assert wgrad_need(cus, g, vec, g.C + xgap, g.C + ygap) <= nws - 256
        assert plan["ws_bytes"] + 256 <= nws, (g.tag, plan, nws)
    else:
        name, nws = "wgrad.refused", 1024
    if ws_bytes is not None:
        nws = ws_bytes
    WS = Guarded.ws(nws, DEV)
    what = f"dwconv2d_wgrad {g.tag} {dname(dtype)} {fname} gaps={xgap},{ygap} off={off} ws={nws} [{name}]"
    rc = call(engine, "sg_dwconv2d_wgrad", sgdt(dtype), CT.byref(d), vptr(X), vptr(DY), DWo.ptr(), pre, CT.byref(st) if st else None,
              WS.ptr(), nws)
    ops = [X, DY, DWo, WS] + B
    if expect:
        refused(rc, expect, what, ops, [DWo])
        return name
    ok(engine, rc, what, ops)
    plan_names(plan, name)
    ref = dw_grads_ref(x.double(), taps(g).double(), dy.double(), g.geom, g.s, g.d, bool(pre), bn_ref(g.C, bn) if bn is not None else None,
                       "dw")
    got = DWo.read()
    assert_written(got, what)
    cmp(got, ref, RTOL, what, form_of(name), "dw", dtype)
    return name


# ================================================================================================ the cases
def stencil_case(engine, g, dtype, views=True, fwd_forms=FWD_FORMS, dgrad_forms=DGRAD_FORMS):
    """Every forward and dgrad form of a stride-1 3x3 'same' layer whose W and C divide by 4, on the run or the strip kernel
    (whichever the switches choose); then ld = C + 4 views on the forward (plain, BN + ReLU) and the plain dgrad."""
    assert dw_run_ok(g)
    names = []
    for _, pre, bn in fwd_forms:
        names.append(fwd_launch(engine, g, dtype, pre, bn))
    for f in dgrad_forms:
        names.append(dgrad_launch(engine, g, dtype, *f))
    if views:
        names.append(fwd_launch(engine, g, dtype, 0, None, 4, 4))
        names.append(fwd_launch(engine, g, dtype, 0, 1, 4, 4))
        names.append(dgrad_launch(engine, g, dtype, xgap=4, ygap=4))
    return names


def wgrad_case(engine, g, dtype, views=True):
    """The four <PRE, BN> forms of the filter gradient of a stride-1 3x3 'same' layer, then ld = C + 4 views of x and dy."""
    names = [wgrad_launch(engine, g, dtype, pre, bn) for _, pre, bn in WGRAD_FORMS]
    if views:
        names.append(wgrad_launch(engine, g, dtype, 0, None, 4, 4))
        names.append(wgrad_launch(engine, g, dtype, 0, 1, 4, 4))
    return names


def generic_case(engine, g, dtype, gap=0, off=False):
    """dw_fwd_kernel / dw_dgrad_kernel / DwWgradOp: pre_relu off and on; x and y as views with ld = C + gap.  off: every operand
    in turn one element past 16-byte alignment (all others aligned).  A window other than 3x3: wgrad refuses, dw untouched."""
    names = []
    for pre in (0, 1):
        for o in (("x", "w", "y") if off else (None,)):
            names.append(fwd_launch(engine, g, dtype, pre, None, gap, gap, o))
        for o in (("dy", "w", "dx") + (("x",) if pre else ()) if off else (None,)):
            names.append(dgrad_launch(engine, g, dtype, pre, xgap=gap, ygap=gap, off=o))
        for o in (("x", "dy") if off else (None,)):
            if (g.KH, g.KW) == (3, 3):
                names.append(wgrad_launch(engine, g, dtype, pre, None, gap, gap, o))
            else:
                names.append(wgrad_launch(engine, g, dtype, pre, None, gap, gap, o, expect=SG_EINVAL))
    return names


def generic_name(g, dtype, gap, off):
    vec = is_vec(g, gap, gap, off)
    w = wgrad_name(REF_CUS, g, vec, g.C + gap, g.C + gap) if (g.KH, g.KW) == (3, 3) else "wgrad.refused"
    return f"{fwd_name(g, dtype, vec, g.C + gap)}+{dgrad_name(g, dtype, vec, g.C + gap)}+{w}"


GENERIC_GEOMS = [dict(H=6, W=8, s=2), dict(H=7, W=5, s=2), dict(H=7, W=8, s=2, same=False), dict(H=3, W=5, d=2), dict(H=3, W=6, d=3),
                 dict(H=6, W=7, KH=5, KW=3), dict(H=5, W=6)]
# C, gap of the x / y views, one operand off: V = 1 by C (1, 5, 45), by one operand off, by ld = C + 1; V = 4 at C = 8 dense and ld = C + 4
GENERIC_FORMS = [(1, 0, False), (1, 4, False), (1, 1, False), (45, 0, False), (45, 4, False), (45, 1, False), (5, 0, False), (5, 4, False), (5, 1, False), (8, 0, False), (8, 4, False), (8, 1, False),
                 (8, 0, True)]
GENERIC = [(Geom(2, C=C, **kw), gap, off) for kw in GENERIC_GEOMS for C, gap, off in GENERIC_FORMS]

RUN_SHAPES = [Geom(2, H, W, C) for H in (1, 2, 3, 6, 62) for W in (4, 8, 12) for C in (4, 20, 260)]
STRIP_SHAPES = [Geom(2, H, W, C) for H in (64, 68, 72) for W in (4, 8, 12) for C in (4, 20, 68)] + [Geom(2, 66, 8, 20)]
# past DW_SUMS_MAX_ROWS: C = 132 is 33 chunks, lc = 64, 4 runs per workgroup: 2 x 31 x 67 = 4154 runs -> 1039 rows > 1024, the runs from
# 4096 on are a second trip; 257 x 4 x 16 = 16448 strips -> 1028 rows > 1024, the strips from 16384 on are a second trip
SUMS_CAP = [Geom(2, 62, 268, 132), Geom(257, 64, 64, 4)]
SUMS_CAP_FORMS = ((1, 1, 1, 1),)

WSTRIP_SHAPES = [Geom(2, H, W, C) for H in (4, 8, 12, 20, 128, 132) for W in (4, 8, 12) for C in (4, 20, 68)]
# S = ceil(strips / 16): 512 strips -> 32 partial rows ("many"); 4608 strips -> 288, capped at 256: slots 0 .. 511 walk a second strip
WSTRIP_MORE = [Geom(2, 128, 128, 4), Geom(9, 64, 256, 4)]
WRUN_SHAPES = [Geom(2, H, W, C) for H in (1, 6, 9) for W in (4, 8, 12) for C in (4, 20, 68)]
WRUN_MORE = [Geom(2, 66, 256, 4)]       # 33792 pixels > 32768: RR = 2

# ew_blocks' cap: more than 16384 x 256 work items (bf16): fwd over the outputs, dgrad over the inputs (stride 2: a quarter of the
# reference's work)
CAPS = [("fwd", Geom(2, 130, 130, 125)), ("dgrad", Geom(2, 130, 130, 125, s=2)), ("fwd", Geom(2, 130, 130, 500)),
        ("dgrad", Geom(2, 130, 130, 500, s=2))]


def cap_case(engine, kind, g):
    return fwd_launch(engine, g, BF16) if kind == "fwd" else dgrad_launch(engine, g, BF16)


def refusal_case(engine, dtype):
    """Every refusal leaves every output with its prefill."""
    far, near = Geom(2, 6, 8, 8, s=2), Geom(2, 6, 8, 8)
    # res / sums / bn on a geometry the run kernels do not take
    dgrad_launch(engine, far, dtype, res=1, expect=SG_EUNSUPPORTED)
    dgrad_launch(engine, far, dtype, sums=1, expect=SG_EUNSUPPORTED)
    fwd_launch(engine, far, dtype, 0, 0, expect=SG_EUNSUPPORTED)
    wgrad_launch(engine, far, dtype, 0, 1, expect=SG_EUNSUPPORTED)
    fwd_launch(engine, Geom(2, 6, 6, 8), dtype, 0, 1, expect=SG_EUNSUPPORTED)          # W % 4 != 0
    # ... with one unaligned operand
    for o in ("dy", "w", "dx", "res"):
        dgrad_launch(engine, near, dtype, res=1, off=o, expect=SG_EUNSUPPORTED)
    for o in ("dy", "dx", "bsx"):
        dgrad_launch(engine, near, dtype, sums=1, off=o, expect=SG_EUNSUPPORTED)
    dgrad_launch(engine, near, dtype, mask=1, res=1, off="x", expect=SG_EUNSUPPORTED)
    for o in ("x", "w", "y", "bn"):
        fwd_launch(engine, near, dtype, 0, 1, off=o, expect=SG_EUNSUPPORTED)
    for o in ("x", "dy", "bn"):
        wgrad_launch(engine, near, dtype, 0, 1, off=o, expect=SG_EUNSUPPORTED)
    # bn with pre_relu; pre_relu without x
    fwd_launch(engine, near, dtype, 1, 0, expect=SG_EINVAL)
    wgrad_launch(engine, near, dtype, 1, 0, expect=SG_EINVAL)
    dgrad_launch(engine, near, dtype, mask=1, no_x=True, expect=SG_EINVAL)
    # the sums workspace one float short of the DW_SUMS_MAX_ROWS x 2 x C floats the launch is entitled to (the query adds 256
    # bytes of slack which the check does not insist on); the filter gradient on 4 bytes, on all three of its kernels
    dgrad_launch(engine, near, dtype, sums=1, ws_short=256 + 4, expect=SG_EWORKSPACE)
    for g in (Geom(2, 8, 8, 8), near, far):
        wgrad_launch(engine, g, dtype, ws_bytes=4, expect=SG_EWORKSPACE)
    # the same launches go through on aligned operands and a workspace of the queried size
    dgrad_launch(engine, near, dtype, sums=1)
    dgrad_launch(engine, near, dtype, sums=1, ws_short=256)


# ================================================================================================ the forms behind switches
CHILD_ENVS = [
    {"SG_DW_FSTRIP": "0", "SG_DW_STRIP": "0"},
    {"SG_DW_FSTRIP": "0", "SG_DW_STRIP": "0", "SG_DW_RR": "1"},
    {"SG_DW_STRIP": "0", "SG_DW_RR": "2"},
    {"SG_DW_FSTRIP": "2"},
    {"SG_DW_FSTRIP": "2", "SG_DW_FSTRIP_HS": "12"},
    {"SG_DW_FSTRIP": "2", "SG_DW_FSTRIP_HS": "6"},
]


def env_label(env):
    return " ".join(f"{k}={env[k]}" for k in SWITCH_NAMES if k in env)


def _child_table(env):
    """(kind, geometry, every name must contain) of one environment."""
    e = env_label(env)
    if e == "SG_DW_FSTRIP=0 SG_DW_STRIP=0":        # the run stencil at H >= 64; the run reducer on H % 4 == 0 maps (RR = 1, and 2)
        return ([("stencil", Geom(2, H, 8, 20), "run.RR2") for H in (64, 68)] + [("stencil", Geom(2, 64, 12, 260), "run.RR2")] +
                [("wgrad", Geom(2, 8, 8, 20), "run.RR1"), ("wgrad", Geom(2, 128, 12, 68), "run.RR1"), ("wgrad", Geom(2, 68, 256, 4), "run.RR2")])
    if e == "SG_DW_FSTRIP=0 SG_DW_STRIP=0 SG_DW_RR=1":
        return ([("stencil", Geom(2, H, 8, 20), "run.RR1") for H in (2, 6, 62, 64)] + [("stencil", Geom(2, 6, 12, 260), "run.RR1")] +
                [("wgrad", Geom(2, 68, 256, 4), "run.RR1"), ("wgrad", Geom(2, 8, 8, 20), "run.RR1")])
    if e == "SG_DW_STRIP=0 SG_DW_RR=2":
        return [("wgrad", Geom(2, H, W, C), "run.RR2") for H, W, C in ((2, 4, 4), (6, 8, 20), (8, 12, 68), (4, 8, 20))]
    if e == "SG_DW_FSTRIP=2":
        return ([("stencil", Geom(2, H, W, 20), "strip.HS") for H in (4, 8, 12, 20) for W in (4, 8, 12)] +
                [("stencil", Geom(2, H, 8, C), "strip.HS") for H in (4, 20) for C in (4, 68)])
    if e == "SG_DW_FSTRIP=2 SG_DW_FSTRIP_HS=12":   # H = 8: HS > H falls back to 4
        return ([("stencil", Geom(2, H, W, C), "strip.HS12") for H in (24, 28) for W, C in ((8, 20), (12, 68))] +
                [("stencil", Geom(2, 8, 8, 20), "strip.HS4")])
    if e == "SG_DW_FSTRIP=2 SG_DW_FSTRIP_HS=6":    # HS % 4 != 0 falls back to 4
        return [("stencil", Geom(2, 8, 8, 20), "strip.HS4"), ("stencil", Geom(2, 12, 12, 68), "strip.HS4")]
    raise AssertionError(f"no case table for '{e}'")


def child_cases(env):
    """(label, function, arguments, what every kernel name of the case must contain) for one environment, both storage types."""
    out = []
    for kind, g, must in _child_table(env):
        for dtype in (F32, BF16):
            fn = stencil_case if kind == "stencil" else wgrad_case
            out.append((f"{kind} {g.tag} {dname(dtype)}", fn, (g, dtype), must))
    return out


def child_names(env):
    """The kernel names of an environment's cases at REF_CUS (no GPU needed)."""
    out = []
    with switched(env):
        for kind, g, must in _child_table(env):
            if kind == "stencil":
                out.append("fwd." + stencil_name(g, 4, g.C, False))
                out.append("dgrad." + stencil_name(g, 4, g.C, True))
            else:
                out.append(wgrad_name(REF_CUS, g, True, g.C, g.C))
            assert must in out[-1], (env, g.tag, must, out[-1])
    return out


def main():
    global QUIET
    QUIET = True
    env = {k: os.environ[k] for k in SWITCH_NAMES if k in os.environ}
    assert any(env == e for e in CHILD_ENVS), f"run with one of {[env_label(e) for e in CHILD_ENVS]} in the environment"
    from building_detection_amd.ops import get_engine
    engine = get_engine(0)
    status = 0
    for label, fn, args, must in child_cases(env):
        try:
            names = fn(engine, *args)
            assert all(must in n for n in names), (must, names)
            kernels = sorted({n.split(".", 1)[1].rsplit(".", 1)[0] for n in names})
            print(f"CASE ok {label} [{' '.join(kernels)}] {len(names)} launches", flush=True)
        except Exception as e:       # the first failure ends the child: nothing more is started on the GPU
            traceback.print_exc()
            print(f"CASE FAIL {label}: {str(e)[:300]}", flush=True)
            status = 1
            break
    print(records_table(), flush=True)
    sys.exit(status)


if __name__ == "__main__":
    main()
