"""The cases of tests/test_conv_forms_gpu.py: sg_conv2d_fwd and sg_conv2d_dgrad (csrc/conv_igemm.hip, the kernels it includes, conv_native.hip, conv_thin.hip)
through the C ABI on tests/_guarded.py arenas, each launch against oracle.tfops.conv2d in float64 (autograd for dx).

A case states, at the end of its id, which kernel FORM its launch takes.  The name comes from the mirrors below of the dispatch
rules - plan_conv_mode, pick_bn, plan_common, x6_ok, x6p_geom, x6w_shares, b16w_shares, pw_wide_width, b16_ks, the PD rule, the
structure (`var`) rule, thin_ok, images_per_2gib - written from the comments of the sources, not by calling the library.  Before a
case launches, run_case() asserts that the mirror's name is the one in the id, that the engine's own plan (sg_conv2d_plan) says the
same field by field on this device, and that sg_conv2d_planes_job and sg_conv2d_caps agree with both.

Form names:
    fwd|dgrad.native.BN<128|64|32>.<scalar|vec|ut>[.b16|.b16>f32|.f32>b16]
    fwd|dgrad.thin.CO<1-4>.<f32|b16|b16>f32>
    fwd|dgrad.slab.x6.BN<..>.v<0|1>[.mf16][.npl1]
    fwd|dgrad.slab.b16.BN<..>.KS<2|4>.PD<1|2>
    fwd|dgrad.slab.x6w.S<1|2>            fwd|dgrad.slab.b16w.S<1-4>
    fwd|dgrad.patch.C<32|64|64m>.BN<32|64|128>
    fwd|dgrad.wide.<x6|b16>.W<384|256>
then the modifiers .skip .perm2 .gm<n> .cb<n> .vpad .sub<nb>+<tail>.  The operands a case brings beyond the plain epilogues (res, pin =
activation planes, bn = BatchNormalization in the loader, bnb, up2 / down2) are listed in its `extra` and run as further launches.

Run as a program (`python tests/_conv_cases.py CHILD` with CHILD_ENVS[CHILD] in the environment: the switches are read once per
process) it runs child_cases(CHILD) and prints one `CASE ok|FAIL ...` line per case, then its records."""
import ctypes as CT
import math
import os
import re
import sys
import time
import traceback

import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from _guarded import Guarded, assert_written, check_all, dw_geom, gaps_keep_prefill, tile_stats_ref, untouched, widen

REF_CUS = 256
F32, BF16, HEAD = 0, 1, 0x100
EPI_BIAS, EPI_RELU, PRO_UP2, EPI_DOWN2 = 1, 2, 16, 32
SG_EINVAL, SG_EWORKSPACE, SG_EUNSUPPORTED = -1, -2, -3
BM, BK = 128, 32
XW_M, XW_N, XW_KD = 128, 256, 32
BW_M, BW_N, BW_KD = 256, 256, 64
PW_BM, PW_BN, PW_BNB_MAXK = 128, 384, 2048
CF_NATIVE, CF_THIN, CF_HEAD, CF_SLAB, CF_PATCH, CF_WIDE = range(6)
CK_NATIVE, CK_THIN, CK_X6, CK_B16, CK_X6W, CK_B16W, CK_PATCH, CK_WIDE = range(1, 9)
KERNEL_NAMES = {1: "native", 2: "thin", 3: "slab.x6", 4: "slab.b16", 5: "slab.x6w", 6: "slab.b16w", 7: "patch", 8: "wide"}
QUIET = False
FAULTED = []     # the first HIP error of this process (run_case): no case is launched after it
RECORDS = []     # (case id, launch, output, measured error / scale, bound): a record, written before anything is asserted


def cdiv(a, b):
    return -(-a // b)


# ================================================================================================ switches
# The switches of csrc/sg_switch.h that a child environment of this file sets; every other switch must be unset (run_case checks).
SWITCH_DEFAULTS = dict(SG_X6_VARIANT=None, SG_CONV_MAX_BYTES=0, SG_X6_MF16=1, SG_DGRAD_PERM2=1, SG_B16_DEEP=1, SG_X6_INTERLEAVE=1)
FOREIGN_SWITCHES = ("SG_CONV_X6", "SG_X6_VPAD", "SG_X6_NOPATCH", "SG_X6P_CHUNKS", "SG_X6_WIDE", "SG_CONV_L2", "SG_CONV_CB", "SG_CONV_GM",
                    "SG_CONV_NOSKIP", "SG_CONV_NOTHIN", "SG_PW_WIDE", "SG_PW_VAR", "SG_B16_KS", "SG_B16_PD", "SG_B16_WIDE",
                    "SG_PW_ABLATE", "SG_X6_ABLATE", "SG_X6P_ABLATE", "SG_X6W_ABLATE", "SG_CONV_ABLATE", "SG_BNB_ABLATE")


def _atoll(v):
    try:
        return int(v.strip())
    except ValueError:
        return 0


def switches_of(env):
    sw = dict(SWITCH_DEFAULTS)
    for k in sw:
        if k in env:
            v = _atoll(env[k])
            sw[k] = (0 if v == 0 else 1) if k in ("SG_X6_MF16", "SG_B16_DEEP") else v     # (OFF0 switches: 0 only when set to 0)
    return sw


SW = switches_of(os.environ)
CHILD_ENVS = {
    "v0": {"SG_X6_VARIANT": "0"},
    "sub": {"SG_CONV_MAX_BYTES": str(2 << 20)},
    "ab": {"SG_X6_MF16": "0", "SG_DGRAD_PERM2": "0", "SG_B16_DEEP": "0", "SG_X6_INTERLEAVE": "0"},
}


class switched:
    """The mirrors as a process with `env` sees them (the parent lists a child's cases and names)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = dict(SW)
        SW.update(switches_of(self.env))

    def __exit__(self, *a):
        SW.update(self.old)


# ================================================================================================ geometry
class Geom:
    """One convolution: x[N, H, W, Cin] -> y[N, Ho, Wo, Cout], TF 'same' padding; xgap / ygap: x_ld - Cin, y_ld - Cout."""

    def __init__(self, N, H, W, Cin, Cout, k=3, s=1, d=1, xgap=0, ygap=0):
        self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.s, self.d, self.xgap, self.ygap = N, H, W, Cin, Cout, k, s, d, xgap, ygap
        self.Ho, self.Wo, self.pt, _, self.pl, _ = dw_geom(H, W, k, k, s, d, True)
        self.xl, self.yl = Cin + xgap, Cout + ygap

    @property
    def tag(self):
        t = f"n{self.N}h{self.H}w{self.W}c{self.Cin}o{self.Cout}k{self.k}"
        if self.s != 1:
            t += f"s{self.s}"
        if self.d != 1:
            t += f"d{self.d}"
        if self.xgap:
            t += f"xg{self.xgap}"
        if self.ygap:
            t += f"yg{self.ygap}"
        return t

    def with_n(self, n):
        return Geom(n, self.H, self.W, self.Cin, self.Cout, self.k, self.s, self.d, self.xgap, self.ygap)

    def desc(self):
        from building_detection_amd._lib import ConvDesc
        return ConvDesc(self.N, self.H, self.W, self.Cin, self.Cout, self.k, self.k, self.s, self.d, self.pt, self.pl, self.Ho, self.Wo,
                        self.xl if self.xgap else 0, self.yl if self.ygap else 0)


class View:
    """IgemmParams' geometry fields of one launch (fill_fwd_params / fill_dgrad_params): C = the depth of one tap of the reduction."""

    def __init__(self, g, dgrad, eb):
        if not dgrad:
            self.H, self.W, self.C, self.x_ld, self.OH, self.OW, self.Nout, self.y_ld = g.H, g.W, g.Cin, g.xl, g.Ho, g.Wo, g.Cout, g.yl
            self.a_mul, self.k_mul, self.off, self.div = g.s, g.d, (-g.pt, -g.pl), 1
            self.M = g.N * g.Ho * g.Wo
            xb = ((g.N * g.H * g.W - 1) * g.xl + g.Cin) * eb
        else:
            self.H, self.W, self.C, self.x_ld, self.OH, self.OW, self.Nout, self.y_ld = g.Ho, g.Wo, g.Cout, g.yl, g.H, g.W, g.Cin, g.xl
            self.a_mul, self.k_mul, self.off, self.div = 1, -g.d, (g.pt, g.pl), g.s
            self.M = g.N * g.H * g.W
            xb = ((g.N * g.Ho * g.Wo - 1) * g.yl + g.Cout) * eb
        self.K = g.k * g.k * self.C
        wb = self.K * self.Nout * 4
        self.x_bytes = xb if xb < (1 << 31) else 0
        self.w_bytes = wb if wb < (1 << 31) else 0
        self.perm2 = 0


# ================================================================================================ mirrors of the dispatch rules
def pick_bn(M, N, cus):
    """Tile width by wave quantisation: the BN in {128, 64} whose tile count wastes the least of its last round of `cus` tiles and of
    its last column tile; the 64-wide tile pays 0.93 (it re-reads A twice as often).  Up to 32 / 64 columns: that width."""
    if N <= 32:
        return 32
    if N <= 64:
        return 64
    best, best_bn = -1.0, 128
    for bn in (128, 64):
        tiles = cdiv(M, BM) * cdiv(N, bn)
        eff = tiles / (cdiv(tiles, cus) * cus) * N / (cdiv(N, bn) * bn) * (1.0 if bn == 128 else 0.93)
        if eff > best:
            best, best_bn = eff, bn
    return best_bn


def plan_common(v, vec, bn, x6, eb):
    """(skip_taps, group_m, cb): the padding-tap elimination for dilated multi-tap launches (and parity-class rows), the grouped
    tile order from four column tiles on (16 row tiles per group while an XCD's eighth of A is at most 2 MiB, else 8; the x6
    kernels only), the channel-block K order (x6 and fp32 kernels: wave-uniform taps, multi-tap, more than 4 slabs per tap in whole
    blocks of 4, one image above 2 MiB)."""
    ntaps, spt = v.K // v.C, v.C // BK
    skip = 1 if (abs(v.k_mul) > 1 and 1 < ntaps <= 64) else 0
    if v.perm2:
        skip = 1
    l2 = 7 if x6 else 2
    ntn = cdiv(v.Nout, bn)
    a_per_xcd = v.x_bytes // 8 if v.x_bytes else (1 << 40)
    gm = (16 if a_per_xcd <= (2 << 20) else 8) if ((l2 & 1) and ntn >= 4) else 1
    ut = vec and v.C % BK == 0 and v.x_bytes != 0 and v.w_bytes != 0
    img_bytes = v.H * v.W * v.x_ld * eb
    cb = 4 if ((l2 & 2) and ut and ntaps > 1 and spt > 4 and spt % 4 == 0 and img_bytes > (2 << 20)) else 0
    return skip, gm, cb


def x6_vpad_c(C):
    return cdiv(C, 32) * 32


def x6_planes_bytes(K, N, npl=3, kd=32):
    return npl * cdiv(K, kd) * kd * cdiv(N, 128) * 128 * 2


def x6_ok(v, vec, force, mode):
    """The bf16-pipe kernels take a launch with 16-byte channel runs, at least 16 output columns, A below 2 GiB and planes below
    2 GiB (every channel count: virtual channel padding); fp32 storage in arithmetic mode 0 never."""
    kmax = (v.K // v.C) * x6_vpad_c(v.C)
    return (force or mode != 0) and vec and v.x_bytes != 0 and x6_planes_bytes(kmax, v.Nout) < (1 << 31) and v.Nout >= 16


def x6p_geom(v, k):
    """The patch form: 3x3, stride 1, dilation 1, SAME; 32 or 64 reduction channels per tap, or chunks of 64 up to 512; H % 8 == 0,
    W % 16 == 0; 32, 64 or a multiple of 128 output columns."""
    if k != 3 or v.K != 9 * v.C:
        return False
    if v.C not in (32, 64) and (v.C % 64 != 0 or v.C > 512):
        return False
    if v.a_mul != 1 or v.div != 1:
        return False
    if not ((v.k_mul == 1 and v.off == (-1, -1)) or (v.k_mul == -1 and v.off == (1, 1))):
        return False
    if v.OH != v.H or v.OW != v.W or v.H % 8 or v.W % 16:
        return False
    return v.Nout in (32, 64) or v.Nout % 128 == 0


def x6w_shares(v):
    """K shares of the planes-in kernel (0: not taken): multi-tap, K >= 2048, tap depth % 32 == 0, last 256-wide column tile at least
    3/4 full, whole 128-pixel tiles per image; 16 workgroups per image: one share, 8 with K / 2 >= 2048: two."""
    if v.div != 1 or v.C % XW_KD != 0 or v.K == v.C or v.K < 2048 or v.K // v.C > 64:
        return 0
    if v.x_ld % 4 != 0 or v.x_bytes == 0 or v.Nout % 4 != 0:
        return 0
    ntn = cdiv(v.Nout, XW_N)
    if v.Nout / (ntn * XW_N) < 0.75:
        return 0
    img_px = v.OH * v.OW
    if img_px < XW_M or img_px % XW_M != 0:
        return 0
    img_wgs = ntn * (img_px // XW_M)
    if img_wgs >= 16:
        return 1
    if img_wgs >= 8 and v.K // 2 >= 2048:
        return 2
    return 0


def b16w_shares(v):
    """K shares of the 256-wide bf16 kernel (0: not taken): tap depth % 64 == 0, K >= 1024, column tiles at least 3/4 full, whole
    256-pixel tiles per image; 16 workgroups per image or as many shares (<= 4, each >= 2048 deep) as make 16."""
    if v.div != 1 or v.C % BW_KD != 0 or v.K < 1024 or v.K // v.C > 64:
        return 0
    if v.x_ld % 8 != 0 or v.x_bytes == 0 or v.Nout % 4 != 0:
        return 0
    ntn = cdiv(v.Nout, BW_N)
    if v.Nout / (ntn * BW_N) < 0.75:
        return 0
    img_px = v.OH * v.OW
    if img_px < BW_M or img_px % BW_M != 0:
        return 0
    img_wgs = ntn * (img_px // BW_M)
    if img_wgs >= 16:
        return 1
    S = min(16 // img_wgs, 4)
    while S > 1 and v.K // S < 2048:
        S -= 1
    return S if (S > 1 and img_wgs * S >= 16) else 0


def pw_wide_width(v):
    """Tile width of the wide pointwise kernel (0: not taken): 1x1, stride 1, K >= 256, >= 6144 rows; of 384 and 256 the width with
    the fewest rounds of 256 workgroups x width, each needing its columns 3/4 full and 256 at least 192 tiles; ties go to 384."""
    if v.K != v.C or v.a_mul != 1 or v.div != 1 or v.off != (0, 0):
        return 0
    if v.K < 256 or v.M < 6144:
        return 0
    ntm = cdiv(v.M, PW_BM)
    best, best_cost = 0, 0
    for bn in (384, 256):
        ntn = cdiv(v.Nout, bn)
        tiles = ntm * ntn
        if v.Nout / (ntn * bn) < 0.75:
            continue
        if bn != 384 and tiles < 192:
            continue
        cost = cdiv(tiles, 256) * bn
        if not best or cost < best_cost:
            best, best_cost = bn, cost
    return best


def b16_ks(c, one_tap):
    """k-steps of 16 per slab of conv_b16_kernel: the deeper of 4 / 2 that keeps every slab inside one tap; one tap: 4."""
    for ks in (4, 2):
        if one_tap or c % (16 * ks) == 0:
            return ks
    return 2


def b16_pd(v):
    """Two prefetched register sets for the long-K (>= 8192) multi-tap FORWARD launches, one everywhere else."""
    return 2 if (v.k_mul > 0 and v.K != v.C and v.K >= 8192 and v.div == 1) else 1


def x6_var(tiles, cus):
    """conv_x6_kernel's structure: up to 3 tiles per CU one double-buffered workgroup per CU (1), above two single-buffered (0)."""
    if SW["SG_X6_VARIANT"] is not None:
        return SW["SG_X6_VARIANT"] & 1
    return 1 if tiles <= 3 * cus else 0


def thin_ok(g):
    return (g.k == 1 and g.s == 1 and g.Cout <= 4 and g.Ho == g.H and g.Wo == g.W and g.Cin % 4 == 0 and g.xl % 4 == 0 and g.Cin >= 16)


def images_per_2gib(g, ebx, eby):
    """Images per launch such that both activation tensors stay under the limit (>= N: the whole batch; 0: one image alone passes it)."""
    per = max(g.H * g.W * g.xl * ebx, g.Ho * g.Wo * g.yl * eby)
    lim = SW["SG_CONV_MAX_BYTES"] if SW["SG_CONV_MAX_BYTES"] > 0 else (1 << 31) - (1 << 20)
    if per * g.N < lim:
        return g.N
    return max(lim // per, 0)


def x6p_up2_geom(g):
    """The fused up-sampling forward / dgrad: 3x3, stride 1, dilation 1, SAME, 64 -> 32, 8 x 16 SOURCE tiles."""
    return (g.k == 3 and g.s == 1 and g.d == 1 and g.pt == 1 and g.pl == 1 and g.Ho == g.H and g.Wo == g.W and g.Cin == 64 and g.Cout == 32
            and g.H % 16 == 0 and g.W % 32 == 0)


def x6wp_geom(g):
    """The patch filter gradient, which must take the layer too: 3x3, stride 1, dilation 1, SAME, Cin and Cout in {32, 64}, H % 4 == 0,
    W % 16 == 0."""
    return (g.k == 3 and g.s == 1 and g.d == 1 and g.pt == 1 and g.pl == 1 and g.Ho == g.H and g.Wo == g.W and g.Cin in (32, 64)
            and g.Cout in (32, 64) and g.H % 4 == 0 and g.W % 16 == 0)


def plan_conv_mode(mode, dt, g, dgrad, flags, not_thin=False):
    """ConvPlan as a dict (csrc/conv_igemm.hip: plan_conv_mode)."""
    b16, head = (dt & 0xff) == BF16, bool(dt & HEAD)
    f32 = not b16 and not head
    eb = 2 if b16 else 4
    pl = dict(family=CF_NATIVE, nb=0, vec=0, perm2=0, npl=0, Ck=0, Ckp=0, K=0, kd=0, Kpad=0, Npad=0, wbn=0, w_bytes=0, x6w_S=0, b16w_S=0,
              deep=0, a_img=0, part_img=0, res=0, bn_in=0, up2=0, bnb=0, planes_in=0)
    x_dense, y_dense = g.xgap == 0, g.ygap == 0
    pl["up2"] = int(f32 and mode == 1 and x6p_up2_geom(g) and x6wp_geom(g))    # (forward and filter gradient both take the patch kernels)
    thin = thin_ok(g) and not not_thin and not (dgrad and (flags & (EPI_BIAS | EPI_RELU)))
    if head:
        pl["family"] = CF_THIN if thin else CF_HEAD
        pl["nb"] = g.N if thin else images_per_2gib(g, 2, 4)
        return pl
    pl["nb"] = images_per_2gib(g, eb, eb)
    if thin:
        pl.update(family=CF_THIN, res=int(dgrad), bn_in=int(not dgrad and f32 and x_dense))
        return pl
    if pl["nb"] < 1 or (dgrad and g.s not in (1, 2)):
        return pl
    v = View(g.with_n(min(pl["nb"], g.N)), dgrad, eb)
    ch = 8 if b16 else 4
    pl["vec"] = int(v.C % ch == 0 and v.x_ld % ch == 0 and v.Nout % 4 == 0)
    vpad_safe = v.C % BK == 0 or v.K == v.C or v.x_ld == v.C       # padded reads must stay inside the tensor
    if not (vpad_safe and x6_ok(v, pl["vec"], b16, mode)):
        return pl
    pl["perm2"] = int(dgrad and SW["SG_DGRAD_PERM2"] != 0 and g.s == 2 and g.d == 1 and g.H % 2 == 0 and g.W % 2 == 0 and g.k * g.k <= 64)
    pl["npl"] = 1 if (b16 or mode == 2) else 3
    pl["Ck"] = pl["Ckp"] = v.C
    pl["K"] = v.K
    if v.C % BK != 0 and v.K != v.C:     # virtual channel padding: whole 32-deep slabs inside one tap
        pl["Ckp"] = x6_vpad_c(v.C)
        pl["K"] = (v.K // v.C) * pl["Ckp"]
        v.C, v.K = pl["Ckp"], pl["K"]
    N = v.Nout
    xw = x6w_shares(v) if pl["npl"] == 3 else 0
    if pl["npl"] == 3 and pl["Ckp"] == pl["Ck"] and x6p_geom(v, g.k) and not (v.C > 64 and xw > 0):
        pl.update(family=CF_PATCH, Kpad=pl["K"], Npad=N, w_bytes=3 * pl["K"] * N * 2,
                  bn_in=int(not dgrad and x_dense and v.C in (32, 64)))
        return pl
    wbn = pw_wide_width(v) if (pl["nb"] >= g.N and (pl["npl"] == 3 or b16)) else 0
    if wbn:
        kd = 16 if pl["npl"] == 3 else 64
        pl.update(family=CF_WIDE, wbn=wbn, Ckp=pl["K"], kd=kd, Kpad=cdiv(pl["K"], kd) * kd, Npad=cdiv(N, wbn) * wbn)
        pl["w_bytes"] = pl["npl"] * pl["Kpad"] * pl["Npad"] * 2
        pl["bnb"] = int(dgrad and pl["npl"] == 3 and x_dense and y_dense and g.Cout + 16 <= PW_BNB_MAXK)
        return pl
    pl.update(family=CF_SLAB, res=int(dgrad), deep=int(b16 and SW["SG_B16_DEEP"] != 0))
    pl["kd"] = 16 * b16_ks(pl["Ckp"], pl["K"] == pl["Ckp"]) if pl["deep"] else 32
    pl["Kpad"], pl["Npad"] = cdiv(pl["K"], pl["kd"]) * pl["kd"], cdiv(N, 128) * 128
    pl["w_bytes"] = x6_planes_bytes(pl["K"], N, pl["npl"], pl["kd"])
    img_part = v.OH * v.OW * N * 4
    if pl["npl"] == 3 and pl["kd"] == XW_KD and xw > 0:
        pl.update(x6w_S=xw, a_img=3 * v.H * v.W * v.C * 2, part_img=xw * img_part if xw > 1 else 0,
                  planes_in=int(pl["Ckp"] == pl["Ck"] and x_dense and y_dense))
    if pl["deep"] and pl["kd"] == BW_KD:
        pl["b16w_S"] = b16w_shares(v)
        pl["part_img"] = pl["b16w_S"] * img_part if pl["b16w_S"] > 1 else 0
    return pl


def ws_bytes_of(pl, images):
    sc = ((images * pl["a_img"] + 255) & ~255) + images * pl["part_img"]
    return ((pl["w_bytes"] + 255) & ~255) + sc if sc else pl["w_bytes"]


def native_vec(dt, g, dgrad, aligned):
    """Channel runs of a native launch: channels and pixel stride of the operand it gathers % 4, that operand 16-byte aligned (bf16: 8),
    and on fp32 storage the other channel count % 4 too."""
    b16, head = (dt & 0xff) == BF16, bool(dt & HEAD)
    ca, cn, ld = (g.Cout, g.Cin, g.yl) if dgrad else (g.Cin, g.Cout, g.xl)
    if ca % 4 or ld % 4:
        return 0
    if head and dgrad:
        return int(aligned == 16)
    if b16:
        return int(aligned >= 8)
    return int(cn % 4 == 0 and aligned == 16)


LAUNCH0 = dict(kernel=0, bn=0, vec=0, ut=0, var=0, mf16=0, ks=0, pd=0, skip_taps=0, group_m=0, cb=0, pc=0, pmulti=0)


def launch_form(cus, dt, g, pl, fast, dgrad, aligned, with_res):
    """sg_conv_launch as a dict: the form of one launch of `g.N` images of plan `pl`."""
    f = dict(LAUNCH0)
    b16, head = (dt & 0xff) == BF16, bool(dt & HEAD)
    if pl["family"] == CF_THIN:
        f.update(kernel=CK_THIN, bn=g.Cout, vec=1)
        return f
    v = View(g, dgrad, 4 if (head and dgrad) else (2 if b16 else 4))
    if pl["family"] == CF_HEAD or not fast:
        vec = native_vec(dt, g, dgrad, aligned)
        bn = pick_bn(v.M, v.Nout, cus)
        f.update(kernel=CK_NATIVE, bn=bn, vec=vec)
        if b16:      # the mixed-storage forms: no tap elimination, no K order, never the wave-uniform-tap form
            f["group_m"] = plan_common(v, False, bn, False, 4)[1]
        else:
            f["skip_taps"], f["group_m"], f["cb"] = plan_common(v, vec, bn, False, 4)
            f["ut"] = int(vec and (v.C % BK == 0 or v.K == v.C) and v.x_bytes != 0 and v.w_bytes != 0)
        return f
    if dgrad and pl["perm2"]:
        v.perm2 = 1
    if pl["family"] == CF_PATCH:
        f.update(kernel=CK_PATCH, bn=min(v.Nout, 128), pc=32 if v.C == 32 else 64, pmulti=int(v.C > 64))
        return f
    if pl["family"] == CF_WIDE:
        f.update(kernel=CK_WIDE, bn=pl["wbn"])
        return f
    v.C, v.K = pl["Ckp"], pl["K"]
    v.w_bytes = pl["w_bytes"]
    if pl["npl"] == 3 and not b16 and pl["x6w_S"] > 0 and not with_res:
        f.update(kernel=CK_X6W, bn=XW_N)
        com = plan_common(v, True, 128, True, 4)
    elif b16 and pl["deep"] and pl["b16w_S"] > 0 and not with_res:
        f.update(kernel=CK_B16W, bn=BW_N)
        com = plan_common(v, True, 128, True, 2)
    elif b16 and pl["deep"]:
        bn = pick_bn(v.M, v.Nout, cus)
        f.update(kernel=CK_B16, bn=bn, ks=b16_ks(v.C, v.K == v.C), pd=b16_pd(v))
        com = plan_common(v, True, bn, True, 2)
    else:
        bn = pick_bn(v.M, v.Nout, cus)
        f.update(kernel=CK_X6, bn=bn, var=x6_var(cdiv(v.M, BM) * cdiv(v.Nout, bn), cus),
                 mf16=int(pl["npl"] == 3 and SW["SG_X6_MF16"] != 0 and v.K != v.C))
        com = plan_common(v, True, bn, True, 2 if b16 else 4)
    f["vec"] = 1
    f["skip_taps"], f["group_m"], f["cb"] = com
    return f


def plan_mirror(cus, mode, dt, g, dgrad, flags=0, aligned=16):
    """sg_conv_plan as a dict, from the mirrors alone."""
    b16, head = (dt & 0xff) == BF16, bool(dt & HEAD)
    ebx = 2 if (b16 or head) else 4
    pl = plan_conv_mode(mode, dt, g, dgrad, flags)
    if pl["family"] == CF_THIN and not (aligned == 16 and (pl["nb"] >= g.N or pl["nb"] < 1 or (g.H * g.W * g.xl * ebx) % 16 == 0)):
        pl = plan_conv_mode(mode, dt, g, dgrad, flags, not_thin=True)
    nb = pl["nb"] if 1 <= pl["nb"] < g.N else g.N
    fast = int(pl["family"] >= CF_SLAB and pl["vec"] and aligned == 16)
    nsub = cdiv(g.N, nb)
    o = {k: pl[k] for k in ("family", "vec", "perm2", "npl", "kd", "Ck", "Ckp", "wbn", "x6w_S", "b16w_S", "deep", "res", "bn_in", "up2", "bnb",
                            "planes_in")}
    o.update(fast=fast, nb=nb, nsub=nsub, tail_n=g.N - (nsub - 1) * nb, ws_bytes=ws_bytes_of(pl, nb), _pl=pl)
    o["main"] = launch_form(cus, dt, g.with_n(nb), pl, fast, dgrad, aligned, False)
    o["tail"] = launch_form(cus, dt, g.with_n(o["tail_n"]), pl, fast, dgrad, aligned, False)
    takes_res = dgrad and pl["res"] and not head and (pl["family"] == CF_THIN or fast)
    o["with_res"] = launch_form(cus, dt, g.with_n(nb), pl, fast, dgrad, aligned, True) if takes_res else dict(LAUNCH0)
    return o


def form_name(o, la, dgrad, dt):
    """The name of launch `la` (a dict) of plan `o` (a dict): see the module docstring."""
    b16, head = (dt & 0xff) == BF16, bool(dt & HEAD)
    k = la["kernel"]
    n = ("dgrad." if dgrad else "fwd.") + KERNEL_NAMES[k]
    if k == CK_NATIVE:
        n += f".BN{la['bn']}." + ("ut" if la["ut"] else ("vec" if la["vec"] else "scalar"))
        n += (".f32>b16" if dgrad else ".b16>f32") if head else (".b16" if b16 else "")
    elif k == CK_THIN:
        n += f".CO{la['bn']}." + ("b16>f32" if head else ("b16" if b16 else "f32"))
    elif k == CK_X6:
        n += f".BN{la['bn']}.v{la['var']}" + (".mf16" if la["mf16"] else "") + (".npl1" if o["npl"] == 1 else "")
    elif k == CK_B16:
        n += f".BN{la['bn']}.KS{la['ks']}.PD{la['pd']}"
    elif k == CK_X6W:
        n += f".S{o['x6w_S']}"
    elif k == CK_B16W:
        n += f".S{o['b16w_S']}"
    elif k == CK_PATCH:
        n += f".C{la['pc']}" + ("m" if la["pmulti"] else "") + f".BN{la['bn']}"
    elif k == CK_WIDE:
        n += (".b16" if b16 else ".x6") + f".W{la['bn']}"
    if la["skip_taps"]:
        n += ".skip"
    if o["perm2"] and k in (CK_X6, CK_B16):
        n += ".perm2"
    if la["group_m"] > 1:
        n += f".gm{la['group_m']}"
    if la["cb"]:
        n += f".cb{la['cb']}"
    if o["Ckp"] != o["Ck"] and o["family"] == CF_SLAB and o["fast"]:
        n += ".vpad"
    if o["nsub"] > 1:
        n += f".sub{o['nb']}+{o['tail_n']}"
    return n


# ================================================================================================ the case tables
class Case:
    """dt: "f32" | "b16" | "head"; mode: the arithmetic on fp32 storage (sg_set_conv_x6); off: the activation operands sit one element
    off their 16-byte boundary (aligned = 0; bf16: 2 bytes); extra: further launches ("pin", "bn", "bninf", "bnb", "bnbrelu", "up2",
    "down2"); name: the form the plain launch takes at 256 CUs; res: the form of the launch with opts->res ("" = the plain one's,
    None = the call refuses res)."""

    def __init__(self, name, g, dt="f32", dgrad=False, mode=1, off=False, extra=(), res=None, flags=0):
        self.name, self.g, self.dt, self.dgrad, self.mode, self.off, self.extra, self.res, self.flags = name, g, dt, dgrad, mode, off, extra, res, flags

    @property
    def dtype(self):
        return {"f32": F32, "b16": BF16, "head": BF16 | HEAD}[self.dt]

    @property
    def id(self):
        t = f"{self.g.tag}-{self.dt}" + (f"-m{self.mode}" if self.mode != 1 else "") + ("-off" if self.off else "")
        if self.flags:
            t += f"-fl{self.flags}"
        return f"{t}-{self.name}"

    def mirror(self, cus=REF_CUS):
        return plan_mirror(cus, self.mode, self.dtype, self.g, self.dgrad, self.flags, 0 if self.off else 16)

    def mirror_name(self, cus=REF_CUS):
        o = self.mirror(cus)
        return form_name(o, o["main"], self.dgrad, self.dtype)

    def mirror_res_name(self, cus=REF_CUS):
        o = self.mirror(cus)
        return form_name(o, o["with_res"], self.dgrad, self.dtype) if o["with_res"]["kernel"] else None


G = Geom
FWD, DG = False, True

CASES = [
    # ---- conv_x6_kernel: structure v0 by tile count (784 tiles of width 32 > 768), BN128 by wave quantisation, ragged everything
    Case("fwd.slab.x6.BN32.v0", G(2, 224, 224, 32, 32, k=1)),
    Case("dgrad.slab.x6.BN32.v0", G(2, 224, 224, 32, 32, k=1), dgrad=DG, res=""),
    Case("fwd.slab.x6.BN128.v1", G(1, 128, 128, 32, 256, k=1)),                # 256 tiles of 128 = one round; 512 of 64 pay 0.93
    Case("fwd.slab.x6.BN128.v1.npl1", G(1, 128, 128, 32, 256, k=1), mode=2),
    Case("fwd.slab.x6.BN64.v1.mf16", G(3, 20, 32, 64, 96)),                    # M = 1920: 15 tiles; fewer than 256 tiles: BN64
    Case("dgrad.slab.x6.BN64.v1.mf16", G(3, 20, 32, 96, 64), dgrad=DG, res=""),
    Case("fwd.slab.x6.BN64.v1.mf16", G(2, 12, 20, 64, 40)),                    # ragged last column tile (40 of 64), M % 128 = 96
    Case("fwd.slab.x6.BN64.v1.mf16.gm16", G(2, 12, 20, 32, 224)),              # 224 columns: four 64-wide tiles, the last half empty
    Case("fwd.slab.x6.BN64.v1", G(2, 12, 20, 200, 96, k=1)),                   # K = 200: K % 32 != 0, one tap (ragged tail masked)
    Case("fwd.slab.x6.BN64.v1.mf16.vpad", G(2, 12, 20, 48, 96)),               # virtual channel padding 48 -> 64
    Case("fwd.slab.x6.BN64.v1.mf16.gm16.vpad", G(1, 12, 20, 304, 256)),        # 304 -> 320
    Case("fwd.native.BN64.vec", G(2, 12, 20, 48, 96, xgap=16)),                # x_ld > Cin: padded reads would leave the tensor
    Case("dgrad.slab.x6.BN64.v1.mf16.vpad", G(2, 12, 20, 96, 48), dgrad=DG, res=""),
    # ---- padding-tap elimination, parity-class rows
    Case("fwd.slab.x6.BN64.v1.mf16.skip", G(1, 32, 32, 64, 96, d=18)),
    Case("fwd.slab.x6.BN64.v1.mf16.skip", G(2, 8, 16, 64, 96, d=6)),           # rows where only the centre tap is live
    Case("dgrad.slab.x6.BN64.v1.mf16.skip", G(2, 8, 16, 96, 64, d=6), dgrad=DG, res=""),
    Case("dgrad.slab.x6.BN64.v1.mf16.skip.perm2", G(2, 16, 24, 64, 96, s=2), dgrad=DG, res=""),
    Case("dgrad.slab.x6.BN64.v1.mf16", G(2, 17, 24, 64, 96, s=2), dgrad=DG, res=""),       # odd H: the rule declines
    Case("dgrad.slab.x6.BN64.v1.skip.perm2", G(2, 16, 16, 128, 256, k=1, s=2), dgrad=DG, res=""),   # the lone 1x1 tap
    # ---- grouped tile order and channel-block K order
    Case("fwd.slab.x6.BN64.v1.mf16.cb4", G(1, 64, 64, 256, 160)),              # one image = 4 MiB > 2 MiB, 8 slabs per tap; 160 / 256 columns: off x6w
    Case("fwd.slab.x6.BN64.v1.mf16", G(1, 32, 32, 256, 160)),                  # its neighbour: 1 MiB image, cb 0
    Case("fwd.slab.x6w.S1.cb4", G(1, 64, 64, 256, 200)),                       # 200 / 256 columns: the planes-in kernel, same K order
    Case("fwd.slab.x6.BN64.v0.gm8", G(1, 192, 176, 128, 256, k=1)),            # A = 16.5 MiB: an XCD's eighth above 2 MiB; 1056 tiles > 768
    # ---- conv_x6w_kernel (planes-in), with and without the caller's planes; res falls to conv_x6_kernel on the same planes
    Case("fwd.slab.x6w.S1", G(1, 32, 64, 256, 256), extra=("pin",)),
    Case("fwd.slab.x6w.S2", G(1, 32, 32, 512, 256), extra=("pin",)),
    Case("fwd.slab.x6w.S1.skip", G(2, 32, 64, 256, 224, d=6), extra=("pin",)),        # dilated, ragged columns at 224
    Case("dgrad.slab.x6w.S1", G(1, 32, 64, 256, 256), dgrad=DG, extra=("pin",), res="dgrad.slab.x6.BN64.v1.mf16.gm16"),
    Case("dgrad.slab.x6w.S2.skip", G(1, 32, 32, 256, 512, d=6), dgrad=DG, res="dgrad.slab.x6.BN64.v1.mf16.skip.gm16"),
    # ---- conv_b16_kernel: KS, PD, BN
    Case("fwd.slab.b16.BN64.KS4.PD2", G(1, 24, 24, 1024, 64), dt="b16"),       # K = 9216 forward; 576 pixels: off b16w
    Case("dgrad.slab.b16.BN64.KS4.PD1", G(1, 24, 24, 64, 1024), dt="b16", dgrad=DG, res=""),
    Case("fwd.slab.b16.BN64.KS2.PD1", G(3, 20, 32, 96, 96), dt="b16"),
    Case("fwd.slab.b16.BN32.KS2.PD1", G(2, 12, 20, 32, 32), dt="b16"),
    Case("fwd.slab.b16.BN64.KS4.PD1", G(2, 12, 20, 200, 96, k=1), dt="b16"),   # one tap, K % 64 != 0
    Case("fwd.slab.b16.BN128.KS4.PD1", G(1, 128, 128, 32, 256, k=1), dt="b16"),
    Case("fwd.slab.b16.BN64.KS2.PD1.vpad", G(2, 12, 20, 80, 96), dt="b16"),      # 80 -> 96 channels per tap
    Case("fwd.slab.b16.BN64.KS4.PD1.vpad", G(2, 12, 20, 48, 96), dt="b16"),      # 48 -> 64
    Case("fwd.slab.b16.BN64.KS4.PD1.skip", G(2, 8, 16, 64, 96, d=6), dt="b16"),
    Case("dgrad.slab.b16.BN64.KS4.PD1.skip.perm2", G(2, 16, 24, 64, 128, s=2), dt="b16", dgrad=DG, res=""),
    # ---- conv_b16w_kernel: S1, S2, S4 from b16w_shares' own arithmetic (workgroups per image = column tiles x pixels / 256; three
    # shares are out of the rule's reach: test_three_shares_are_out_of_the_rules_reach)
    Case("fwd.slab.b16w.S1", G(1, 64, 64, 128, 256), dt="b16"),                # 16 workgroups, K = 1152
    Case("fwd.slab.b16w.S2", G(1, 32, 64, 512, 256), dt="b16"),                # 8 workgroups, K = 4608
    Case("fwd.slab.b16.BN64.KS4.PD1.gm16", G(1, 32, 32, 768, 256), dt="b16"),  # 4 workgroups, K = 6912: 3 shares of 2304 make 12 < 16
    Case("fwd.slab.b16w.S4", G(1, 32, 32, 1024, 256), dt="b16"),               # 4 workgroups, K = 9216
    Case("dgrad.slab.b16w.S2", G(1, 32, 64, 256, 512), dt="b16", dgrad=DG, res="dgrad.slab.b16.BN64.KS4.PD1.gm16"),
    # ---- conv_x6p_kernel: the nine <C, BN> forms, forward and dgrad; one tile (8 x 16) and the persistent walk
    Case("fwd.patch.C32.BN32", G(1, 8, 16, 32, 32), extra=("bn", "bninf")),
    Case("fwd.patch.C32.BN64", G(2, 8, 16, 32, 64)),
    Case("fwd.patch.C32.BN128", G(2, 16, 16, 32, 128)),
    Case("fwd.patch.C64.BN32", G(2, 8, 32, 64, 32), extra=("bn", "bninf")),
    Case("fwd.patch.C64.BN64", G(3, 96, 128, 64, 64)),                         # 288 pixel tiles > 256 CUs x workgroups: the walk
    Case("fwd.patch.C64.BN128", G(1, 8, 16, 64, 256)),
    Case("fwd.patch.C64m.BN32", G(1, 8, 16, 128, 32)),
    Case("fwd.patch.C64m.BN64", G(2, 16, 16, 256, 64)),
    Case("fwd.patch.C64m.BN128", G(1, 8, 16, 512, 128)),
    Case("dgrad.patch.C32.BN32", G(2, 8, 16, 32, 32), dgrad=DG),
    Case("dgrad.patch.C64.BN32", G(2, 16, 16, 32, 64), dgrad=DG),
    Case("dgrad.patch.C64m.BN64", G(1, 8, 32, 64, 128), dgrad=DG),
    Case("dgrad.patch.C32.BN128", G(1, 16, 16, 128, 32), dgrad=DG),
    Case("dgrad.patch.C32.BN64", G(1, 8, 16, 64, 32), dgrad=DG),
    Case("dgrad.patch.C64.BN64", G(1, 8, 16, 64, 64), dgrad=DG),
    Case("dgrad.patch.C64.BN128", G(1, 8, 16, 128, 64), dgrad=DG),
    Case("dgrad.patch.C64m.BN32", G(1, 8, 16, 32, 128), dgrad=DG),
    Case("dgrad.patch.C64m.BN64", G(1, 8, 16, 64, 256), dgrad=DG),             # chunks at 256 channels
    Case("dgrad.patch.C64m.BN128", G(1, 8, 16, 128, 512), dgrad=DG),           # ... and at 512
    Case("fwd.patch.C64.BN32", G(1, 16, 32, 64, 32), extra=("up2",)),
    Case("dgrad.patch.C32.BN64", G(1, 16, 32, 64, 32), dgrad=DG, extra=("down2",)),
    # ---- pw_wide_kernel
    Case("fwd.wide.x6.W384", G(1, 96, 64, 264, 728, k=1)),                     # 6144 rows exactly; K % 16 != 0; ragged 728
    Case("fwd.wide.x6.W384", G(1, 97, 64, 256, 384, k=1)),                     # 6144 + 64 rows: ragged last row tile
    Case("fwd.wide.x6.W256", G(2, 96, 64, 256, 1024, k=1)),                    # 96 x 4 = 384 tiles
    Case("dgrad.wide.x6.W384", G(1, 96, 64, 384, 256, k=1), dgrad=DG, extra=("bnb", "bnbrelu")),
    Case("fwd.wide.b16.W384", G(1, 96, 64, 296, 728, k=1), dt="b16"),          # K % 64 != 0
    Case("dgrad.wide.b16.W384", G(1, 96, 64, 384, 256, k=1), dt="b16", dgrad=DG),
    Case("fwd.slab.x6.BN128.v1", G(1, 6143, 1, 256, 384, k=1)),               # one row short of 6144: must not be wide
    # ---- thin kernels
    Case("fwd.thin.CO1.f32", G(2, 9, 7, 64, 1, k=1), extra=("bn",)),
    Case("fwd.thin.CO2.f32", G(2, 9, 7, 32, 2, k=1)),
    Case("fwd.thin.CO3.f32", G(1, 5, 7, 20, 3, k=1)),
    Case("fwd.thin.CO4.f32", G(2, 9, 7, 48, 4, k=1)),
    Case("fwd.thin.CO1.b16", G(2, 9, 7, 64, 1, k=1), dt="b16"),
    Case("fwd.thin.CO2.b16", G(2, 9, 7, 32, 2, k=1), dt="b16"),
    Case("fwd.thin.CO3.b16", G(1, 5, 7, 24, 3, k=1), dt="b16"),
    Case("fwd.thin.CO4.b16", G(2, 9, 7, 48, 4, k=1), dt="b16"),
    Case("fwd.thin.CO1.b16>f32", G(2, 9, 7, 64, 1, k=1), dt="head"),
    Case("fwd.thin.CO2.b16>f32", G(2, 9, 7, 32, 2, k=1), dt="head"),
    Case("fwd.thin.CO3.b16>f32", G(1, 5, 7, 24, 3, k=1), dt="head"),
    Case("fwd.thin.CO4.b16>f32", G(2, 9, 7, 48, 4, k=1), dt="head"),
    Case("dgrad.thin.CO1.f32", G(2, 9, 7, 64, 1, k=1), dgrad=DG, res=""),
    Case("dgrad.thin.CO2.f32", G(2, 9, 7, 32, 2, k=1), dgrad=DG, res=""),
    Case("dgrad.thin.CO3.b16", G(1, 5, 7, 24, 3, k=1), dt="b16", dgrad=DG, res=""),
    Case("dgrad.thin.CO4.b16", G(2, 9, 7, 48, 4, k=1), dt="b16", dgrad=DG, res=""),
    Case("dgrad.thin.CO2.b16>f32", G(2, 9, 7, 32, 2, k=1), dt="head", dgrad=DG),
    Case("dgrad.native.BN32.scalar", G(2, 9, 7, 32, 2, k=1), dgrad=DG, flags=EPI_BIAS | EPI_RELU),   # bias / ReLU leave the thin family
    Case("fwd.native.BN32.scalar", G(2, 9, 7, 32, 2, k=1), off=True),          # x 4 bytes off: PLAN_NOT_THIN
    Case("fwd.native.BN32.scalar.b16", G(2, 9, 7, 32, 2, k=1), dt="b16", off=True),        # bf16: 2 bytes off
    # ---- igemm_conv_kernel: scalar, vec, ut, the mixed storage forms, BN128, and every fast family's fallback
    Case("fwd.native.BN32.scalar", G(2, 24, 20, 3, 32, s=2)),
    Case("fwd.native.BN64.scalar.skip", G(1, 16, 16, 45, 45, d=4)),
    Case("fwd.native.BN128.scalar", G(1, 128, 128, 3, 256, k=1)),
    Case("fwd.native.BN64.vec", G(2, 12, 20, 48, 96), mode=0),                 # C % 32 != 0 and multi-tap: a slab straddles taps
    Case("fwd.native.BN64.ut", G(2, 12, 20, 64, 96), mode=0),
    Case("dgrad.native.BN64.ut", G(2, 12, 20, 96, 64), dgrad=DG, mode=0),
    Case("fwd.native.BN32.vec.b16", G(2, 12, 20, 12, 12), dt="b16"),           # 12 channels: no 16-byte runs of bf16, 8-byte ones
    Case("fwd.native.BN32.vec.b16>f32", G(2, 12, 12, 64, 2), dt="head"),
    Case("dgrad.native.BN64.scalar.f32>b16", G(2, 12, 12, 64, 2), dt="head", dgrad=DG),
    Case("fwd.native.BN64.scalar", G(3, 20, 32, 64, 96), off=True),            # slab.x6's fallback
    Case("fwd.native.BN32.scalar", G(1, 8, 16, 32, 32), off=True),             # patch's
    Case("fwd.native.BN64.scalar", G(1, 96, 64, 264, 728, k=1), off=True),     # wide's
    Case("fwd.native.BN64.scalar.b16", G(3, 20, 32, 96, 96), dt="b16", off=True),          # slab.b16's
    Case("dgrad.native.BN64.scalar", G(3, 20, 32, 96, 64), dgrad=DG, off=True),
]

# one concat-slice pair per family: x_ld > Cin and y_ld > Cout
SLICE_CASES = [
    Case("fwd.slab.x6.BN64.v1.mf16", G(3, 20, 32, 64, 96, xgap=32, ygap=8)),
    Case("dgrad.slab.x6.BN64.v1.mf16", G(3, 20, 32, 96, 64, xgap=8, ygap=32), dgrad=DG, res=""),
    Case("fwd.slab.b16.BN64.KS4.PD1", G(3, 20, 32, 64, 96, xgap=64, ygap=8), dt="b16"),
    Case("fwd.slab.x6w.S1.cb4", G(1, 32, 64, 256, 256, xgap=32, ygap=4)),
    Case("fwd.slab.b16w.S2.cb4", G(1, 32, 64, 512, 256, xgap=64, ygap=8), dt="b16"),
    Case("fwd.patch.C32.BN32", G(2, 8, 16, 32, 32, xgap=32, ygap=4)),
    Case("fwd.wide.x6.W384", G(1, 96, 64, 256, 384, k=1, xgap=64, ygap=4)),
    Case("fwd.thin.CO2.f32", G(2, 9, 7, 32, 2, k=1, xgap=32, ygap=3)),
    Case("dgrad.thin.CO2.f32", G(2, 9, 7, 32, 2, k=1, xgap=32, ygap=3), dgrad=DG, res=""),
    Case("fwd.native.BN32.scalar", G(2, 24, 20, 3, 32, s=2, xgap=5, ygap=3)),
]

# SG_CONV_MAX_BYTES = 2 MiB: three images of 768 KiB go as sub-batches of two and one
SUB_CASES = [
    Case("fwd.slab.x6.BN64.v1.mf16.sub2+1", G(3, 32, 32, 192, 192)),
    Case("dgrad.slab.x6.BN64.v1.mf16.sub2+1", G(3, 32, 32, 192, 192), dgrad=DG, res=""),
    Case("fwd.slab.b16.BN64.KS4.PD1.gm16.sub2+1", G(3, 32, 32, 384, 384), dt="b16"),
    Case("fwd.patch.C64.BN64.sub2+1", G(3, 32, 96, 64, 64)),
    Case("fwd.slab.x6.BN64.v1.gm16.sub2+1", G(13, 16, 32, 256, 384, k=1)),     # 6656 rows: wide in one launch, never in sub-batches
    Case("fwd.thin.CO2.f32.sub2+1", G(3, 64, 48, 64, 2, k=1)),
    Case("fwd.native.BN32.vec.b16.sub2+1", G(3, 97, 61, 60, 2, k=1), dt="b16"),   # 710040 bytes per image: not a multiple of 16, leaves thin
    Case("fwd.native.BN64.scalar.sub2+1", G(3, 64, 64, 45, 45)),
]


def child_cases(child):
    """The cases a child process runs, with the names its mirror gives them (`with switched(CHILD_ENVS[child])` in the parent)."""
    if child == "sub":
        return list(SUB_CASES)
    base = [c for c in CASES + SLICE_CASES if ".slab.x6." in c.name or ".slab.b16." in c.name or ".slab.b16w" in c.name]
    if child == "v0":
        base = [c for c in base if ".slab.x6." in c.name or (c.res and ".slab.x6." in c.res)]
    out = []
    for c in base:
        n = Case(c.name, c.g, c.dt, c.dgrad, c.mode, c.off, c.extra, c.res, c.flags)
        n.name = n.mirror_name()
        if n.res is not None:
            r = n.mirror_res_name()
            n.res = "" if r == n.name else r
        out.append(n)
    return out


# The forms every pull request must keep reachable: whole names up to the modifier boundary (base_of), of a plain launch or of a
# launch with res, in the main tables or - the v0 structure of the shapes that are v1 by tile count - in the SG_X6_VARIANT=0 child;
# and every modifier as a whole token of some name.
_MODIFIERS = re.compile(r"(\.skip|\.perm2|\.gm\d+|\.cb\d+|\.vpad|\.sub\d+\+\d+)+$")


def base_of(name):
    return _MODIFIERS.sub("", name)


REQUIRED_FORMS = (
    ["fwd.slab.x6.BN32.v0", "dgrad.slab.x6.BN32.v0", "fwd.slab.x6.BN64.v0", "fwd.slab.x6.BN64.v1", "dgrad.slab.x6.BN64.v1",
     "fwd.slab.x6.BN64.v1.mf16", "dgrad.slab.x6.BN64.v1.mf16", "fwd.slab.x6.BN128.v1", "fwd.slab.x6.BN128.v1.npl1",
     "fwd.slab.x6.BN128.v0", "fwd.slab.x6.BN64.v0.mf16", "dgrad.slab.x6.BN64.v0.mf16", "dgrad.slab.x6.BN64.v0"]
    + ["fwd.slab.b16.BN64.KS4.PD2", "dgrad.slab.b16.BN64.KS4.PD1", "fwd.slab.b16.BN64.KS2.PD1", "fwd.slab.b16.BN32.KS2.PD1",
       "fwd.slab.b16.BN64.KS4.PD1", "fwd.slab.b16.BN128.KS4.PD1"]
    + ["fwd.slab.x6w.S1", "fwd.slab.x6w.S2", "dgrad.slab.x6w.S1", "dgrad.slab.x6w.S2"]
    + ["fwd.slab.b16w.S1", "fwd.slab.b16w.S2", "fwd.slab.b16w.S4", "dgrad.slab.b16w.S2"]
    + [f"{d}.patch.C{c}.BN{bn}" for d in ("fwd", "dgrad") for c in ("32", "64", "64m") for bn in (32, 64, 128)]
    + ["fwd.wide.x6.W384", "fwd.wide.x6.W256", "dgrad.wide.x6.W384", "fwd.wide.b16.W384", "dgrad.wide.b16.W384"]
    + [f"fwd.thin.CO{n}.{s}" for n in (1, 2, 3, 4) for s in ("f32", "b16", "b16>f32")]
    + ["dgrad.thin.CO1.f32", "dgrad.thin.CO2.f32", "dgrad.thin.CO3.b16", "dgrad.thin.CO4.b16", "dgrad.thin.CO2.b16>f32"]
    + ["fwd.native.BN32.scalar", "fwd.native.BN64.scalar", "fwd.native.BN128.scalar", "fwd.native.BN64.vec", "fwd.native.BN64.ut",
       "dgrad.native.BN64.ut", "dgrad.native.BN32.scalar", "dgrad.native.BN64.scalar", "fwd.native.BN32.vec.b16",
       "fwd.native.BN32.scalar.b16", "fwd.native.BN64.scalar.b16", "fwd.native.BN32.vec.b16>f32", "dgrad.native.BN64.scalar.f32>b16"]
)
REQUIRED_MODIFIERS = ("skip", "perm2", "gm8", "gm16", "cb4", "vpad", "sub2+1")
REQUIRED_EXTRAS = ("pin", "bn", "bninf", "bnb", "bnbrelu", "up2", "down2")


def all_case_names():
    names = []
    for c in CASES + SLICE_CASES + SUB_CASES:
        names.append(c.name)
        if c.res:
            names.append(c.res)
    with switched(CHILD_ENVS["v0"]):
        names += [c.name for c in child_cases("v0")]
    return names


def missing_forms(names=None, extras=None):
    names = all_case_names() if names is None else names
    extras = {e for c in CASES for e in c.extra} if extras is None else extras
    bases = {base_of(n) for n in names}
    tokens = {t for n in names for t in n[len(base_of(n)):].split(".") if t}
    return ([f for f in REQUIRED_FORMS if f not in bases] + ["." + m for m in REQUIRED_MODIFIERS if m not in tokens]
            + [e for e in REQUIRED_EXTRAS if e not in extras])


# ================================================================================================ operands and references
def bf16r(t):
    return t.bfloat16().float()


def rnd(gen, *shape):
    return (torch.rand(*shape, generator=gen) * 2.0 - 1.0).float()


_OPS = {}


def operands(c, pipe_w):
    """The host operands of a case and its float64 references, computed once: x (dgrad: dy and res), w, biases, and
    ref(flags) -> y / dx.  Storage bf16: activations rounded (normal, then rounded); pipe_w: the kernel rounds the weights to bf16
    (the bf16-pipe kernels of bf16 storage and arithmetic mode 2 - not the native and thin kernels), so the reference starts from
    the rounded weights; mode 2 also rounds the fp32 activations on their way into LDS."""
    key = (c.g.tag, c.dt, c.dgrad, c.mode, pipe_w)
    if key in _OPS:
        return _OPS[key]
    from oracle import tfops as T
    g = c.g
    gen = torch.Generator().manual_seed(sum(map(ord, c.g.tag)) + 7 * c.dgrad)
    b16 = c.dt != "f32"
    act = (lambda *s: bf16r(torch.randn(*s, generator=gen))) if b16 else (lambda *s: rnd(gen, *s))
    w = rnd(gen, g.k, g.k, g.Cin, g.Cout) * (1.0 / math.sqrt(g.k * g.k * g.Cin))
    wr = bf16r(w) if pipe_w else w
    o = dict(w=w)
    if not c.dgrad:
        x = act(g.N, g.H, g.W, g.Cin)
        xr = bf16r(x) if (pipe_w and not b16) else x
        o["x"] = x
        o["bias"] = rnd(gen, g.Cout) * 3.0        # large enough to move the channel means
        with torch.no_grad():
            o["lin"] = T.conv2d(xr.double(), wr.double(), None, g.s, g.d, "same")
    else:
        dy = act(g.N, g.Ho, g.Wo, g.Cout)
        if c.dt == "head":                        # the few-channel side is fp32
            dy = rnd(gen, g.N, g.Ho, g.Wo, g.Cout)
        dyr = bf16r(dy) if (pipe_w and c.dt == "f32") else dy
        o["dy"] = dy
        o["bias"] = rnd(gen, g.Cin) * 3.0
        o["res"] = act(g.N, g.H, g.W, g.Cin)
        xz = torch.zeros(g.N, g.H, g.W, g.Cin, dtype=torch.float64, requires_grad=True)
        y = T.conv2d(xz, wr.double(), None, g.s, g.d, "same")
        (o["lin"],) = torch.autograd.grad(y, xz, dyr.double())
    _OPS[key] = o
    return o


def epilogue_ref(o, flags, res=None):
    r = o["lin"]
    if flags & EPI_BIAS:
        r = r + o["bias"].double()
    if flags & EPI_RELU:
        r = torch.relu(r)
    if res is not None:
        r = r + res.double()
    return r


def bound_of(c, pipe_w, out_b16):
    """The project's bounds: fp32 storage 2e-5 of max|ref| (tests/test_ops_gpu.py), bf16 products on rounded operands 1e-5, a bf16
    output one bf16 ulp, 2^-8."""
    if out_b16:
        return 2.0 ** -8
    return 1e-5 if (pipe_w and c.dt == "f32") else 2e-5


def record(cid, launch, qty, rel, bound):
    RECORDS.append((cid, launch, qty, rel, bound))
    if not QUIET:
        print(f"REC {cid} {launch} {qty} rel={rel:.3e} bound={bound:.3e}")


def compare(cid, launch, qty, got, ref, bound, scale=None):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (cid, launch, qty, tuple(got.shape), tuple(ref.shape))
    scale = ref.abs().max().item() if scale is None else scale
    fin = bool(torch.isfinite(got).all())
    err = (got - ref).abs().max().item() if fin else float("inf")
    record(cid, launch, qty, err / scale if scale > 0 else (0.0 if err == 0 else float("inf")), bound)
    assert fin, f"{cid} {launch} {qty}: non-finite values in the result"
    assert err <= bound * scale, f"{cid} {launch} {qty}: max err {err:.3e} > {bound:.3e} * {scale:.3e} (rel {err / max(scale, 1e-300):.2e})"


# ================================================================================================ the runner
PLAN_FIELDS = ("family", "fast", "nb", "nsub", "tail_n", "vec", "perm2", "npl", "kd", "Ck", "Ckp", "wbn", "x6w_S", "b16w_S", "deep", "res",
               "bn_in", "up2", "bnb", "planes_in", "ws_bytes")


def assert_plan(engine, c, cid):
    """Mirror == id, engine plan == mirror field by field, planes job and caps agree.  Returns (mirror plan, engine plan)."""
    from building_detection_amd import _lib
    for k in FOREIGN_SWITCHES:
        assert k not in os.environ, f"{k} is set: the mirrors of tests/_conv_cases.py are written for its default"
    cus = int(engine.lib.sg_num_cus(engine.h))
    assert cus == REF_CUS, f"the case shapes are chosen at {REF_CUS} CUs; this device has {cus}"
    assert int(engine.lib.sg_get_conv_x6()) == c.mode
    o = c.mirror(cus)
    name = form_name(o, o["main"], c.dgrad, c.dtype)
    assert name == c.name, f"{cid}: the mirror names {name}"
    d = c.g.desc()
    pl = _lib.ConvPlan()
    rc = engine.lib.sg_conv2d_plan(engine.h, c.dtype, CT.byref(d), int(c.dgrad), c.flags, 0 if c.off else 16, CT.byref(pl))
    assert rc == 0, engine.lib.sg_last_error()
    for k in PLAN_FIELDS:
        assert getattr(pl, k) == o[k], f"{cid}: sg_conv2d_plan.{k} = {getattr(pl, k)}, the mirror says {o[k]}"
    for which in ("main", "tail", "with_res"):
        for k in LAUNCH0:
            assert getattr(getattr(pl, which), k) == o[which][k], f"{cid}: sg_conv2d_plan.{which}.{k} = {getattr(getattr(pl, which), k)}, the mirror says {o[which][k]}"
    assert _lib.conv_form_name(pl, pl.main, c.dgrad, c.dtype) == c.name
    rname = form_name(o, o["with_res"], c.dgrad, c.dtype) if o["with_res"]["kernel"] else None
    want = c.name if c.res == "" else c.res
    assert rname == want, f"{cid}: with res the mirror names {rname}, the case says {want}"
    if not c.off and not c.flags:      # both queries answer for aligned operands and no flags
        job, nbytes = _lib.PlanesJob(), CT.c_size_t(0)
        assert engine.lib.sg_conv2d_planes_job(engine.h, c.dtype, CT.byref(d), int(c.dgrad), CT.byref(job), CT.byref(nbytes)) == 0
        kind = {CF_SLAB: 1, CF_PATCH: 2, CF_WIDE: 3}.get(o["family"], 0)
        assert job.kind == kind, f"{cid}: sg_conv2d_planes_job.kind = {job.kind}, the plan's family says {kind}"
        if kind:
            p0 = o["_pl"]
            got = (job.npl, job.K, job.Ck, job.Ckp, job.kd, job.Kpad, job.Npad)
            assert got == (p0["npl"], p0["K"], p0["Ck"], p0["Ckp"], p0["kd"], p0["Kpad"], p0["Npad"]), (cid, got)
            assert nbytes.value == ws_bytes_of(p0, c.g.N)
        caps = _lib.ConvCaps()
        assert engine.lib.sg_conv2d_caps(engine.h, c.dtype, CT.byref(d), int(c.dgrad), CT.byref(caps)) == 0
        assert caps.thin == int(o["family"] == CF_THIN) and caps.planes_in == o["planes_in"], cid
        if c.dgrad:
            assert caps.bnb == o["bnb"], cid
        else:
            assert caps.up2 == o["up2"], cid
            assert caps.bn_in <= o["bn_in"], cid      # (the filter gradient must take the operand too)
    return o, pl


def _tt(c, side):
    """torch dtype of an operand: "x" (the Cin side) or "y" (the Cout side)."""
    if c.dt == "f32":
        return torch.float32
    if c.dt == "head" and side == "y":
        return torch.float32
    return torch.bfloat16


def _arena(t, ld, dev, off=False, role="in"):
    """A [..][C] host tensor as a guarded operand of pixel stride ld (the gap columns NaN)."""
    C = t.shape[-1]
    return Guarded(widen(t, ld) if ld != C else t.reshape(-1, C), dev, off=off, role=role)


def _read(gd, C, ld, shape, what):
    t = gd.read()
    if ld != C:
        gaps_keep_prefill(t, C, 0, what)
        t = t[:, :C].contiguous()
    return t.reshape(shape)


def launch(engine, c, o, pl, flags, cid, tag, res=None, inplace=False, stats=False, pin=False, bn=None, bnb=None, up2=False, down2=False,
           expect=0):
    """One call on guarded arenas; returns the output (None for a refused call).  Bands, input bits, written-ness, the workspace's
    far band and - for a refused call - the untouched outputs are checked here."""
    from building_detection_amd import _lib
    g, dev = c.g, "cuda"
    d = g.desc()
    dg = c.dgrad
    tx, ty = _tt(c, "x"), _tt(c, "y")
    keep, opts = [], _lib.ConvOpts()
    wsn = int(engine.lib.sg_conv2d_dgrad_ws_bytes(CT.byref(d)) if dg else engine.lib.sg_conv2d_fwd_ws_bytes(CT.byref(d)))
    assert pl.ws_bytes <= wsn or not pl.fast, f"{cid}: the plan's workspace {pl.ws_bytes} exceeds the query's {wsn}"
    gws = Guarded.ws(wsn, dev)
    opts.ws, opts.ws_bytes = gws.ptr(), wsn
    gw = Guarded(o["w"], dev)
    gb = Guarded(o["bias"], dev) if (flags & EPI_BIAS) else None
    if not dg:
        xs = o["x"]
        if up2:
            xs = o["x_src"]
        ga = _arena(xs.to(tx), g.xl, dev, off=c.off)
        oshape, oC, old, odt = (g.N, g.Ho, g.Wo, g.Cout), g.Cout, g.yl, ty
    else:
        ga = _arena(o["dy"].to(ty), g.yl, dev, off=c.off)
        oshape, oC, old, odt = ((g.N, g.H // 2, g.W // 2, g.Cin) if down2 else (g.N, g.H, g.W, g.Cin)), g.Cin, g.xl, tx
    if inplace:
        gout = _arena(res.to(odt), old, dev, off=c.off, role="out")
    else:
        gout = Guarded.out((math.prod(oshape[:3]), old), odt, dev, off=c.off)
    gres = None
    if res is not None:
        if inplace:
            opts.res = gout.ptr()
        else:
            gres = _arena(res.to(odt), old, dev, off=c.off)
            opts.res = gres.ptr()
    gst, tiles = None, CT.c_int(-1)
    if stats:
        gst = Guarded.out((max(int(engine.lib.sg_conv2d_fwd_stats_bytes(CT.byref(d))) // 4, 1),), torch.float32, dev)
        opts.stats, opts.tiles_out = gst.ptr(), CT.pointer(tiles)
    if pin:
        src = (o["dy"] if dg else o["x"]).cuda()
        planes = engine.split_planes(src).cpu()
        gp = Guarded(planes, dev)
        keep.append(gp)
        opts.a_planes = gp.ptr()
    if bn is not None:
        keep += [Guarded(t, dev) for t in bn[:4]]
        bq = _lib.BnIn(*(t.ptr() for t in keep[-4:]), int(bn[4]), int(bn[5]), 1e-3)
        opts.bn_in = CT.pointer(bq)
    gdz = None
    if bnb is not None:
        gx_, gm_, gi_, gg_, gbt_, gdg_, gdb_ = (Guarded(t, dev) for t in bnb[:7])
        gdz = Guarded.out(tuple(bnb[0].shape), torch.float32, dev)
        keep += [gx_, gm_, gi_, gg_, gbt_, gdg_, gdb_]
        bq2 = _lib.BnBwdIn(gx_.ptr(), gm_.ptr(), gi_.ptr(), gg_.ptr(), gbt_.ptr() if bnb[7] else None, gdg_.ptr(), gdb_.ptr(), gdz.ptr(),
                           int(bnb[7]), bnb[0].shape[0])
        opts.bnb = CT.pointer(bq2)
    fl = flags | (PRO_UP2 if up2 else 0) | (EPI_DOWN2 if down2 else 0)
    fn = engine.lib.sg_conv2d_dgrad if dg else engine.lib.sg_conv2d_fwd
    rc = fn(engine.h, engine.stream, c.dtype, CT.byref(d), ga.ptr(), gw.ptr(), gb.ptr() if gb else None, gout.ptr(), fl, CT.byref(opts))
    torch.cuda.synchronize()
    what = f"{cid} {tag}"
    check_all([x for x in [ga, gw, gb, gout, gres, gws, gst, gdz] + keep if x is not None], what)
    assert rc == expect, f"{what}: rc = {rc}, expected {expect}: {engine.lib.sg_last_error()}"
    if rc:
        if not inplace:
            untouched(gout, what)
        for x in (gst, gdz, gws):
            if x is not None:
                untouched(x, what)
        return None
    y = _read(gout, oC, old, oshape, what)
    assert_written(y, what)
    out = dict(y=y)
    if stats:
        out["tiles"] = tiles.value
        out["stats"] = gst.read()
        if tiles.value == 0:
            untouched(gst, what + " (no statistics promised)")
    if gdz is not None:
        out["dz"] = gdz.read()
        assert_written(out["dz"], what + " dz")
    return out


def run_case(engine, c):
    """Every launch of one case; raises on the first failure."""
    cid = c.id
    assert not FAULTED, f"{cid}: not launched - an earlier case of this process left the device in error: {FAULTED[0]}"
    prev = engine.lib.sg_set_conv_x6(c.mode)
    try:
        _run_case(engine, c, cid)
    except RuntimeError as e:      # a HIP error (torch raises it from the synchronize): nothing more is launched by this process
        FAULTED.append(f"{cid}: {e}")
        raise
    finally:
        engine.lib.sg_set_conv_x6(prev)
        _OPS.clear()      # (operands and float64 references of one case at a time)


def _run_case(engine, c, cid):
    o_m, pl = assert_plan(engine, c, cid)
    g, dg = c.g, c.dgrad
    k = o_m["main"]["kernel"]
    pipe_w = k in (CK_X6, CK_B16, CK_X6W, CK_B16W, CK_PATCH, CK_WIDE) and o_m["npl"] == 1
    o = operands(c, pipe_w)
    out_b16 = _tt(c, "x" if dg else "y") == torch.bfloat16
    bound = bound_of(c, pipe_w, out_b16)
    if not dg:
        variants = [("plain", 0), ("bias", EPI_BIAS), ("relu", EPI_RELU), ("bias+relu", EPI_BIAS | EPI_RELU)]
        if c.flags:
            variants = [("flags", c.flags)]
        for tag, fl in variants:
            r = launch(engine, c, o, pl, fl, cid, tag)
            compare(cid, tag, "y", r["y"], epilogue_ref(o, fl), bound)
        # the statistics ride in the plane kernels' epilogue, for a whole batch in one launch and without a ReLU
        r = launch(engine, c, o, pl, EPI_BIAS, cid, "stats", stats=True)
        ref = epilogue_ref(o, EPI_BIAS)
        compare(cid, "stats", "y", r["y"], ref, bound)
        want_tiles = cdiv(g.N * g.Ho * g.Wo, BM) if (o_m["fast"] and o_m["nsub"] == 1) else 0
        assert r["tiles"] == want_tiles, f"{cid}: tiles_out = {r['tiles']}, expected {want_tiles}"
        if want_tiles:
            st = r["stats"][:want_tiles * 2 * g.Cout].reshape(want_tiles, 2, g.Cout)
            assert_written(st, cid + " stats")
            flat = ref.reshape(-1, g.Cout)
            if k == CK_PATCH:      # the patch kernel's tiles are 8 x 16 pixel patches, in (image, patch row, patch column) order
                flat = ref.reshape(g.N, g.Ho // 8, 8, g.Wo // 16, 16, g.Cout).permute(0, 1, 3, 2, 4, 5).reshape(-1, g.Cout)
            sref = tile_stats_ref(flat)
            sabs = tile_stats_ref(flat.abs())[:, 0].max().item()       # the largest tile sum of |y| (the ragged tile with its own rows)
            compare(cid, "stats", "sum", st[:, 0], sref[:, 0], 2e-5, scale=sabs)
            compare(cid, "stats", "sqsum", st[:, 1], sref[:, 1], 1e-4)
        r = launch(engine, c, o, pl, EPI_RELU, cid, "relu+stats", stats=True)
        assert r["tiles"] == 0, f"{cid}: statistics promised behind a fused ReLU"
        compare(cid, "relu+stats", "y", r["y"], epilogue_ref(o, EPI_RELU), bound)
    else:
        fl = c.flags
        r = launch(engine, c, o, pl, fl, cid, "plain")
        compare(cid, "plain", "dx", r["y"], epilogue_ref(o, fl), bound)
        takes_res = o_m["with_res"]["kernel"] != 0

        def res_scale(flags):
            """conv_b16_kernel stages its output tile in LDS as bf16 and adds `res` to the STAGED values, rounding a second time
            ("the tile's bf16 values + res in fp32, rounded again", conv_b16.h) - the arithmetic of the unfused pair, a bf16 dx and a
            bf16 add.  Two roundings of at most 2^-8 each, the first relative to the value before `res`, the second to the result:
            |err| <= 2^-8 (max|ref before res| + max|ref|).  Measured against the single-rounding bound 2^-8 max|ref| the form reaches
            1.4 (K = 9216, 24 x 24).  Every other kernel adds `res` in fp32 before its one rounding and keeps the plain bound."""
            if o_m["with_res"]["kernel"] == CK_B16 and out_b16:
                return epilogue_ref(o, flags).abs().max().item() + epilogue_ref(o, flags, o["res"]).abs().max().item()
            return None

        if takes_res:
            r = launch(engine, c, o, pl, fl, cid, "res", res=o["res"])
            compare(cid, "res", "dx", r["y"], epilogue_ref(o, fl, o["res"]), bound, scale=res_scale(fl))
            r = launch(engine, c, o, pl, fl, cid, "res=dx", res=o["res"], inplace=True)
            compare(cid, "res=dx", "dx", r["y"], epilogue_ref(o, fl, o["res"]), bound, scale=res_scale(fl))
        else:
            launch(engine, c, o, pl, fl, cid, "res refused", res=o["res"], expect=SG_EUNSUPPORTED)
        if o_m["family"] != CF_THIN and not fl and c.dt != "head":      # Conv2DTranspose forward: bias (Cin entries) and ReLU
            r = launch(engine, c, o, pl, EPI_BIAS | EPI_RELU, cid, "bias+relu")
            compare(cid, "bias+relu", "dx", r["y"], epilogue_ref(o, EPI_BIAS | EPI_RELU), bound)
            if takes_res:
                r = launch(engine, c, o, pl, EPI_BIAS, cid, "bias+res", res=o["res"])
                compare(cid, "bias+res", "dx", r["y"], epilogue_ref(o, EPI_BIAS, o["res"]), bound, scale=res_scale(EPI_BIAS))
    for e in c.extra:
        EXTRAS[e](engine, c, o, o_m, pl, cid, bound)


# ---- further operands -----------------------------------------------------------------------------------------------------------
def _extra_pin(engine, c, o, o_m, pl, cid, bound):
    """The caller's activation planes (sg_split_planes) instead of the split in the launch: the same bits."""
    assert o_m["planes_in"] == 1, cid
    a = launch(engine, c, o, pl, 0, cid, "plain")
    b = launch(engine, c, o, pl, 0, cid, "pin", pin=True)
    compare(cid, "pin", "dx" if c.dgrad else "y", b["y"], epilogue_ref(o, 0), bound)
    assert torch.equal(a["y"], b["y"]), f"{cid}: the launch on the caller's planes differs from the launch that splits A itself"


def _bn_params(C, seed):
    gen = torch.Generator().manual_seed(seed)
    return rnd(gen, C) * 0.3, rnd(gen, C) * 0.5 + 1.5, rnd(gen, C) + 1.5, rnd(gen, C) * 0.3


def _extra_bn(engine, c, o, o_m, pl, cid, bound, infer=False):
    """BatchNormalization -> ReLU in the loader, training statistics (bninf: inference, `invstd` is the moving variance)."""
    from oracle import tfops as T
    assert o_m["bn_in"] == 1, cid
    g = c.g
    mean, inv, gam, bet = _bn_params(g.Cin, g.Cin + infer)
    second = inv if not infer else inv.abs() + 0.1            # a variance
    r = launch(engine, c, o, pl, EPI_BIAS, cid, "bninf" if infer else "bn", bn=(mean, second, gam, bet, 1, int(infer)))
    istd = second.double() if not infer else 1.0 / torch.sqrt(second.double() + 1e-3)
    xn = torch.relu(((o["x"].double() - mean.double()) * istd) * gam.double() + bet.double())
    with torch.no_grad():
        ref = T.conv2d(xn, o["w"].double(), o["bias"].double(), g.s, g.d, "same")
    compare(cid, "bninf" if infer else "bn", "y", r["y"], ref, bound)


def _extra_bnb(engine, c, o, o_m, pl, cid, bound, relu=False):
    """The BatchNormalization backward apply in the wide pointwise dgrad's A path, as
    tests/test_ops_gpu.py::test_batchnorm_backward_apply_in_the_pointwise_dgrad holds it: dz and dx have the BITS of the unfused pair
    (sg_bn_train_bwd's apply, then the plain launch of this case on that dz), and dz is within 2e-5 of float64 (dx too, here)."""
    from oracle import tfops as T
    assert o_m["bnb"] == 1, cid
    g = c.g
    rows = g.N * g.Ho * g.Wo
    gen = torch.Generator().manual_seed(g.Cout + relu)
    xb = rnd(gen, g.N, g.Ho, g.Wo, g.Cout)
    gam, bet = rnd(gen, g.Cout) + 1.5, rnd(gen, g.Cout) * 0.3
    # the unfused pair on the engine: the layer's statistics, its backward sums and apply, then the convolution's plain dgrad
    xd, gd, bd, dyd = xb.cuda(), gam.cuda(), bet.cuda(), o["dy"].cuda()
    z, mean, inv = engine.bn_train_fwd(xd, gd, bd, torch.zeros(g.Cout).cuda(), torch.ones(g.Cout).cuda(), relu=relu)
    dz_un, dgam, dbet = engine.bn_train_bwd(xd, z, dyd, gd, mean, inv, relu=relu, beta=bd)
    torch.cuda.synchronize()
    tag = "bnbrelu" if relu else "bnb"
    dx_un = launch(engine, c, dict(o, dy=dz_un.cpu()), pl, 0, cid, tag + " unfused")["y"]
    # float64
    x64 = xb.double().reshape(rows, g.Cout)
    m64, i64 = mean.cpu().double(), inv.cpu().double()
    xhat = (x64 - m64) * i64
    gg = o["dy"].double().reshape(rows, g.Cout)
    if relu:
        gg = gg * ((xhat * gam.double() + bet.double()) > 0)
    dz64 = gam.double() * i64 * ((gg - gg.sum(0) / rows) - xhat * (gg * xhat).sum(0) / rows)
    xz = torch.zeros(g.N, g.H, g.W, g.Cin, dtype=torch.float64, requires_grad=True)
    (dx64,) = torch.autograd.grad(T.conv2d(xz, o["w"].double(), None, 1, 1, "same"), xz, dz64.reshape(g.N, g.Ho, g.Wo, g.Cout))
    r = launch(engine, c, o, pl, 0, cid, tag,
               bnb=(xb.reshape(rows, g.Cout), mean.cpu(), inv.cpu(), gam, bet, dgam.cpu(), dbet.cpu(), relu))
    compare(cid, tag, "dz", r["dz"], dz64, 2e-5)
    compare(cid, tag, "dx", r["y"], dx64, 2e-5)
    assert torch.equal(r["dz"].reshape(-1), dz_un.cpu().reshape(-1)), f"{cid} {tag}: dz is not the bits of sg_bn_train_bwd's apply"
    assert torch.equal(r["y"], dx_un), f"{cid} {tag}: dx is not the bits of the unfused pair"


def _extra_up2(engine, c, o, o_m, pl, cid, bound):
    """UpSampling2D(2) -> Conv2D 3x3 in one launch (x is the source), as tests/test_ops_gpu.py::
    test_upsampling_fused_into_the_3x3_convolution states it: within the fp32 bound of float64 on the materialised tensor, within 1e-5
    of the unfused pair (the summed taps round differently: no bit equality promised), and no more than three times the unfused
    pair's own error from float64 (+ 5e-7)."""
    from oracle import tfops as T
    assert o_m["up2"] == 1, cid
    g = c.g
    gen = torch.Generator().manual_seed(11)
    src = rnd(gen, g.N, g.H // 2, g.W // 2, g.Cin)
    up = src.repeat_interleave(2, 1).repeat_interleave(2, 2).contiguous()
    with torch.no_grad():
        ref = T.conv2d(up.double(), o["w"].double(), o["bias"].double(), 1, 1, "same")
    y_un = launch(engine, c, dict(o, x=up), pl, EPI_BIAS, cid, "up2 unfused")["y"]
    r = launch(engine, c, dict(o, x_src=src), pl, EPI_BIAS, cid, "up2", up2=True)
    compare(cid, "up2", "y", r["y"], ref, bound)
    compare(cid, "up2", "y vs unfused", r["y"], y_un, 1e-5)
    e_f, e_u = (r["y"].double() - ref).abs().max().item(), (y_un.double() - ref).abs().max().item()
    assert e_f <= 3 * e_u + 5e-7, f"{cid} up2: sub-pixel form {e_f:.2e} from fp64, unfused pair {e_u:.2e}"


def _extra_down2(engine, c, o, o_m, pl, cid, bound):
    """The input gradient of the same pair: dx of the SOURCE = the 2 x 2 cell sums of the plain dgrad - within the fp32 bound of
    float64 and the BITS of the unfused pair (the plain launch, then sg_upsample_nearest_bwd: same products, same order of additions)."""
    assert o_m["up2"] == 1, cid
    g = c.g
    full = epilogue_ref(o, 0)
    ref = full.reshape(g.N, g.H // 2, 2, g.W // 2, 2, g.Cin).sum((2, 4))
    plain = launch(engine, c, o, pl, 0, cid, "plain")["y"]
    dx_un = engine.upsample_bwd(plain.cuda(), (g.N, g.H // 2, g.W // 2, g.Cin), 2)
    torch.cuda.synchronize()
    r = launch(engine, c, o, pl, 0, cid, "down2", down2=True)
    compare(cid, "down2", "dx", r["y"], ref, bound)
    assert torch.equal(r["y"], dx_un.cpu()), f"{cid} down2: not the bits of the unfused pair"


EXTRAS = dict(pin=_extra_pin, bn=_extra_bn, bninf=lambda *a: _extra_bn(*a, infer=True), bnb=_extra_bnb,
              bnbrelu=lambda *a: _extra_bnb(*a, relu=True), up2=_extra_up2, down2=_extra_down2)


def records_table():
    return "\n".join(f"REC {cid} {la} {q} rel={rel:.3e} bound={b:.3e}" for cid, la, q, rel, b in RECORDS)


def main(child):
    """A child process: the cases of `child` under the environment's switches, one line per case."""
    from building_detection_amd.ops import get_engine
    env = CHILD_ENVS[child]
    for k, v in env.items():
        assert os.environ.get(k) == v, f"{k} must be {v} in the environment of child {child}"
    engine = get_engine(0)
    global QUIET
    QUIET = True
    bad = 0
    for c in child_cases(child):
        t0 = time.time()
        try:
            run_case(engine, c)
            print(f"CASE ok {c.id} {time.time() - t0:.2f}s", flush=True)
        except Exception:
            bad += 1
            print(f"CASE FAIL {c.id}\n{traceback.format_exc()}", flush=True)
    print(records_table())
    print(f"DONE {child} failed={bad}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
