"""The cases of tests/test_wgrad_forms_gpu.py: the filter gradient (sg_conv2d_wgrad, sg_conv2d_wgrad_planes; plan_wgrad and
plan_wgrad_launch in csrc/conv_igemm.hip, the kernels in conv_native.hip, conv_thin.hip, conv_x6.h, conv_x6p.hip, conv_pw.h) through
the C ABI on tests/_guarded.py arenas, each launch against oracle.tfops.conv2d in float64 (autograd for dw, the pixel sum of dy for
dbias) on the operands as the kernel sees them.

A case states, at the end of its id, which kernel FORM its launch takes.  The name comes from the mirror below of plan_wgrad and
plan_wgrad_launch - thin_ok, wgrad_pw_wide_geom, x6wp_geom, x6p_up2_geom, wgrad_x6_geom / wgrad_x6_ok, wgrad_bn, the vec / fast /
planes / skip_slabs / tap_inner rules, the three share rules (wgrad_slab_split, wgrad_pw_wide_plan, x6wp_grid), the fallbacks'
S <= S0, images_per_2gib, the workspace layout - written from the comments and rules of the sources, never by calling the library.
Before a case launches, run_case() asserts that the mirror's name is the one in the id and that the engine's own plan
(sg_conv2d_wgrad_plan) says the same field by field, `main` and `tail`, on this device.

Form names:
    wgrad.thin.CO<1-4>.<f32|b16|b16>f32>
    wgrad.wide.<x6|b16>
    wgrad.patch.C<32|64>x<32|64>.<x6|npl1|b16>
    wgrad.slab.x6.BN<128|64|32>.<x6|npl1|b16>
    wgrad.planes.BN<128|64|32>
    wgrad.native.BN<128|64|32>.<scalar|vec|fast1|fast2>[.b16|.b16>f32]
then the modifiers .skip .tapin .S<n> .sub<nb>+<tail> .up2 .wv0 (x6: three bf16 planes per fp32 operand, six passes; npl1: fp32
storage in arithmetic mode 2, one plane; b16: bf16 storage; b16>f32: bf16 x with fp32 dy, the softmax head).

Run as a program (`python tests/_wgrad_cases.py CHILD` with CHILD_ENVS[CHILD] in the environment: the switches are read once per
process) it runs child_cases(CHILD) and prints one `CASE ok|FAIL ...` line per case, then its records."""
import ctypes as CT
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

from _conv_cases import Geom, cdiv, x6p_up2_geom
from _guarded import Guarded, assert_written, check_all, seg_plan, untouched, widen

REF_CUS = 256
F32, BF16, HEAD, UP2 = 0, 1, 0x100, 0x200
SG_EINVAL, SG_EWORKSPACE, SG_EUNSUPPORTED = -1, -2, -3
BM, BK = 128, 32
PW_BM, PW_BN = 128, 384
WG_THIN, WG_WIDE, WG_PATCH, WG_SLAB_X6, WG_SLAB_NATIVE, WG_HEAD32, WG_PLANES = range(1, 8)
BOUND = 2e-5     # tests/test_ops_gpu.py, tests/test_wgrad_plan_gpu.py: fp32 accumulation of exact products, of max|ref|
QUIET = False
FAULTED = []     # the first HIP error of this process (run_case): no case is launched after it
RECORDS = []     # (case id, launch, output, measured error / scale, bound): a record, written before anything is asserted


# ================================================================================================ switches
# The switches of csrc/sg_switch.h that this file's mirror knows; every other SG_* variable must be unset (run_case checks).
SWITCH_DEFAULTS = dict(SG_CONV_MAX_BYTES=0, SG_PW_WIDE=1, SG_WPW_VAR=1, SG_WGRAD_FAST1=0, SG_CONV_NOSKIP=0, SG_CONV_L2=None,
                       SG_X6_NOWPATCH=0, SG_CONV_NOTHIN=0)
_FLAGS = ("SG_WGRAD_FAST1", "SG_CONV_NOSKIP", "SG_X6_NOWPATCH", "SG_CONV_NOTHIN")      # on when the variable exists, whatever its value


def _atoll(v):
    try:
        return int(v.strip())
    except ValueError:
        return 0


def switches_of(env):
    sw = dict(SWITCH_DEFAULTS)
    for k in sw:
        if k in env:
            sw[k] = 1 if k in _FLAGS else _atoll(env[k])
    return sw


SW = switches_of(os.environ)
CHILD_ENVS = {
    "sub": {"SG_CONV_MAX_BYTES": str(1 << 20), "SG_PW_WIDE": "2"},
    "pw2": {"SG_PW_WIDE": "2"},
    "ab": {"SG_WPW_VAR": "0", "SG_WGRAD_FAST1": "1", "SG_CONV_NOSKIP": "1", "SG_X6_NOWPATCH": "1", "SG_CONV_NOTHIN": "1", "SG_CONV_L2": "0"},
}


class switched:
    """The mirror as a process with `env` sees it (the parent lists a child's cases and names)."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = dict(SW)
        SW.update(switches_of(self.env))

    def __exit__(self, *a):
        SW.update(self.old)


def foreign_switches(env):
    return sorted(k for k in env if k.startswith("SG_") and k not in SWITCH_DEFAULTS)


# ================================================================================================ mirror of the plan
def thin_ok(g):
    return (not SW["SG_CONV_NOTHIN"] and g.k == 1 and g.s == 1 and g.Cout <= 4 and g.Ho == g.H and g.Wo == g.W and g.Cin % 4 == 0
            and g.xl % 4 == 0 and g.Cin >= 16)


def x6wp_geom(g):
    """The patch filter gradient: 3x3, stride 1, dilation 1, SAME, Cin and Cout in {32, 64}, H % 4 == 0, W % 16 == 0."""
    return (not SW["SG_X6_NOWPATCH"] and g.k == 3 and g.s == 1 and g.d == 1 and g.pt == 1 and g.pl == 1 and g.Ho == g.H and g.Wo == g.W
            and g.Cin in (32, 64) and g.Cout in (32, 64) and g.H % 4 == 0 and g.W % 16 == 0)


def x6wp_grid(cus, g):
    """Workgroups = partial slabs of the patch kernel: two per CU, fewer when there are fewer 4 x 16 tiles."""
    return min(g.N * (g.H // 4) * (g.W // 16), 2 * cus)


def wgrad_bn(cout):
    return 128 if cout > 64 else (64 if cout > 32 else 32)


def wgrad_x6_geom(g):
    """wgrad_x6_kernel: stride 1 SAME, or stride 2 with dilation 1 and the output the input subsampled; Wo % 32 == 0, Cout >= 16."""
    geom = (g.s == 1 and g.Ho == g.H and g.Wo == g.W) or (g.s == 2 and g.d == 1 and g.Ho == (g.H + 1) // 2 and g.Wo == (g.W + 1) // 2)
    return geom and g.Wo % BK == 0 and g.Cout >= 16


def wgrad_x6_ok(g, vec, force, mode, xb, yb):
    sh = (g.pt * g.W + g.pl + 64 * g.s) * g.xl * 4
    return bool((force or mode != 0) and vec and wgrad_x6_geom(g) and xb != 0 and yb != 0 and xb + 2 * sh < (1 << 31))


def wgrad_pw_wide_geom(g, eb):
    """The wide pointwise filter gradient: 1x1, stride 1, no padding, 16-byte channel runs; SG_PW_WIDE=2: every such layer; else
    >= 6144 pixels, Cin >= 256, the last 128-row and 384-column tiles at least 3/4 full."""
    on = SW["SG_PW_WIDE"]
    if not on or g.k != 1 or g.s != 1 or g.pt != 0 or g.pl != 0:
        return False
    ch = 8 if eb == 2 else 4
    if g.xl % ch or g.yl % ch or g.Cin % ch or g.Cout % ch:
        return False
    if on == 2:
        return True
    if g.N * g.Ho * g.Wo < 6144 or g.Cin < 256:
        return False
    return g.Cout / (cdiv(g.Cout, PW_BN) * PW_BN) >= 0.75 and g.Cin / (cdiv(g.Cin, PW_BM) * PW_BM) >= 0.75


def wgrad_pw_wide_plan(cus, g, kp):
    """(S, k-steps per share): tiles x S fills the CUs once, at least 8 k-steps of kp pixels per share."""
    tiles = cdiv(g.Cin, PW_BM) * cdiv(g.Cout, PW_BN)
    nks = cdiv(g.N * g.Ho * g.Wo, kp)
    s = max(cus // tiles, 1)
    if s > nks // 8:
        s = nks // 8 if nks // 8 > 0 else 1
    steps = cdiv(nks, s)
    return cdiv(nks, steps), steps


def wgrad_slab_split(cus, g, b16):
    """Shares of the slab kernels' pixel reduction: modelled time = padded MFMA work / (fraction of the 2 x CUs slots busy over whole
    waves x rate) + the traffic of S partial slabs at 3 TB/s both ways + 3 us; the first S that beats the best so far by 0.1 % wins;
    at least 8 slabs per share, at most 512 shares, partial slabs at most 384 MiB.  Same double arithmetic as the source."""
    K, P = g.k * g.k * g.Cin, g.N * g.Ho * g.Wo
    bn = wgrad_bn(g.Cout)
    tiles = cdiv(K, BM) * cdiv(g.Cout, bn)
    nslab = cdiv(P, BK)
    slots = 2 * cus
    flops = 2.0 * float(tiles) * BM * bn * float(P)
    x6_rate = (wgrad_x6_geom(g) or (g.s == 2 and g.d == 1 and g.Wo % BK == 0 and g.Cout >= 16)) and g.Cin % 4 == 0
    rate = 110.0 * 1e12 if x6_rate else 110e12      # (SG_WGRAD_PLAN_RATE and _B16 default to 110: the three rates coincide; b16 unused)
    maxS = min(max(nslab // 8, 1), 512)
    best_t, best_S = 1e300, 1
    for S in range(1, maxS + 1):
        wgs = tiles * S
        eff = float(wgs) / float(cdiv(wgs, slots) * slots)
        part_bytes = float(S) * float(K) * g.Cout * 4.0 if S > 1 else 0.0
        if part_bytes > float(384 << 20):
            break
        t = flops / (eff * rate) + 2.0 * part_bytes / 3.0e12 + (3e-6 if S > 1 else 0.0)
        if t < best_t * 0.999:
            best_t, best_S = t, S
    return best_S


def images_per_2gib(g):
    """Images per launch such that both activation tensors stay under the limit, counted at 4 bytes per element for either storage."""
    per = max(g.H * g.W * g.xl * 4, g.Ho * g.Wo * g.yl * 4)
    lim = SW["SG_CONV_MAX_BYTES"] if SW["SG_CONV_MAX_BYTES"] > 0 else (1 << 31) - (1 << 20)
    if per * g.N < lim:
        return g.N
    return max(lim // per, 0)


def conv_l2(x6):
    if SW["SG_CONV_L2"] is not None:
        return SW["SG_CONV_L2"] & 7
    return 7 if x6 else 2


def extents(dt, g):
    """WgradParams' x_bytes / dy_bytes: 0 = beyond the 2 GiB of a buffer descriptor."""
    b16, head, up = (dt & 0xff) == BF16, bool(dt & HEAD), 1 if dt & UP2 else 0
    eb = 2 if b16 else 4
    eby = 4 if head else eb
    xb = ((g.N * (g.H >> up) * (g.W >> up) - 1) * g.xl + g.Cin) * eb
    yb = ((g.N * g.Ho * g.Wo - 1) * g.yl + g.Cout) * eby
    return (xb if xb < (1 << 31) else 0), (yb if yb < (1 << 31) else 0)


LAUNCH0 = dict(family=0, bn=0, vec=0, fast=0, planes=0, skip_slabs=0, tap_inner=0, stagger=0, S=0, steps=0, step_px=0)


def launch_mirror(cus, mode, dt, gm, n, ax, ay):
    """plan_wgrad_launch: `n` images of `gm`, the geometry of the whole batch or of a full sub-batch."""
    f = dict(LAUNCH0)
    b16, head = (dt & 0xff) == BF16, bool(dt & HEAD)
    g = gm.with_n(n)
    taps = g.k * g.k
    P = n * g.Ho * g.Wo
    nslab = cdiv(P, BK)
    thin = thin_ok(gm)
    if thin and ax == 16:
        f.update(family=WG_THIN, S=1)
        return f
    xb, yb = extents(dt, g)
    a16 = ax == 16 and ay == 16
    dma = a16 and xb != 0 and yb != 0 and not head
    wide = not thin and (b16 or mode == 1) and wgrad_pw_wide_geom(gm, 2 if b16 else 4)
    ch = 8 if b16 else 4
    patch = not thin and not wide and x6wp_geom(gm) and (b16 or mode != 0) and g.xl % ch == 0 and g.yl % ch == 0
    npl = 1 if (b16 or mode == 2) else 3
    if thin:
        S0 = 1
    elif wide:
        kp = 32 if b16 else 16
        S0, _ = wgrad_pw_wide_plan(cus, gm, kp)
        if dma:
            S, steps = wgrad_pw_wide_plan(cus, g, kp)
            if S > S0:      # never more partial slabs than a full sub-batch
                steps = cdiv(cdiv(P, kp), S0)
                S = cdiv(cdiv(P, kp), steps)
            f.update(family=WG_WIDE, planes=npl, step_px=kp, S=S, steps=steps)
            return f
    elif patch:
        S0 = x6wp_grid(cus, gm)
        if dma:
            S = x6wp_grid(cus, g)
            f.update(family=WG_PATCH, planes=npl, S=S, step_px=BK, steps=cdiv(nslab, S))
            return f
    else:
        S0 = wgrad_slab_split(cus, gm, b16)
    ns = nslab if (thin or wide or patch) else cdiv(gm.N * g.Ho * g.Wo, BK)
    f["steps"] = cdiv(ns, S0)
    f["S"] = cdiv(ns, f["steps"])
    f["step_px"] = BK
    f["bn"] = wgrad_bn(g.Cout)
    g4 = g.Cin % 4 == 0 and g.xl % 4 == 0 and g.Cout % 4 == 0 and g.yl % 4 == 0
    g8 = g.Cin % 8 == 0 and g.xl % 8 == 0 and g.Cout % 8 == 0 and g.yl % 8 == 0
    if head:
        f.update(family=WG_HEAD32, vec=4 if (g4 and ax >= 8 and ay == 16) else 0)
        return f
    vec = (g8 if b16 else g4) and a16
    skip = int(not SW["SG_CONV_NOSKIP"] and g.d > 1 and taps > 1)
    if wgrad_x6_ok(g, vec, b16, mode, xb, yb):
        f.update(family=WG_SLAB_X6, vec=8 if b16 else 4, planes=npl, skip_slabs=skip,
                 tap_inner=int(bool(conv_l2(True) & 4) and taps > 1 and g.Cin % BM == 0), stagger=0)
        return f
    f["family"] = WG_SLAB_NATIVE
    if b16:
        f["vec"] = 4 if (g4 and ax >= 8 and ay >= 8) else 0
        return f
    f.update(vec=4 if vec else 0, skip_slabs=skip, tap_inner=int(bool(conv_l2(False) & 4) and taps > 1 and g.Cin % BM == 0), stagger=1)
    if vec and g.s == 1 and g.Ho == g.H and g.Wo == g.W and xb != 0 and yb != 0:
        two = (not SW["SG_WGRAD_FAST1"] and g.Wo % BK == 0 and (taps == 1 or g.Cin % BM == 0) and xb + 2 * 32 * g.xl * 4 < (1 << 31))
        f["fast"] = 2 if two else 1
    return f


PLAN0 = dict(chunks=0, nb=0, tail_n=0, max_parts=0, bn_in=0, up2=0, dw_part_bytes=0, bias_part_bytes=0, bias_off=0, ws_bytes=0)


def fwd_bn_in(mode, dt, g):
    """plan_conv(...).bn_in of the layer's forward, for the two families whose filter gradient can take the operand: thin (fp32,
    dense x) and the patch forward (fp32 in arithmetic mode 1, H % 8 == 0, W % 16 == 0, dense x)."""
    if dt != F32 or g.xgap:
        return 0
    if thin_ok(g):
        return 1
    from _conv_cases import plan_conv_mode
    return int(plan_conv_mode(mode, dt, g, False, 0)["bn_in"])


def plan_mirror(cus, mode, dt, g, ax=16, ay=16, planes=False):
    """plan_wgrad as a dict (main / tail: launch dicts); family 0 everywhere: the planes-in call does not cover the layer."""
    none = dict(PLAN0, main=dict(LAUNCH0), tail=dict(LAUNCH0))
    K, P = g.k * g.k * g.Cin, g.N * g.Ho * g.Wo
    if planes:
        if mode != 1 or g.s != 1 or g.Ho != g.H or g.Wo != g.W or g.Wo % 32 or g.Cin % 8 or g.Cout % 8 or g.Cout < 16 or g.xgap or g.ygap:
            return none
        xp, yp = g.N * g.H * g.W * g.Cin * 2, P * g.Cout * 2
        sh = (g.pt * g.W + g.pl + 64) * g.Cin * 4
        if 3 * xp + 2 * sh >= (1 << 31) or 3 * yp >= (1 << 31):
            return none
        dt, ax, ay = F32, 16, 16
    nb = images_per_2gib(g)
    chunked = 1 <= nb < g.N and not thin_ok(g)
    o = dict(PLAN0)
    o["nb"] = nb if chunked else g.N
    o["chunks"] = cdiv(g.N, nb) if chunked else 1
    o["tail_n"] = g.N - (o["chunks"] - 1) * o["nb"]
    gm = g.with_n(o["nb"])
    o["main"] = launch_mirror(cus, mode, dt, gm, o["nb"], ax, ay)
    o["tail"] = dict(o["main"]) if o["tail_n"] == o["nb"] else launch_mirror(cus, mode, dt, gm, o["tail_n"], ax, ay)
    if planes:
        if o["main"]["family"] != WG_SLAB_X6 or o["chunks"] > 1:
            return none
        o["main"].update(family=WG_PLANES, vec=8, stagger=0)
        o["tail"] = dict(o["main"])
    m = o["main"]
    o["max_parts"] = (o["chunks"] - 1) * m["S"] + o["tail"]["S"]
    if o["chunks"] > 1:
        o["dw_part_bytes"] = o["chunks"] * m["S"] * K * g.Cout * 4
    elif m["family"] == WG_THIN:
        o["dw_part_bytes"] = seg_plan(cus, g.N * g.H * g.W, g.Cin, True, nout=min(g.Cout, 4))["part_bytes"]
    else:
        o["dw_part_bytes"] = m["S"] * K * g.Cout * 4 if m["S"] > 1 else 0
    o["bias_part_bytes"] = 0 if planes else max(seg_plan(cus, P, g.Cout, True)["part_bytes"], seg_plan(cus, P, g.Cout, False)["part_bytes"])
    o["bias_off"] = (o["dw_part_bytes"] + 255) & ~255
    o["ws_bytes"] = o["dw_part_bytes"] + o["bias_part_bytes"] + 512
    f32 = (dt & 0xff) == F32 and not dt & HEAD
    o["bn_in"] = int(m["family"] in (WG_THIN, WG_PATCH) and f32 and not dt & UP2 and not g.xgap and fwd_bn_in(mode, dt & 0xff, g))
    o["up2"] = int(m["family"] == WG_PATCH and not dt & HEAD and x6p_up2_geom(g))
    return o


def form_name(o, la, dt, g):
    """The name of launch `la` (a dict) of plan `o` (a dict): see the module docstring."""
    b16, head = (dt & 0xff) == BF16, bool(dt & HEAD)
    st = "b16>f32" if head else ("b16" if b16 else "f32")
    pipe = "b16" if b16 else ("npl1" if la["planes"] == 1 else "x6")
    fam = la["family"]
    if fam == WG_THIN:
        n = f"wgrad.thin.CO{g.Cout}.{st}"
    elif fam == WG_WIDE:
        n = f"wgrad.wide.{pipe}"
    elif fam == WG_PATCH:
        n = f"wgrad.patch.C{g.Cin}x{g.Cout}.{pipe}"
    elif fam == WG_SLAB_X6:
        n = f"wgrad.slab.x6.BN{la['bn']}.{pipe}"
    elif fam == WG_PLANES:
        n = f"wgrad.planes.BN{la['bn']}"
    elif fam in (WG_SLAB_NATIVE, WG_HEAD32):
        kind = {2: "fast2", 1: "fast1"}.get(la["fast"], "vec" if la["vec"] else "scalar")
        n = f"wgrad.native.BN{la['bn']}.{kind}" + ("" if st == "f32" else "." + st)
    else:
        return "wgrad.none"
    if la["skip_slabs"]:
        n += ".skip"
    if la["tap_inner"]:
        n += ".tapin"
    if la["S"] > 1:
        n += f".S{la['S']}"
    if o["chunks"] > 1:
        n += f".sub{o['nb']}+{o['tail_n']}"
    if dt & UP2 and o["up2"]:
        n += ".up2"
    if fam == WG_WIDE and not b16 and SW["SG_WPW_VAR"] != 1:
        n += ".wv0"
    return n


# ================================================================================================ the case tables
def align_class(off):
    return 16 if off % 16 == 0 else (8 if off % 8 == 0 else 0)


class WCase:
    """dt: "f32" | "b16" | "head"; mode: the arithmetic on fp32 storage (sg_set_conv_x6); xoff / yoff: bytes that x / dy sit behind a
    16-byte boundary; bn: BatchNormalization -> ReLU in the loader; up2: x is the source of a 2x nearest up-sampling (SG_X_UP2); pin:
    also the planes-in call, its bits against this launch; name: the form the launch takes at 256 CUs."""

    def __init__(self, name, g, dt="f32", mode=1, xoff=0, yoff=0, bn=False, up2=False, pin=None):
        self.name, self.g, self.dt, self.mode, self.xoff, self.yoff, self.bn, self.up2, self.pin = name, g, dt, mode, xoff, yoff, bn, up2, pin

    def copy(self):
        return WCase(self.name, self.g, self.dt, self.mode, self.xoff, self.yoff, self.bn, self.up2, self.pin)

    @property
    def dtype(self):
        return {"f32": F32, "b16": BF16, "head": BF16 | HEAD}[self.dt] | (UP2 if self.up2 else 0)

    @property
    def id(self):
        t = f"{self.g.tag}-{self.dt}" + (f"-m{self.mode}" if self.mode != 1 else "")
        t += (f"-x+{self.xoff}" if self.xoff else "") + (f"-y+{self.yoff}" if self.yoff else "")
        t += ("-bn" if self.bn else "") + ("-up2" if self.up2 else "") + ("-pin" if self.pin else "")
        return f"{t}-{self.name}"

    def mirror(self, cus=REF_CUS):
        return plan_mirror(cus, self.mode, self.dtype, self.g, align_class(self.xoff), align_class(self.yoff))

    def mirror_name(self, cus=REF_CUS):
        o = self.mirror(cus)
        return form_name(o, o["main"], self.dtype, self.g)

    def mirror_pin_name(self, cus=REF_CUS):
        o = plan_mirror(cus, self.mode, F32, self.g, planes=True)
        return form_name(o, o["main"], F32, self.g) if o["main"]["family"] else None


G, W = Geom, WCase

CASES = [
    # ---- wgrad_x6_kernel (stride 1 SAME or stride 2, Wo % 32 == 0, Cout >= 16): tile widths, ragged tiles, strides, shares
    W("wgrad.slab.x6.BN32.x6", G(1, 8, 32, 4, 16)),                             # K = 36: one row tile holds all nine taps
    W("wgrad.slab.x6.BN64.x6", G(1, 8, 32, 48, 48)),                            # K = 432: the ragged last row tile spans taps
    W("wgrad.slab.x6.BN32.b16", G(1, 8, 32, 48, 24), dt="b16"),                 # Cout = 24: threads past the 24 columns of a 32-wide tile
    W("wgrad.slab.x6.BN32.npl1", G(1, 8, 32, 48, 24), mode=2),
    W("wgrad.slab.x6.BN64.npl1", G(1, 8, 32, 48, 48), mode=2),
    W("wgrad.slab.x6.BN64.b16", G(1, 8, 32, 48, 48), dt="b16"),
    W("wgrad.slab.x6.BN128.x6", G(1, 8, 32, 48, 136)),                          # second column tile 8 wide
    W("wgrad.slab.x6.BN128.npl1", G(1, 8, 32, 48, 136), mode=2),
    W("wgrad.slab.x6.BN128.b16", G(1, 8, 32, 48, 136), dt="b16"),
    W("wgrad.slab.x6.BN128.x6.S8", G(2, 64, 64, 64, 128, s=2)),                 # stride 2, W = 64: pad_l = 0
    W("wgrad.slab.x6.BN64.x6.S4", G(1, 63, 63, 32, 48, s=2)),                      # stride 2, odd extent: pad_l = 1
    W("wgrad.slab.x6.BN64.b16.S4", G(1, 63, 63, 32, 48, s=2), dt="b16"),
    W("wgrad.slab.x6.BN64.x6", G(1, 16, 64, 64, 64, k=1, s=2)),                 # 1x1 stride 2
    W("wgrad.slab.x6.BN64.x6.S7", G(3, 20, 32, 64, 64, k=1)),                   # a share crosses an image boundary; the last is short
    W("wgrad.slab.x6.BN64.b16.S7", G(3, 20, 32, 64, 64, k=1), dt="b16"),
    W("wgrad.slab.x6.BN128.x6.tapin", G(1, 8, 32, 256, 136)),                   # tap-inner order with two column tiles
    W("wgrad.slab.x6.BN128.b16.tapin", G(1, 8, 32, 256, 136), dt="b16"),
    W("wgrad.slab.x6.BN128.x6.skip.tapin.S8", G(2, 32, 32, 256, 256, d=6), pin="wgrad.planes.BN128.skip.tapin.S8"),
    # ---- padding-slab elimination: dilation >= H (row tiles with no live slab write zeros), dilation >= W (only the column test)
    W("wgrad.slab.x6.BN64.x6.skip.S2", G(1, 16, 32, 32, 48, d=18)),
    W("wgrad.slab.x6.BN64.npl1.skip.S2", G(1, 16, 32, 32, 48, d=18), mode=2),
    W("wgrad.slab.x6.BN64.b16.skip.S2", G(1, 16, 32, 32, 48, d=18), dt="b16"),
    W("wgrad.slab.x6.BN64.x6.skip.S8", G(1, 64, 32, 32, 48, d=36)),
    W("wgrad.slab.x6.BN128.x6.skip.S8", G(1, 64, 32, 48, 80, d=3), pin="wgrad.planes.BN128.skip.S8"),
    # ---- pixel-stride gaps
    W("wgrad.slab.x6.BN64.x6", G(1, 8, 32, 48, 48, xgap=4, ygap=8)),
    W("wgrad.slab.x6.BN64.b16", G(1, 8, 32, 48, 48, xgap=8, ygap=16), dt="b16"),
    W("wgrad.native.BN32.vec", G(2, 17, 19, 8, 32, s=2, xgap=4, ygap=4)),
    W("wgrad.native.BN128.fast1", G(3, 2, 24, 8, 72, xgap=8, ygap=4)),
    W("wgrad.native.BN32.fast2", G(1, 8, 32, 40, 8, k=1, xgap=8, ygap=4)),
    W("wgrad.native.BN32.vec.b16", G(2, 12, 20, 12, 12, xgap=4, ygap=8), dt="b16"),
    # ---- planes-in: the three tile widths, the bits of the fp32-operand launch
    W("wgrad.slab.x6.BN32.x6", G(1, 8, 32, 48, 24), pin="wgrad.planes.BN32"),
    W("wgrad.slab.x6.BN64.x6", G(1, 8, 32, 40, 56), pin="wgrad.planes.BN64"),
    W("wgrad.slab.x6.BN128.x6", G(1, 8, 32, 48, 72), pin="wgrad.planes.BN128"),
    # ---- igemm_wgrad_kernel, fp32: fast2 (arithmetic mode 0, or fewer than 16 output channels), fast1, vec, scalar; three widths each
    W("wgrad.native.BN32.fast2", G(1, 8, 32, 40, 8, k=1)),                      # Cout < 16 in any mode
    W("wgrad.native.BN64.fast2", G(1, 8, 32, 40, 48, k=1), mode=0),
    W("wgrad.native.BN128.fast2", G(1, 8, 32, 128, 72), mode=0),
    W("wgrad.native.BN128.fast2.skip", G(1, 8, 32, 128, 72, d=2), mode=0),
    W("wgrad.native.BN64.fast2.S7", G(3, 20, 32, 64, 64, k=1), mode=0),
    W("wgrad.native.BN32.fast1.skip", G(3, 2, 24, 8, 32, d=2)),                 # Wo = 24, H = 2: (oh, ow) recomputed per visited slab
    W("wgrad.native.BN64.fast1", G(3, 2, 10, 8, 48)),                           # Wo = 10: oh wraps several times per slab step
    W("wgrad.native.BN64.fast1.skip", G(3, 2, 10, 8, 48, d=2)),
    W("wgrad.native.BN128.fast1", G(3, 2, 24, 8, 72)),
    W("wgrad.native.BN64.fast1", G(1, 8, 32, 40, 48), mode=0),                  # multi-tap with Cin % 128 != 0: a tile spans taps
    W("wgrad.native.BN32.vec", G(2, 17, 19, 8, 32, s=2)),
    W("wgrad.native.BN64.vec", G(2, 17, 19, 64, 64, s=2)),
    W("wgrad.native.BN128.vec", G(2, 17, 19, 8, 72, s=2)),
    W("wgrad.native.BN32.scalar", G(2, 24, 20, 3, 32, s=2)),
    W("wgrad.native.BN64.scalar", G(1, 8, 32, 48, 48), xoff=4),                 # x 4 bytes off
    W("wgrad.native.BN128.scalar", G(1, 8, 32, 48, 136), yoff=4),               # dy 4 bytes off
    W("wgrad.native.BN64.scalar", G(1, 8, 32, 48, 48), xoff=8, yoff=8),         # class 8 is no 16-byte run of fp32
    W("wgrad.native.BN32.scalar.S2", G(2, 16, 20, 3, 5)),                       # K * Cout % 4 != 0: the scalar reduce of the shares
    # ---- ... bf16 storage and the softmax head
    W("wgrad.native.BN32.vec.b16", G(2, 12, 20, 12, 12), dt="b16", xoff=8, yoff=8),      # alignment class 8
    W("wgrad.native.BN64.vec.b16", G(2, 12, 20, 12, 36), dt="b16", xoff=8, yoff=8),
    W("wgrad.native.BN128.vec.b16", G(2, 12, 20, 12, 68), dt="b16"),
    W("wgrad.native.BN32.scalar.b16", G(2, 12, 20, 12, 12), dt="b16", xoff=2),
    W("wgrad.native.BN64.scalar.b16", G(1, 8, 32, 48, 48), dt="b16", yoff=2),
    W("wgrad.native.BN128.scalar.b16", G(2, 12, 20, 6, 66), dt="b16"),
    W("wgrad.native.BN32.vec.b16>f32", G(2, 12, 12, 64, 4), dt="head", xoff=8),          # x class 8, dy class 16
    W("wgrad.native.BN32.scalar.b16>f32", G(2, 12, 12, 64, 2), dt="head"),
    W("wgrad.native.BN32.vec.b16>f32.S4", G(2, 24, 24, 64, 4), dt="head"),               # more than one share
    # ---- wgrad_pw_wide_kernel / _b16_kernel at the defaults: the smallest admitted shape, and two images
    W("wgrad.wide.x6.S48", G(1, 96, 64, 256, 384, k=1)),
    W("wgrad.wide.b16.S24", G(1, 96, 64, 256, 384, k=1), dt="b16"),
    W("wgrad.wide.x6.S48", G(2, 48, 64, 256, 384, k=1)),
    W("wgrad.native.BN128.scalar.S48", G(1, 96, 64, 256, 384, k=1), xoff=4),    # the slab fallback within the wide plan's shares
    # ---- the patch kernel: four channel pairs x three arithmetic forms; one tile, more tiles than slots, up2, BatchNormalization, gaps
    W("wgrad.patch.C32x32.x6.S30", G(2, 20, 48, 32, 32)),
    W("wgrad.patch.C32x64.x6", G(1, 4, 16, 32, 64)),                            # one tile: all four borders in one patch
    W("wgrad.patch.C64x32.x6.S8", G(1, 16, 32, 64, 32)),
    W("wgrad.patch.C64x64.x6.S512", G(3, 96, 128, 64, 64)),                     # 576 tiles > 512 slots
    W("wgrad.patch.C32x32.npl1.S30", G(2, 20, 48, 32, 32), mode=2),
    W("wgrad.patch.C32x64.npl1", G(1, 4, 16, 32, 64), mode=2),
    W("wgrad.patch.C64x32.npl1.S8", G(1, 16, 32, 64, 32), mode=2),
    W("wgrad.patch.C64x64.npl1.S6", G(1, 12, 32, 64, 64), mode=2),
    W("wgrad.patch.C32x32.b16.S30", G(2, 20, 48, 32, 32), dt="b16"),
    W("wgrad.patch.C32x64.b16", G(1, 4, 16, 32, 64), dt="b16"),
    W("wgrad.patch.C64x32.b16.S8", G(1, 16, 32, 64, 32), dt="b16"),
    W("wgrad.patch.C64x64.b16.S6", G(1, 12, 32, 64, 64), dt="b16"),
    W("wgrad.patch.C64x32.x6.S8.up2", G(1, 16, 32, 64, 32), up2=True),
    W("wgrad.patch.C32x32.x6.S36", G(2, 24, 48, 32, 32), bn=True),              # H % 8 == 0: the forward is a patch launch too
    W("wgrad.patch.C32x32.x6.S30", G(2, 20, 48, 32, 32, xgap=4, ygap=8)),
    W("wgrad.native.BN32.scalar.S30", G(2, 20, 48, 32, 32), xoff=4),            # 60 slabs in the patch plan's 30 shares
    # ---- the thin kernels: Cout 1-4 x three storage forms; 63 pixels; more than one reduction part; BatchNormalization; a gap
    W("wgrad.thin.CO1.f32", G(1, 3, 21, 64, 1, k=1)),
    W("wgrad.thin.CO2.f32", G(2, 9, 7, 48, 2, k=1), bn=True),
    W("wgrad.thin.CO3.f32", G(1, 5, 7, 20, 3, k=1)),
    W("wgrad.thin.CO4.f32", G(2, 72, 64, 48, 4, k=1)),                          # 9216 pixels: more than one reduction part
    W("wgrad.thin.CO1.b16", G(1, 3, 21, 64, 1, k=1), dt="b16"),
    W("wgrad.thin.CO2.b16", G(2, 72, 64, 48, 2, k=1), dt="b16"),
    W("wgrad.thin.CO3.b16", G(1, 5, 7, 24, 3, k=1), dt="b16"),
    W("wgrad.thin.CO4.b16", G(2, 9, 7, 48, 4, k=1), dt="b16"),
    W("wgrad.thin.CO1.b16>f32", G(1, 3, 21, 64, 1, k=1), dt="head"),
    W("wgrad.thin.CO2.b16>f32", G(2, 72, 64, 48, 2, k=1), dt="head"),
    W("wgrad.thin.CO3.b16>f32", G(1, 5, 7, 24, 3, k=1), dt="head"),
    W("wgrad.thin.CO4.b16>f32", G(2, 9, 7, 48, 4, k=1), dt="head"),
    W("wgrad.thin.CO2.f32", G(2, 9, 7, 32, 2, k=1, xgap=32, ygap=2)),
    W("wgrad.thin.CO2.f32", G(2, 9, 7, 48, 2, k=1), yoff=4),                    # dy off its boundary: read by scalar loads, still thin
    W("wgrad.thin.CO3.b16", G(1, 5, 7, 24, 3, k=1), dt="b16", yoff=2),
    W("wgrad.native.BN32.scalar", G(2, 9, 7, 48, 2, k=1), xoff=4),              # 126 pixels = 4 slabs, straight into dw
]

# SG_PW_WIDE=2: every aligned 1x1 stride-1 layer is a wide launch - pixel tails, shares of 1-4 k-steps, ragged tiles
PW2_CASES = [
    W("wgrad.wide.x6", G(1, 5, 10, 36, 388, k=1)),                              # 50 pixels: 4 k-steps of 16, the last of 2 pixels
    W("wgrad.wide.b16", G(1, 5, 10, 40, 392, k=1), dt="b16"),                   # 2 k-steps of 32, the last of 18 pixels
    W("wgrad.wide.x6", G(1, 1, 16, 36, 388, k=1)),                              # one k-step
    W("wgrad.wide.x6", G(1, 3, 11, 36, 388, k=1)),                              # 33 pixels: 3 k-steps
    W("wgrad.wide.x6", G(1, 2, 16, 136, 36, k=1)),                              # 2 k-steps; the second 128-row tile 8 rows
    W("wgrad.wide.b16", G(1, 2, 16, 136, 40, k=1), dt="b16"),                   # one k-step
    W("wgrad.wide.x6", G(1, 5, 10, 36, 388, k=1, xgap=4, ygap=8)),              # pixel strides above the channel counts
    W("wgrad.wide.b16", G(1, 5, 10, 40, 392, k=1, xgap=8, ygap=16), dt="b16"),
    W("wgrad.wide.x6.S2", G(2, 10, 13, 36, 388, k=1)),                          # 260 pixels: 17 k-steps in shares of 9 and 8
    W("wgrad.wide.b16.S2", G(2, 16, 17, 40, 392, k=1), dt="b16"),               # 544 pixels: 17 k-steps of 32
    W("wgrad.native.BN128.scalar", G(1, 5, 10, 36, 388, k=1), xoff=4),          # the slab fallback within the wide plan's one share
    W("wgrad.native.BN128.scalar.b16", G(1, 5, 10, 40, 392, k=1), dt="b16", xoff=2),
]

# SG_CONV_MAX_BYTES = 1 MiB (and SG_PW_WIDE=2): three images of 384 KiB go as sub-batches of two and one
SUB_CASES = [
    W("wgrad.slab.x6.BN64.x6.S8.sub2+1", G(3, 32, 32, 96, 64)),
    W("wgrad.slab.x6.BN64.b16.S8.sub2+1", G(3, 32, 32, 96, 64), dt="b16"),
    W("wgrad.patch.C64x64.x6.S64.sub2+1", G(3, 32, 64, 64, 64)),
    W("wgrad.wide.x6.S16.sub2+1", G(3, 32, 32, 96, 64, k=1)),
    W("wgrad.native.BN64.vec.S6.sub2+1", G(3, 64, 48, 32, 48, s=2)),
    # 89 images of 23040 bytes: 45 + 44; the last sub-batch wants 11 shares and is cut back to the 10 of a full one
    W("wgrad.wide.x6.S10.sub45+44", G(89, 4, 8, 180, 36, k=1)),
]


def renamed(cases):
    """Copies of `cases` under the names the mirror gives them now (inside `with switched(...)`)."""
    out = []
    for c in cases:
        n = c.copy()
        n.name = n.mirror_name()
        if n.pin:
            n.pin = n.mirror_pin_name()
        out.append(n)
    return out


def child_cases(child):
    """The cases a child process runs, with the names its mirror gives them (`with switched(CHILD_ENVS[child])` in the parent)."""
    if child == "sub":
        return list(SUB_CASES)
    if child == "pw2":
        return list(PW2_CASES)
    # ab: what changes form (without the fused operands, which the families that are switched off were the ones to take)
    return [n for c, n in zip(CASES, renamed(CASES)) if (n.name != c.name or n.pin != c.pin) and not (c.bn or c.up2)]


# The forms every pull request must keep reachable: whole names up to the modifier boundary (base_of) of a launch in the main table
# or in a child's, and every modifier as a token of some name.
_MODIFIERS = re.compile(r"(\.skip|\.tapin|\.S\d+|\.sub\d+\+\d+|\.up2|\.wv0)+$")


def base_of(name):
    return _MODIFIERS.sub("", name)


REQUIRED_FORMS = (
    [f"wgrad.thin.CO{n}.{s}" for n in (1, 2, 3, 4) for s in ("f32", "b16", "b16>f32")]
    + ["wgrad.wide.x6", "wgrad.wide.b16"]
    + [f"wgrad.patch.C{a}x{b}.{p}" for a in (32, 64) for b in (32, 64) for p in ("x6", "npl1", "b16")]
    + [f"wgrad.slab.x6.BN{bn}.{p}" for bn in (128, 64, 32) for p in ("x6", "npl1", "b16")]
    + [f"wgrad.planes.BN{bn}" for bn in (128, 64, 32)]
    + [f"wgrad.native.BN{bn}.{k}" for bn in (128, 64, 32) for k in ("scalar", "vec", "fast1", "fast2")]
    + [f"wgrad.native.BN{bn}.{k}.b16" for bn in (128, 64, 32) for k in ("scalar", "vec")]
    + ["wgrad.native.BN32.vec.b16>f32", "wgrad.native.BN32.scalar.b16>f32"]      # (SG_HEAD_F32 needs Cout <= 4: the 32-wide tile only)
)
REQUIRED_MODIFIERS = ("skip", "tapin", "S", "sub", "up2", "wv0")


def all_case_names():
    names = []
    for c in CASES:
        names += [c.name] + ([c.pin] if c.pin else [])
    for child, env in CHILD_ENVS.items():
        with switched(env):
            for c in child_cases(child):
                names += [c.name] + ([c.pin] if c.pin else [])
    return names


def missing_forms(names=None):
    names = all_case_names() if names is None else names
    bases = {base_of(n) for n in names}
    tokens = {re.sub(r"^(S|sub)\d.*$", r"\1", t) for n in names for t in n[len(base_of(n)):].split(".") if t}
    return [f for f in REQUIRED_FORMS if f not in bases] + ["." + m for m in REQUIRED_MODIFIERS if m not in tokens]


# ================================================================================================ operands and references
def bf16r(t):
    return t.bfloat16().float()


def rnd(gen, *shape):
    return (torch.rand(*shape, generator=gen) * 2.0 - 1.0).float()


def bn_params(C):
    gen = torch.Generator().manual_seed(C)
    return rnd(gen, C) * 0.3, rnd(gen, C) * 0.5 + 1.5, rnd(gen, C) + 1.5, rnd(gen, C) * 0.3


def last_slab_pixels(c, la):
    """The pixels (flat over N x Ho x Wo) of the reduction's last slab: the last P % 32 pixels or the last 32; the wide kernels: the
    last k-step; the patch kernel: the last row of 4 x 16 tiles."""
    g = c.g
    P = g.N * g.Ho * g.Wo
    if la["family"] == WG_PATCH:
        return range(P - 4 * g.Wo, P)
    px = la["step_px"] if la["family"] == WG_WIDE else BK
    return range(P - (P % px or px), P)


def storage_operands(c):
    """x (the source, under up2) and dy as the launch stores them, as fp32 host tensors."""
    g = c.g
    gen = torch.Generator().manual_seed(sum(map(ord, g.tag)))
    x = rnd(gen, g.N, g.H // 2, g.W // 2, g.Cin) if c.up2 else rnd(gen, g.N, g.H, g.W, g.Cin)
    dy = rnd(gen, g.N, g.Ho, g.Wo, g.Cout)
    if c.dt != "f32":
        x = bf16r(x)
        if c.dt == "b16":
            dy = bf16r(dy)
    return x, dy


def _dw_ref(g, x64, dy64):
    from oracle import tfops as T
    wr = torch.zeros(g.k, g.k, g.Cin, g.Cout, dtype=torch.float64, requires_grad=True)
    (dw,) = torch.autograd.grad(T.conv2d(x64, wr, None, g.s, g.d, "same"), wr, dy64)
    return dw


def references(c, la, without_last=False):
    """(dw, dbias) in float64 on the operands as the kernel of launch `la` sees them: fp32 storage on one bf16 plane (arithmetic mode
    2) multiplies operands rounded to nearest-even; the bias gradient sums dy as stored.  BatchNormalization in the loader: normalised
    in float64 first; up2: the materialised up-sampled tensor.  without_last: dw without the contribution of last_slab_pixels."""
    g = c.g
    x, dy = storage_operands(c)
    db = dy.double().reshape(-1, g.Cout).sum(0)
    if c.dt == "f32" and la["planes"] == 1:
        x, dy = bf16r(x), bf16r(dy)
    x64, dy64 = x.double(), dy.double()
    if c.bn:
        mean, inv, gam, bet = (t.double() for t in bn_params(g.Cin))
        x64 = torch.relu(((x64 - mean) * inv) * gam + bet)
    if c.up2:
        x64 = x64.repeat_interleave(2, 1).repeat_interleave(2, 2)
    if without_last:
        dy64 = dy64.clone().reshape(-1, g.Cout)
        px = last_slab_pixels(c, la)
        dy64[px.start:px.stop] = 0
        dy64 = dy64.reshape(g.N, g.Ho, g.Wo, g.Cout)
    return _dw_ref(g, x64, dy64), db


def record(cid, launch, qty, rel, bound):
    RECORDS.append((cid, launch, qty, rel, bound))
    if not QUIET:
        print(f"REC {cid} {launch} {qty} rel={rel:.3e} bound={bound:.3e}")


def compare(cid, launch, qty, got, ref, bound=BOUND):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (cid, launch, qty, tuple(got.shape), tuple(ref.shape))
    scale = ref.abs().max().item()
    fin = bool(torch.isfinite(got).all())
    err = (got - ref).abs().max().item() if fin else float("inf")
    record(cid, launch, qty, err / scale if scale > 0 else (0.0 if err == 0 else float("inf")), bound)
    assert fin, f"{cid} {launch} {qty}: non-finite values in the result"
    assert err <= bound * scale, f"{cid} {launch} {qty}: max err {err:.3e} > {bound:.3e} * {scale:.3e} (rel {err / max(scale, 1e-300):.2e})"


# ================================================================================================ the runner
LAUNCH_FIELDS = tuple(LAUNCH0)
PLAN_FIELDS = tuple(PLAN0)


def engine_plan(engine, c, aligned, planes=False):
    from building_detection_amd import _lib
    d = c.g.desc()
    pl = _lib.WgradPlan()
    rc = engine.lib.sg_conv2d_wgrad_plan(engine.h, F32 if planes else c.dtype, CT.byref(d), aligned, int(planes), CT.byref(pl))
    return rc, pl


def plans_equal(pl, o, what):
    for k in PLAN_FIELDS:
        assert getattr(pl, k) == o[k], f"{what}: sg_conv2d_wgrad_plan.{k} = {getattr(pl, k)}, the mirror says {o[k]}"
    for which in ("main", "tail"):
        for k in LAUNCH_FIELDS:
            got = getattr(getattr(pl, which), k)
            assert got == o[which][k], f"{what}: sg_conv2d_wgrad_plan.{which}.{k} = {got}, the mirror says {o[which][k]}"


def assert_plan(engine, c, cid):
    """Mirror == id; engine plan == mirror field by field, main and tail; the workspace query and sg_conv2d_caps agree.  Returns the
    mirror's plan of the launch (the plan query takes one alignment class for both tensors: a case with two is held to the query at
    each of them, and to the rules for the pair)."""
    from building_detection_amd import _lib
    bad = foreign_switches(os.environ)
    assert not bad, f"{bad} set: the mirror of tests/_wgrad_cases.py knows {sorted(SWITCH_DEFAULTS)} and the defaults of every other switch"
    assert SW == switches_of(os.environ), "the switches changed after this module was imported"
    cus = int(engine.lib.sg_num_cus(engine.h))
    assert cus == REF_CUS, f"the case shapes are chosen at {REF_CUS} CUs; this device has {cus}"
    assert int(engine.lib.sg_get_conv_x6()) == c.mode
    o = c.mirror(cus)
    name = form_name(o, o["main"], c.dtype, c.g)
    assert name == c.name, f"{cid}: the mirror names {name}"
    d = c.g.desc()
    for a in sorted({align_class(c.xoff), align_class(c.yoff)}):
        rc, pl = engine_plan(engine, c, a)
        assert rc == 0, engine.lib.sg_last_error()
        oa = plan_mirror(cus, c.mode, c.dtype, c.g, a, a)
        plans_equal(pl, oa, f"{cid} (aligned {a})")
        assert _lib.wgrad_form_name(pl, pl.main, c.dtype, d, SW["SG_WPW_VAR"]) == form_name(oa, oa["main"], c.dtype, c.g)
    assert o["ws_bytes"] <= engine.lib.sg_conv2d_wgrad_ws_bytes(engine.h, CT.byref(d)), f"{cid}: the workspace exceeds the storage-blind query's"
    if c.dt != "head":
        caps = _lib.ConvCaps()
        assert engine.lib.sg_conv2d_caps(engine.h, c.dtype & 0xff, CT.byref(d), 0, CT.byref(caps)) == 0
        o16 = plan_mirror(cus, c.mode, c.dtype & 0xff, c.g)
        op = plan_mirror(cus, c.mode, F32, c.g, planes=True)
        assert caps.wgrad_planes == int(c.dt == "f32" and op["main"]["family"] != 0), cid
        assert caps.bn_in == o16["bn_in"], f"{cid}: sg_conv2d_caps.bn_in = {caps.bn_in}, the mirror says {o16['bn_in']}"
        assert caps.up2 <= o16["up2"], cid      # (the forward must take the up-sampling too)
    return o


def _tt(c, side):
    if c.dt == "f32" or (c.dt == "head" and side == "y"):
        return torch.float32
    return torch.bfloat16


def _operand(t, ld, off_bytes, dev):
    """A [..][C] host tensor as a guarded input of pixel stride ld (gap columns NaN), `off_bytes` behind the arena's 16-byte boundary
    (the skipped bytes are 0xFF like the band).  Returns (arena, device pointer)."""
    C = t.shape[-1]
    flat = (widen(t, ld) if ld != C else t.reshape(-1, C)).reshape(-1)
    es = flat.element_size()
    assert off_bytes % es == 0
    lead = off_bytes // es
    if lead:
        pad = torch.full((lead * es,), 0xFF, dtype=torch.uint8).view(flat.dtype)
        flat = torch.cat([pad, flat])
    ga = Guarded(flat, dev)
    return ga, ga.ptr(lead)


def launch(engine, c, ws_bytes, cid, tag, expect=0, bn=None, dt=None, x=None, ws_off=0):
    """One sg_conv2d_wgrad call on guarded arenas -> (dw, dbias), or None for a refused call.  Bands, input bits, written-ness, the
    workspace's band right behind ws_bytes and - for a refused call - the untouched outputs are checked here."""
    from building_detection_amd import _lib
    g, dev = c.g, "cuda"
    d = g.desc()
    xs, dys = storage_operands(c)
    if x is not None:
        xs = x
    gx, px = _operand(xs.to(_tt(c, "x")), g.xl, c.xoff, dev)
    gdy, pdy = _operand(dys.to(_tt(c, "y")), g.yl, c.yoff, dev)
    gdw = Guarded.out((g.k, g.k, g.Cin, g.Cout), torch.float32, dev)
    gdb = Guarded.out((g.Cout,), torch.float32, dev)
    gws = Guarded.ws(ws_bytes + ws_off, dev)
    o = _lib.ConvOpts()
    o.ws, o.ws_bytes = gws.ptr() + ws_off, ws_bytes
    keep = []
    if bn is not None:
        keep = [Guarded(t, dev) for t in bn]
        bq = _lib.BnIn(*(t.ptr() for t in keep), 1, 0, 1e-3)
        o.bn_in = CT.pointer(bq)
    rc = engine.lib.sg_conv2d_wgrad(engine.h, engine.stream, c.dtype if dt is None else dt, CT.byref(d), px, pdy, gdw.ptr(), gdb.ptr(), CT.byref(o))
    torch.cuda.synchronize()
    what = f"{cid} {tag}"
    check_all([gx, gdy, gdw, gdb, gws] + keep, what)
    assert rc == expect, f"{what}: rc = {rc}, expected {expect}: {engine.lib.sg_last_error()}"
    if rc:
        for t in (gdw, gdb, gws):
            untouched(t, what)
        return None
    dw, db = gdw.read(), gdb.read()
    assert_written(dw, what + " dw")
    assert_written(db, what + " dbias")
    return dw, db


def launch_planes(engine, c, ws_bytes, cid, expect=0):
    """sg_conv2d_wgrad_planes on the caller's planes (sg_split_planes of the fp32 operands) -> dw or None."""
    g, dev = c.g, "cuda"
    d = g.desc()
    xs, dys = storage_operands(c)
    gx = Guarded(engine.split_planes(xs.cuda()).cpu(), dev)
    gdy = Guarded(engine.split_planes(dys.cuda()).cpu(), dev)
    gdw = Guarded.out((g.k, g.k, g.Cin, g.Cout), torch.float32, dev)
    gws = Guarded.ws(ws_bytes, dev)
    rc = engine.lib.sg_conv2d_wgrad_planes(engine.h, engine.stream, CT.byref(d), gx.ptr(), gdy.ptr(), gdw.ptr(), gws.ptr(), ws_bytes)
    torch.cuda.synchronize()
    check_all([gx, gdy, gdw, gws], f"{cid} pin")
    assert rc == expect, f"{cid} pin: rc = {rc}, expected {expect}: {engine.lib.sg_last_error()}"
    if rc:
        untouched(gdw, f"{cid} pin")
        untouched(gws, f"{cid} pin")
        return None
    dw = gdw.read()
    assert_written(dw, f"{cid} pin dw")
    return dw


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


def _run_case(engine, c, cid):
    o = assert_plan(engine, c, cid)
    bn = bn_params(c.g.Cin) if c.bn else None
    if c.bn:
        assert o["bn_in"] == 1, f"{cid}: the plan takes no BatchNormalization"
    if c.up2:
        assert o["up2"] == 1, f"{cid}: the plan takes no up-sampling source"
    dw_ref, db_ref = references(c, o["main"])
    launch(engine, c, o["ws_bytes"] - 1, cid, "ws-1", expect=SG_EWORKSPACE, bn=bn)
    dw, db = launch(engine, c, o["ws_bytes"], cid, "plain", bn=bn)
    compare(cid, "plain", "dw", dw, dw_ref)
    compare(cid, "plain", "dbias", db, db_ref)
    if c.pin:
        op = plan_mirror(REF_CUS, c.mode, F32, c.g, planes=True)
        assert form_name(op, op["main"], F32, c.g) == c.pin, f"{cid}: the mirror names the planes-in launch {form_name(op, op['main'], F32, c.g)}"
        rc, pl = engine_plan(engine, c, 16, planes=True)
        assert rc == 0, engine.lib.sg_last_error()
        plans_equal(pl, op, f"{cid} planes-in")
        assert (op["main"]["S"], op["main"]["steps"]) == (o["main"]["S"], o["main"]["steps"]), "the planes-in launch keeps the fp32 plan's shares"
        d = c.g.desc()
        assert pl.ws_bytes == engine.lib.sg_conv2d_wgrad_planes_ws_bytes(engine.h, CT.byref(d))
        launch_planes(engine, c, op["ws_bytes"] - 1, cid, expect=SG_EWORKSPACE)
        dwp = launch_planes(engine, c, op["ws_bytes"], cid)
        compare(cid, "pin", "dw", dwp, dw_ref)
        assert torch.equal(dwp, dw), f"{cid}: planes-in and fp32-operand filter gradient differ"


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
