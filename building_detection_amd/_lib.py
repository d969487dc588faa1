"""ctypes binding of libsegengine.so (the C ABI declared in include/segengine.h).

This is the only place the Python host touches native code.  There is NO CPU fallback: if the shared library
is missing, or no gfx950 device is visible when a context is requested, the import / call fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsegengine.so")

SG_F32, SG_BF16, SG_I64 = 0, 1, 2
SG_HEAD_F32 = 0x100  # OR-ed into the dtype of a thin 1x1 conv on bf16 storage: its few-channel side is fp32 (softmax head)
SG_COMM_ID_BYTES = 128
SG_EPI_BIAS, SG_EPI_RELU = 1, 2
SG_PRO_UP2, SG_EPI_DOWN2 = 16, 32   # UpSampling2D(2) -> Conv2D 3x3 fused: forward prologue / dgrad epilogue (segengine.h)
SG_X_UP2 = 0x200                   # ... and the dtype flag of its filter gradient
SG_ACT_RELU, SG_ACT_SIGMOID = 0, 1
SG_LOSS_CE2, SG_LOSS_FOCAL, SG_LOSS_EDGE_FOCAL = 0, 1, 2
SG_MAX_CLASSES = 32   # the C-class head: sg_softmax_*, sg_lossn_*, sg_confusion_matrix, sg_argmax_max_u8
SG_AUGMENT_MAX_ITEMS = 64
SG_AUG_FLIP_UD, SG_AUG_FLIP_LR, SG_AUG_SWAP_RB, SG_AUG_THRESHOLD = 1, 2, 4, 8
SG_WARP_MAX_ITEMS = 32
SG_WARP_NEAREST, SG_WARP_REFLECT, SG_WARP_COLOR = 1, 2, 4
SG_WARP_NOISE_STREAM, SG_WARP_NOISE_KEY = 0x6E6F6973, 0x77617270
SG_SCENE_MAX_ITEMS = 64
SG_SYM_FLIP_UD, SG_SYM_FLIP_LR, SG_SYM_TRANSPOSE = 1, 2, 4
SG_RESIZE_BILINEAR, SG_RESIZE_NEAREST = 0, 1
SG_RESIZE_MAX_EXTENT = 16384   # sg_resize_*, sg_prob_resize_accumulate: every extent
SG_OPT_ADAM, SG_OPT_SGD = 0, 1
SG_OPT_AMSGRAD, SG_OPT_NESTEROV, SG_OPT_EMA = 1, 2, 4
SG_OPT_CLIP_NONE, SG_OPT_CLIP_VALUE, SG_OPT_CLIP_NORM, SG_OPT_CLIP_GLOBAL = 0, 1, 2, 3
SG_OPT_SEG_DECAY = 1


class SgError(RuntimeError):
    pass


class PlanesJob(C.Structure):
    """Mirror of `sg_planes_job` (include/segengine.h): one weight tensor -> its prepared bf16 operand planes."""

    _fields_ = [("w_off", C.c_int64), ("out_off", C.c_int64)] + [(n, C.c_int32) for n in (
        "kind", "K", "N", "Kpad", "Npad", "Ck", "Ckp", "s_tap", "s_k", "s_n", "npl", "block0", "nblocks", "kd")]


SG_WS_PREPARED = C.c_size_t(-1).value


class AugmentItem(C.Structure):
    """Mirror of `sg_augment_item` (include/segengine.h): one output tile of sg_augment_u8."""
    _fields_ = [(n, C.c_int32) for n in ("src", "n", "shift", "flags")]


class WarpItem(C.Structure):
    """Mirror of `sg_warp_item` (include/segengine.h): one output tile of sg_warp_u8."""
    _fields_ = ([(n, C.c_int32) for n in ("src", "sh", "sw", "flags", "a00", "a01", "a10", "a11")] +
                [("b0", C.c_int64), ("b1", C.c_int64), ("sample", C.c_uint64), ("fill", C.c_int32), ("noise_q12", C.c_int32),
                 ("m", C.c_int32 * 9), ("off", C.c_int32 * 3)])


def warp_item(src=0, sh=0, sw=0, flags=0, a=(65536, 0, 0, 65536), b=(0, 0), sample=0, fill=0, noise_q12=0,
              m=(4096, 0, 0, 0, 4096, 0, 0, 0, 4096), off=(0, 0, 0)):
    """A WarpItem from Python values; the defaults are the identity map and the identity colour matrix."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    return WarpItem(int(src), int(sh), int(sw), int(flags), a[0], a[1], a[2], a[3], b[0], b[1], int(sample) & (2 ** 64 - 1),
                    int(fill), int(noise_q12), (C.c_int32 * 9)(*[int(v) for v in m]), (C.c_int32 * 3)(*[int(v) for v in off]))


class SceneItem(C.Structure):
    """Mirror of `sg_scene_item` (include/segengine.h): one tile window of sg_scene_tiles_u8 / sg_prob_accumulate."""
    _fields_ = [(n, C.c_int32) for n in ("y0", "x0", "sym", "reserved")]


class RegionDesc(C.Structure):
    """Mirror of `sg_region_desc` (include/segengine.h): a region-overlap loss, alone or added to a pointwise loss."""
    _fields_ = ([(n, C.c_int32) for n in ("C", "y_cols", "images", "point_kind")] + [("rows_per_image", C.c_int64)] +
                [(n, C.c_float) for n in ("a", "b", "smooth", "gamma", "point_weight", "region_weight")] +
                [("class_w", C.c_float * SG_MAX_CLASSES), ("point_alpha", C.c_float * SG_MAX_CLASSES)])


class MineDesc(C.Structure):
    """Mirror of `sg_mine_desc` (include/segengine.h): a pointwise loss averaged over the hard rows only."""
    _fields_ = ([(n, C.c_int32) for n in ("C", "y_cols", "kind", "reserved")] + [("rows", C.c_int64), ("min_kept", C.c_int64)] +
                [("thresh", C.c_float), ("alpha", C.c_float * SG_MAX_CLASSES)])


class LovaszDesc(C.Structure):
    """Mirror of `sg_lovasz_desc` (include/segengine.h): the Lovasz-Softmax loss, alone or added to a pointwise loss."""
    _fields_ = ([(n, C.c_int32) for n in ("C", "y_cols", "images", "classes_all")] + [("rows_per_image", C.c_int64)] +
                [(n, C.c_int32) for n in ("point_kind", "reserved")] + [(n, C.c_float) for n in ("point_weight", "lovasz_weight")] +
                [("point_alpha", C.c_float * SG_MAX_CLASSES)])


class OptimChunk(C.Structure):
    """Mirror of `sg_optim_chunk` (include/segengine.h): a 16-byte aligned run of one parameter's elements."""
    _fields_ = [("start", C.c_int64), ("length", C.c_int32), ("segment", C.c_int32)]


class OptimSeg(C.Structure):
    """Mirror of `sg_optim_seg` (include/segengine.h): one trainable parameter's chunks and flags."""
    _fields_ = [(n, C.c_int32) for n in ("chunk_begin", "chunk_end", "flags", "reserved")]


class OptimTable(C.Structure):
    """Mirror of `sg_optim_table` (include/segengine.h): the chunk table in host and in device memory."""
    _fields_ = [("chunks", C.c_void_p), ("segs", C.c_void_p), ("chunks_dev", C.c_void_p), ("segs_dev", C.c_void_p),
                ("nchunks", C.c_int32), ("nseg", C.c_int32), ("n", C.c_int64)]


class OptimDesc(C.Structure):
    """Mirror of `sg_optim_desc` (include/segengine.h): the update rule of sg_optim_step."""
    _fields_ = ([(n, C.c_int32) for n in ("kind", "flags", "clip")] + [(n, C.c_float) for n in (
        "beta1", "beta2", "eps", "momentum", "weight_decay", "clip_c", "ema_momentum", "grad_scale")])


class ConvDesc(C.Structure):
    """Mirror of `sg_conv_desc` (include/segengine.h)."""

    _fields_ = [(n, C.c_int32) for n in (
        "N", "H", "W", "Cin", "Cout", "KH", "KW", "stride", "dilation", "pad_t", "pad_l", "Ho", "Wo",
        "x_ld", "y_ld")]


class BnIn(C.Structure):
    """Mirror of `sg_bn_in` (include/segengine.h): a BatchNormalization (+ReLU) applied to a convolution's input in its loader."""

    _fields_ = [("mean", C.c_void_p), ("invstd", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("relu", C.c_int32), ("infer", C.c_int32), ("eps", C.c_float)]


class BnBwdIn(C.Structure):
    """Mirror of `sg_bn_bwd_in` (include/segengine.h): a BatchNormalization's backward apply evaluated inside a pointwise dgrad."""

    _fields_ = [("x", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("dz", C.c_void_p), ("relu", C.c_int32), ("rows", C.c_int64)]


class ConvOpts(C.Structure):
    """Mirror of `sg_conv_opts` (include/segengine.h): the optional operands of sg_conv2d_fwd / _dgrad / _wgrad (all-zero = plain)."""

    _fields_ = [("ws", C.c_void_p), ("ws_bytes", C.c_size_t), ("stats", C.c_void_p), ("tiles_out", C.POINTER(C.c_int)),
                ("a_planes", C.c_void_p), ("res", C.c_void_p), ("bn_in", C.POINTER(BnIn)), ("bnb", C.POINTER(BnBwdIn))]


class DwBnSums(C.Structure):
    """Mirror of `sg_dw_bnsums` (include/segengine.h): the BatchNormalization whose backward sums sg_dwconv2d_dgrad also produces."""

    _fields_ = [("x", C.c_void_p), ("mean", C.c_void_p), ("invstd", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("relu", C.c_int), ("dgamma", C.c_void_p), ("dbeta", C.c_void_p), ("ws", C.c_void_p), ("ws_bytes", C.c_size_t)]


class ConvCaps(C.Structure):
    """Mirror of `sg_conv_caps` (include/segengine.h): what the launches of one convolution can take (sg_conv2d_caps)."""

    _fields_ = [(n, C.c_int) for n in ("thin", "bn_in", "up2", "bnb", "planes_in", "wgrad_planes")]


class DwPlan(C.Structure):
    """Mirror of `sg_dw_plan` (include/segengine.h): the plan one depthwise launch runs by (sg_dwconv2d_plan)."""

    _fields_ = [(n, C.c_int) for n in ("family", "V", "RR", "lc", "HS", "nhs", "count", "gx", "gy", "S", "seg_V", "seg_TX", "seg_gx",
                                       "seg_S", "bn", "res", "sums")] + [("ws_bytes", C.c_size_t)]


class BnPlan(C.Structure):
    """Mirror of `sg_bn_plan_t` (include/segengine.h): the plan one BatchNormalization call runs by (sg_bn_plan)."""

    _fields_ = [(n, C.c_int) for n in ("V", "cols", "prow", "gx", "gy", "seg_V", "seg_TX", "seg_TY", "seg_gx", "seg_S", "fused",
                                       "fin_lanes")] + [("ws_bytes", C.c_size_t)]


class WgradLaunch(C.Structure):
    """Mirror of `sg_wgrad_launch` (include/segengine.h): one launch of a filter-gradient plan."""

    _fields_ = [(n, C.c_int) for n in ("family", "bn", "vec", "fast", "planes", "skip_slabs", "tap_inner", "stagger", "S", "steps",
                                       "step_px")]


class WgradPlan(C.Structure):
    """Mirror of `sg_wgrad_plan` (include/segengine.h): the plan one filter-gradient call runs by (sg_conv2d_wgrad_plan)."""

    _fields_ = ([("main", WgradLaunch), ("tail", WgradLaunch)] +
                [(n, C.c_int) for n in ("chunks", "nb", "tail_n", "max_parts", "bn_in", "up2")] +
                [(n, C.c_size_t) for n in ("dw_part_bytes", "bias_part_bytes", "bias_off", "ws_bytes")])


SG_WG_THIN, SG_WG_WIDE, SG_WG_PATCH, SG_WG_SLAB_X6, SG_WG_SLAB_NATIVE, SG_WG_HEAD32, SG_WG_PLANES = range(1, 8)
WG_FAMILY_NAMES = {0: "none", 1: "thin", 2: "wide", 3: "patch", 4: "slab-x6", 5: "slab-native", 6: "head32", 7: "planes-in"}


class ConvLaunch(C.Structure):
    """Mirror of `sg_conv_launch` (include/segengine.h): the kernel form of one forward / input-gradient launch."""

    _fields_ = [(n, C.c_int) for n in ("kernel", "bn", "vec", "ut", "var", "mf16", "ks", "pd", "skip_taps", "group_m", "cb", "pc",
                                       "pmulti")]


class ConvPlan(C.Structure):
    """Mirror of `sg_conv_plan` (include/segengine.h): the plan one forward / input-gradient call runs by (sg_conv2d_plan)."""

    _fields_ = ([("main", ConvLaunch), ("tail", ConvLaunch), ("with_res", ConvLaunch)] +
                [(n, C.c_int) for n in ("family", "fast", "nb", "nsub", "tail_n", "vec", "perm2", "npl", "kd", "Ck", "Ckp", "wbn",
                                        "x6w_S", "b16w_S", "deep", "res", "bn_in", "up2", "bnb", "planes_in")] +
                [("ws_bytes", C.c_size_t)])


SG_CF_NATIVE, SG_CF_THIN, SG_CF_HEAD, SG_CF_SLAB, SG_CF_PATCH, SG_CF_WIDE = range(6)
CONV_FAMILY_NAMES = {0: "native", 1: "thin", 2: "head", 3: "slab", 4: "patch", 5: "wide"}
SG_CK_NATIVE, SG_CK_THIN, SG_CK_X6, SG_CK_B16, SG_CK_X6W, SG_CK_B16W, SG_CK_PATCH, SG_CK_WIDE = range(1, 9)
CONV_KERNEL_NAMES = {0: "none", 1: "native", 2: "thin", 3: "slab.x6", 4: "slab.b16", 5: "slab.x6w", 6: "slab.b16w", 7: "patch",
                     8: "wide"}


def conv_form_name(pl: ConvPlan, la: ConvLaunch, dgrad: bool, dt: int, operands=()) -> str:
    """The name of one launch `la` of plan `pl` (DESIGN.md, appendix "convolution form names"):
        fwd|dgrad.native.BN<w>.<scalar|vec|ut>[.b16|.b16>f32|.f32>b16]      fwd|dgrad.thin.CO<n>.<f32|b16|b16>f32>
        fwd|dgrad.slab.x6.BN<w>.v<0|1>[.mf16][.npl1]                        fwd|dgrad.slab.b16.BN<w>.KS<2|4>.PD<1|2>
        fwd|dgrad.slab.x6w.S<1|2>        fwd|dgrad.slab.b16w.S<1-4>         fwd|dgrad.patch.C<32|64|64m>.BN<w>
        fwd|dgrad.wide.<x6|b16>.W<384|256>
    then the operands the call brings (`operands`, e.g. "bn", "res", "pin", "up2", "down2", "bnb"), then the modifiers
    .skip .perm2 .gm<n> .cb<n> .vpad .sub<nb>+<tail>."""
    b16, head = (dt & 0xff) == SG_BF16, bool(dt & SG_HEAD_F32)
    n = ("dgrad." if dgrad else "fwd.") + CONV_KERNEL_NAMES[la.kernel]
    k = la.kernel
    if k == SG_CK_NATIVE:
        n += f".BN{la.bn}." + ("ut" if la.ut else ("vec" if la.vec else "scalar"))
        n += (".f32>b16" if dgrad else ".b16>f32") if head else (".b16" if b16 else "")
    elif k == SG_CK_THIN:
        n += f".CO{la.bn}." + ("b16>f32" if head else ("b16" if b16 else "f32"))
    elif k == SG_CK_X6:
        n += f".BN{la.bn}.v{la.var}" + (".mf16" if la.mf16 else "") + (".npl1" if pl.npl == 1 else "")
    elif k == SG_CK_B16:
        n += f".BN{la.bn}.KS{la.ks}.PD{la.pd}"
    elif k == SG_CK_X6W:
        n += f".S{pl.x6w_S}"
    elif k == SG_CK_B16W:
        n += f".S{pl.b16w_S}"
    elif k == SG_CK_PATCH:
        n += f".C{la.pc}" + ("m" if la.pmulti else "") + f".BN{la.bn}"
    elif k == SG_CK_WIDE:
        n += (".b16" if b16 else ".x6") + f".W{la.bn}"
    n += "".join("." + o for o in operands)
    if la.skip_taps:
        n += ".skip"
    if pl.perm2 and k in (SG_CK_X6, SG_CK_B16):
        n += ".perm2"
    if la.group_m > 1:
        n += f".gm{la.group_m}"
    if la.cb:
        n += f".cb{la.cb}"
    if pl.Ckp != pl.Ck and pl.family == SG_CF_SLAB and pl.fast:
        n += ".vpad"
    if pl.nsub > 1:
        n += f".sub{pl.nb}+{pl.tail_n}"
    return n


def wgrad_form_name(pl: WgradPlan, la: WgradLaunch, dt: int, d: ConvDesc, wpw_var: int = 1) -> str:
    """The name of one launch `la` of filter-gradient plan `pl` of convolution `d` (DESIGN.md, appendix "filter-gradient form names"):
        wgrad.thin.CO<n>.<f32|b16|b16>f32>        wgrad.wide.<x6|b16>        wgrad.patch.C<cin>x<cout>.<x6|npl1|b16>
        wgrad.slab.x6.BN<w>.<x6|npl1|b16>         wgrad.planes.BN<w>         wgrad.native.BN<w>.<scalar|vec|fast1|fast2>[.b16|.b16>f32]
    then the modifiers .skip .tapin .S<n> .sub<nb>+<tail> .up2 .wv0.  dt: the call's dtype with its flags; wpw_var: SG_WPW_VAR of the
    process (the one form a plan does not name: wgrad_pw_wide_kernel<0>)."""
    b16, head = (dt & 0xff) == SG_BF16, bool(dt & SG_HEAD_F32)
    st = "b16>f32" if head else ("b16" if b16 else "f32")
    pipe = "b16" if b16 else ("npl1" if la.planes == 1 else "x6")
    fam = la.family
    if fam == SG_WG_THIN:
        n = f"wgrad.thin.CO{d.Cout}.{st}"
    elif fam == SG_WG_WIDE:
        n = f"wgrad.wide.{pipe}"
    elif fam == SG_WG_PATCH:
        n = f"wgrad.patch.C{d.Cin}x{d.Cout}.{pipe}"
    elif fam == SG_WG_SLAB_X6:
        n = f"wgrad.slab.x6.BN{la.bn}.{pipe}"
    elif fam == SG_WG_PLANES:
        n = f"wgrad.planes.BN{la.bn}"
    elif fam in (SG_WG_SLAB_NATIVE, SG_WG_HEAD32):
        kind = {2: "fast2", 1: "fast1"}.get(la.fast, "vec" if la.vec else "scalar")
        n = f"wgrad.native.BN{la.bn}.{kind}" + ("" if st == "f32" else "." + st)
    else:
        return "wgrad.none"
    if la.skip_slabs:
        n += ".skip"
    if la.tap_inner:
        n += ".tapin"
    if la.S > 1:
        n += f".S{la.S}"
    if pl.chunks > 1:
        n += f".sub{pl.nb}+{pl.tail_n}"
    if (dt & SG_X_UP2) and pl.up2:
        n += ".up2"
    if fam == SG_WG_WIDE and not b16 and wpw_var != 1:
        n += ".wv0"
    return n


class SegPlan(C.Structure):
    """Mirror of `sg_seg_plan_t` (include/segengine.h): the segment reducer's plan (sg_seg_plan)."""

    _fields_ = [(n, C.c_int) for n in ("V", "TX", "TY", "gx", "S")] + [("part_bytes", C.c_size_t)]


_vp, _i, _i64, _f, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_op = C.POINTER(ConvOpts)
_dp = C.POINTER(ConvDesc)
_pp = C.POINTER(C.c_void_p)
_fp = C.POINTER(C.c_float)

# name -> (restype, argtypes).  Kept in the order of include/segengine.h.
_SIGNATURES = {
    "sg_abi_version": (_i, []),
    "sg_last_error": (C.c_char_p, []),
    "sg_set_conv_x6": (_i, [_i]),
    "sg_create": (_i, [_i, _pp]),
    "sg_destroy": (_i, [_vp]),
    "sg_num_cus": (_i, [_vp]),
    "sg_conv2d_fwd": (_i, [_vp, _vp, _i, _dp, _vp, _vp, _vp, _vp, _i, _op]),
    "sg_conv2d_fwd_ws_bytes": (_sz, [_dp]),
    "sg_conv2d_fwd_stats_bytes": (_sz, [_dp]),
    "sg_get_conv_x6": (_i, []),
    "sg_conv2d_planes_job": (_i, [_vp, _i, _dp, _i, C.POINTER(PlanesJob), C.POINTER(C.c_size_t)]),
    "sg_prepare_planes": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
    "sg_bn_tiles_ws_bytes": (_sz, [_vp, _i, _i]),
    "sg_bn_train_fwd_tiles": (_i, [_vp, _vp, _i, _i64, _i, _vp, _i, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _i, _vp, _sz]),
    "sg_bn_apply": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "sg_conv2d_dgrad_ws_bytes": (_sz, [_dp]),
    "sg_conv2d_dgrad": (_i, [_vp, _vp, _i, _dp, _vp, _vp, _vp, _vp, _i, _op]),
    "sg_conv2d_wgrad_ws_bytes": (_sz, [_vp, _dp]),
    "sg_conv2d_wgrad": (_i, [_vp, _vp, _i, _dp, _vp, _vp, _vp, _vp, _op]),
    "sg_conv2d_caps": (_i, [_vp, _i, _dp, _i, C.POINTER(ConvCaps)]),
    "sg_conv2d_plan": (_i, [_vp, _i, _dp, _i, _i, _i, C.POINTER(ConvPlan)]),
    "sg_split_planes": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp]),
    "sg_conv2d_wgrad_planes_ws_bytes": (_sz, [_vp, _dp]),
    "sg_conv2d_wgrad_planes": (_i, [_vp, _vp, _dp, _vp, _vp, _vp, _vp, _sz]),
    "sg_conv2d_wgrad_plan": (_i, [_vp, _i, _dp, _i, _i, C.POINTER(WgradPlan)]),
    "sg_bias_grad_ws_bytes": (_sz, [_vp, _i64, _i]),
    "sg_bias_grad": (_i, [_vp, _vp, _i, _i64, _i, _i, _vp, _vp, _vp, _sz]),
    "sg_dwconv2d_fwd": (_i, [_vp, _vp, _i, _dp, _vp, _vp, _vp, _i, C.POINTER(BnIn)]),
    "sg_dwconv2d_dgrad": (_i, [_vp, _vp, _i, _dp, _vp, _vp, _vp, _vp, _i, _vp, C.POINTER(DwBnSums)]),
    "sg_dwconv2d_dgrad_bnsums_ws_bytes": (_sz, [_vp, _dp]),
    "sg_dwconv2d_wgrad_ws_bytes": (_sz, [_vp, _dp]),
    "sg_dwconv2d_wgrad": (_i, [_vp, _vp, _i, _dp, _vp, _vp, _vp, _i, C.POINTER(BnIn), _vp, _sz]),
    "sg_dwconv2d_plan": (_i, [_vp, _i, _dp, _i, _i, _i, C.POINTER(DwPlan)]),
    "sg_dense_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i]),
    "sg_bn_ws_bytes": (_sz, [_vp, _i64, _i]),
    "sg_bn_train_fwd": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _i, _vp, _sz]),
    "sg_bn_train_bwd": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz]),
    "sg_bn_train_bwd_apply": (_i, [_vp, _vp, _i, _i64, _i] + [_vp] * 9 + [_i]),
    "sg_bn_train_bwd_thin_ok": (_i, [_vp, _i, _i64, _i, _i, _i]),
    "sg_bn_train_bwd_thin": (_i, [_vp, _vp, _i, _i64, _i, _i, _i] + [_vp] * 10 + [_i, _vp, _sz]),
    "sg_bn_infer": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _i]),
    "sg_add2_bn": (_i, [_vp, _vp, _i, _i64, _i] + [_vp] * 11 + [_i, _i, _f, _i, _i]),
    "sg_gn_ws_bytes": (_sz, [_vp, _i, _i, _i64, _i, _i]),
    "sg_gn_fwd": (_i, [_vp, _vp, _i, _i, _i64, _i, _i] + [_vp] * 6 + [_f, _i, _vp, _sz]),
    "sg_gn_bwd": (_i, [_vp, _vp, _i, _i, _i64, _i, _i] + [_vp] * 9 + [_i, _vp, _sz]),
    "sg_bn_plan": (_i, [_vp, _i, _i64, _i, _i, _i, C.POINTER(BnPlan)]),
    "sg_seg_plan": (_i, [_vp, _i, _i, _i64, _i, _i, _i, C.POINTER(SegPlan)]),
    "sg_act_fwd": (_i, [_vp, _vp, _i, _i, _i64, _vp, _vp]),
    "sg_act_bwd": (_i, [_vp, _vp, _i, _i, _i64, _vp, _vp, _vp, _i]),
    "sg_add_n": (_i, [_vp, _vp, _i, _i, _pp, _i64, _vp, _i]),
    "sg_copy_channels": (_i, [_vp, _vp, _i, _i64, _i, _vp, _i, _i, _vp, _i, _i, _i]),
    "sg_softmax2_fwd": (_i, [_vp, _vp, _i, _i64, _vp, _vp]),
    "sg_softmax2_bwd": (_i, [_vp, _vp, _i, _i64, _vp, _vp, _vp]),
    "sg_softmax_fwd": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp]),
    "sg_softmax_bwd": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _vp]),
    "sg_softmax_branch_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sg_softmax_branch_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sg_bcast_mul_fwd": (_i, [_vp, _vp, _i, _i, _i64, _i, _i, _vp, _vp, _vp, _i]),
    "sg_bcast_mul_bwd_ws_bytes": (_sz, [_vp, _i, _i64, _i, _i]),
    "sg_bcast_mul_bwd": (_i, [_vp, _vp, _i, _i, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _sz]),
    "sg_scse_fwd": (_i, [_vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp]),
    "sg_scse_bwd_ws_bytes": (_sz, [_vp, _i, _i64, _i]),
    "sg_scse_bwd": (_i, [_vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "sg_scse_bwd_sums": (_i, [_vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "sg_scse_bwd_final": (_i, [_vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "sg_bam_fwd": (_i, [_vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp]),
    "sg_bam_bwd_ws_bytes": (_sz, [_vp, _i, _i64, _i]),
    "sg_bam_bwd": (_i, [_vp, _vp, _i, _i, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz]),
    "sg_dropout": (_i, [_vp, _vp, _i, _i64, _i64, _i, _i64, C.c_uint32, C.c_uint32, _f, _vp, _vp, _vp]),
    "sg_maxpool_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "sg_maxpool_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "sg_maxpool_fwd_idx": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sg_maxpool_bwd_idx": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "sg_avgpool_ws_bytes": (_sz, [_vp, _i, _i, _i, _i, _i, _i]),
    "sg_avgpool_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz]),
    "sg_avgpool_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "sg_upsample_nearest_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "sg_upsample_nearest_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i]),
    "sg_upsample_bilinear_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "sg_upsample_bilinear_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i]),
    "sg_resize_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i]),
    "sg_resize_bwd": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _i]),
    "sg_loss_ws_bytes": (_sz, [_vp, _i64]),
    "sg_loss_fwd": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _vp, _sz]),
    "sg_loss_bwd": (_i, [_vp, _vp, _i, _i64, _i, _vp, _vp, _vp, _f]),
    "sg_confusion_counts": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp]),
    "sg_lossn_ws_bytes": (_sz, [_vp, _i64]),
    "sg_lossn_fwd": (_i, [_vp, _vp, _i, _i64, _i, _i, _fp, _vp, _vp, _vp, _vp, _sz]),
    "sg_lossn_bwd": (_i, [_vp, _vp, _i, _i64, _i, _i, _fp, _vp, _vp, _vp, _f]),
    "sg_confusion_matrix": (_i, [_vp, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "sg_loss_region_ws_bytes": (_sz, [_vp, C.POINTER(RegionDesc)]),
    "sg_loss_region_fwd": (_i, [_vp, _vp, C.POINTER(RegionDesc), _vp, _vp, _vp, _vp, _vp, _sz]),
    "sg_loss_region_bwd": (_i, [_vp, _vp, C.POINTER(RegionDesc), _vp, _vp, _vp, _vp, _f]),
    "sg_loss_mined_ws_bytes": (_sz, [_vp, C.POINTER(MineDesc)]),
    "sg_loss_mined_fwd": (_i, [_vp, _vp, C.POINTER(MineDesc), _vp, _vp, _vp, _vp, _vp, _sz]),
    "sg_loss_mined_bwd": (_i, [_vp, _vp, C.POINTER(MineDesc), _vp, _vp, _vp, _vp, _f]),
    "sg_sort_pairs_ws_bytes": (_sz, [_vp, _i64, _i64, _i]),
    "sg_sort_pairs_u32": (_i, [_vp, _vp, _i64, _i64, _i, _vp, _vp, _vp, _vp, _vp, _sz]),
    "sg_loss_lovasz_ws_bytes": (_sz, [_vp, C.POINTER(LovaszDesc)]),
    "sg_loss_lovasz_fwd": (_i, [_vp, _vp, C.POINTER(LovaszDesc), _vp, _vp, _vp, _vp, _vp, _sz]),
    "sg_loss_lovasz_bwd": (_i, [_vp, _vp, C.POINTER(LovaszDesc), _vp, _vp, _vp, _vp, _f]),
    "sg_adam_step": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _f]),
    "sg_adam_step_lr": (_i, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f]),
    "sg_optim_norms_ws_bytes": (_sz, [_i]),
    "sg_optim_grad_norms": (_i, [_vp, _vp, C.POINTER(OptimTable), _vp, _f, _vp, _vp, _sz]),
    "sg_optim_step": (_i, [_vp, _vp, C.POINTER(OptimDesc), C.POINTER(OptimTable), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp]),
    "sg_edge_labels": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    "sg_resize_linear_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp]),
    "sg_augment_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _i, _i, _i, _vp]),
    "sg_warp_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, C.c_uint64, _i, _i, _vp]),
    "sg_argmax_accumulate_i8": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _i]),
    "sg_argmax_max_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _i, _i, _i, _i]),
    "sg_scene_tiles_u8": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _i, _vp]),
    "sg_prob_accumulate": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _f, _vp, _vp, _i, _i]),
    "sg_prob_finalize": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "sg_prob_resize_accumulate": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _f, _vp, _vp, _i, _i]),
    "sg_vote_ge": (_i, [_vp, _vp, _i, _pp, _i64, _i, _vp]),
    "sg_mask_objects_ws_bytes": (_sz, [_i, _i]),
    "sg_mask_objects": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _sz, _vp, _vp, _i, _vp, _vp]),
    "sg_mask_split_words": (_i64, [_i, _i, _i, _i, _i, _i]),
    "sg_mask_split": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "sg_objects_label_ws_bytes": (_sz, [_i, _i]),
    "sg_objects_label": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _sz, _vp, _vp, _i, _vp]),
    "sg_objects_overlap_ws_bytes": (_sz, [_i64]),
    "sg_objects_overlap": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i64, _vp, _sz, _vp, _vp]),
    "sg_object_distances_ws_bytes": (_sz, [_i, _i, _i]),
    "sg_object_distances": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp, _vp]),
    "sg_separation_weights": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _f, _f, _vp]),
    "sg_u8_to_f32": (_i, [_vp, _vp, _i64, _vp, _vp, _f, _f]),
    "sg_cast": (_i, [_vp, _vp, _i, _i, _i64, _vp, _vp]),
    "sg_fill_f32": (_i, [_vp, _vp, _vp, _i64, _f]),
    "sg_trace_mark": (_i, [_vp, _vp, _i, _i]),
    "sg_scale_f32": (_i, [_vp, _vp, _vp, _i64, _f]),
    "sg_comm_probe": (_i, [_vp]),
    "sg_comm_unique_id": (_i, [_vp]),
    "sg_comm_init": (_i, [_vp, _i, _i, _i, _pp]),
    "sg_comm_allreduce_sum": (_i, [_vp, _vp, _i, _vp, _i64]),
    "sg_comm_rank": (_i, [_vp]),
    "sg_comm_nranks": (_i, [_vp]),
    "sg_comm_destroy": (_i, [_vp]),
}

_lib = None
_lock = threading.Lock()


def load():
    """dlopen libsegengine.so (once) and attach the signatures.  Raises SgError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        # torch must be imported first: it brings its own HIP runtime (libamdhip64) and a second copy loaded
        # ahead of it by this library would not see the device torch allocates on.
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise SgError(
                f"{LIB_PATH} is missing - build it with `make -C building_detection_amd/csrc` "
                "(or __graft_entry__.build()).  There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the ABI and the binding diverge
            fn.restype = res
            fn.argtypes = args
        if lib.sg_abi_version() != 1:
            raise SgError(f"libsegengine ABI {lib.sg_abi_version()} != binding ABI 1")
        _lib = lib
    return _lib


def exported_symbols():
    return list(_SIGNATURES)


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().sg_last_error().decode("utf-8", "replace")
        raise SgError(f"{what or 'libsegengine'} failed (rc={rc}): {msg}")


class Context:
    """One `sg_ctx` per device (creation fails without a gfx950 GPU)."""

    def __init__(self, device: int = 0):
        lib = load()
        h = C.c_void_p()
        check(lib.sg_create(device, C.byref(h)), "sg_create")
        self.handle = h
        self.device = device
        self.num_cus = lib.sg_num_cus(h)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                load().sg_destroy(self.handle)
                self.handle = None
        except Exception:
            pass
