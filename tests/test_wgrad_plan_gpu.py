"""The GEMM filter gradient (csrc/conv_igemm.hip: sg_conv2d_wgrad, sg_conv2d_wgrad_planes) by kernel family, through the C ABI, with
the plan it runs by (sg_conv2d_wgrad_plan) asserted before every launch.  Operands are tests/_guarded.py arenas: NaN guard bands,
NaN-prefilled outputs, inputs whose bits must survive and a workspace of exactly plan.ws_bytes with a band right behind it.
Reference and tolerance are tests/test_ops_gpu.py's: oracle.tfops.conv2d in float64 (bf16 cases: on the bf16-rounded operands),
max|got - ref| <= 2e-5 * max|ref| for dw and dbias (fp32 accumulation of fp32 / exact bf16 products).

Every case id ends in the family the plan must name at 256 CUs, written down here from the rules of plan_wgrad, not read back:
    thin         1x1, stride 1, Cout <= 4, Cin % 4 == 0, Cin >= 16, x 16-byte aligned
    wide         1x1, stride 1, no padding, >= 6144 pixels, Cin >= 256, tiles of 128 x 384 at least 3/4 full (fp32: arithmetic mode 1)
    patch        3x3, stride 1, dilation 1, SAME, Cin and Cout in {32, 64}, H % 4 == 0, W % 16 == 0
    slab-x6      stride 1 SAME, or stride 2 with dilation 1 and Ho = ceil(H / 2); Wo % 32 == 0, Cout >= 16, 16-byte channel runs
    slab-native  everything else (here: Wo = 10; Cin = 3; the fallbacks of thin / wide / patch when x sits 4 bytes off)
    head32       bf16 x with fp32 dy that is not thin
    planes-in    stride 1 SAME, Wo % 32 == 0, channels % 8 == 0, Cout >= 16, dense, a slab-x6 layer in fp32"""
import ctypes as CT

import pytest
import torch

from building_detection_amd import _lib
from oracle import tfops as T
from test_ops_gpu import close, rnd
from _guarded import Guarded, assert_written, check_all, untouched

pytestmark = pytest.mark.gpu

F32, BF16 = _lib.SG_F32, _lib.SG_BF16
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
NAMES = _lib.WG_FAMILY_NAMES

# tag: (N, H, W, Cin, Cout, k, stride, dilation)
SHAPES = {
    "thin": (2, 9, 7, 48, 2, 1, 1, 1),
    "wide": (1, 96, 64, 256, 384, 1, 1, 1),          # P = 6144, the smallest wgrad_pw_wide_geom admits
    "patch": (2, 20, 48, 32, 32, 3, 1, 1),
    "x6_s1_d3": (1, 64, 32, 48, 80, 3, 1, 3),
    "x6_s2": (2, 64, 64, 64, 128, 3, 2, 1),
    "native": (2, 17, 19, 64, 64, 3, 2, 1),
    "stem_c3": (2, 24, 20, 3, 32, 3, 2, 1),
    "planes": (2, 32, 32, 256, 256, 3, 1, 6),
    "head": (2, 12, 12, 64, 2, 3, 1, 1),
    # the patch case with H % 8 == 0: a BatchNormalization goes into the loaders of forward and filter gradient together, and at
    # H = 20 the forward takes the im2col kernel, which has none
    "patch_h24": (2, 24, 48, 32, 32, 3, 1, 1),
}
# (shape, storage, family, and the fields of plan.main that the rules fix: tile width, channels per load, bf16 planes per operand)
CASES = [
    ("thin", "f32", "thin", dict(bn=0, S=1)),
    ("wide", "f32", "wide", dict(planes=3, step_px=16, S=48, steps=8)),      # 2 tiles -> 128 shares, capped at 384 k-steps / 8
    ("patch", "f32", "patch", dict(planes=3, S=30)),                        # 2 x 5 x 3 tiles < 512 slots
    ("x6_s1_d3", "f32", "slab-x6", dict(bn=128, vec=4, planes=3, skip_slabs=1, tap_inner=0)),
    ("x6_s2", "f32", "slab-x6", dict(bn=128, vec=4, planes=3, skip_slabs=0)),
    ("native", "f32", "slab-native", dict(bn=64, vec=4, fast=0, planes=0)),
    ("stem_c3", "f32", "slab-native", dict(bn=32, vec=0, fast=0, planes=0)),
    ("planes", "f32", "slab-x6", dict(bn=128, vec=4, planes=3, skip_slabs=1, tap_inner=1)),
    ("thin", "bf16", "thin", dict(S=1)),
    ("wide", "bf16", "wide", dict(planes=1, step_px=32, S=24, steps=8)),     # 192 k-steps of 32 pixels / 8
    ("patch", "bf16", "patch", dict(planes=1, S=30)),
    ("x6_s1_d3", "bf16", "slab-x6", dict(bn=128, vec=8, planes=1, skip_slabs=1)),
    ("x6_s2", "bf16", "slab-x6", dict(bn=128, vec=8, planes=1)),
    ("native", "bf16", "slab-native", dict(bn=64, vec=4, planes=0, skip_slabs=0)),
    ("head", "head32", "head32", dict(bn=32, vec=0)),                       # Cout = 2: no 4-channel loads of dy
]
# x 4 bytes off its 16-byte boundary: the slab kernels' scalar form, with at most the aligned plan's shares
FALLBACKS = [
    ("thin", "slab-native", dict(bn=32, vec=0, S=1, steps=4)),               # 126 pixels = 4 slabs, straight into dw
    ("wide", "slab-native", dict(bn=128, vec=0, S=48, steps=4)),             # 192 slabs in the wide plan's 48 shares
    ("patch", "slab-native", dict(bn=32, vec=0, S=30, steps=2)),             # 60 slabs in the patch plan's 30 shares
]


def _id(shape, storage, family):
    return f"{shape}-{storage}-{family}"


def _desc(engine, shape):
    n, h, w, cin, cout, k, s, dil = SHAPES[shape]
    return engine.conv_desc((n, h, w, cin), cout, k, k, s, dil, "same")


_REF = {}


def _operands(shape, storage):
    """x, dy on the host (bf16 storage: rounded) and the fp64 dw / dbias of T.conv2d; computed once per (shape, storage)."""
    key = (shape, storage)
    if key not in _REF:
        n, h, w, cin, cout, k, s, dil = SHAPES[shape]
        g = torch.Generator().manual_seed(sum(map(ord, shape)))
        x = rnd(g, n, h, w, cin)
        ho, wo = -(-h // s), -(-w // s)
        dy = rnd(g, n, ho, wo, cout)
        if storage != "f32":
            x = x.bfloat16().float()
            if storage == "bf16":
                dy = dy.bfloat16().float()
        _REF[key] = (x, dy) + _reference(x, dy, SHAPES[shape])
    return _REF[key]


def _reference(x, dy, geom):
    n, h, w, cin, cout, k, s, dil = geom
    wr = torch.zeros(k, k, cin, cout, dtype=torch.float64, requires_grad=True)
    br = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    T.conv2d(x.double(), wr, br, s, dil, "same").backward(dy.double())
    return wr.grad, br.grad


def _dtypes(storage):
    if storage == "f32":
        return F32, torch.float32, torch.float32
    if storage == "bf16":
        return BF16, torch.bfloat16, torch.bfloat16
    return BF16 | _lib.SG_HEAD_F32, torch.bfloat16, torch.float32


def _plan(engine, d, dt, aligned=16, planes=False):
    pl = _lib.WgradPlan()
    rc = engine.lib.sg_conv2d_wgrad_plan(engine.h, dt, CT.byref(d), aligned, 1 if planes else 0, CT.byref(pl))
    return rc, pl


def _assert_plan(engine, pl, family, fields, what):
    cus = int(engine.lib.sg_num_cus(engine.h))
    assert cus == 256, f"the expected plans are written for 256 CUs, this device has {cus}"
    assert NAMES[pl.main.family] == family, f"{what}: the plan names {NAMES[pl.main.family]}, the rules say {family}"
    for k, v in fields.items():
        assert getattr(pl.main, k) == v, f"{what}: plan.main.{k} = {getattr(pl.main, k)}, the rules say {v}"
    assert pl.chunks == 1 and pl.max_parts == pl.main.S
    assert pl.bias_off % 256 == 0 and pl.bias_off >= pl.dw_part_bytes and pl.bias_off + pl.bias_part_bytes <= pl.ws_bytes
    assert pl.ws_bytes == pl.dw_part_bytes + pl.bias_part_bytes + 512


def _launch(engine, dt, d, x, dy, ws_bytes, x_off=False, bn=None, planes=False):
    """One call on guarded arenas -> (rc, dw, dbias or None); guards, input bits and the workspace's far band checked."""
    dev = "cuda"
    gx, gdy = Guarded(x, dev, off=x_off), Guarded(dy, dev)
    gdw = Guarded.out((d.KH, d.KW, d.Cin, d.Cout), torch.float32, dev)
    gdb = None if planes else Guarded.out((d.Cout,), torch.float32, dev)
    gws = Guarded.ws(ws_bytes, dev)
    keep = []
    if planes:
        rc = engine.lib.sg_conv2d_wgrad_planes(engine.h, engine.stream, CT.byref(d), gx.ptr(), gdy.ptr(), gdw.ptr(), gws.ptr(), ws_bytes)
    else:
        o = _lib.ConvOpts()
        o.ws, o.ws_bytes = gws.ptr(), ws_bytes
        if bn is not None:
            keep = [Guarded(t, dev) for t in bn[:4]]
            bq = _lib.BnIn(*(t.ptr() for t in keep), int(bn[4]), 0, 1e-3)
            o.bn_in = CT.pointer(bq)
        rc = engine.lib.sg_conv2d_wgrad(engine.h, engine.stream, dt, CT.byref(d), gx.ptr(), gdy.ptr(),
                                        gdw.ptr(), gdb.ptr(), CT.byref(o))
    torch.cuda.synchronize()
    ops = [gx, gdy, gdw, gws] + keep + ([] if gdb is None else [gdb])
    check_all(ops, "filter gradient")
    if rc:
        untouched(gdw, "dw")
        if gdb is not None:
            untouched(gdb, "dbias")
        return rc, None, None
    dw = gdw.read()
    assert_written(dw, "dw")
    db = None
    if gdb is not None:
        db = gdb.read()
        assert_written(db, "dbias")
    return 0, dw, db


@pytest.mark.parametrize("shape,storage,family,fields", CASES, ids=[_id(*c[:3]) for c in CASES])
def test_every_family_at_its_smallest_shape(engine, shape, storage, family, fields):
    dt, tx, ty = _dtypes(storage)
    d = _desc(engine, shape)
    x, dy, dw_ref, db_ref = _operands(shape, storage)
    rc, pl = _plan(engine, d, dt)
    assert rc == 0
    _assert_plan(engine, pl, family, fields, _id(shape, storage, family))
    assert pl.ws_bytes <= engine.lib.sg_conv2d_wgrad_ws_bytes(engine.h, CT.byref(d))
    rc, dw, db = _launch(engine, dt, d, x.to(tx), dy.to(ty), pl.ws_bytes)
    assert rc == 0, engine.lib.sg_last_error()
    close(dw, dw_ref, what=f"{shape} {storage} dw")
    close(db, db_ref, what=f"{shape} {storage} dbias")


def test_planes_in_has_the_bits_of_the_fp32_operands(engine):
    d = _desc(engine, "planes")
    x, dy, dw_ref, _ = _operands("planes", "f32")
    rc, pl = _plan(engine, d, F32, planes=True)
    assert rc == 0
    _assert_plan(engine, pl, "planes-in", dict(bn=128, vec=8, planes=3, skip_slabs=1, tap_inner=1), "planes-in")
    rc, pf = _plan(engine, d, F32)
    assert rc == 0 and (pl.main.S, pl.main.steps) == (pf.main.S, pf.main.steps), "the planes-in launch keeps the fp32 plan's shares"
    assert pl.bias_part_bytes == 0 and pl.ws_bytes == engine.lib.sg_conv2d_wgrad_planes_ws_bytes(engine.h, CT.byref(d))
    assert engine.conv2d_caps(d).wgrad_planes == 1
    xp, dyp = engine.split_planes(x.cuda()).cpu(), engine.split_planes(dy.cuda()).cpu()
    rc, dw, _ = _launch(engine, F32, d, xp, dyp, pl.ws_bytes, planes=True)
    assert rc == 0
    close(dw, dw_ref, what="planes-in dw")
    rc, dw32, _ = _launch(engine, F32, d, x, dy, pf.ws_bytes)
    assert rc == 0 and torch.equal(dw, dw32), "planes-in and fp32-operand filter gradient differ"
    # a layer of another family has no planes-in plan: all-zero, the entry point's code
    rc, none = _plan(engine, _desc(engine, "patch"), F32, planes=True)
    assert rc == EUNSUPPORTED and none.main.family == 0 and none.ws_bytes == 0
    assert engine.conv2d_caps(_desc(engine, "patch")).wgrad_planes == 0


@pytest.mark.parametrize("shape,family,fields", FALLBACKS, ids=[_id(c[0], "f32-x+4", c[1]) for c in FALLBACKS])
def test_fallbacks_of_unaligned_operands_are_plans_of_their_own(engine, shape, family, fields):
    d = _desc(engine, shape)
    x, dy, dw_ref, db_ref = _operands(shape, "f32")
    rc, pl = _plan(engine, d, F32, aligned=0)
    assert rc == 0
    _assert_plan(engine, pl, family, fields, _id(shape, "f32-x+4", family))
    assert pl.bn_in == 0 and pl.up2 == 0
    assert pl.ws_bytes <= engine.lib.sg_conv2d_wgrad_ws_bytes(engine.h, CT.byref(d))
    rc, dw, db = _launch(engine, F32, d, x, dy, pl.ws_bytes, x_off=True)
    assert rc == 0
    close(dw, dw_ref, what=f"{shape} unaligned dw")
    close(db, db_ref, what=f"{shape} unaligned dbias")


@pytest.mark.parametrize("shape", ["patch_h24", "thin"])
def test_batchnorm_in_the_loader_runs_where_the_plan_says(engine, shape):
    d = _desc(engine, shape)
    assert NAMES[_plan(engine, d, F32)[1].main.family] == ("thin" if shape == "thin" else "patch")
    x, dy, _, _ = _operands(shape, "f32")
    cin = d.Cin
    g = torch.Generator().manual_seed(cin)
    mean, inv, gam, bet = rnd(g, cin) * 0.3, rnd(g, cin) * 0.5 + 1.5, rnd(g, cin) + 1.5, rnd(g, cin) * 0.3
    rc, pl = _plan(engine, d, F32)
    assert rc == 0 and pl.bn_in == 1 and engine.conv2d_caps(d).bn_in == 1
    rc, dw, db = _launch(engine, F32, d, x, dy, pl.ws_bytes, bn=(mean, inv, gam, bet, True))
    assert rc == 0
    xn = torch.relu(((x.double() - mean.double()) * inv.double()) * gam.double() + bet.double())
    dw_ref, db_ref = _reference(xn, dy, SHAPES[shape])
    close(dw, dw_ref, what=f"{shape} BatchNormalization -> ReLU -> dw")
    close(db, db_ref, what=f"{shape} dbias")


def test_fused_operands_outside_the_plan_are_refused_untouched(engine):
    d = _desc(engine, "x6_s1_d3")
    x, dy, _, _ = _operands("x6_s1_d3", "f32")
    cin = d.Cin
    bn = (torch.zeros(cin), torch.ones(cin), torch.ones(cin), torch.zeros(cin), True)
    rc, pl = _plan(engine, d, F32)
    assert rc == 0 and pl.bn_in == 0 and pl.up2 == 0
    caps = engine.conv2d_caps(d)
    assert caps.bn_in == 0 and caps.up2 == 0
    rc, _, _ = _launch(engine, F32, d, x, dy, pl.ws_bytes, bn=bn)
    assert rc == EUNSUPPORTED
    rc, pu = _plan(engine, d, F32 | _lib.SG_X_UP2)
    assert rc == 0 and pu.up2 == 0
    rc, _, _ = _launch(engine, F32 | _lib.SG_X_UP2, d, x[:, ::2, ::2].contiguous(), dy, pu.ws_bytes)
    assert rc == EUNSUPPORTED
    # the patch filter gradient of a layer whose forward is not a patch launch (H % 8 != 0): no BatchNormalization for either
    dp = _desc(engine, "patch")
    rc, pp = _plan(engine, dp, F32)
    assert rc == 0 and NAMES[pp.main.family] == "patch" and pp.bn_in == 0 and engine.conv2d_caps(dp).bn_in == 0
    # the up-sampling convolution itself (64 -> 32 on a 16 x 32 grid): plan and capability query agree that it is covered
    du = engine.conv_desc((1, 16, 32, 64), 32, 3, 3, 1, 1, "same")
    rc, pu = _plan(engine, du, F32 | _lib.SG_X_UP2)
    assert rc == 0 and NAMES[pu.main.family] == "patch" and pu.up2 == 1 and engine.conv2d_caps(du).up2 == 1
    # what the entry point refuses outright, the query answers all-zero with the same code
    rc, bad = _plan(engine, d, F32 | _lib.SG_HEAD_F32)
    assert rc == EINVAL and bad.main.family == 0 and bad.ws_bytes == 0
