"""sg_gn_fwd / sg_gn_bwd (csrc/groupnorm.hip) against plain float64 (tests/_groupnorm_ref.py), through the C ABI itself.

Every operand sits between NaN guard bands (tests/_guarded.py), outputs are prefilled with NaN, the workspace has exactly
sg_gn_ws_bytes bytes.  Tolerances, all as max|got - ref| <= tol * max|ref|: 2e-5 fp32 element-wise (y), 1e-4 for results of
reductions (mean, invstd, dx, dgamma, dbeta), 2^-7 for bf16-stored results; y gets on top what BatchNormalization's forward test
gives for save_mean being an fp32 number, |gamma| invstd ulp32(mean) / 2.  A group of zero variance has invstd = 1 / sqrt(eps),
thirty times everyone else's: it is compared on its own scale.  bf16 references start from the bf16-rounded inputs.

The shapes (N, HW, C, G), and why:
  (2, 25, 12, 3)                      Cg = 4: a group is one 16-byte chunk
  (2, 25, 12, 4)                      Cg = 3: groups straddle chunks
  (3, 25, 12, 1), (3, 25, 12, 12)     layer / instance normalisation
  (2, 9, 26, 2)                       Cg = 13, C % 4 != 0: the scalar form
  (2, 9, 7, 7) one element off        unaligned tensors: the scalar form
  (2, 9, 16, 2), (2, 9, 12, 3)        bf16: 8 channels per lane, and C % 8 != 0 (4 per lane)
  (1, 1, 16, 2), (4, 1, 8, 8)         HW = 1 (behind Dense); the latter has zero variance everywhere: y = beta, dx = 0
  (2, 2100, 8, 2), (2, 2101, 8, 2)    the reducer splits the rows over a few slabs; 2101: the last slab is short
  (2, 16400, 8, 2)                    32 slabs and more (fp32), the last one short
  (2, 25, 12, 4) without gamma, beta  scale=False, center=False"""
import ctypes as CT

import pytest
import torch

import _groupnorm_ref as R
from _guarded import Guarded, assert_written, regime, seg_plan, short_last_slab, ulp32, untouched
from building_detection_amd._lib import SegPlan
from test_bandwidth_variants_gpu import BF16, DEV, F32, G, GO, call, done, gen, push, rnd, sgdt, tol

pytestmark = pytest.mark.gpu

SG_EINVAL = -1
EPS = R.EPS
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
CASES = [pytest.param(s, False, True, id="x".join(map(str, s))) for s in R.SHAPES if s != (2, 9, 7, 7)]
CASES.append(pytest.param((2, 9, 7, 7), True, True, id="2x9x7x7-offset"))
CASES.append(pytest.param((2, 25, 12, 4), False, False, id="2x25x12x4-noparams"))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def close_gn(got, ref, tol_, what, extra=None, apart=None):
    """|got - ref| <= tol * max|ref| + extra, the elements of `apart` (a bool mask) on their own max|ref|; prints the figure."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite values in the result"
    over = (got - ref).abs()
    if extra is not None:
        over = (over - extra.expand_as(over)).clamp_min(0.0)
    apart = torch.zeros_like(ref, dtype=torch.bool) if apart is None else apart.expand_as(ref)
    for sel, name in ((apart, "apart"), (~apart, "rest")):
        if sel.any():
            scale, err = ref[sel].abs().max().item(), over[sel].max().item()
            print(f"{what} [{name}]: max err {err:.3e}, scale {scale:.3e}, rel {err / max(scale, 1e-300):.2e} (tol {tol_:.1e})")
            assert err <= tol_ * scale, f"{what} [{name}]: max err {err:.3e} > {tol_:.3e} * {scale:.3e}"


def ws_bytes(engine, dtype, N, HW, C, Gr):
    return engine.lib.sg_gn_ws_bytes(engine.h, sgdt(dtype), N, HW, C, Gr)


class Inputs:
    pass


def make_inputs(shape, dtype, params=True, kind="plain", tag=""):
    """x (storage type, nothing on a fused ReLU's boundary), dy, fp32 gamma / beta, and the float64 statistics of the stored x."""
    N, HW, C, Gr = shape
    g = gen(f"gn{shape}.{dtype}.{params}.{kind}.{tag}")
    I = Inputs()
    I.shape, I.dtype = shape, dtype
    Cg = C // Gr
    if kind == "cancel":                       # 100 + U(-1, 1); the second group of every image constant
        x = 100.0 + rnd(g, N, HW, C)
        x[:, :, Cg:2 * Cg] = 100.25
    else:
        x = rnd(g, N, HW, C) * (0.5 + 1.5 * torch.rand(C, generator=g)) + rnd(g, C)
    I.gamma = ((rnd(g, C) + 1.5) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)).float() if params else None
    I.beta = push(rnd(g, C) * 0.5, 2.0 ** -7).float() if params else None
    g64 = None if I.gamma is None else I.gamma.double()
    b64 = None if I.beta is None else I.beta.double()
    x64, I.margin = R.off_boundary(x.to(dtype).double(), g64, b64, Gr, dtype)
    I.x = x64.to(dtype)
    assert torch.equal(I.x.double(), x64)
    I.x64, I.g64, I.b64 = x64, g64, b64
    I.dy = rnd(g, N, HW, C, dtype=dtype)
    I.mean, var = R.stats(x64, Gr)
    I.invstd = 1.0 / torch.sqrt(var + EPS)
    I.mean32, I.invstd32 = I.mean.float(), I.invstd.float()
    # the mask from the fp32-rounded statistics the backward is handed is the reference's mask
    t64 = R.affine(x64, g64, b64, I.mean, I.invstd, Gr)[0]
    t32 = R.affine(x64, g64, b64, I.mean32.double(), I.invstd32.double(), Gr)[0]
    assert torch.equal(t64 > 0, t32 > 0)
    I.const = (var == 0).repeat_interleave(Cg, dim=1).unsqueeze(1)     # [N][1][C]: channels of zero-variance groups
    return I


def run_fwd(engine, I, relu, off=False):
    N, HW, C, Gr = I.shape
    nws = ws_bytes(engine, I.dtype, N, HW, C, Gr)
    X = G(I.x, off)
    Gm = None if I.gamma is None else G(I.gamma, off)
    Bt = None if I.beta is None else G(I.beta, off)
    Y, SM, SI, W = GO((N, HW, C), I.dtype, off), GO((N, Gr), F32, off), GO((N, Gr), F32, off), Guarded.ws(nws, DEV)
    what = f"sg_gn_fwd {I.shape} {I.dtype} off={off} relu={relu}"
    rc = call(engine, "sg_gn_fwd", sgdt(I.dtype), N, HW, C, Gr, X.ptr(), Gm and Gm.ptr(), Bt and Bt.ptr(), Y.ptr(), SM.ptr(), SI.ptr(),
              EPS, relu, W.ptr(), nws)
    done(engine, rc, what, *[o for o in (X, Gm, Bt, Y, SM, SI, W) if o is not None])
    for o in (Y, SM, SI):
        assert_written(o.read(), what)
    return Y.read(), SM.read(), SI.read(), what


def run_bwd(engine, I, relu, off=False):
    N, HW, C, Gr = I.shape
    nws = ws_bytes(engine, I.dtype, N, HW, C, Gr)
    X, DY, SM, SI = G(I.x, off), G(I.dy, off), G(I.mean32, off), G(I.invstd32, off)
    Gm = None if I.gamma is None else G(I.gamma, off)
    Bt = None if I.beta is None else G(I.beta, off)
    DX, W = GO((N, HW, C), I.dtype, off), Guarded.ws(nws, DEV)
    DG = None if I.gamma is None else GO((C,), F32, off)
    DB = None if I.beta is None else GO((C,), F32, off)
    what = f"sg_gn_bwd {I.shape} {I.dtype} off={off} relu={relu}"
    rc = call(engine, "sg_gn_bwd", sgdt(I.dtype), N, HW, C, Gr, X.ptr(), DY.ptr(), Gm and Gm.ptr(), Bt and Bt.ptr(), SM.ptr(), SI.ptr(),
              DX.ptr(), DG and DG.ptr(), DB and DB.ptr(), relu, W.ptr(), nws)
    done(engine, rc, what, *[o for o in (X, DY, SM, SI, Gm, Bt, DX, DG, DB, W) if o is not None])
    for o in (DX, DG, DB):
        if o is not None:
            assert_written(o.read(), what)
    return DX.read(), None if DG is None else DG.read(), None if DB is None else DB.read(), what


def check_fwd(I, y, mean, invstd, relu, what):
    N, HW, C, Gr = I.shape
    yr, mr, ir = R.fwd(I.x64, I.g64, I.b64, Gr, EPS, relu=bool(relu))
    zero_var = I.const[:, 0, ::C // Gr]                                 # [N][G]
    close_gn(mean, mr, 1e-4, what + " mean")
    close_gn(invstd, ir, 1e-4, what + " invstd", apart=zero_var)
    gabs = torch.ones(C, dtype=torch.float64) if I.g64 is None else I.g64.abs()
    extra = gabs * (ir * ulp32(mr) / 2).repeat_interleave(C // Gr, dim=1).unsqueeze(1)      # [N][1][C]
    close_gn(y, yr, tol(I.dtype), what + " y", extra=extra)


def check_bwd(I, dx, dgamma, dbeta, relu, what):
    Gr = I.shape[3]
    dxr, dgr, dbr = R.bwd(I.x64, I.dy.double(), I.g64, I.b64, I.mean32.double(), I.invstd32.double(), Gr, relu=bool(relu))
    close_gn(dx, dxr, tol(I.dtype, True), what + " dx", apart=I.const)
    if dgamma is not None:
        close_gn(dgamma, dgr, 1e-4, what + " dgamma")
    if dbeta is not None:
        close_gn(dbeta, dbr, 1e-4, what + " dbeta")


# ================================================================================================ the table
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,off,params", CASES)
def test_forward_and_backward_against_float64(engine, shape, off, params, dtype):
    I = make_inputs(shape, dtype, params)
    ys, dxs = {}, {}
    for relu in (0, 1):
        y, mean, invstd, what = run_fwd(engine, I, relu, off)
        check_fwd(I, y, mean, invstd, relu, what)
        ys[relu] = y
        y2, mean2, invstd2, _ = run_fwd(engine, I, relu, off)          # a second launch: the same bits
        assert all(torch.equal(bits(a), bits(b)) for a, b in ((y, y2), (mean, mean2), (invstd, invstd2))), what
        dx, dg, db, what = run_bwd(engine, I, relu, off)
        check_bwd(I, dx, dg, db, relu, what)
        dx2, dg2, db2, _ = run_bwd(engine, I, relu, off)
        assert all(a is None or torch.equal(bits(a), bits(b)) for a, b in ((dx, dx2), (dg, dg2), (db, db2))), what
        dxs[relu] = dx
    # the fused ReLU is the ReLU of the unfused output, bit for bit
    assert torch.equal(bits(ys[1]), bits(torch.relu(ys[0].float()).to(dtype))), f"{shape}: relu = 1 is not relu(relu = 0)"
    if shape == (4, 1, 8, 8):     # zero variance everywhere: y = beta, dx = 0, all finite (the checks above saw no NaN)
        assert torch.equal(ys[0].float(), I.beta.to(dtype).float().expand(4, 1, 8))
        assert not dxs[0].float().any() and not dxs[1].float().any()


def test_row_split_regimes_are_the_ones_the_table_names(engine):
    """The three long shapes reach the reducer's "few" and "many" regimes on THIS device (sg_seg_plan, the plan the launches take),
    with a short last slab, so the table above cannot silently cover one regime only."""
    cus = engine.lib.sg_num_cus(engine.h)
    want = {2100: ("few", False), 2101: ("few", True), 16400: ("many", True)}
    for rows, (reg, short) in want.items():
        p = SegPlan()
        assert engine.lib.sg_seg_plan(engine.h, 2, 2, rows, 8, 1, 0, CT.byref(p)) == 0
        mirror = seg_plan(cus, rows, 8, True, nout=2)
        assert (p.V, p.TX, p.TY, p.gx, p.S) == tuple(mirror[k] for k in ("V", "TX", "TY", "gx", "S"))
        assert regime(p.S) == reg and short_last_slab(rows, p.S) == short, (rows, p.S)
        # the workspace: the partial rows of both images (the larger of the vector and the scalar plan), the per-(n, c) totals
        # and the per-(n, g) pair
        part = max(mirror["part_bytes"], seg_plan(cus, rows, 8, False, nout=2)["part_bytes"])
        assert ws_bytes(engine, F32, 2, rows, 8, 2) == 2 * part + 2 * 8 * 2 * 8 + 2 * 2 * 2 * 4


# ================================================================================================ further properties
@pytest.mark.parametrize("dtype", DTYPES)
def test_cancellation_and_a_constant_group(engine, dtype):
    """x = 100 + U(-1, 1): the per-channel pivot keeps the single-pass variance; one group of every image is constant."""
    I = make_inputs((2, 300, 12, 3), dtype, True, kind="cancel")
    assert I.const.any() and not I.const.all()
    for relu in (0, 1):
        y, mean, invstd, what = run_fwd(engine, I, relu)
        check_fwd(I, y, mean, invstd, relu, what + " cancel")
        dx, dg, db, what = run_bwd(engine, I, relu)
        check_bwd(I, dx, dg, db, relu, what + " cancel")


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_image_does_not_depend_on_its_batch(engine, dtype):
    """Image 0 of [a, b], of [a, c] and of [a] alone: identical bits in y and dx - what the layer exists for.  The shape splits the
    rows over several slabs, so the order of the partial sums is part of the claim."""
    shape = (2, 2101, 8, 2)
    A, B = make_inputs(shape, dtype, True, tag="ab"), make_inputs(shape, dtype, True, tag="ac")
    for I in (B,):                       # same first image, same parameters; everything else differs
        I.x = torch.cat([A.x[:1], I.x[1:]])
        I.dy = torch.cat([A.dy[:1], I.dy[1:]])
        I.gamma, I.beta = A.gamma, A.beta
        I.mean32, I.invstd32 = torch.cat([A.mean32[:1], I.mean32[1:]]), torch.cat([A.invstd32[:1], I.invstd32[1:]])
    S = Inputs()
    S.shape, S.dtype, S.gamma, S.beta = (1,) + shape[1:], dtype, A.gamma, A.beta
    S.x, S.dy, S.mean32, S.invstd32 = A.x[:1], A.dy[:1], A.mean32[:1], A.invstd32[:1]
    assert not torch.equal(A.x[1], B.x[1])
    for relu in (0, 1):
        ya, ma, ia, _ = run_fwd(engine, A, relu)
        dxa = run_bwd(engine, A, relu)[0]
        for I in (B, S):
            yb, mb, ib, what = run_fwd(engine, I, relu)
            dxb = run_bwd(engine, I, relu)[0]
            assert torch.equal(bits(ya[0]), bits(yb[0])) and torch.equal(bits(ma[0]), bits(mb[0])) and torch.equal(bits(ia[0]), bits(ib[0])), what
            assert torch.equal(bits(dxa[0]), bits(dxb[0])), what


@pytest.mark.parametrize("bad", [(2, 25, 12, 5), (2, 25, 12, 0), (2, 25, 12, -1), (0, 25, 12, 3)], ids=str)
def test_refused_inputs_write_nothing(engine, bad):
    N, HW, C, Gr = bad
    assert ws_bytes(engine, F32, N, HW, C, Gr) == 0
    n, g_ = max(N, 2), 4
    g = gen("gnrefuse")
    X, DY, Gm, Bt = G(rnd(g, n, HW, C)), G(rnd(g, n, HW, C)), G(rnd(g, C)), G(rnd(g, C))
    SM, SI = G(rnd(g, n, g_)), G(rnd(g, n, g_, lo=0.5, hi=2.0))
    Y, OM, OI, DX, DG, DB = GO((n, HW, C), F32), GO((n, g_), F32), GO((n, g_), F32), GO((n, HW, C), F32), GO((C,), F32), GO((C,), F32)
    W = Guarded.ws(1 << 16, DEV)
    rc = call(engine, "sg_gn_fwd", 0, N, HW, C, Gr, X.ptr(), Gm.ptr(), Bt.ptr(), Y.ptr(), OM.ptr(), OI.ptr(), EPS, 1, W.ptr(), 1 << 16)
    assert rc == SG_EINVAL, rc
    rc = call(engine, "sg_gn_bwd", 0, N, HW, C, Gr, X.ptr(), DY.ptr(), Gm.ptr(), Bt.ptr(), SM.ptr(), SI.ptr(), DX.ptr(), DG.ptr(), DB.ptr(),
              1, W.ptr(), 1 << 16)
    assert rc == SG_EINVAL, rc
    torch.cuda.synchronize()
    for o in (Y, OM, OI, DX, DG, DB, W):
        untouched(o, f"refused {bad}")


def test_a_short_workspace_is_refused(engine):
    N, HW, C, Gr = 2, 25, 12, 3
    nws = ws_bytes(engine, F32, N, HW, C, Gr)
    g = gen("gnshort")
    X, DY, SM, SI = G(rnd(g, N, HW, C)), G(rnd(g, N, HW, C)), G(rnd(g, N, Gr)), G(rnd(g, N, Gr))
    DX, W = GO((N, HW, C), F32), Guarded.ws(nws, DEV)
    rc = call(engine, "sg_gn_bwd", 0, N, HW, C, Gr, X.ptr(), DY.ptr(), None, None, SM.ptr(), SI.ptr(), DX.ptr(), None, None, 0, W.ptr(),
              nws - 1)
    assert rc == -2, rc
    torch.cuda.synchronize()
    untouched(DX, "short workspace")
    untouched(W, "short workspace")
