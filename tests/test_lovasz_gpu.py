"""sg_loss_lovasz_* on the GPU against the numpy reference (tests/_lovasz_ref.py): every operand between guard bands
(tests/_guarded.py), outputs NaN-prefilled, the workspace exactly as long as the header's formula says, at the 16-byte aligned
start and ONE ELEMENT further.

Tolerances.  The reduced scalars: TOL_RED = 1e-4 of |ref| (the suite's).  g and dp: TOL = 2e-5 of max |ref| through `close`, AND
element by element |got - ref| <= 8 * 2^-24 * |ref|: g_k is one fp32 rounding of a double followed by at most three fp32
multiplies (1 / (images n_c), lovasz_weight * grad_scale, their product with g), eight ulp is twice that.  Neighbouring ranks
differ by at least 1 / U > 7e-6 relative at these row counts, so a pixel placed one rank off fails.  An element whose reference
is 0 must be +0.0f to the bit.
With a pointwise term, dp = pg + s * g where pg is the pointwise gradient.  pg's own fp32 expression (logf of p + 1e-7 next
to p = 1) is no eight-ulp quantity against float64 - tests/test_multiclass_gpu.py holds it at TOL - so there the element-wise
bound is taken against pg AS sg_lossn_bwd WRITES IT (same grad_scale * point_weight, the same bits by contract) plus the
float64 Lovasz part: |dp - (pg + s g_ref)| <= 8 * 2^-24 * (|pg| + |s g_ref|).  `close` still holds dp to the all-float64
reference at TOL."""
import ctypes as C_
import zlib

import numpy as np
import pytest
import torch

import _lovasz_ref as LR
import _multiclass_ref as MR
from _guarded import Guarded, assert_written, check_all, close, untouched

pytestmark = pytest.mark.gpu

SG_EINVAL, SG_EWORKSPACE = -1, -2
DEV = "cuda"
F32 = torch.float32
TOL, TOL_RED = 2e-5, 1e-4
ULP8 = 8 * 2.0 ** -24
T = 2048                                # SG_SORT_TILE
OFFS = [pytest.param(False, id="aligned"), pytest.param(True, id="offset")]
ROWS = (1, 63, 64, 65, 257, 2049, 70001)


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) % (2 ** 31))


def G(t, off=False):
    return Guarded(t, DEV, off=off)


def GO(shape, off=False, dtype=F32):
    return Guarded.out(shape, dtype, DEV, off=off)


def alpha_for(C):
    return tuple(round(0.35 + 0.3 * c / (C - 1), 4) for c in range(C))


def f32(v):
    return float(np.float32(v))


def c_desc(C, y_cols, images, n, all_=False, kind=-1, pw=0.0, lw=1.0, alpha=None):
    from building_detection_amd._lib import LovaszDesc
    d = LovaszDesc(C=C, y_cols=y_cols, images=images, classes_all=int(all_), rows_per_image=n, point_kind=kind, reserved=0,
                   point_weight=pw, lovasz_weight=lw)
    for c in range(min(C, len(d.point_alpha))):
        d.point_alpha[c] = 1.0 if alpha is None else alpha[c]
    return d


def ws_formula(C, images, n):
    """include/segengine.h: 4 * (4 N + S * 256 * (tiles + 1) + 3 * S * tiles + 3 * S + sg_loss_parts)."""
    S, tiles, rows = images * C, -(-n // T), images * n
    parts = min(max(-(-rows // 1024), 1), 2048)
    return 4 * (4 * rows * C + S * 256 * (tiles + 1) + 3 * S * tiles + 3 * S + parts)


def ws_bytes(engine, cd):
    return engine.lib.sg_loss_lovasz_ws_bytes(engine.h, C_.byref(cd))


def fwd(engine, cd, P, Y, L, GR, W, nws):
    return engine.lib.sg_loss_lovasz_fwd(engine.h, engine.stream, C_.byref(cd), P.ptr(), Y.ptr(), L.ptr(), GR.ptr(), W.ptr(), nws)


def bwd(engine, cd, P, Y, GR, D, scale):
    return engine.lib.sg_loss_lovasz_bwd(engine.h, engine.stream, C_.byref(cd), P.ptr(), Y.ptr(), GR.ptr(), D.ptr(), scale)


def done(engine, rc, what, *ops):
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    check_all(ops, what)


def bits(t):
    return t.contiguous().view(torch.int32)


def elementwise(got, ref, what, slack=None):
    """|got - ref| <= 8 * 2^-24 * |ref| (or * slack) at every element; ref == 0 -> +0.0f to the bit."""
    got64, ref = got.double().numpy(), np.asarray(ref, np.float64)
    bound = ULP8 * (np.abs(ref) if slack is None else slack)
    err = np.abs(got64 - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"{what}: worst element at {worst * 8:.2f} ulp of the 8 allowed")
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements beyond 8 ulp, worst {worst * 8:.1f} ulp"
    if slack is None:
        zero = torch.from_numpy(ref == 0)
        assert (bits(got)[zero] == 0).all(), f"{what}: an element whose reference is 0 is not +0.0f"


def check(engine, p, yt, images=1, all_=False, kind=-1, pw=0.0, lw=1.0, alpha=None, off=False, scales=(1.0, 0.25), tag=""):
    """Both calls on one input: the three scalars, g and dp against the reference, the bands, and a second call's bits."""
    rows, C = p.shape
    y_cols, n = yt.shape[1], rows // images
    what = f"lovasz rows={rows} C={C} y_cols={y_cols} images={images} all={all_} kind={kind} pw={pw} lw={lw} off={off} {tag}"
    pw, lw = f32(pw), f32(lw)
    al = None if alpha is None else tuple(f32(a) for a in alpha)
    cd = c_desc(C, y_cols, images, n, all_, kind, pw, lw, al)
    nws = ws_bytes(engine, cd)
    assert nws == ws_formula(C, images, n), what
    P, Y = G(p, off), G(yt, off)
    L, GR, W = GO((3,), off), GO((rows, C), off), Guarded.ws(nws, DEV)
    done(engine, fwd(engine, cd, P, Y, L, GR, W, nws), what, P, Y, L, GR, W)
    ref = LR.lovasz_ref(p.numpy(), yt.numpy(), images, all_)
    lp = MR.loss_ref(kind, p.double(), yt.double(), al).item() if kind >= 0 else 0.0
    out, g = L.read(), GR.read()
    assert_written(g, what + " g")
    print(f"{what}: L_lovasz {out[2].item():.7f} ref {ref['loss']:.7f}; L_point {out[1].item():.7f} ref {lp:.7f}")
    if np.isnan(ref["loss"]):
        assert torch.isnan(out[0]) and torch.isnan(out[2]), what + ": the NaN does not show in L"
    else:
        close(out, torch.tensor([pw * lp + lw * ref["loss"], lp, ref["loss"]], dtype=torch.float64), TOL_RED, what + " {L, Lp, Ll}")
        close(out[2:], torch.tensor([ref["loss"]], dtype=torch.float64), TOL_RED, what + " L_lovasz")
        if kind >= 0:
            close(out[1:2], torch.tensor([lp], dtype=torch.float64), TOL_RED, what + " L_point")
        else:
            assert out[1].item() == 0.0
    close(g, torch.from_numpy(ref["g"]), TOL, what + " g")
    elementwise(g, ref["g"], what + " g")
    L2, GR2, W2 = GO((3,), off), GO((rows, C), off), Guarded.ws(nws, DEV)
    done(engine, fwd(engine, cd, P, Y, L2, GR2, W2, nws), what + " again", L2, GR2, W2)
    assert torch.equal(bits(L2.read()), bits(out)) and torch.equal(bits(GR2.read()), bits(g)), what + ": the forward call is not reproducible"
    GI = G(g, off)
    for gs in scales:
        D = GO((rows, C), off)
        done(engine, bwd(engine, cd, P, Y, GI, D, gs), what + " bwd", P, Y, GI, D)
        dp = D.read()
        assert_written(dp, what + " bwd")
        sl = float(np.float32(gs) * np.float32(lw))
        if kind < 0:
            close(dp, torch.from_numpy(sl * ref["g"]), TOL, what + f" dp scale={gs}")
            elementwise(dp, sl * ref["g"], what + f" dp scale={gs}")
        else:
            spw = float(np.float32(gs) * np.float32(pw))
            full = MR.loss_bwd_ref(kind, p.double(), yt.double(), al, spw) + torch.from_numpy(sl * ref["g"])
            close(dp, full, TOL, what + f" dp scale={gs}")
            DN = GO((rows, C), off)
            a = None if al is None else (C_.c_float * C)(*al)
            rc = engine.lib.sg_lossn_bwd(engine.h, engine.stream, kind, rows, C, y_cols, a, P.ptr(), Y.ptr(), DN.ptr(), spw)
            done(engine, rc, what + " lossn_bwd", DN)
            pg = DN.read().double().numpy()
            elementwise(dp, pg + sl * ref["g"], what + f" dp scale={gs} (pointwise part as sg_lossn_bwd writes it)",
                        slack=np.abs(pg) + np.abs(sl * ref["g"]))
            # ... and the Lovasz part alone: dp - pg (exact in float64) against s g_ref at the issue's 8 ulp of |s g_ref|, plus the one
            # rounding of the sum, an ulp (2^-23) of |dp|.  Where s g_ref is 0 this asks dp == pg.
            part, want = dp.double().numpy() - pg, sl * ref["g"]
            over = np.abs(part - want) - (ULP8 * np.abs(want) + 2.0 ** -23 * np.abs(dp.double().numpy()))
            print(f"{what} dp - pg scale={gs}: worst excess {over.max():.3e} (<= 0 passes)")
            assert (over <= 0).all(), f"{what}: the Lovasz part of dp is off at {int((over > 0).sum())} elements, worst by {over.max():.3e}"
        D2 = GO((rows, C), off)
        done(engine, bwd(engine, cd, P, Y, GI, D2, gs), what + " bwd again", D2)
        assert torch.equal(bits(D2.read()), bits(dp)), what + ": the backward call is not reproducible"
    return ref, out, g


# ================================================================================================ inputs
def labels_from(t, C, y_cols, g):
    yt = torch.zeros(len(t), y_cols)
    yt[torch.arange(len(t)), t] = 1.0
    if y_cols == 2 * C:
        yt[:, C:] = torch.rand(len(t), C, generator=g) * 1.5 + 0.25
    return yt.contiguous()


def inputs(name, g, rows, C, y_cols, images=1):
    """(p, y_true) of one of the issue's input sets."""
    p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, y_cols)
    t = yt[:, :C].argmax(1)
    if name == "random":
        return p, yt
    if name == "quantised":                                       # multiples of 1/8: heavy ties, the stable order decides g
        return (torch.round(p * 8) / 8).contiguous(), yt
    if name == "absent":                                          # the last class occurs nowhere
        return p, labels_from(torch.where(t == C - 1, torch.zeros_like(t), t), C, y_cols, g)
    if name == "absent_in_one_image":                             # ... or not in the first image only
        n = rows // images
        t2 = t.clone()
        t2[:n] = torch.where(t[:n] == C - 1, torch.zeros_like(t[:n]), t[:n])
        t2[-1] = C - 1
        return p, labels_from(t2, C, y_cols, g)
    if name == "one_class":
        return p, labels_from(torch.full_like(t, C - 1), C, y_cols, g)
    if name == "zero_and_one":                                    # certain rows, right and wrong
        p = p.clone()
        for j in range(0, rows, 3):
            p[j] = 0.0
            p[j, (t[j] + (j // 3) % 2) % C] = 1.0
        return p, yt
    assert name == "nan_row"
    p = p.clone()
    p[rows // 2, t[rows // 2]] = float("nan")
    return p, yt


INPUTS = ("random", "quantised", "absent", "absent_in_one_image", "one_class", "zero_and_one", "nan_row")


# ================================================================================================ loss and gradient
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", (2, 3, 5, 11, 32))   # 11: the bounded C <= 16 form of the kernels
def test_loss_and_gradient(engine, C, off):
    for j, rows in enumerate(ROWS):
        if C == 32 and rows > 2049:
            continue
        for images in ((1, 3) if rows <= 257 else (1,)):
            kind = (-1, 0, 1, 2)[(j + images) % 4]
            y_cols = 2 * C if kind == 2 or (rows + images) % 2 else C
            g = gen(f"lg{rows}{C}{images}")
            p, yt = inputs("random", g, rows * images, C, y_cols)
            alpha = alpha_for(C) if kind > 0 else None
            pw, lw = (0.0, 1.0) if kind < 0 else (0.75, 0.5)
            check(engine, p, yt, images, all_=bool(j % 2), kind=kind, pw=pw, lw=lw, alpha=alpha, off=off,
                  scales=(1.0, 0.25) if rows <= 2049 else (0.25,))


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("name", INPUTS)
def test_input_sets(engine, name, off):
    for rows, C, images in ((65, 2, 1), (257, 3, 3), (2049, 5, 1), (T + 1, 3, 1), (63, 32, 3)):
        for all_ in (False, True):
            g = gen(f"{name}{rows}{C}{images}")
            y_cols = 2 * C if rows % 2 and C != 3 else C
            p, yt = inputs(name, g, rows * images, C, y_cols, images)
            kind = 2 if y_cols == 2 * C and name != "nan_row" else -1      # a NaN pointwise gradient is sg_lossn_bwd's business
            ref, out, _ = check(engine, p, yt, images, all_, kind=kind, pw=1.0 if kind >= 0 else 0.0, lw=1.0,
                                alpha=alpha_for(C) if kind > 0 else None, off=off, scales=(0.5,), tag=name)
            # (at 63 rows and 32 classes other classes are missing from an image as well: the counts are the reference's)
            assert (ref["n_c"] == (C if all_ else ref["used"].sum(1))).all() and (ref["n_c"] >= 1).all()
            if name == "absent":
                assert not ref["used"][:, C - 1].any() or all_
            if name == "absent_in_one_image" and images > 1 and not all_:
                assert not ref["used"][0, C - 1] and ref["used"][-1, C - 1]
            if name == "one_class":
                assert (ref["n_c"] == (C if all_ else 1)).all()
            if name == "nan_row":
                assert np.isnan(ref["loss"])
            if name == "quantised":
                assert len(np.unique(p.numpy())) <= 9


@pytest.mark.parametrize("C", (2, 5))
def test_all_against_present_on_an_absent_class(engine, C):
    """G = 0 under "all": g_1 = 1, so the class adds its largest probability, and n_c is C instead of C - 1."""
    rows = 2049
    g = gen(f"ap{C}")
    p, yt = inputs("absent", g, rows, C, C)
    r0, o0, g0 = check(engine, p, yt, 1, False, scales=(1.0,))
    r1, o1, g1 = check(engine, p, yt, 1, True, scales=(1.0,))
    extra = float(p[:, C - 1].max())
    close(o1[2:], torch.tensor([(o0[2].item() * (C - 1) + extra) / C], dtype=torch.float64), TOL_RED, "all against present")
    assert (bits(g0[:, C - 1]) == 0).all() and int((g1[:, C - 1] != 0).sum()) == 1
    assert g1[int(p[:, C - 1].argmax()), C - 1].item() == f32(1.0 / C)


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", (2, 3, 11, 32))
def test_lovasz_weight_zero_gives_the_bits_of_lossn_bwd(engine, C, off):
    for rows, y_cols in ((257, 2 * C), (2049, C)):
        g = gen(f"zero{rows}{C}")
        p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, y_cols)
        P, Y = G(p, off), G(yt, off)
        alpha = alpha_for(C)
        al = (C_.c_float * C)(*alpha)
        for kind in ((0, 1, 2) if y_cols == 2 * C else (0, 1)):
            cd = c_desc(C, y_cols, 1, rows, False, kind, 1.0, 0.0, alpha)
            nws = ws_bytes(engine, cd)
            L, GR, W = GO((3,), off), GO((rows, C), off), Guarded.ws(nws, DEV)
            done(engine, fwd(engine, cd, P, Y, L, GR, W, nws), "fwd", L, GR, W)
            GI = G(GR.read(), off)
            for gs in (1.0, 0.5):
                D, Dn = GO((rows, C), off), GO((rows, C), off)
                done(engine, bwd(engine, cd, P, Y, GI, D, gs), "bwd", D, GI)
                rc = engine.lib.sg_lossn_bwd(engine.h, engine.stream, kind, rows, C, y_cols, al, P.ptr(), Y.ptr(), Dn.ptr(), gs)
                done(engine, rc, "lossn_bwd", Dn)
                assert torch.equal(bits(D.read()), bits(Dn.read())), f"C={C} rows={rows} kind={kind} scale={gs}: not the bits of sg_lossn_bwd"
            out = L.read()
            assert bits(out[0:1]).item() == bits(out[1:2]).item()          # L = 1 * L_point + 0 * L_lovasz


# ================================================================================================ refusals
def test_refusals_write_nothing(engine):
    C, n, images = 3, 65, 2
    rows = n * images
    g = gen("refuse")
    p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, 2 * C)
    nan, inf = float("nan"), float("inf")
    bad = [("C=1", dict(C=1)), ("C=33", dict(C=33)), ("C=0", dict(C=0)), ("y_cols", dict(y_cols=4)), ("edge without weights", dict(y_cols=3)),
           ("images=0", dict(images=0)), ("images<0", dict(images=-1)), ("images=65536", dict(images=65536)),
           ("classes_all=2", dict(classes_all=2)), ("classes_all=-1", dict(classes_all=-1)),
           ("n=0", dict(rows_per_image=0)), ("n<0", dict(rows_per_image=-5)), ("rows*C=2^31", dict(rows_per_image=2 ** 31 // 6 + 1)),
           ("rows=2^31", dict(rows_per_image=2 ** 30)), ("kind=3", dict(point_kind=3)), ("kind=-2", dict(point_kind=-2)),
           ("reserved", dict(reserved=1)), ("pw<0", dict(point_weight=-0.5)), ("pw nan", dict(point_weight=nan)),
           ("pw inf", dict(point_weight=inf)), ("lw<0", dict(lovasz_weight=-1.0)), ("lw nan", dict(lovasz_weight=nan)),
           ("lw inf", dict(lovasz_weight=inf)), ("both 0", dict(point_weight=0.0, lovasz_weight=0.0)),
           ("lw=0 without a pointwise term", dict(point_kind=-1, lovasz_weight=0.0)),
           ("alpha inf", dict(alpha=(0.5, inf, 0.5))), ("alpha nan", dict(alpha=(nan, 0.5, 0.5)))]
    P, Y = G(p), G(yt)
    good = c_desc(C, 2 * C, images, n, True, 2, 1.0, 0.5, alpha_for(C))
    nws = ws_bytes(engine, good)
    assert nws == ws_formula(C, images, n)
    L, GR, W, D = GO((3,)), GO((rows, C)), Guarded.ws(nws, DEV), GO((rows, C))
    GI = G(torch.zeros(rows, C))
    for name, kw in bad:
        cd = c_desc(C, 2 * C, images, n, True, 2, 1.0, 0.5, kw.pop("alpha", alpha_for(C)))
        for k, v in kw.items():
            setattr(cd, k, v)
        assert ws_bytes(engine, cd) == 0, name
        assert fwd(engine, cd, P, Y, L, GR, W, nws) == SG_EINVAL, name
        assert bwd(engine, cd, P, Y, GI, D, 1.0) == SG_EINVAL, name
    null = type("Null", (), {"ptr": staticmethod(lambda: None)})
    for i in range(5):                                                        # a null pointer in every position
        ops = [P, Y, L, GR, W]
        ops[i] = null
        assert fwd(engine, good, *ops, nws) == (SG_EWORKSPACE if i == 4 else SG_EINVAL), i
    for i in range(4):
        ops = [P, Y, GI, D]
        ops[i] = null
        assert bwd(engine, good, *ops, 1.0) == SG_EINVAL, i
    assert engine.lib.sg_loss_lovasz_fwd(engine.h, engine.stream, None, P.ptr(), Y.ptr(), L.ptr(), GR.ptr(), W.ptr(), nws) == SG_EINVAL
    assert engine.lib.sg_loss_lovasz_bwd(engine.h, engine.stream, None, P.ptr(), Y.ptr(), GI.ptr(), D.ptr(), 1.0) == SG_EINVAL
    assert engine.lib.sg_loss_lovasz_ws_bytes(engine.h, None) == 0
    assert fwd(engine, good, P, Y, L, GR, W, nws - 1) == SG_EWORKSPACE         # one byte short
    torch.cuda.synchronize()
    for o in (L, GR, W, D):
        untouched(o, "refusals")
    check_all((P, Y, GI), "refusals")
    # ... and the same operands are taken once the descriptor is right
    done(engine, fwd(engine, good, P, Y, L, GR, W, nws), "good", P, Y, L, GR, W)
    ref = LR.lovasz_ref(p.numpy(), yt.numpy(), images, True)
    close(L.read()[2:], torch.tensor([ref["loss"]], dtype=torch.float64), TOL_RED, "good")
    elementwise(GR.read(), ref["g"], "good g")


# ================================================================================================ wrappers
def test_engine_wrappers(engine):
    from building_detection_amd import losses as LS
    C, n, hw = 3, 2, 33
    g = gen("wrap")
    rows = n * hw * hw
    p, yt = MR.class_probs(g, rows, C).reshape(n, hw, hw, C), MR.class_labels(g, rows, C, 2 * C).reshape(n, hw, hw, 2 * C)
    pd, yd = p.to(DEV), yt.to(DEV)
    for loss in (LS.lovasz_loss, LS.lovasz_loss.with_options("all", True),
                 LS.compound(LS.edge_focal_loss.with_alpha(alpha_for(C)), LS.lovasz_loss.with_options(per_image=True), 0.5, 2.0)):
        r = LS.resolve_lovasz(loss, C)
        out, gl = engine.loss_lovasz_fwd(r, pd, yd)
        dp = engine.loss_lovasz_bwd(r, pd, yd, gl, 0.5)
        assert tuple(out.shape) == (3,) and tuple(gl.shape) == (rows, C) and dp.shape == pd.shape
        images = n if r["per_image"] else 1
        ref = LR.lovasz_ref(p.reshape(-1, C).numpy(), yt.reshape(-1, 2 * C).numpy(), images, r["classes_all"])
        al = None if r["point_alpha"] is None else tuple(f32(a) for a in r["point_alpha"])
        lp = MR.loss_ref(r["point_kind"], p.reshape(-1, C).double(), yt.reshape(-1, 2 * C).double(), al).item() if r["point_kind"] >= 0 else 0.0
        close(out, torch.tensor([r["point_weight"] * lp + r["lovasz_weight"] * ref["loss"], lp, ref["loss"]], dtype=torch.float64),
              TOL_RED, "wrapper loss")
        elementwise(gl.cpu(), ref["g"], "wrapper g")
        full = torch.from_numpy(0.5 * r["lovasz_weight"] * ref["g"])
        if r["point_kind"] >= 0:
            full = full + MR.loss_bwd_ref(r["point_kind"], p.reshape(-1, C).double(), yt.reshape(-1, 2 * C).double(), al, 0.5 * r["point_weight"])
        close(dp.reshape(-1, C), full, TOL, "wrapper dp")
        for wrong in (gl[:-1], gl.double(), gl.reshape(-1), gl.cpu(), gl.t(), None):
            with pytest.raises(ValueError, match="g "):
                engine.loss_lovasz_bwd(r, pd, yd, wrong)


# ================================================================================================ inside a model
def build(C):
    from building_detection_amd import zoo
    return zoo.BUILDERS["hrnet"]((32, 32, 3), C)


@pytest.mark.parametrize("C", (2, 3))
def test_lovasz_loss_in_a_model_eager_and_captured(engine, C):
    from building_detection_amd import losses as LS
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.runtime import GraphedTrainStep
    alpha = (0.35, 0.65) if C == 2 else alpha_for(C)
    point = LS.edge_focal_loss if C == 2 else LS.edge_focal_loss.with_alpha(alpha)
    loss = LS.compound(point, LS.lovasz_loss)
    metrics = [LS.PA, LS.IoU, LS.MIoU, LS.F1_score]
    ma, mb = build(C), build(C)
    mb.set_weights(ma.get_weights())
    ma.compile(optimizer="adam", loss=loss, metrics=metrics)
    mb.compile(optimizer="adam", loss=loss, metrics=metrics, jit_compile=True)
    assert ma.last_loss_terms() is None
    x, y = synthetic_batch(2, 32, 32, seed=41, num_classes=C)
    logs = ma.test_on_batch(x, y)
    p = torch.from_numpy(ma.predict(x)).reshape(-1, C)
    yt = torch.from_numpy(y).reshape(-1, 2 * C).float()
    al = tuple(f32(a) for a in alpha)
    ref = LR.lovasz_ref(p.numpy(), yt.numpy())
    lp = MR.loss_ref(2, p.double(), yt.double(), al).item()
    terms = ma.last_loss_terms()
    print(f"C={C}: test_on_batch loss {logs['loss']:.7f}, float64 on predict's probabilities {lp + ref['loss']:.7f}; {terms}")
    close(torch.tensor([logs["loss"]]), torch.tensor([lp + ref["loss"]], dtype=torch.float64), TOL_RED, "test_on_batch loss")
    assert set(terms) == {"loss", "pointwise", "lovasz"} and terms["loss"] == logs["loss"]
    close(torch.tensor([terms["pointwise"], terms["lovasz"]]), torch.tensor([lp, ref["loss"]], dtype=torch.float64), TOL_RED, "terms")
    assert set(logs) == {"loss", "PA", "IoU", "MIoU", "F1_score"}
    # the plain pointwise loss on the same weights reports another loss and no terms
    md = build(C)
    md.set_weights(ma.get_weights())
    md.compile(optimizer="adam", loss=point)
    l0 = md.test_on_batch(x, y)["loss"]
    close(torch.tensor([l0]), torch.tensor([lp], dtype=torch.float64), TOL_RED, "the plain loss is the pointwise term")
    assert l0 != logs["loss"] and md.last_loss_terms() is None
    for i in range(5):
        x, y = synthetic_batch(2, 32, 32, seed=80 + i, num_classes=C)
        (la, ca), (lb, cb) = ma.train_on_batch(x, y, return_device_scalars=True), mb.train_on_batch(x, y, return_device_scalars=True)
        assert la.numel() == 1 and torch.equal(la, lb) and torch.equal(ca, cb), (i, la, lb, ca, cb)     # steps 3 and 4 are replays
        ta, tb = ma.last_loss_terms(), mb.last_loss_terms()
        assert ta == tb and ta["loss"] == la.item() and ta["lovasz"] > 0 and ta["pointwise"] > 0, (i, ta, tb)
        assert ma._logs(la, ca) == mb._logs(lb, cb) and np.isfinite(la.item())
    # a test_on_batch between replays leaves ITS terms; the next replay gives the model back the graph's own
    xv, yv = synthetic_batch(2, 32, 32, seed=70, num_classes=C)
    va, vb = ma.test_on_batch(xv, yv), mb.test_on_batch(xv, yv)
    assert va == vb and ma.last_loss_terms() == mb.last_loss_terms() and mb.last_loss_terms()["loss"] == vb["loss"]
    x, y = synthetic_batch(2, 32, 32, seed=71, num_classes=C)
    (la, ca), (lb, cb) = ma.train_on_batch(x, y, return_device_scalars=True), mb.train_on_batch(x, y, return_device_scalars=True)
    ta, tb = ma.last_loss_terms(), mb.last_loss_terms()
    assert torch.equal(la, lb) and ta == tb and tb["loss"] == lb.item() and tb["loss"] != vb["loss"], (ta, tb, vb)
    # a second captured shape (one image): its graph's terms after its steps, the first graph's again after a step of the first
    for i in range(4):
        x1, y1 = synthetic_batch(1, 32, 32, seed=75 + i, num_classes=C)
        (la, ca), (lb, cb) = ma.train_on_batch(x1, y1, return_device_scalars=True), mb.train_on_batch(x1, y1, return_device_scalars=True)
        ta, tb = ma.last_loss_terms(), mb.last_loss_terms()
        assert torch.equal(la, lb) and ta == tb and tb["loss"] == lb.item(), (i, ta, tb)
    assert len(mb._train_graphs) == 2
    x, y = synthetic_batch(2, 32, 32, seed=79, num_classes=C)
    (la, ca), (lb, cb) = ma.train_on_batch(x, y, return_device_scalars=True), mb.train_on_batch(x, y, return_device_scalars=True)
    ta, tb = ma.last_loss_terms(), mb.last_loss_terms()
    assert torch.equal(la, lb) and ta == tb and tb["loss"] == lb.item(), (ta, tb)
    # four more steps with no host read in between: the replays queue up behind one another
    queued = []
    for m in (ma, mb):
        for i in range(4):
            x, y = synthetic_batch(2, 32, 32, seed=90 + i, num_classes=C)
            last = m.train_on_batch(x, y, return_device_scalars=True)
        queued.append((last[0].clone(), last[1].clone(), m.last_loss_terms()))
    (la, ca, ta), (lb, cb, tb) = queued
    assert torch.equal(la, lb) and torch.equal(ca, cb) and ta == tb, (la, lb, ta, tb)
    assert len(mb._train_graphs) == 2 and all(isinstance(s, GraphedTrainStep) for s in mb._train_graphs.values())
    for s in mb._train_graphs.values():   # each graph keeps the state of ITS forward call: g [rows, C] and the three terms
        rows = s.y.numel() // s.y.shape[-1]
        g, terms = s.loss_state.carry, s.loss_state.terms
        assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (rows, C) and g.is_contiguous()
        assert terms.is_cuda and terms.dtype == torch.float32 and tuple(terms.shape) == (3,)
    assert not getattr(ma, "_train_graphs", None)
    for wa, wb in zip(ma.get_weights(), mb.get_weights()):
        assert np.array_equal(wa, wb)
    assert any(not np.array_equal(w0, w1) for w0, w1 in zip(build(C).get_weights(), ma.get_weights()))
