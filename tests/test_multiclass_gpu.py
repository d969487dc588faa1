"""The C-class head on the GPU: sg_softmax_*, sg_lossn_*, sg_confusion_matrix and sg_argmax_max_u8 against float64, every
operand between guard bands (tests/_guarded.py), outputs NaN-prefilled, at the 16-byte aligned start and ONE ELEMENT further
(a row is C floats: the kernels promise nothing beyond 4-byte alignment); their equality with the 2-class entry points at
C = 2; what they refuse; and whole models of 3, 4 and 5 classes against the CPU oracle (oracle/models.py takes num_classes).

Tolerances are those of tests/test_bandwidth_variants_gpu.py: 2e-5 of max|ref| for fp32 element-wise results, 1e-4 for the
reduced loss scalar, integers exact."""
import ctypes as C_
import zlib

import numpy as np
import pytest
import torch

import _fit_check as FC
import _multiclass_ref as R
from _guarded import Guarded, assert_written, check_all, close, untouched

pytestmark = pytest.mark.gpu

SG_F32, SG_EINVAL = 0, -1
DEV = "cuda"
F32 = torch.float32
TOL, TOL_RED = 2e-5, 1e-4
OFFS = [pytest.param(False, id="aligned"), pytest.param(True, id="offset")]
ROWS = (1, 63, 64, 65, 257, 4099)     # a wave less one / exactly one / one more; two blocks; 17 blocks with a ragged last one
EW_CAP = 8192 * 256                   # rows after which the grids of the softmax kernels and sg_lossn_bwd take a second trip
RED_CAP = 2048 * 1024                 # sg_lossn_fwd / sg_confusion_matrix: cdiv(rows, 256 * 4) workgroups, clamped to 2048 above this


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) % (2 ** 31))


def rnd(g, *shape, lo=-1.0, hi=1.0):
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).float()


def call(engine, name, *args):
    return getattr(engine.lib, name)(engine.h, engine.stream, *args)


def done(engine, rc, what, *ops):
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    check_all(ops, what)


def G(t, off=False, role="in"):
    return Guarded(t, DEV, off=off, role=role)


def GO(shape, dtype, off=False):
    return Guarded.out(shape, dtype, DEV, off=off)


def alpha_arg(alpha):
    return None if alpha is None else (C_.c_float * len(alpha))(*[float(a) for a in alpha])


# ================================================================================================ softmax
def _softmax_case(engine, rows, C, off, z=None, tag=""):
    g = gen(f"sm{rows}{C}{off}{tag}")
    if z is None:
        z = rnd(g, rows, C, lo=-4, hi=4)
    dp = rnd(g, rows, C)
    what = f"softmax rows={rows} C={C} off={off} {tag}"
    ref = R.softmax_ref(z.double())
    Z, P = G(z, off), GO((rows, C), F32, off)
    done(engine, call(engine, "sg_softmax_fwd", SG_F32, rows, C, Z.ptr(), P.ptr()), what, Z, P)
    p = P.read()
    assert_written(p, what)
    assert (p >= 0).all() and (p <= 1).all(), what
    close(p.double().sum(1), torch.ones(rows, dtype=torch.float64), TOL, what + " sum")
    close(p, ref, TOL, what)
    ZP = G(z, off, role="out")                       # in place: p == z
    done(engine, call(engine, "sg_softmax_fwd", SG_F32, rows, C, ZP.ptr(), ZP.ptr()), what + " in place", ZP)
    assert torch.equal(ZP.read(), p), what + ": the in-place result differs from the out-of-place one"
    Pi, DP, DZ = G(ref.float(), off), G(dp, off), GO((rows, C), F32, off)
    done(engine, call(engine, "sg_softmax_bwd", SG_F32, rows, C, Pi.ptr(), DP.ptr(), DZ.ptr()), what + " bwd", Pi, DP, DZ)
    dz = DZ.read()
    assert_written(dz, what + " bwd")
    close(dz, R.softmax_bwd_ref(ref.float().double(), dp.double()), TOL, what + " bwd")


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", (2, 3, 4, 5, 7, 8, 16, 21, 32))
def test_softmax(engine, C, off):
    for rows in ROWS:
        _softmax_case(engine, rows, C, off)


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", (3, 8, 21))
def test_softmax_equal_logits_and_a_spread_of_80(engine, C, off):
    rows = 257
    g = gen(f"smx{C}")
    z = rnd(g, rows, C, lo=-4, hi=4)
    z[::7] = 1.25                                     # rows of equal logits: p = 1 / C
    _softmax_case(engine, rows, C, off, z=z, tag="equal")
    z = rnd(g, rows, C, lo=-4, hi=4)
    z[torch.arange(rows), torch.arange(rows) % C] += 80.0      # exp(80) overflows fp32 without the max subtraction
    z[::5, 0] -= 80.0
    _softmax_case(engine, rows, C, off, z=z, tag="spread")


def test_softmax_wrapped_grid(engine):
    _softmax_case(engine, EW_CAP + 1027, 3, True, tag="wrap")


# ================================================================================================ loss
def _loss_case(engine, rows, C, y_cols, kinds, scales, off, p=None, yt=None, fwd=True, tag=""):
    g = gen(f"loss{rows}{C}{y_cols}{tag}")
    if p is None:
        p, yt = R.class_probs(g, rows, C), R.class_labels(g, rows, C, y_cols)
    alpha = [float(a) for a in (torch.rand(C, generator=g) * 1.5 + 0.1)]       # random positive class weights
    nws = engine.lib.sg_lossn_ws_bytes(engine.h, rows)
    for kind in kinds:
        what = f"lossn kind={kind} rows={rows} C={C} y_cols={y_cols} off={off} {tag}"
        al = alpha_arg(alpha)
        if fwd:
            P, Y, L, W = G(p, off), G(yt, off), GO((1,), F32, off), Guarded.ws(nws, DEV)
            rc = call(engine, "sg_lossn_fwd", kind, rows, C, y_cols, al, P.ptr(), Y.ptr(), L.ptr(), W.ptr(), nws)
            done(engine, rc, what, P, Y, L, W)
            ref = R.loss_ref(kind, p.double(), yt.double(), alpha).reshape(1)
            close(L.read(), ref, TOL_RED, what + " fwd")
            L2 = GO((1,), F32)
            done(engine, call(engine, "sg_lossn_fwd", kind, rows, C, y_cols, al, P.ptr(), Y.ptr(), L2.ptr(), W.ptr(), nws), what, L2)
            assert torch.equal(L.read(), L2.read()), what + ": the loss scalar is not reproducible"
        for gs in scales:
            P, Y, DP = G(p, off), G(yt, off), GO((rows, C), F32, off)
            done(engine, call(engine, "sg_lossn_bwd", kind, rows, C, y_cols, al, P.ptr(), Y.ptr(), DP.ptr(), gs), what, P, Y, DP)
            dp = DP.read()
            assert_written(dp, what)
            close(dp, R.loss_bwd_ref(kind, p.double(), yt.double(), alpha, gs), TOL, what + f" bwd scale={gs}")


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", (2, 3, 5, 8, 21))
def test_lossn(engine, C, off):
    for rows in ROWS:
        _loss_case(engine, rows, C, 2 * C, (0, 1, 2), (1.0, 0.25), off)
        _loss_case(engine, rows, C, C, (0, 1), (1.0, 0.25), off)


def test_lossn_without_weights_is_cross_entropy_with_ones(engine):
    rows, Cn = 257, 5
    g = gen("ce-null")
    p, yt = R.class_probs(g, rows, Cn), R.class_labels(g, rows, Cn, Cn)
    P, Y, L, W = G(p), G(yt), GO((1,), F32), Guarded.ws(engine.lib.sg_lossn_ws_bytes(engine.h, rows), DEV)
    done(engine, call(engine, "sg_lossn_fwd", 0, rows, Cn, Cn, None, P.ptr(), Y.ptr(), L.ptr(), W.ptr(), W.nb), "CE NULL", P, Y, L, W)
    close(L.read(), R.loss_ref(0, p.double(), yt.double()).reshape(1), TOL_RED, "CE with alpha = NULL")
    DP = GO((rows, Cn), F32)
    done(engine, call(engine, "sg_lossn_bwd", 0, rows, Cn, Cn, None, P.ptr(), Y.ptr(), DP.ptr(), 1.0), "CE NULL bwd", P, Y, DP)
    close(DP.read(), R.loss_bwd_ref(0, p.double(), yt.double(), None, 1.0), TOL, "CE with alpha = NULL, bwd")


@pytest.mark.parametrize("C", (2, 3, 5))
def test_lossn_at_probabilities_zero_and_one(engine, C):
    # p exactly one-hot, the label on the 1 and on a 0 in turn: log(0 + 1e-7), 1 / (0 + 1e-7) and (1 - 1)^2 stay finite
    rows = 64
    p = torch.zeros(rows, C)
    p[torch.arange(rows), torch.arange(rows) % C] = 1.0
    yt = R.class_labels(gen(f"edge{C}"), rows, C, 2 * C)
    t = (torch.arange(rows) // C) % C
    yt[:, :C] = torch.nn.functional.one_hot(t, C).float()
    assert ((p * yt[:, :C]).sum(1) == 1).any() and ((p * yt[:, :C]).sum(1) == 0).any()
    for off in (False, True):
        _loss_case(engine, rows, C, 2 * C, (0, 1, 2), (1.0, 0.25), off, p=p, yt=yt, tag="01")


def test_lossn_many_partial_blocks(engine):
    _loss_case(engine, 600001, 3, 6, (0, 1, 2), (1.0,), False, tag="parts")     # 586 partial sums (no clamp), a ragged last block


def test_lossn_wrapped_grids(engine):
    # sg_lossn_bwd's grid caps at 8192 blocks of 256 rows; sg_lossn_fwd's partial count at 2048 blocks of 1024 rows
    _loss_case(engine, EW_CAP + 1027, 3, 3, (1,), (0.25,), True, fwd=False, tag="wrap")
    rows = RED_CAP + 1027
    assert engine.lib.sg_lossn_ws_bytes(engine.h, rows) == 2048 * 4 + 256 == engine.lib.sg_lossn_ws_bytes(engine.h, RED_CAP)
    assert engine.lib.sg_lossn_ws_bytes(engine.h, RED_CAP - 1024) == 2047 * 4 + 256
    _loss_case(engine, rows, 3, 3, (1,), (), True, tag="cap")


# ================================================================================================ confusion matrix
def _confusion_inputs(rows, C, y_cols, tag):
    g = gen(f"conf{rows}{C}{y_cols}{tag}")
    p, yt = R.class_probs(g, rows, C), R.class_labels(g, rows, C, y_cols)
    r = torch.rand(rows, generator=g)
    a, b = torch.randint(0, C, (rows,), generator=g), torch.randint(0, C, (rows,), generator=g)
    tie = r < 0.15                                   # planted ties in p: two (or, a == b, one) entries share the maximum
    p[tie, a[tie]] = 2.0
    p[tie, b[tie]] = 2.0
    p[(r > 0.2) & (r < 0.25)] = 1.0 / C              # every class ties -> class 0
    ty = (r > 0.3) & (r < 0.45)                      # ... and in y_true: a second 1, all ones, all zeros
    yt[ty, a[ty]] = 1.0
    yt[(r > 0.5) & (r < 0.55), :C] = 1.0
    yt[(r > 0.6) & (r < 0.65), :C] = 0.0
    return p, yt.contiguous()      # the reference compares the same fp32 numbers: a near-tie is resolved alike


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", (2, 3, 5, 21, 32))
def test_confusion_matrix(engine, C, off):
    for rows, y_cols in ((1, C), (63, 2 * C), (65, C), (257, 2 * C), (4099, C), (4099, 2 * C)):
        start = torch.arange(C * C, dtype=torch.int64) * 3 + 5          # a non-zero `out`: the counts are accumulated
        want, O = start.clone(), G(start, role="out")
        for call_no in range(2):                                         # two calls into the same out
            p, yt = _confusion_inputs(rows, C, y_cols, f"c{call_no}")
            if rows >= 257:
                top = p.max(1, keepdim=True).values
                assert ((p == top).sum(1) > 1).any() and (yt[:, :C].sum(1) != 1).any()
            want += R.confusion_matrix_ref(p, yt)
            P, Y = G(p, off), G(yt, off)
            done(engine, call(engine, "sg_confusion_matrix", rows, C, y_cols, P.ptr(), Y.ptr(), O.ptr()),
                 f"confusion rows={rows} C={C}", P, Y, O)
            assert torch.equal(O.read(), want), (rows, C, y_cols, call_no, O.read(), want)
        assert int(want.sum()) == int(start.sum()) + 2 * rows


@pytest.mark.parametrize("C", (3, 32))
def test_confusion_matrix_one_cell_and_every_cell(engine, C):
    rows = 5 * C * C + 3
    eye = torch.eye(C)
    # every row on the cell (truth C-1, prediction 1): one LDS address for the whole wave
    p, yt = eye[torch.ones(rows, dtype=torch.long)] * 0.5 + 0.1, eye[torch.full((rows,), C - 1)]
    O = G(torch.zeros(C * C, dtype=torch.int64), role="out")
    P, Y = G(p.contiguous()), G(yt.contiguous())
    done(engine, call(engine, "sg_confusion_matrix", rows, C, C, P.ptr(), Y.ptr(), O.ptr()), "one cell", P, Y, O)
    want = torch.zeros(C * C, dtype=torch.int64)
    want[(C - 1) * C + 1] = rows
    assert torch.equal(O.read(), want)
    # every cell hit: row i falls on cell i mod C^2 (up to 64 distinct cells in one wave)
    cell = torch.arange(rows) % (C * C)
    p, yt = eye[cell % C] * 0.5 + 0.1, eye[cell // C]
    O = G(torch.zeros(C * C, dtype=torch.int64), role="out")
    P, Y = G(p.contiguous()), G(yt.contiguous())
    done(engine, call(engine, "sg_confusion_matrix", rows, C, C, P.ptr(), Y.ptr(), O.ptr()), "every cell", P, Y, O)
    got = O.read()
    assert (got >= 5).all() and torch.equal(got, torch.bincount(cell, minlength=C * C))
    assert torch.equal(got, R.confusion_matrix_ref(p, yt))


def test_confusion_matrix_wrapped_grid(engine):
    rows, Cn = RED_CAP + 1027, 3                      # the grid is clamped to 2048 workgroups: more than 1024 rows for some
    p, yt = _confusion_inputs(rows, Cn, Cn, "wrap")
    O = G(torch.zeros(Cn * Cn, dtype=torch.int64), role="out")
    P, Y = G(p, True), G(yt, True)
    done(engine, call(engine, "sg_confusion_matrix", rows, Cn, Cn, P.ptr(), Y.ptr(), O.ptr()), "confusion wrap", P, Y, O)
    assert torch.equal(O.read(), R.confusion_matrix_ref(p, yt))


# ================================================================================================ class-map canvas
def _tile(g, TH, TW, C):
    p = R.class_probs(g, TH * TW, C).reshape(TH, TW, C)
    r = torch.rand(TH, TW, generator=g)
    a, b = torch.randint(0, C, (TH, TW), generator=g), torch.randint(0, C, (TH, TW), generator=g)
    tie = r < 0.2                                     # planted ties: the lowest index wins
    ii, jj = torch.nonzero(tie, as_tuple=True)
    p[ii, jj, a[tie]] = 2.0
    p[ii, jj, b[tie]] = 2.0
    p[(r > 0.3) & (r < 0.35)] = 1.0 / C
    return p.contiguous()


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", (2, 3, 5, 21, 32))
def test_argmax_max_u8(engine, C, off):
    g = gen(f"amax{C}")
    CH, CW, TH, TW = 37, 53, 19, 23
    start = torch.randint(0, C, (CH, CW), generator=g).to(torch.uint8)
    start[torch.rand(CH, CW, generator=g) < 0.5] = 0
    # inside; hanging over the top-left, the bottom-right, the top-right and the bottom-left corner; fully outside
    for (y0, x0) in ((5, 7), (-6, -9), (CH - 8, CW - 11), (-3, CW - 5), (CH - 4, -10), (CH + 2, 3)):
        p = _tile(g, TH, TW, C)
        want = R.argmax_max_ref(start, p, y0, x0)
        K, P = G(start, role="out"), G(p, off)
        done(engine, call(engine, "sg_argmax_max_u8", P.ptr(), C, TH, TW, K.ptr(), CH, CW, y0, x0), f"argmax_max {y0},{x0}", P, K)
        assert torch.equal(K.read(), want), (C, y0, x0)
        if (y0, x0) == (CH + 2, 3):
            assert torch.equal(want, start)
    # two overlapping tiles in both orders give the same canvas
    pa, pb = _tile(g, TH, TW, C), _tile(g, TH, TW, C)
    res = []
    for order in (((pa, 4, 6), (pb, 10, 15)), ((pb, 10, 15), (pa, 4, 6))):
        K, want = G(torch.zeros(CH, CW, dtype=torch.uint8), role="out"), torch.zeros(CH, CW, dtype=torch.uint8)
        for p, y0, x0 in order:
            P = G(p, off)
            done(engine, call(engine, "sg_argmax_max_u8", P.ptr(), C, TH, TW, K.ptr(), CH, CW, y0, x0), "overlap", P)
            want = R.argmax_max_ref(want, p, y0, x0)
        K.fetch().check("overlap")
        assert torch.equal(K.read(), want)
        res.append(K.read())
    assert torch.equal(res[0], res[1])


# ================================================================================================ C = 2: the 2-class entry points
@pytest.mark.parametrize("off", OFFS)
def test_two_classes_equal_the_two_class_entry_points(engine, off):
    """Bit for bit, but for the loss scalar (its per-row sum is shaped differently: the reduced tolerance).  The 2-class calls
    read float2 pairs and stay on the aligned start; `off` moves the operands of the C-class calls by one element."""
    for rows in (1, 65, 4099):
        g = gen(f"eq{rows}")
        z, dpz = rnd(g, rows, 2, lo=-4, hi=4), rnd(g, rows, 2)
        z[::9, 1] += 80.0
        outs = []
        for name, extra, o in (("sg_softmax2_fwd", (), False), ("sg_softmax_fwd", (2,), off)):
            Z, P = G(z, o), GO((rows, 2), F32, o)
            done(engine, call(engine, name, SG_F32, rows, *extra, Z.ptr(), P.ptr()), name, Z, P)
            outs.append(P.read())
        assert torch.equal(outs[0], outs[1]), f"softmax forward rows={rows}"
        p = outs[0]
        outs = []
        for name, extra, o in (("sg_softmax2_bwd", (), False), ("sg_softmax_bwd", (2,), off)):
            P, D, Z = G(p, o), G(dpz, o), GO((rows, 2), F32, o)
            done(engine, call(engine, name, SG_F32, rows, *extra, P.ptr(), D.ptr(), Z.ptr()), name, P, D, Z)
            outs.append(Z.read())
        assert torch.equal(outs[0], outs[1]), f"softmax backward rows={rows}"
        for y_cols in (2, 4):
            yt = R.class_labels(g, rows, 2, y_cols)
            for kind in ((0, 1, 2) if y_cols == 4 else (0, 1)):
                alpha = (0.5, 0.5) if kind == 1 else (0.35, 0.65)
                for gs in (1.0, 0.25):
                    P, Y, D = G(p), G(yt), GO((rows, 2), F32)
                    done(engine, call(engine, "sg_loss_bwd", kind, rows, y_cols, P.ptr(), Y.ptr(), D.ptr(), gs), "loss_bwd", P, Y, D)
                    P, Y, Dn = G(p, off), G(yt, off), GO((rows, 2), F32, off)
                    done(engine, call(engine, "sg_lossn_bwd", kind, rows, 2, y_cols, alpha_arg(alpha), P.ptr(), Y.ptr(), Dn.ptr(), gs),
                         "lossn_bwd", P, Y, Dn)
                    assert torch.equal(D.read(), Dn.read()), f"loss backward kind={kind} rows={rows} y_cols={y_cols} scale={gs}"
                nws = engine.lib.sg_loss_ws_bytes(engine.h, rows)
                assert nws == engine.lib.sg_lossn_ws_bytes(engine.h, rows)
                P, Y, L, W = G(p), G(yt), GO((1,), F32), Guarded.ws(nws, DEV)
                done(engine, call(engine, "sg_loss_fwd", kind, rows, y_cols, P.ptr(), Y.ptr(), L.ptr(), W.ptr(), nws), "loss_fwd", P, Y, L, W)
                P, Y, Ln, W = G(p, off), G(yt, off), GO((1,), F32, off), Guarded.ws(nws, DEV)
                done(engine, call(engine, "sg_lossn_fwd", kind, rows, 2, y_cols, alpha_arg(alpha), P.ptr(), Y.ptr(), Ln.ptr(), W.ptr(), nws),
                     "lossn_fwd", P, Y, Ln, W)
                close(Ln.read(), L.read().double(), TOL_RED, f"loss forward kind={kind} rows={rows}")
            pc, ytc = _confusion_inputs(rows, 2, y_cols, "eq")
            P, Y, O4 = G(pc), G(ytc), G(torch.zeros(4, dtype=torch.int64), role="out")
            done(engine, call(engine, "sg_confusion_counts", rows, y_cols, P.ptr(), Y.ptr(), O4.ptr()), "counts", P, Y, O4)
            P, Y, OM = G(pc, off), G(ytc, off), G(torch.zeros(4, dtype=torch.int64), role="out")
            done(engine, call(engine, "sg_confusion_matrix", rows, 2, y_cols, P.ptr(), Y.ptr(), OM.ptr()), "matrix", P, Y, OM)
            tp, tn, fp, fn = O4.read().tolist()
            assert OM.read().tolist() == [tn, fp, fn, tp], (rows, y_cols)
    # the canvas: `canvas > 0` of the class map is the accumulated int8 >= 1
    g = gen("eqcanvas")
    CH, CW, TH, TW = 40, 44, 24, 20
    K8 = G(torch.zeros(CH, CW, dtype=torch.int8), role="out")
    KU = G(torch.zeros(CH, CW, dtype=torch.uint8), role="out")
    for (y0, x0) in ((0, 0), (10, 12), (-5, 30), (30, -4)):
        p = _tile(g, TH, TW, 2)
        P = G(p)
        done(engine, call(engine, "sg_argmax_accumulate_i8", P.ptr(), TH, TW, K8.ptr(), CH, CW, y0, x0), "accumulate", P)
        P = G(p, off)
        done(engine, call(engine, "sg_argmax_max_u8", P.ptr(), 2, TH, TW, KU.ptr(), CH, CW, y0, x0), "max", P)
    K8.fetch().check("int8 canvas")
    KU.fetch().check("uint8 canvas")
    assert torch.equal(KU.read() > 0, K8.read() >= 1) and (KU.read() > 0).any() and (KU.read() == 0).any()


# ================================================================================================ refusals
def test_refusals_write_nothing(engine):
    rows = 65
    g = gen("refuse")
    al = alpha_arg([0.5] * 33)
    for Cn, y_cols, kind in ((1, 1, 0), (33, 33, 0), (33, 66, 2), (5, 7, 1), (5, 4, 0), (5, 11, 2), (5, 5, 2), (2, 2, 2), (5, 5, 3)):
        what = f"C={Cn} y_cols={y_cols} kind={kind}"
        p, yt = rnd(g, rows, Cn, lo=0, hi=1), rnd(g, rows, max(y_cols, 1), lo=0, hi=1)
        class_count = Cn in (1, 33)
        nws = engine.lib.sg_lossn_ws_bytes(engine.h, rows)
        P, Y, L, W = G(p), G(yt), GO((1,), F32), Guarded.ws(nws, DEV)
        assert call(engine, "sg_lossn_fwd", kind, rows, Cn, y_cols, al, P.ptr(), Y.ptr(), L.ptr(), W.ptr(), nws) == SG_EINVAL, what
        DP = GO((rows, Cn), F32)
        assert call(engine, "sg_lossn_bwd", kind, rows, Cn, y_cols, al, P.ptr(), Y.ptr(), DP.ptr(), 1.0) == SG_EINVAL, what
        outs = [L, W, DP]
        if class_count or kind != 2 and y_cols not in (Cn, 2 * Cn):
            O = G(torch.full((max(Cn * Cn, 4),), 7, dtype=torch.int64), role="out")
            assert call(engine, "sg_confusion_matrix", rows, Cn, y_cols, P.ptr(), Y.ptr(), O.ptr()) == SG_EINVAL, what
            outs.append(O)
        if class_count:
            Po, Dz = GO((rows, Cn), F32), GO((rows, Cn), F32)
            assert call(engine, "sg_softmax_fwd", SG_F32, rows, Cn, P.ptr(), Po.ptr()) == SG_EINVAL, what
            assert call(engine, "sg_softmax_bwd", SG_F32, rows, Cn, P.ptr(), Y.ptr(), Dz.ptr()) == SG_EINVAL, what
            K = G(torch.full((8, 8), 9, dtype=torch.uint8), role="out")
            assert call(engine, "sg_argmax_max_u8", P.ptr(), Cn, 5, 5, K.ptr(), 8, 8, 0, 0) == SG_EINVAL, what
            outs += [Po, Dz, K]
        torch.cuda.synchronize()
        for o in outs:
            untouched(o, what)
        check_all((P, Y), what)
    # null pointers, rows <= 0, the focal kinds without class weights
    p, yt = R.class_probs(g, rows, 3), R.class_labels(g, rows, 3, 6)
    P, Y, L, W, DP = G(p), G(yt), GO((1,), F32), Guarded.ws(1024, DEV), GO((rows, 3), F32)
    a3 = alpha_arg([0.5, 0.5, 0.5])
    assert call(engine, "sg_lossn_fwd", 1, rows, 3, 6, None, P.ptr(), Y.ptr(), L.ptr(), W.ptr(), W.nb) == SG_EINVAL
    assert call(engine, "sg_lossn_bwd", 2, rows, 3, 6, None, P.ptr(), Y.ptr(), DP.ptr(), 1.0) == SG_EINVAL
    assert call(engine, "sg_lossn_fwd", 1, 0, 3, 6, a3, P.ptr(), Y.ptr(), L.ptr(), W.ptr(), W.nb) == SG_EINVAL
    assert call(engine, "sg_lossn_bwd", 1, -1, 3, 6, a3, P.ptr(), Y.ptr(), DP.ptr(), 1.0) == SG_EINVAL
    assert call(engine, "sg_lossn_bwd", 1, rows, 3, 6, a3, None, Y.ptr(), DP.ptr(), 1.0) == SG_EINVAL
    assert call(engine, "sg_confusion_matrix", 0, 3, 6, P.ptr(), Y.ptr(), DP.ptr()) == SG_EINVAL
    assert call(engine, "sg_confusion_matrix", rows, 3, 6, P.ptr(), None, DP.ptr()) == SG_EINVAL
    assert call(engine, "sg_softmax_fwd", SG_F32, rows, 3, None, DP.ptr()) == SG_EINVAL
    assert call(engine, "sg_softmax_fwd", 1, rows, 3, P.ptr(), DP.ptr()) == SG_EINVAL          # fp32 only
    assert call(engine, "sg_softmax_bwd", SG_F32, -1, 3, P.ptr(), P.ptr(), DP.ptr()) == SG_EINVAL
    assert call(engine, "sg_argmax_max_u8", P.ptr(), 3, 0, 5, DP.ptr(), 8, 8, 0, 0) == SG_EINVAL
    torch.cuda.synchronize()
    for o in (L, W, DP):
        untouched(o, "null / rows")


# ================================================================================================ whole models
MODELS = [("hrnet", 64, 5, {}), ("scse", 64, 3, {}), ("v3plus", 128, 4, {"aspp_pool": 8})]
IDS = [f"{m[0]}-{m[2]}" for m in MODELS]


def build(name, size, C, kw, dtype=None):
    from building_detection_amd import mixed_precision as MP, zoo
    MP.set_global_policy(dtype or "float32")
    try:
        return zoo.BUILDERS[name]((size, size, 3), C, **kw)
    finally:
        MP.set_global_policy("float32")


def class_weights(C):
    return [round(0.35 + 0.3 * c / (C - 1), 4) for c in range(C)]      # (.35 ... .65), the two ends of the reference's pair


def oracle_infer(name, ws, x, C, kw, dtype):
    from oracle import models as M
    P = M.Params(weights=ws, dtype=dtype)
    with torch.no_grad():
        return M.BUILDERS[name](P, torch.from_numpy(x).to(dtype), training=False, num_classes=C, **kw).double().numpy()


def oracle_train(name, ws, x, y, C, kw, dtype):
    from oracle import models as M
    P = M.Params(weights=ws, dtype=dtype)
    p = M.BUILDERS[name](P, torch.from_numpy(x).to(dtype), training=True, num_classes=C, **kw)
    loss = R.loss_ref(2, p, torch.from_numpy(y).to(dtype), class_weights(C))     # the test's own C-class edge focal loss
    loss.backward()
    return P, p.detach(), loss.item(), [t.grad.double().numpy() for t in P.trainable_tensors()]


def stir(model, seed=5):
    """Non-trivial BatchNormalization moving statistics and biases, as test_models_gpu.test_inference_parity sets them."""
    ws = model.get_weights()
    rng = np.random.default_rng(seed)
    for i, p in enumerate(model.params):
        if p.kind == "moving_mean":
            ws[i] = rng.normal(0, 0.1, p.shape).astype(np.float32)
        elif p.kind == "moving_var":
            ws[i] = rng.uniform(0.5, 1.5, p.shape).astype(np.float32)
        elif p.kind in ("bias", "beta"):
            ws[i] = rng.normal(0, 0.05, p.shape).astype(np.float32)
    model.set_weights(ws)
    return ws


@pytest.mark.parametrize("name,size,C,kw", MODELS, ids=IDS)
def test_inference_parity(engine, name, size, C, kw):
    from building_detection_amd.data import synthetic_batch
    model = build(name, size, C, kw)
    x, _ = synthetic_batch(2, size, size, seed=11, num_classes=C)
    ws = stir(model)
    pg = model.predict(x.astype(np.float64))
    assert pg.dtype == np.float32 and pg.shape == (2, size, size, C)
    np.testing.assert_allclose(pg.sum(-1), 1.0, atol=1e-5)
    p32 = oracle_infer(name, ws, x, C, kw, torch.float32)
    p64 = oracle_infer(name, ws, x, C, kw, torch.float64)
    err_gpu32, err_gpu64 = float(np.abs(pg - p32).max()), float(np.abs(pg - p64).max())
    err_cpu64 = float(np.abs(p32 - p64).max())
    print(f"{name} C={C}: |gpu-cpu32|={err_gpu32:.2e} |gpu-fp64|={err_gpu64:.2e} |cpu32-fp64|={err_cpu64:.2e}")
    assert err_gpu32 <= 1e-3, f"{name}: max |p_gpu - p_cpu| = {err_gpu32:.3e} > 1e-3"
    assert err_gpu64 <= 4 * err_cpu64 + 1e-4, f"{name}: gpu fp32 error {err_gpu64:.3e} vs cpu fp32 error {err_cpu64:.3e}"
    TIE = max(1e-6, 2 * err_cpu64)
    top2 = np.sort(p64, axis=-1)[..., -2:]
    strict = (top2[..., 1] - top2[..., 0]) > TIE
    mg, mc = R.argmax_low(torch.from_numpy(pg)).numpy(), R.argmax_low(torch.from_numpy(p64)).numpy()
    bad, excused = int((mg != mc)[strict].sum()), int((mg != mc)[~strict].sum())
    print(f"{name} C={C}: class maps: {int((~strict).sum())} of {strict.size} pixels inside the top-1 / top-2 margin {TIE:.1e}, "
          f"{excused} of them differ; outside the margin {bad} differ")
    assert bad == 0, f"{name}: {bad} class-map pixels differ where the oracle's margin exceeds {TIE:.1e}"


@pytest.mark.parametrize("name,size,C,kw", MODELS, ids=IDS)
def test_train_step_parity(engine, name, size, C, kw):
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.losses import edge_focal_loss, metrics_from_matrix, PA, IoU, MIoU, F1_score
    model = build(name, size, C, kw)
    x, y = synthetic_batch(2, size, size, seed=23, num_classes=C)
    ws0 = model.get_weights()
    model.compile(optimizer="adam", loss=edge_focal_loss.with_alpha(class_weights(C)), metrics=[PA, IoU, MIoU, F1_score])
    model.optimizer.lr = 1e-3
    logs = model.train_on_batch(x, y)
    grads_g = [g.astype(np.float64) for g in model.get_gradients()]
    ws1 = model.get_weights()
    P32, p32, loss32, g32 = oracle_train(name, ws0, x, y, C, kw, torch.float32)
    _, _, loss64, g64 = oracle_train(name, ws0, x, y, C, kw, torch.float64)
    print(f"{name} C={C}: loss gpu {logs['loss']:.7f} cpu32 {loss32:.7f} fp64 {loss64:.7f}")
    assert abs(logs["loss"] - loss64) <= 5 * abs(loss32 - loss64) + 1e-5 * abs(loss64), (logs["loss"], loss32, loss64)
    cm = metrics_from_matrix(R.confusion_matrix_ref(p32.float(), torch.from_numpy(y)).reshape(C, C).numpy())
    ref = R.metrics_ref64(R.confusion_matrix_ref(p32.float(), torch.from_numpy(y)).reshape(C, C).numpy())
    for k in ("PA", "IoU", "MIoU", "F1_score"):
        print(f"{name} C={C}: {k} gpu {logs[k]:.6f} oracle {cm[k]:.6f}")
        assert abs(cm[k] - ref[k]) <= 1e-6
        assert abs(logs[k] - cm[k]) <= 2e-3, (k, logs[k], cm[k])  # a near-tie pixel may flip a count
    names = [p.name for p in model.params if p.trainable]
    FC.compare_gradients(f"{name}-{C}", names, grads_g, g32, g64)
    for i, p in enumerate(model.params):
        if not p.trainable:
            np.testing.assert_allclose(ws1[i], P32.tensors[i].detach().numpy(), rtol=1e-4, atol=1e-5, err_msg=p.name)


# contract of tests/test_bf16_gpu.py::test_model_bf16_against_fp32_engine
MAX_DP_MEAN, MAX_FLIP = 5e-3, 1e-2


def test_bf16_storage_with_a_thin_head(engine):
    """hrnet 64 x 64 with 3 classes (the thin 1x1 head kernels, fp32 head under bf16 storage) against the fp32 engine."""
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.losses import edge_focal_loss, PA, IoU, MIoU, F1_score
    Cn = 3
    m32, m16 = build("hrnet", 64, Cn, {}, "float32"), build("hrnet", 64, Cn, {}, "mixed_bfloat16")
    assert m16.compute_dtype == "bfloat16" and m32.compute_dtype == "float32"
    ws = stir(m32)
    m16.set_weights(ws)
    x, y = synthetic_batch(2, 64, 64, seed=11, num_classes=Cn)
    p32, p16 = m32.predict(x), m16.predict(x)
    assert p16.dtype == np.float32 and p16.shape == (2, 64, 64, Cn) and np.allclose(p16.sum(-1), 1.0, atol=1e-5)
    dp_mean = float(np.abs(p16 - p32).mean())
    flip = float((p16.argmax(-1) != p32.argmax(-1)).mean())
    for m in (m32, m16):
        m.compile(optimizer="adam", loss=edge_focal_loss.with_alpha(class_weights(Cn)), metrics=[PA, IoU, MIoU, F1_score])
    l32, l16 = m32.train_on_batch(x, y), m16.train_on_batch(x, y)
    g32, g16 = m32.get_gradients(), m16.get_gradients()
    tail = []
    for p_, a_, b_ in list(zip([q for q in m32.params if q.trainable], g32, g16))[-2:]:   # the softmax head
        n2 = float(np.square(a_.astype(np.float64)).sum())
        if n2 > 0:
            tail.append((p_.name, float(np.sqrt(np.square(b_.astype(np.float64) - a_).sum() / n2))))
    print(f"bf16 hrnet C={Cn}: mean|dp| {dp_mean:.2e}, argmax flips {flip:.2e}, loss fp32 {l32['loss']:.5f} bf16 {l16['loss']:.5f}, "
          f"last-layer gradient rel-L2 {tail}")
    assert dp_mean <= MAX_DP_MEAN and flip <= MAX_FLIP
    assert abs(l16["loss"] - l32["loss"]) <= 3e-2 * abs(l32["loss"])
    assert all(r <= 0.1 for _, r in tail), tail
    rt = m16._runtime()
    assert rt.w_train.dtype == torch.float32 and rt.g_train.dtype == torch.float32


def test_bf16_storage_names_the_head_the_convolution_code_refuses(engine):
    """hrnet 64 x 64 with 5 classes under bf16 storage: the convolution code keeps an fp32 head (SG_HEAD_F32) of at most four
    output channels and refuses this one (SG_EINVAL from sg_conv2d_fwd, asserted here on the launch itself); the model says so
    when it is built and names the shape.  The same model trains in fp32 (test_train_step_parity[hrnet-5])."""
    from building_detection_amd._lib import SG_BF16, SG_HEAD_F32
    with pytest.raises(ValueError, match=r"64,64,\d+\] with 5 classes"):
        build("hrnet", 64, 5, {}, "mixed_bfloat16")
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=DEV)
    w, y = torch.zeros(1, 1, 64, 5, device=DEV), torch.full((1, 8, 8, 5), float("nan"), device=DEV)
    d = engine.conv_desc((1, 8, 8, 64), 5, 1, 1, 1, 1, "same")
    rc = engine.lib.sg_conv2d_fwd(engine.h, engine.stream, SG_BF16 | SG_HEAD_F32, C_.byref(d), x.data_ptr(), w.data_ptr(), None,
                                  y.data_ptr(), 0, None)
    assert rc == SG_EINVAL and "SG_HEAD_F32" in engine.lib.sg_last_error().decode() and torch.isnan(y).all()


def test_captured_train_step_is_bit_identical_to_the_eager_one(engine):
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.losses import edge_focal_loss, PA, IoU, MIoU, F1_score
    from building_detection_amd.runtime import GraphedTrainStep
    Cn = 5
    ma, mb = build("hrnet", 32, Cn, {}), build("hrnet", 32, Cn, {})
    mb.set_weights(ma.get_weights())
    loss = edge_focal_loss.with_alpha(class_weights(Cn))
    ma.compile(optimizer="adam", loss=loss, metrics=[PA, IoU, MIoU, F1_score])
    mb.compile(optimizer="adam", loss=loss, metrics=[PA, IoU, MIoU, F1_score], jit_compile=True)
    for i in range(5):
        x, y = synthetic_batch(2, 32, 32, seed=70 + i, num_classes=Cn)
        (la, ca), (lb, cb) = ma.train_on_batch(x, y, return_device_scalars=True), mb.train_on_batch(x, y, return_device_scalars=True)
        assert ca.numel() == Cn * Cn and int(ca.sum()) == 2 * 32 * 32
        assert torch.equal(la, lb) and torch.equal(ca, cb), (i, la, lb, ca, cb)
        assert ma._logs(la, ca) == mb._logs(lb, cb)
    assert len(mb._train_graphs) == 1 and isinstance(next(iter(mb._train_graphs.values())), GraphedTrainStep)
    assert not getattr(ma, "_train_graphs", None)
    for wa, wb in zip(ma.get_weights(), mb.get_weights()):
        assert np.array_equal(wa, wb)


def test_detection_returns_the_class_map(engine, tmp_path):
    """pipeline.detection on a 600 x 700 image with a 4-class hrnet: the class map is the host restatement (per-tile argmax,
    merged by maximum) of the engine's own per-tile probabilities."""
    from PIL import Image
    from building_detection_amd import pipeline as PL
    Cn, h, w = 4, 600, 700
    model = build("hrnet", 512, Cn, {})
    stir(model)
    img = np.random.default_rng(3).integers(0, 256, (h, w, 3), dtype=np.uint8)
    got = PL.detection(img, str(tmp_path), model, "cls", batch=4, reference_jloop=False)
    assert got.shape == (h, w) and got.dtype == np.uint8 and set(np.unique(got)) <= set(range(Cn)) and len(np.unique(got)) > 1
    assert np.array_equal(np.asarray(Image.open(tmp_path / "cls.png")), got)
    (ch, cw), origins = PL.tile_origins(h, w, False)
    assert len(origins) == 4
    canvas_img = np.zeros((ch, cw, 3))
    canvas_img[:h, :w, :] = img.astype(np.float64) / 127.5 - 1
    want = torch.zeros(ch, cw, dtype=torch.uint8)
    tiles = np.stack([canvas_img[i:i + 512, j:j + 512, :] for i, j in origins]).astype(np.float32)
    p = model.predict_device(torch.from_numpy(tiles).to(DEV)).cpu()
    assert p.shape == (4, 512, 512, Cn)
    for k, (i, j) in enumerate(origins):
        want = R.argmax_max_ref(want, p[k], i, j)
    assert np.array_equal(got, want.numpy()[:h, :w])
    with pytest.raises(ValueError, match="class map"):
        PL.vote([got] * 5)
