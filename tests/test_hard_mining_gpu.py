"""sg_loss_mined_* on the GPU against the float64 reference (tests/_hard_mining_ref.py): every operand between guard bands
(tests/_guarded.py), outputs NaN-prefilled, the workspace exactly as long as the query says, at the 16-byte aligned start and
ONE ELEMENT further.  The selection is exact on bits, so T and n_kept are compared with `==`; the loss and the gradient use the
project's tolerances (tests/test_region_loss_gpu.py): 1e-4 of |ref| for the reduced scalar, 2e-5 of max|ref| for the
element-wise gradient.  Then what the calls refuse, the Engine wrappers, and a mined loss inside a model, eager and captured."""
import ctypes as C_
import zlib

import numpy as np
import pytest
import torch

import _hard_mining_ref as HR
import _multiclass_ref as MR
from _guarded import Guarded, assert_written, check_all, close, untouched

pytestmark = pytest.mark.gpu

SG_EINVAL, SG_EWORKSPACE = -1, -2
DEV = "cuda"
F32 = torch.float32
TOL, TOL_RED = 2e-5, 1e-4
OFFS = [pytest.param(False, id="aligned"), pytest.param(True, id="offset")]
ROWS = (1, 63, 64, 65, 257, 2049, 70001)
CLASSES = (2, 3, 5, 11, 32)   # 11: the bounded C <= 16 form of the kernels
RED_CAP = 2048 * 1024                 # rows after which the 2048 workgroups take a second trip
TAB_WORDS = 8 + 3 * 2048              # the state words and the three digit tables of the workspace
DENORMAL = 1e-40


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) % (2 ** 31))


def G(t, off=False):
    return Guarded(t, DEV, off=off)


def GO(shape, off=False, dtype=F32):
    return Guarded.out(shape, dtype, DEV, off=off)


def alpha_for(C):
    return tuple(round(0.35 + 0.3 * c / (C - 1), 4) for c in range(C))


def c_desc(C, y_cols, kind, rows, k, thresh, alpha=None):
    from building_detection_amd._lib import MineDesc
    d = MineDesc(C=C, y_cols=y_cols, kind=kind, reserved=0, rows=rows, min_kept=k, thresh=thresh)
    for c in range(min(C, len(d.alpha))):
        d.alpha[c] = 1.0 if alpha is None else alpha[c]
    return d


def ws_bytes(engine, cd):
    return engine.lib.sg_loss_mined_ws_bytes(engine.h, C_.byref(cd))


def fwd(engine, cd, P, Y, L, S, W, nws):
    return engine.lib.sg_loss_mined_fwd(engine.h, engine.stream, C_.byref(cd), P.ptr(), Y.ptr(), L.ptr(), S.ptr(), W.ptr(), nws)


def bwd(engine, cd, P, Y, S, D, scale):
    return engine.lib.sg_loss_mined_bwd(engine.h, engine.stream, C_.byref(cd), P.ptr(), Y.ptr(), S.ptr(), D.ptr(), scale)


def done(engine, rc, what, *ops):
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    check_all(ops, what)


def record(sel):
    """(T bits, the zero word, n_kept) of the int32 [4] record."""
    w = sel.numpy().view(np.uint32)
    return int(w[0]), int(w[1]), int(w[2]) | (int(w[3]) << 32)


def f32(v):
    return float(np.float32(v))


class Case:
    """p and y_true of one shape, uploaded once; select() and grads() run the calls on them."""

    def __init__(self, engine, p, yt, off, tag=""):
        self.engine, self.p, self.yt, self.off = engine, p, yt, off
        self.rows, self.C = p.shape
        self.y_cols = yt.shape[1]
        self.P, self.Y = G(p, off), G(yt, off)
        self.keys = HR.keys_ref(p, yt, self.C)
        self.tag = tag

    def select(self, k, thresh, kind=0, alpha=None, loss=True, again=False):
        """The forward call: T and n_kept exact, the loss within TOL_RED (a NaN loss where the reference's is).  Returns
        (reference, record tensor)."""
        e, rows, C = self.engine, self.rows, self.C
        what = f"mined rows={rows} C={C} y_cols={self.y_cols} kind={kind} k={k} thresh={thresh!r} off={self.off} {self.tag}"
        thresh = f32(thresh)
        cd = c_desc(C, self.y_cols, kind, rows, k, thresh, alpha)
        nws = ws_bytes(e, cd)
        parts = min(max(-(-rows // 1024), 1), 2048)
        assert nws == 4 * (rows + TAB_WORDS + 2 * parts), what
        L, S, W = GO((1,), self.off), GO((4,), self.off, torch.int32), Guarded.ws(nws, DEV)
        done(e, fwd(e, cd, self.P, self.Y, L, S, W, nws), what, self.P, self.Y, L, S, W)
        al = None if alpha is None else tuple(f32(a) for a in alpha)
        ref = HR.mined_ref(kind, self.p, self.yt, al, thresh, k)
        tb, zero, n = record(S.read())
        assert (tb, zero, n) == (ref["T_bits"], 0, ref["n_kept"]), \
            f"{what}: record T={tb:#010x} n_kept={n}, reference T={ref['T_bits']:#010x} n_kept={ref['n_kept']}"
        assert n >= k and np.array_equal(self.keys <= ref["T"], ref["kept"].numpy())
        got = L.read()
        if torch.isnan(ref["loss"]).any():
            assert torch.isnan(got).all(), what
        elif loss:
            close(got, ref["loss"], TOL_RED, what + " loss")
        else:
            assert torch.isfinite(got).all(), what
        if again:
            L2, S2, W2 = GO((1,), self.off), GO((4,), self.off, torch.int32), Guarded.ws(nws, DEV)
            done(e, fwd(e, cd, self.P, self.Y, L2, S2, W2, nws), what + " again", L2, S2, W2)
            assert torch.equal(L2.read().view(torch.int32), got.view(torch.int32)) and torch.equal(S2.read(), S.read()), \
                what + ": the forward call is not reproducible"
        return ref, S.read(), cd, what

    def grads(self, k, thresh, kind, alpha, scales=(1.0, 0.25)):
        ref, sel, cd, what = self.select(k, thresh, kind, alpha, again=True)
        e, rows, C = self.engine, self.rows, self.C
        SI = G(sel, self.off)
        al = None if alpha is None else tuple(f32(a) for a in alpha)
        for gs in scales:
            D = GO((rows, C), self.off)
            done(e, bwd(e, cd, self.P, self.Y, SI, D, gs), what + " bwd", self.P, self.Y, SI, D)
            dp = D.read()
            assert_written(dp, what + " bwd")
            close(dp, HR.mined_ref(kind, self.p, self.yt, al, f32(thresh), k, scale=gs)["grad"], TOL, what + f" bwd scale={gs}")
            dropped = dp[~ref["kept"]]
            assert (dropped.view(torch.int32) == 0).all(), what + ": a dropped row's gradient is not +0.0"
            D2 = GO((rows, C), self.off)
            done(e, bwd(e, cd, self.P, self.Y, SI, D2, gs), what + " bwd again", D2)
            assert torch.equal(D2.read().view(torch.int32), dp.view(torch.int32)), what + ": the backward call is not reproducible"
        return ref


def with_keys(g, rows, C, y_cols, keys):
    """p whose true-class entries are `keys` (fp32, to the bit); the other entries share what is left of 1 (at least 1e-3)."""
    yt = MR.class_labels(g, rows, C, y_cols)
    t = yt[:, :C].argmax(1)
    keys = torch.as_tensor(np.asarray(keys, np.float32))
    rest = ((1.0 - keys.double()).clamp_min(1e-3) / (C - 1)).float()
    p = rest.reshape(-1, 1).repeat(1, C)
    p[torch.arange(rows), t] = keys
    return p.contiguous(), yt


def ks(rows):
    return sorted({1, max(1, rows // 3), rows})


# ================================================================================================ the select is exact
def keyset(name, g, rows, C):
    """(p, y_true, [(k, thresh), ...]) of one of the issue's key sets at one shape."""
    y_cols = 2 * C if rows % 2 else C
    if name == "random":
        p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, y_cols)
        return p, yt, [(k, 0.0) for k in ks(rows)] + [(max(1, rows // 3), 0.7)]
    if name == "equal":
        p, yt = with_keys(g, rows, C, y_cols, np.full(rows, 0.37, np.float32))
        return p, yt, [(k, t) for k in ks(rows) for t in (0.0, 0.37, 0.9)]
    if name == "low_digit":                                       # 0.5 + j 2^-24: neighbours in fp32, only the low bits differ
        keys = (0.5 + np.arange(rows, dtype=np.float64) * 2.0 ** -24).astype(np.float32)
        assert len(np.unique(keys)) == rows
        keys = keys[torch.randperm(rows, generator=g).numpy()]
        p, yt = with_keys(g, rows, C, y_cols, keys)
        return p, yt, [(k, 0.0) for k in ks(rows)] + [(max(1, rows // 3), 0.5)]
    if name == "two_values":                                      # a < b, k at count(a) and one past it
        na = max(1, rows // 2)
        keys = np.where(torch.randperm(rows, generator=g).numpy() < na, np.float32(0.25), np.float32(0.75)).astype(np.float32)
        p, yt = with_keys(g, rows, C, y_cols, keys)
        return p, yt, [(k, 0.0) for k in sorted(set(ks(rows)) | {na, min(rows, na + 1)})]
    if name == "zero_denormal_one":
        keys = HR.keys_ref(MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, C), C).copy()
        for j, v in enumerate((0.0, DENORMAL, 1.0)):
            keys[(j * 31 + 5) % rows] = np.float32(v)
        if rows >= 3:
            assert (keys == 0).any() and (keys == np.float32(DENORMAL)).any() and (keys == 1).any() and np.float32(DENORMAL) > 0
        p, yt = with_keys(g, rows, C, y_cols, keys)
        return p, yt, [(k, t) for k in sorted(set(ks(rows)) | {min(rows, 2), min(rows, 3)}) for t in (0.0, DENORMAL)]
    p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, y_cols)
    keys = HR.keys_ref(p, yt, C)
    order = np.sort(keys)
    if name == "thresh_is_a_key":
        return p, yt, [(k, float(keys[rows // 2])) for k in ks(rows)] + [(max(1, rows // 3), float(order[max(1, rows // 3) - 1]))]
    assert name == "thresh_around_qk"
    out = []
    for k in ks(rows):
        qk = float(order[k - 1])
        out += [(k, qk * 0.5), (k, min(1.0, (qk + 1.0) * 0.5))]
    return p, yt, out


KEYSETS = ("random", "equal", "low_digit", "two_values", "zero_denormal_one", "thresh_is_a_key", "thresh_around_qk")


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("name", KEYSETS)
def test_select_is_exact(engine, name, C, off):
    """T and n_kept to the bit.  The loss is held to TOL_RED where p is a softmax output; the planted keys are not (a key of
    exactly 1 makes the row's term log(1 + 1e-7), which fp32 rounds to log(1 + 2^-23) in sg_lossn_fwd's expression too): there
    the loss only has to be finite, and test_loss_and_gradient holds it to the reference."""
    natural = name in ("random", "thresh_is_a_key", "thresh_around_qk")
    for rows in ROWS:
        p, yt, cases = keyset(name, gen(f"{name}{rows}{C}"), rows, C)
        case = Case(engine, p, yt, off, tag=name)
        for n, (k, thresh) in enumerate(cases):
            case.select(k, thresh, kind=0, loss=natural, again=(n == 0))


def test_a_nan_key_counts_as_zero_and_shows_in_the_loss(engine):
    rows, C = 257, 3
    g = gen("nan")
    p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, C)
    t = yt[:, :C].argmax(1)
    p[100, t[100]] = float("nan")
    case = Case(engine, p, yt, False, tag="nan")
    assert HR.bits(case.keys[100]) == 0
    ref, _, _, _ = case.select(1, 0.0)                            # the NaN row is the one hardest row
    assert ref["n_kept"] == 1 and ref["T_bits"] == 0 and torch.isnan(ref["loss"]).all()
    ref, _, _, _ = case.select(rows // 3, 0.2)
    assert torch.isnan(ref["loss"]).all()


def test_past_the_part_cap(engine):
    rows, C = RED_CAP + 5, 2
    g = gen("cap")
    p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, C)
    case = Case(engine, p, yt, True, tag="cap")
    assert ws_bytes(engine, c_desc(C, C, 0, rows, 1, 0.0)) == 4 * (rows + TAB_WORDS + 2 * 2048)
    case.grads(rows // 3, 0.0, 0, None, scales=(1.0,))
    case.select(rows // 3, 0.7, again=False)


# ================================================================================================ loss and gradient
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("kind", (0, 1, 2))
def test_loss_and_gradient(engine, kind, off):
    for C in CLASSES:
        for rows in (65, 257, 2049):
            y_cols = 2 * C if kind == 2 or rows % 2 else C
            g = gen(f"lg{kind}{rows}{C}")
            case = Case(engine, MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, y_cols), off)
            alpha = None if kind == 0 else alpha_for(C)
            ref = case.grads(max(1, rows // 3), 0.0, kind, alpha)
            assert ref["n_kept"] < rows
            order = np.sort(case.keys)
            ref = case.grads(rows // 10, float(order[rows // 2]), kind, alpha, scales=(0.25,))     # the threshold decides
            assert rows // 2 < ref["n_kept"] < rows


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("C", CLASSES)
def test_thresh_one_is_the_plain_loss(engine, C, off):
    for rows, y_cols in ((257, 2 * C), (2049, C)):
        g = gen(f"one{rows}{C}")
        p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, y_cols)
        case = Case(engine, p, yt, off)
        alpha = alpha_for(C)
        al = (C_.c_float * C)(*alpha)
        for kind in ((0, 1, 2) if y_cols == 2 * C else (0, 1)):
            ref, sel, cd, what = case.select(1, 1.0, kind, alpha)
            assert ref["n_kept"] == rows and ref["T_bits"] == 0x3F800000
            nws = ws_bytes(engine, cd)
            L, S, W = GO((1,)), GO((4,), False, torch.int32), Guarded.ws(nws, DEV)
            done(engine, fwd(engine, cd, case.P, case.Y, L, S, W, nws), what, L, S, W)
            nwn = engine.lib.sg_lossn_ws_bytes(engine.h, rows)
            Ln, Wn = GO((1,)), Guarded.ws(nwn, DEV)
            rc = engine.lib.sg_lossn_fwd(engine.h, engine.stream, kind, rows, C, y_cols, al, case.P.ptr(), case.Y.ptr(), Ln.ptr(),
                                         Wn.ptr(), nwn)
            done(engine, rc, what + " lossn_fwd", Ln, Wn)
            close(L.read(), Ln.read().double(), TOL_RED, what + " against sg_lossn_fwd")
            D, Dn, SI = GO((rows, C), off), GO((rows, C), off), G(sel)
            done(engine, bwd(engine, cd, case.P, case.Y, SI, D, 0.5), what + " bwd", D, SI)
            rc = engine.lib.sg_lossn_bwd(engine.h, engine.stream, kind, rows, C, y_cols, al, case.P.ptr(), case.Y.ptr(), Dn.ptr(), 0.5)
            done(engine, rc, what + " lossn_bwd", Dn)
            close(D.read(), Dn.read().double(), TOL, what + " against sg_lossn_bwd")


# ================================================================================================ refusals
def test_refusals_write_nothing(engine):
    C, rows = 3, 65
    g = gen("refuse")
    p, yt = MR.class_probs(g, rows, C), MR.class_labels(g, rows, C, 2 * C)
    nan, inf = float("nan"), float("inf")
    bad = [("C=1", dict(C=1)), ("C=33", dict(C=33)), ("C=0", dict(C=0)), ("y_cols", dict(y_cols=4)), ("edge without weights", dict(y_cols=3)),
           ("kind=3", dict(kind=3)), ("kind=-1", dict(kind=-1)), ("reserved", dict(reserved=1)), ("rows=0", dict(rows=0)),
           ("rows<0", dict(rows=-5)), ("rows=2^32", dict(rows=2 ** 32, min_kept=1)), ("k=0", dict(min_kept=0)), ("k<0", dict(min_kept=-1)),
           ("k>rows", dict(min_kept=rows + 1)), ("thresh<0", dict(thresh=-0.001)), ("thresh>1", dict(thresh=1.001)),
           ("thresh nan", dict(thresh=nan)), ("thresh inf", dict(thresh=inf)), ("alpha inf", dict(alpha=(0.5, inf, 0.5))),
           ("alpha nan", dict(alpha=(nan, 0.5, 0.5)))]
    P, Y = G(p), G(yt)
    good = c_desc(C, 2 * C, 2, rows, 20, 0.25, alpha_for(C))
    nws = ws_bytes(engine, good)
    assert nws == 4 * (rows + TAB_WORDS + 2)
    L, S, W, D = GO((1,)), GO((4,), False, torch.int32), Guarded.ws(nws, DEV), GO((rows, C))
    SI = G(torch.tensor([0x3F000000, 0, rows, 0], dtype=torch.int32))
    for name, kw in bad:
        cd = c_desc(C, 2 * C, 2, rows, 20, 0.25, kw.pop("alpha", alpha_for(C)))
        for k, v in kw.items():
            setattr(cd, k, v)
        assert ws_bytes(engine, cd) == 0, name
        assert fwd(engine, cd, P, Y, L, S, W, nws) == SG_EINVAL, name
        assert bwd(engine, cd, P, Y, SI, D, 1.0) == SG_EINVAL, name
    null = type("Null", (), {"ptr": staticmethod(lambda: None)})
    for i in range(5):                                                        # a null pointer in every position
        ops = [P, Y, L, S, W]
        ops[i] = null
        assert fwd(engine, good, *ops, nws) == (SG_EWORKSPACE if i == 4 else SG_EINVAL), i
    for i in range(4):
        ops = [P, Y, SI, D]
        ops[i] = null
        assert bwd(engine, good, *ops, 1.0) == SG_EINVAL, i
    assert engine.lib.sg_loss_mined_fwd(engine.h, engine.stream, None, P.ptr(), Y.ptr(), L.ptr(), S.ptr(), W.ptr(), nws) == SG_EINVAL
    assert engine.lib.sg_loss_mined_bwd(engine.h, engine.stream, None, P.ptr(), Y.ptr(), SI.ptr(), D.ptr(), 1.0) == SG_EINVAL
    assert engine.lib.sg_loss_mined_ws_bytes(engine.h, None) == 0
    assert fwd(engine, good, P, Y, L, S, W, nws - 1) == SG_EWORKSPACE          # one byte short
    torch.cuda.synchronize()
    for o in (L, S, W, D):
        untouched(o, "refusals")
    check_all((P, Y, SI), "refusals")
    # ... and the same operands are taken once the descriptor is right
    done(engine, fwd(engine, good, P, Y, L, S, W, nws), "good", P, Y, L, S, W)
    assert_written(L.read(), "good")
    ref = HR.mined_ref(2, p, yt, tuple(f32(a) for a in alpha_for(C)), 0.25, 20)
    assert record(S.read()) == (ref["T_bits"], 0, ref["n_kept"])
    SG = G(S.read())
    done(engine, bwd(engine, good, P, Y, SG, D, 1.0), "good bwd", P, Y, SG, D)
    close(D.read(), ref["grad"], TOL, "good bwd")


# ================================================================================================ wrappers
def test_engine_wrappers(engine):
    from building_detection_amd import losses as LS
    C, n, hw = 3, 2, 33
    g = gen("wrap")
    rows = n * hw * hw
    p, yt = MR.class_probs(g, rows, C).reshape(n, hw, hw, C), MR.class_labels(g, rows, C, 2 * C).reshape(n, hw, hw, 2 * C)
    pd, yd = p.to(DEV), yt.to(DEV)
    for loss, k in ((LS.hard_mining(LS.edge_focal_loss.with_alpha(alpha_for(C)), 0.3, 0.25), -(-rows // 4)),
                    (LS.hard_mining(LS.binary_crossentropy, 0.0, 100), 100), (LS.hard_mining(LS.focal_loss, 1.0, 1), 1)):
        r = LS.resolve_mining(loss, C)
        out, sel = engine.loss_mined_fwd(r, pd, yd)
        dp = engine.loss_mined_bwd(r, pd, yd, sel, 0.5)
        assert tuple(out.shape) == (1,) and tuple(sel.shape) == (4,) and sel.dtype == torch.int32 and dp.shape == pd.shape
        al = None if r["alpha"] is None else tuple(f32(a) for a in r["alpha"])
        ref = HR.mined_ref(r["kind"], p.reshape(-1, C), yt.reshape(-1, 2 * C), al, f32(r["thresh"]), k, scale=0.5)
        assert record(sel.cpu()) == (ref["T_bits"], 0, ref["n_kept"])
        close(out, ref["loss"], TOL_RED, "wrapper loss")
        close(dp.reshape(-1, C), ref["grad"], TOL, "wrapper dp")
        for wrong in (sel[:3], sel.float(), sel.reshape(2, 2), sel.cpu(), None):
            with pytest.raises(ValueError, match="sel"):
                engine.loss_mined_bwd(r, pd, yd, wrong)


# ================================================================================================ inside a model
def build(C):
    from building_detection_amd import zoo
    return zoo.BUILDERS["hrnet"]((32, 32, 3), C)


@pytest.mark.parametrize("C", (2, 3))
def test_mined_loss_in_a_model_eager_and_captured(engine, C):
    from building_detection_amd import losses as LS
    from building_detection_amd.data import synthetic_batch
    from building_detection_amd.runtime import GraphedTrainStep
    alpha = (0.35, 0.65) if C == 2 else alpha_for(C)
    point = LS.edge_focal_loss if C == 2 else LS.edge_focal_loss.with_alpha(alpha)
    thresh, frac = 0.4, 0.25
    loss = LS.hard_mining(point, thresh, frac)
    metrics = [LS.PA, LS.IoU, LS.MIoU, LS.F1_score]
    ma, mb = build(C), build(C)
    mb.set_weights(ma.get_weights())
    ma.compile(optimizer="adam", loss=loss, metrics=metrics)
    mb.compile(optimizer="adam", loss=loss, metrics=metrics, jit_compile=True)
    assert ma.last_hard_mining() is None
    x, y = synthetic_batch(2, 32, 32, seed=41, num_classes=C)
    rows = 2 * 32 * 32
    logs = ma.test_on_batch(x, y)
    p = torch.from_numpy(ma.predict(x)).reshape(-1, C)
    yt = torch.from_numpy(y).reshape(-1, 2 * C).float()
    al = tuple(f32(a) for a in alpha)
    ref = HR.mined_ref(2, p, yt, al, f32(thresh), rows // 4)
    hm = ma.last_hard_mining()
    print(f"C={C}: test_on_batch loss {logs['loss']:.7f}, float64 on predict's probabilities {ref['loss'].item():.7f}; {hm}")
    close(torch.tensor([logs["loss"]]), ref["loss"], TOL_RED, "test_on_batch loss")
    assert hm == dict(threshold=float(ref["T"]), kept=ref["n_kept"], rows=rows) and set(logs) == {"loss", "PA", "IoU", "MIoU", "F1_score"}
    # thresh = 1 keeps every pixel: the unwrapped loss on the same weights
    mc = build(C)
    mc.set_weights(ma.get_weights())
    mc.compile(optimizer="adam", loss=LS.hard_mining(point, 1.0, frac))
    md = build(C)
    md.set_weights(ma.get_weights())
    md.compile(optimizer="adam", loss=point)
    l1, l0 = mc.test_on_batch(x, y)["loss"], md.test_on_batch(x, y)["loss"]
    close(torch.tensor([l1]), torch.tensor([l0], dtype=torch.float64), TOL_RED, "thresh = 1 against the unwrapped loss")
    assert mc.last_hard_mining() == dict(threshold=1.0, kept=rows, rows=rows) and md.last_hard_mining() is None
    assert l1 != logs["loss"]
    for i in range(5):
        x, y = synthetic_batch(2, 32, 32, seed=80 + i, num_classes=C)
        (la, ca), (lb, cb) = ma.train_on_batch(x, y, return_device_scalars=True), mb.train_on_batch(x, y, return_device_scalars=True)
        assert la.numel() == 1 and torch.equal(la, lb) and torch.equal(ca, cb), (i, la, lb, ca, cb)     # steps 3 and 4 are replays
        ha, hb = ma.last_hard_mining(), mb.last_hard_mining()
        assert ha == hb and rows // 4 <= ha["kept"] <= rows and ha["threshold"] >= f32(thresh), (i, ha, hb)
        assert ma._logs(la, ca) == mb._logs(lb, cb) and np.isfinite(la.item())
    # four more steps with no host read in between: the replays queue up behind one another
    queued = []
    for m in (ma, mb):
        for i in range(4):
            x, y = synthetic_batch(2, 32, 32, seed=90 + i, num_classes=C)
            last = m.train_on_batch(x, y, return_device_scalars=True)
        queued.append((last[0].clone(), last[1].clone(), m.last_hard_mining()))
    (la, ca, ha), (lb, cb, hb) = queued
    assert torch.equal(la, lb) and torch.equal(ca, cb) and ha == hb, (la, lb, ha, hb)
    assert ha["threshold"] >= f32(thresh) and ha["kept"] >= rows // 4
    assert len(mb._train_graphs) == 1 and isinstance(next(iter(mb._train_graphs.values())), GraphedTrainStep)
    sel = next(iter(mb._train_graphs.values())).loss_state.carry   # the record the graph's backward pass reads
    assert sel.is_cuda and sel.dtype == torch.int32 and tuple(sel.shape) == (4,) and not getattr(ma, "_train_graphs", None)
    for wa, wb in zip(ma.get_weights(), mb.get_weights()):
        assert np.array_equal(wa, wb)
    assert any(not np.array_equal(w0, w1) for w0, w1 in zip(build(C).get_weights(), ma.get_weights()))
