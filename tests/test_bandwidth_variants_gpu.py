"""Every variant of the HBM-bound kernels (csrc/pointwise.hip, the pooling / up-sampling kernels of csrc/resample.hip, the loss,
Adam, metrics and tail kernels of csrc/train.hip) against plain float64 torch on the CPU, through the C ABI itself.

Each entry point picks one of several kernels at launch time; every case below names the dispatch predicate it satisfies.
Operands are tests/_guarded.py arenas (NaN guard bands, NaN-prefilled outputs, workspaces of exactly the queried size), their
start either 16-byte aligned or one element further (the scalar kernels the dispatch code promises for such tensors).
Tolerances, as max|got - ref| <= tol * max|ref|: 2e-5 fp32 element-wise, 1e-4 fp32 reduced (tests/test_ops_gpu.py), 2^-7 for
bf16-stored results (tests/test_bf16_gpu.py); integer and pure-copy results are exact.  bf16 references start from the same
bf16-rounded inputs (and, on an accumulate, the bf16-rounded prior output).

The two-float-per-row entry points (sg_softmax2_*, sg_loss_*, sg_confusion_counts, sg_argmax_accumulate_i8) have no alignment
dispatch: they read a row as one 8-byte pair, so their "offset" variant moves the tensor by one ROW (8 bytes, no longer
16-byte aligned); sg_adam_step* refuse unaligned arenas (asserted)."""
import ctypes as C
import zlib

import pytest
import torch

from _guarded import (Guarded, adam_ref, assert_written, avgpool_bwd_ref, avgpool_ref, check_all, close, confusion_ref,
                            loss_bwd_ref, loss_ref, maxpool_bwd_ref, maxpool_ref, pool_geom, regime, same_outside, seg_plan_s,
                            sigmoid, upsample_bwd_ref, upsample_ref)

gpu = pytest.mark.gpu

SG_F32, SG_BF16, SG_EINVAL = 0, 1, -1
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
OFFS = [pytest.param(False, id="aligned"), pytest.param(True, id="offset")]
EW_CAP = 8192 * 256      # work items after which pointwise.hip's / train.hip's grid-stride loops take a second trip
SP_CAP = 16384 * 256     # the same for resample.hip's ew_blocks


def sgdt(dtype):
    return SG_BF16 if dtype == BF16 else SG_F32


def tol(dtype, reduced=False):
    return 2.0 ** -7 if dtype == BF16 else (1e-4 if reduced else 2e-5)


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) % (2 ** 31))


def rnd(g, *shape, dtype=F32, lo=-1.0, hi=1.0):
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).float().to(dtype)


def push(t, eps=1e-3):
    """No |value| < eps: nothing sits on a ReLU mask's boundary (2^-7 is exact in bf16)."""
    far = torch.where(t.float() >= 0, 2.0 ** -7, -(2.0 ** -7)).to(t.dtype)
    return torch.where(t.float().abs() < eps, far, t)


def call(engine, name, *args):
    return getattr(engine.lib, name)(engine.h, engine.stream, *args)


def done(engine, rc, what, *ops):
    """The launch returned 0, every band and every input is byte-identical."""
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    check_all(ops, what)


def G(t, off=False, role="in"):
    return Guarded(t, DEV, off=off, role=role)


def GO(shape, dtype, off=False):
    return Guarded.out(shape, dtype, DEV, off=off)


def out_or_prior(prior, acc, off):
    """An accumulating output starts from `prior`; a plain one from NaN."""
    return G(prior, off, role="out") if acc else GO(prior.shape, prior.dtype, off)


# ================================================================================================ harness self-checks (CPU)
def test_band_check_fires_on_an_overwritten_guard_byte():
    for where in (3, -5):
        o = Guarded(torch.zeros(7), "cpu", role="out")
        o.check("clean")
        o.after = None
        o.dev[where] = 0          # the planted error: the test itself overwrites one guard byte
        with pytest.raises(AssertionError, match="band"):
            o.fetch().check("planted")
    i = Guarded(torch.zeros(7), "cpu", off=True, role="in")
    i.dev[i.start + 9] = 1        # ... and one byte of an input
    with pytest.raises(AssertionError, match="input operand"):
        i.fetch().check("planted")
    assert i.ptr() % 16 == 4 and Guarded(torch.zeros(7, dtype=BF16), "cpu", off=True).ptr() % 16 == 2


def test_unwritten_output_check_fires_on_one_left_nan():
    for dtype in (F32, BF16):
        o = Guarded.out((5, 3), dtype, "cpu")
        assert torch.isnan(o.read().float()).all()
        y = torch.ones(5, 3, dtype=dtype)
        assert_written(y, "written")
        y[2, 1] = float("nan")    # the planted error: one element keeps its prefill
        with pytest.raises(AssertionError, match="prefill"):
            assert_written(y, "planted")
    b = torch.zeros(9, dtype=torch.uint8)
    assert_written(b)
    b[4] = 0xFF
    with pytest.raises(AssertionError, match="prefill"):
        assert_written(b)
    w = torch.arange(12.0).reshape(3, 4)
    w2 = w.clone()
    w2[:, 1:3] = -1
    same_outside(w2, w, slice(1, 3))
    w2[1, 3] = 0
    with pytest.raises(AssertionError, match="outside"):
        same_outside(w2, w, slice(1, 3))


def test_numeric_comparison_fires_on_twice_the_tolerance():
    ref = torch.linspace(-3, 3, 101, dtype=torch.float64)
    for dtype, reduced in ((F32, False), (F32, True), (BF16, False)):
        t = tol(dtype, reduced)
        close(ref + 0.9 * t * 3, ref, t, "inside")
        bad = ref.clone()
        bad[17] += 2 * t * 3      # the planted error: the reference perturbed by 2 x tol x max|ref|
        with pytest.raises(AssertionError, match="max err"):
            close(ref, bad, t, "planted")
    with pytest.raises(AssertionError, match="non-finite"):
        close(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 1.0]), 1.0)


# ================================================================================================ element-wise
EW_SIZES = (1, 3, 4, 8, 1020, 1027)   # n % 4 != 0 -> V = 1; 4, 1020: V = 4 (1020 % 8 = 4: the bf16 "4 but not 8" form); 8: bf16 V = 8


def _act_case(engine, dtype, off, n, tag, fwd=True, bwd=True):
    dt, g = sgdt(dtype), gen(f"act{tag}{n}{dtype}{off}")
    x = push(rnd(g, n, dtype=dtype, lo=-4, hi=4))
    dy = rnd(g, n, dtype=dtype)
    for act in (0, 1):
        what = f"act={act} n={n} {dtype} off={off}"
        ref = torch.relu(x.double()) if act == 0 else sigmoid(x.double())
        if fwd:
            X, Y = G(x, off), GO((n,), dtype, off)
            done(engine, call(engine, "sg_act_fwd", dt, act, n, X.ptr(), Y.ptr()), "act_fwd " + what, X, Y)
            assert_written(Y.read(), what)
            close(Y.read(), ref, tol(dtype), "act_fwd " + what)
        if not bwd:
            continue
        y = ref.to(dtype)         # the backward is expressed through the stored OUTPUT
        if act == 0:              # the ReLU mask [y > 0]: float32 and float64 agree on every element
            assert torch.equal(y.float() > 0, x.double() > 0) and not ((y.float() != 0) & (y.float().abs() < 1e-3)).any()
        d = dy.double() * (y.double() > 0) if act == 0 else dy.double() * y.double() * (1 - y.double())
        for acc in (0, 1):
            prior = rnd(g, n, dtype=dtype)
            Yi, DY, DX = G(y, off), G(dy, off), out_or_prior(prior, acc, off)
            done(engine, call(engine, "sg_act_bwd", dt, act, n, Yi.ptr(), DY.ptr(), DX.ptr(), acc), "act_bwd " + what, Yi, DY, DX)
            assert_written(DX.read(), what)
            close(DX.read(), d + prior.double() if acc else d, tol(dtype), f"act_bwd {what} acc={acc}")


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_act(engine, dtype, off):
    for n in EW_SIZES:
        _act_case(engine, dtype, off, n, "small")


def _add_n_case(engine, dtype, offs, n, k, relu):
    """offs: per-operand offsets, operand k is the output."""
    dt, g = sgdt(dtype), gen(f"addn{n}{k}{relu}{dtype}{offs}")
    xs = [rnd(g, n, dtype=dtype) for _ in range(k)]
    if relu:   # keep every sum away from the ReLU's decision boundary
        s = sum(x.double() for x in xs)
        xs[0] = torch.where(s.abs() < 1e-3, xs[0].float() + 0.25, xs[0].float()).to(dtype)
    s = sum(x.double() for x in xs)
    if relu:
        s32 = xs[0].float()
        for x in xs[1:]:
            s32 = s32 + x.float()
        assert (s.abs() >= 1e-3).all() and torch.equal(s32 > 0, s > 0)
    XS, Y = [G(x, o) for x, o in zip(xs, offs)], GO((n,), dtype, offs[k])
    arr = (C.c_void_p * k)(*[X.ptr() for X in XS])
    what = f"add_n n={n} k={k} relu={relu} {dtype} offs={offs}"
    done(engine, call(engine, "sg_add_n", dt, k, arr, n, Y.ptr(), relu), what, Y, *XS)
    assert_written(Y.read(), what)
    close(Y.read(), torch.relu(s) if relu else s, tol(dtype), what)


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_n(engine, dtype, off):
    for n in EW_SIZES:
        for k in (1, 2, 5, 8):
            for relu in (0, 1):
                _add_n_case(engine, dtype, (off,) * (k + 1), n, k, relu)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_add_n_one_unaligned_operand_of_several(engine, dtype):
    # n % 8 == 0 and every pointer but ONE aligned: `vec` must fall to the scalar kernel for all operands
    for which in (0, 2, 5):      # an input in front, one in the middle, the output
        offs = tuple(i == which for i in range(6))
        _add_n_case(engine, dtype, offs, 1024, 5, 1)


@gpu
def test_elementwise_wrapped(engine):
    # scalar kernels (n odd -> V = 1): ew_blocks(n) caps at 8192 blocks once n > 8192 * 256, so n = 8192 * 256 + 1027 sends the
    # first 1027 threads round the grid-stride loop a second time; fp32 (4 bytes x 2.1 M = 8 MB per operand)
    n = EW_CAP + 1027
    _act_case(engine, F32, False, n, "wrap")
    _add_n_case(engine, F32, (False,) * 3, n, 2, 1)
    # the vector kernel once: act_fwd_kernel<4> on bf16 (n % 4 == 0, aligned), n / 4 = 8192 * 256 + 259 items, 17 MB per operand
    _act_case(engine, BF16, False, 4 * (EW_CAP + 259), "wrapv", bwd=False)


# ------------------------------------------------------------------------------------------------ sg_copy_channels
COPY_GEOMS = [
    # C, src_ld, src_off, dst_ld, dst_off
    (16, 32, 8, 40, 16),   # everything % 8 == 0: bf16 V = 8, fp32 V = 4
    (12, 20, 4, 28, 12),   # everything % 4 == 0, nothing % 8: V = 4 in both types
    (8, 16, 8, 24, 4),     # dst_off % 8 = 4 alone takes bf16 from V = 8 to V = 4
    (5, 9, 3, 11, 5),      # odd: V = 1
    (8, 10, 0, 16, 8),     # src_ld % 4 = 2 alone: V = 1
]


def _copy_case(engine, dtype, off, rows, geom, acc):
    Cc, sld, soff, dld, doff = geom
    dt, g = sgdt(dtype), gen(f"copy{rows}{geom}{dtype}{off}{acc}")
    src, prior = rnd(g, rows, sld, dtype=dtype), rnd(g, rows, dld, dtype=dtype)
    start = prior.clone()
    if not acc:
        start[:, doff:doff + Cc] = float("nan")
    S, D = G(src, off), G(start, off, role="out")
    what = f"copy rows={rows} {geom} {dtype} off={off} acc={acc}"
    done(engine, call(engine, "sg_copy_channels", dt, rows, Cc, S.ptr(), sld, soff, D.ptr(), dld, doff, acc), what, S, D)
    got = D.read()
    same_outside(got, start, slice(doff, doff + Cc), what)
    sl = got[:, doff:doff + Cc]
    assert_written(sl, what)
    if acc:
        close(sl, prior[:, doff:doff + Cc].double() + src[:, soff:soff + Cc].double(), tol(dtype), what)
    else:
        assert torch.equal(sl, src[:, soff:soff + Cc]), what + ": a copy is exact"


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_copy_channels(engine, dtype, off):
    for geom in COPY_GEOMS:
        for rows in (1, 257):
            for acc in (0, 1):
                _copy_case(engine, dtype, off, rows, geom, acc)


@gpu
def test_copy_channels_wrapped(engine):
    # scalar kernel (C = 5): rows * C = 419 700 * 5 = 2 098 500 > 8192 * 256 work items
    for acc in (0, 1):
        _copy_case(engine, F32, False, 419700, (5, 7, 1, 6, 1), acc)


# ------------------------------------------------------------------------------------------------ softmax
def _mixed_logits(g, *shape, dtype=F32):
    z = rnd(g, *shape, dtype=dtype, lo=-3, hi=3).float()
    r = torch.rand(*shape, generator=g)
    z = torch.where(r < 0.1, torch.full_like(z, 80.0), z)
    z = torch.where(r > 0.9, torch.full_like(z, -80.0), z)
    return z.to(dtype)


def _softmax2_case(engine, rows, off):
    g = gen(f"sm2{rows}{off}")
    lead = 1 if off else 0      # one ROW (8 bytes) further: the kernels read float2 pairs
    z = _mixed_logits(g, rows + lead, 2)
    dp = rnd(g, rows + lead, 2)
    what = f"softmax2 rows={rows} off={off}"
    Z, P = G(z), GO((rows + lead, 2), F32)
    done(engine, call(engine, "sg_softmax2_fwd", SG_F32, rows, Z.ptr(2 * lead), P.ptr(2 * lead)), what, Z, P)
    p = P.read()
    assert torch.isnan(p[:lead]).all()
    p = p[lead:]
    ref = torch.softmax(z[lead:].double(), dim=1)
    assert torch.isfinite(p).all() and (p >= 0).all() and (p <= 1).all(), what
    close(p.double().sum(1), torch.ones(rows, dtype=torch.float64), tol(F32), what + " sum")
    close(p, ref, tol(F32), what)
    pin = torch.cat([torch.zeros(lead, 2), ref.float()])
    Pi, DP, DZ = G(pin), G(dp), GO((rows + lead, 2), F32)
    done(engine, call(engine, "sg_softmax2_bwd", SG_F32, rows, Pi.ptr(2 * lead), DP.ptr(2 * lead), DZ.ptr(2 * lead)), what, Pi, DP, DZ)
    p64, g64 = ref.float().double(), dp[lead:].double()
    dz = DZ.read()
    assert torch.isnan(dz[:lead]).all()
    assert_written(dz[lead:], what)
    close(dz[lead:], p64 * (g64 - (g64 * p64).sum(1, keepdim=True)), tol(F32), what + " bwd")


@gpu
@pytest.mark.parametrize("off", OFFS)
def test_softmax2(engine, off):
    for rows in (1, 257):
        _softmax2_case(engine, rows, off)


@gpu
def test_softmax2_wrapped(engine):
    _softmax2_case(engine, EW_CAP + 1027, False)   # rows > 8192 * 256: one thread per row, capped grid


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_branch(engine, dtype, off):
    dt = sgdt(dtype)
    for N, Cc in ((3, 45), (2, 260)):    # N * C = 135 (part of one block) and 520 (two blocks and 8 threads): never % 256 == 0
        for B in (1, 2, 3, 5):
            g = gen(f"smb{N}{Cc}{B}{dtype}{off}")
            z, dp = _mixed_logits(g, N, B, Cc, dtype=dtype), rnd(g, N, B, Cc, dtype=dtype)
            what = f"softmax_branch N={N} B={B} C={Cc} {dtype} off={off}"
            Z, P = G(z, off), GO((N, B, Cc), dtype, off)
            done(engine, call(engine, "sg_softmax_branch_fwd", dt, N, B, Cc, Z.ptr(), P.ptr()), what, Z, P)
            p, ref = P.read().float(), torch.softmax(z.double(), dim=1)
            assert torch.isfinite(p).all() and (p >= 0).all() and (p <= 1).all(), what
            close(p.double().sum(1), torch.ones(N, Cc, dtype=torch.float64), tol(dtype), what + " sum")
            close(p, ref, tol(dtype), what)
            pin = ref.to(dtype)
            Pi, DP, DZ = G(pin, off), G(dp, off), GO((N, B, Cc), dtype, off)
            done(engine, call(engine, "sg_softmax_branch_bwd", dt, N, B, Cc, Pi.ptr(), DP.ptr(), DZ.ptr()), what, Pi, DP, DZ)
            p64, g64 = pin.double(), dp.double()
            assert_written(DZ.read(), what)
            close(DZ.read(), p64 * (g64 - (g64 * p64).sum(1, keepdim=True)), tol(dtype), what + " bwd")


# ================================================================================================ gates
# C: 4 (vector: one chunk, TX = 1; row reduce G = 1, 64 rows per wave), 8 (G = 2, TX = 2; bf16 C % 8 = 0), 36 (C % 8 = 4: the
# bf16 V = 4-not-8 form; G = 16 with 9 chunks), 45 (scalar: BAM's odd C, G = 64, TX = 16, gx = 3), 64 (G = 16, TX = 16), 260
# (65 chunks: G = 64 and a second trip over C, gx = 5), 728 (182 chunks: three trips, gx = 12).  With offset pointers every one
# of them takes the scalar kernels instead (G = 4, 8, 64, ...).
GATE_CS = (4, 8, 36, 45, 64, 260, 728)


def _gate_inputs(N, HW, Cc, dtype, tag):
    g = gen(f"gate{N}{HW}{Cc}{dtype}{tag}")
    t = {k: rnd(g, N, HW, Cc, dtype=dtype) for k in ("x", "dy", "prior")}
    t["gc"], t["gs"] = rnd(g, N, Cc, dtype=dtype), rnd(g, N, HW, dtype=dtype)
    t["lc"], t["ls"] = rnd(g, N, Cc, dtype=dtype, lo=-2, hi=2), rnd(g, N, HW, dtype=dtype, lo=-2, hi=2)
    return t


def _split(engine, N, HW, Cc, off, want, query="sg_bcast_mul_bwd_ws_bytes"):
    """The workspace size and the regime of the channel reduction, read back from the query: S = (bytes - 256) / (N C 4)."""
    args = (N, HW, Cc, 0) if query == "sg_bcast_mul_bwd_ws_bytes" else (N, HW, Cc)
    ws = getattr(engine.lib, query)(engine.h, *args)
    assert (ws - 256) % (N * Cc * 4) == 0
    S_q, cus = (ws - 256) // (N * Cc * 4), engine.lib.sg_num_cus(engine.h)
    S_vec, S_sc = seg_plan_s(cus, HW, Cc, True), seg_plan_s(cus, HW, Cc, False)
    assert S_q == max(S_vec, S_sc), (S_q, S_vec, S_sc)      # the query covers the vector and the scalar plan
    S_run = S_vec if (Cc % 4 == 0 and not off) else S_sc     # ... and this launch takes this one
    if want is not None:
        assert regime(S_run) == want, f"N={N} HW={HW} C={Cc} off={off}: S={S_run} (query {S_q}, {cus} CUs) is not '{want}'"
        if regime(S_vec) == regime(S_sc):
            assert regime(S_q) == want
    return ws


def _bcast_fwd(engine, t, N, HW, Cc, dtype, off, modes=(0, 1)):
    dt, x = sgdt(dtype), t["x"]
    for mode in modes:
        gt = t["gc"] if mode == 0 else t["gs"]
        prod = x.double() * (gt.double()[:, None, :] if mode == 0 else gt.double()[:, :, None])
        for acc in (0, 1):
            what = f"bcast_mul_fwd mode={mode} acc={acc} N={N} HW={HW} C={Cc} {dtype} off={off}"
            X, Gt, Y = G(x, off), G(gt, off), out_or_prior(t["prior"], acc, off)
            done(engine, call(engine, "sg_bcast_mul_fwd", dt, N, HW, Cc, mode, X.ptr(), Gt.ptr(), Y.ptr(), acc), what, X, Gt, Y)
            assert_written(Y.read(), what)
            close(Y.read(), prod + t["prior"].double() if acc else prod, tol(dtype), what)


def _bcast_bwd(engine, t, N, HW, Cc, dtype, off, modes=(0, 1), want=None):
    dt, x, dy = sgdt(dtype), t["x"], t["dy"]
    for mode in modes:
        gt = t["gc"] if mode == 0 else t["gs"]
        g64 = gt.double()[:, None, :] if mode == 0 else gt.double()[:, :, None]
        dg = (dy.double() * x.double()).sum(1 if mode == 0 else 2)
        nws = _split(engine, N, HW, Cc, off, want) if mode == 0 else engine.lib.sg_bcast_mul_bwd_ws_bytes(engine.h, N, HW, Cc, 1)
        for acc in (0, 1):
            what = f"bcast_mul_bwd mode={mode} acc={acc} N={N} HW={HW} C={Cc} {dtype} off={off}"
            X, Gt, DY, DX = G(x, off), G(gt, off), G(dy, off), out_or_prior(t["prior"], acc, off)
            DG, W = GO(gt.shape, dtype, off), Guarded.ws(nws, DEV)
            rc = call(engine, "sg_bcast_mul_bwd", dt, N, HW, Cc, mode, X.ptr(), Gt.ptr(), DY.ptr(), DX.ptr(), DG.ptr(), acc, W.ptr(), nws)
            done(engine, rc, what, X, Gt, DY, DX, DG, W)
            assert_written(DX.read(), what)
            assert_written(DG.read(), what)
            close(DX.read(), dy.double() * g64 + (t["prior"].double() if acc else 0), tol(dtype), what + " dx")
            close(DG.read(), dg, tol(dtype, True), what + " dg")


def _scse(engine, t, N, HW, Cc, dtype, off, fwd=True, want=None):
    dt, x, dy, s, c = sgdt(dtype), t["x"], t["dy"], t["ls"], t["lc"]
    what = f"scse N={N} HW={HW} C={Cc} {dtype} off={off}"
    ss, sc = sigmoid(s.double()), sigmoid(c.double())
    gate = ss[:, :, None] + sc[:, None, :]
    if fwd:
        X, S_, C_, Y = G(x, off), G(s, off), G(c, off), GO(x.shape, dtype, off)
        done(engine, call(engine, "sg_scse_fwd", dt, N, HW, Cc, X.ptr(), S_.ptr(), C_.ptr(), Y.ptr()), what, X, S_, C_, Y)
        assert_written(Y.read(), what)
        close(Y.read(), x.double() * gate, tol(dtype), what + " fwd")
    nws = _split(engine, N, HW, Cc, off, want, "sg_scse_bwd_ws_bytes")
    X, S_, C_, DY = G(x, off), G(s, off), G(c, off), G(dy, off)
    DX, DS, DC, W = GO(x.shape, dtype, off), GO(s.shape, dtype, off), GO(c.shape, dtype, off), Guarded.ws(nws, DEV)
    rc = call(engine, "sg_scse_bwd", dt, N, HW, Cc, X.ptr(), S_.ptr(), C_.ptr(), DY.ptr(), DX.ptr(), DS.ptr(), DC.ptr(), W.ptr(), nws)
    done(engine, rc, what, X, S_, C_, DY, DX, DS, DC, W)
    for o in (DX, DS, DC):
        assert_written(o.read(), what)
    xd = x.double() * dy.double()
    close(DX.read(), dy.double() * gate, tol(dtype), what + " dx")
    close(DS.read(), ss * (1 - ss) * xd.sum(2), tol(dtype, True), what + " ds")
    close(DC.read(), sc * (1 - sc) * xd.sum(1), tol(dtype, True), what + " dc")


def _bam(engine, t, N, HW, Cc, dtype, off, fwd=True, want=None):
    dt, x, dy, mc, ms = sgdt(dtype), t["x"], t["dy"], t["lc"], t["ls"]
    what = f"bam N={N} HW={HW} C={Cc} {dtype} off={off}"
    gate = sigmoid(mc.double()[:, None, :] + ms.double()[:, :, None])
    if fwd:
        X, MC, MS, Y = G(x, off), G(mc, off), G(ms, off), GO(x.shape, dtype, off)
        done(engine, call(engine, "sg_bam_fwd", dt, N, HW, Cc, X.ptr(), MC.ptr(), MS.ptr(), Y.ptr()), what, X, MC, MS, Y)
        assert_written(Y.read(), what)
        close(Y.read(), x.double() * (1 + gate), tol(dtype), what + " fwd")
    nws = _split(engine, N, HW, Cc, off, want, "sg_bam_bwd_ws_bytes")
    X, MC, MS, DY = G(x, off), G(mc, off), G(ms, off), G(dy, off)
    DX, DMC, DMS, W = GO(x.shape, dtype, off), GO(mc.shape, dtype, off), GO(ms.shape, dtype, off), Guarded.ws(nws, DEV)
    rc = call(engine, "sg_bam_bwd", dt, N, HW, Cc, X.ptr(), MC.ptr(), MS.ptr(), DY.ptr(), DX.ptr(), DMC.ptr(), DMS.ptr(), W.ptr(), nws)
    done(engine, rc, what, X, MC, MS, DY, DX, DMC, DMS, W)
    for o in (DX, DMC, DMS):
        assert_written(o.read(), what)
    term = x.double() * dy.double() * gate * (1 - gate)
    close(DX.read(), dy.double() * (1 + gate), tol(dtype), what + " dx")
    close(DMS.read(), term.sum(2), tol(dtype, True), what + " dms")
    close(DMC.read(), term.sum(1), tol(dtype, True), what + " dmc")


@gpu
@pytest.mark.parametrize("Cc", GATE_CS)
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gates_small_map(engine, dtype, off, Cc):
    # N = 3, HW = 63: 189 rows are no multiple of any rows-per-wave (64 / G), and with G <= 2 one wave spans two images;
    # HW = 63 <= 16 TY for every plan (TY >= 16): the channel reductions run with S = 1 (asserted from the query)
    N, HW = 3, 63
    t = _gate_inputs(N, HW, Cc, dtype, "small")
    _bcast_fwd(engine, t, N, HW, Cc, dtype, off)
    _bcast_bwd(engine, t, N, HW, Cc, dtype, off, want="one")
    _scse(engine, t, N, HW, Cc, dtype, off, want="one")
    _bam(engine, t, N, HW, Cc, dtype, off, want="one")


GATE_SPLITS = [
    # N, HW, C, regime (aligned, offset).  seg_plan: S = min(ceil(4 CUs / gx), ceil(HW / 4 TY)), 1 if HW <= 16 TY.
    (2, 1024, 45, ("few", "few")),     # scalar, TX = TY = 16, gx = 3: HW / 64 = 16 partial rows (any part with >= 12 CUs)
    (2, 1024, 64, ("few", "few")),     # TX = TY = 16, gx = 1 (vector) / 4 (scalar): 16
    (2, 1024, 728, ("few", "few")),    # gx = 12 / 46 column blocks, each split 16 ways (needs >= 12 / 46 * 4 CUs: 184 at the most)
    (2, 4096, 45, ("many", "many")),   # HW / 64 = 64 >= 32: the 16-lane finalize kernel (>= 48 CUs)
    (2, 4096, 64, ("many", "many")),   # the same on the vector plan (>= 16 CUs) and the scalar one (>= 64 CUs)
    (2, 4096, 4, ("one", "few")),      # vector: one chunk, TY = 256, HW = 4096 <= 16 TY: S = 1; scalar: TX = 4, TY = 64: S = 16
]


@gpu
@pytest.mark.parametrize("case", GATE_SPLITS, ids=lambda c: f"hw{c[1]}c{c[2]}")
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_channel_reductions_split(engine, dtype, off, case):
    """dg of sg_bcast_mul_bwd mode 0 (ChanDotOp kind 0), dc of sg_scse_bwd (kind 1), dmc of sg_bam_bwd (BamChanOp) with the rows
    of an image split over S workgroups: partial rows, then seg_finalize_kernel with 4 lanes (S < 32) or 16 (S >= 32)."""
    N, HW, Cc, want = case
    t = _gate_inputs(N, HW, Cc, dtype, "split")
    _bcast_bwd(engine, t, N, HW, Cc, dtype, off, modes=(0,), want=want[off])
    _scse(engine, t, N, HW, Cc, dtype, off, fwd=False, want=want[off])
    _bam(engine, t, N, HW, Cc, dtype, off, fwd=False, want=want[off])


@gpu
def test_gates_wrapped(engine):
    # rowcol_kernel<., 1>: rows * C = 2 * 23 400 * 45 = 2 106 000 > 8192 * 256 items (C odd: scalar); fd_hw divides by 23 400
    N, HW, Cc = 2, 23400, 45
    _bcast_fwd(engine, _gate_inputs(N, HW, Cc, F32, "wrap"), N, HW, Cc, F32, False, modes=(1,))
    # row_reduce_kernel<., 1>: C = 4 through offset pointers is scalar, G = 4, 16 rows per wave, 64 per block: blocks =
    # ceil(524 800 / 64) = 8200 > 8192, so the first eight blocks' waves take a second trip
    N, HW, Cc = 2, 262400, 4
    _bcast_bwd(engine, _gate_inputs(N, HW, Cc, F32, "wrap"), N, HW, Cc, F32, True, modes=(1,))


# ================================================================================================ pooling
POOLS = [pytest.param((3, 2, True), id="k3s2same"), pytest.param((2, 2, False), id="k2s2valid"), pytest.param((2, 4, False), id="k2s4valid")]


def _maxpool_case(engine, dtype, off, cfg, N, H, W, Cc, ref_dtype=torch.float64, bwd=True):
    k, s, same = cfg
    (Ho, pt), (Wo, pl) = pool_geom(H, k, s, same), pool_geom(W, k, s, same)
    dt, g = sgdt(dtype), gen(f"maxpool{cfg}{N}{H}{W}{Cc}{dtype}{off}")
    x = torch.randint(-3, 4, (N, H, W, Cc), generator=g).to(dtype)      # quantised: ties in most windows, exact in bf16
    dy = rnd(g, N, Ho, Wo, Cc, dtype=dtype)
    geo = (N, H, W, Cc, k, s, pt, pl, Ho, Wo)
    what = f"maxpool {cfg} {N}x{H}x{W}x{Cc} {dtype} off={off}"
    yref, iref = maxpool_ref(x.to(ref_dtype), k, s, pt, pl, Ho, Wo)
    assert (iref != 255).all()
    X, Y = G(x, off), GO((N, Ho, Wo, Cc), dtype, off)
    done(engine, call(engine, "sg_maxpool_fwd", dt, *geo, X.ptr(), Y.ptr()), what + " fwd", X, Y)
    assert torch.equal(Y.read().to(ref_dtype), yref), what + " fwd: a window maximum is exact"
    X, Y, I = G(x, off), GO((N, Ho, Wo, Cc), dtype, off), GO((N, Ho, Wo, Cc), torch.uint8, off)
    done(engine, call(engine, "sg_maxpool_fwd_idx", dt, *geo, X.ptr(), Y.ptr(), I.ptr()), what + " fwd_idx", X, Y, I)
    assert torch.equal(Y.read().to(ref_dtype), yref), what + " fwd_idx"
    assert torch.equal(I.read(), iref), what + " fwd_idx: first-maximum cell bytes"
    if not bwd:
        return
    dref = maxpool_bwd_ref(dy.to(ref_dtype), iref, k, s, pt, pl, H, W)
    X, Yi, DY, DX = G(x, off), G(yref.to(dtype), off), G(dy, off), GO((N, H, W, Cc), dtype, off)
    done(engine, call(engine, "sg_maxpool_bwd", dt, *geo, X.ptr(), Yi.ptr(), DY.ptr(), DX.ptr()), what + " bwd", X, Yi, DY, DX)
    DY2, Ii, DX2 = G(dy, off), G(iref, off), GO((N, H, W, Cc), dtype, off)
    done(engine, call(engine, "sg_maxpool_bwd_idx", dt, *geo, DY2.ptr(), Ii.ptr(), DX2.ptr()), what + " bwd_idx", DY2, Ii, DX2)
    a, b = DX.read(), DX2.read()
    assert_written(a, what)
    assert_written(b, what)
    assert torch.equal(a.view(torch.int16 if dtype == BF16 else torch.int32), b.view(torch.int16 if dtype == BF16 else torch.int32)), \
        what + ": the index backward is not bit-identical to the recomputing one"
    close(a, dref, tol(dtype), what + " bwd")
    close(b, dref, tol(dtype), what + " bwd_idx")


@gpu
@pytest.mark.parametrize("Cc", (5, 8, 24))     # 5: V = 1; 8, 24: V = 4 when aligned (idx as packed words), V = 1 when offset
@pytest.mark.parametrize("cfg", POOLS)
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_maxpool(engine, dtype, off, cfg, Cc):
    # odd H and W: 'same' pads one side only / the valid windows leave a remainder; k = 2 stride 4 leaves rows in no window
    _maxpool_case(engine, dtype, off, cfg, 2, 11, 13, Cc)


@gpu
def test_maxpool_wrapped(engine):
    # scalar kernels (C = 5), resample.hip's ew_blocks caps at 16384 blocks: the backward kernels walk N H W C = 917 * 917 * 5 =
    # 4 204 445 > 16384 * 256 input elements (17 MB in fp32)
    _maxpool_case(engine, F32, False, (2, 2, False), 1, 917, 917, 5, ref_dtype=torch.float32)
    # ... and the forward kernels N Ho Wo C = 917 * 917 * 5 output elements: H = W = 1835 (odd), bf16 (34 MB)
    _maxpool_case(engine, BF16, False, (2, 2, False), 1, 1835, 1835, 5, ref_dtype=torch.float32, bwd=False)


AVGPOOLS = [
    # N, H, W, C, kh, kw, regime of the window reduction (rows = kh * kw)
    (2, 19, 21, 8, 8, 8, "one"),       # H % kh = 3, W % kw = 5; 64 rows <= 16 TY: S = 1 (vector, TX = 2)
    (2, 19, 21, 5, 8, 8, "one"),       # the same, scalar
    (2, 7, 11, 12, 2, 3, "one"),       # rectangular, H % kh = 1, W % kw = 2
    (2, 7, 11, 45, 3, 2, "one"),       # kh > kw, scalar, gx = 3
    (2, 32, 32, 64, 32, 32, "few"),    # global pool of 1024 rows: S = 16
    (2, 64, 64, 64, 64, 64, "many"),   # global pool of 4096 rows: S = 64 >= 32 (16-lane finalize)
    (2, 64, 64, 45, 64, 64, "many"),   # the same, scalar
]


def _avgpool_bwd_case(engine, dtype, off, N, H, W, Cc, kh, kw, dy, prior, what):
    dt, Ho, Wo = sgdt(dtype), H // kh, W // kw
    dref = avgpool_bwd_ref(dy.double(), H, W, kh, kw)
    for acc in (0, 1):
        DY, DX = G(dy, off), out_or_prior(prior, acc, off)
        done(engine, call(engine, "sg_avgpool_bwd", dt, N, H, W, Cc, kh, kw, DY.ptr(), DX.ptr(), acc), what + f" bwd acc={acc}", DY, DX)
        dx = DX.read()
        assert_written(dx, what)
        close(dx, dref + prior.double() if acc else dref, tol(dtype), what + f" bwd acc={acc}")
        rem, want_rem = dx.clone(), (prior if acc else torch.zeros_like(prior)).clone()
        rem[:, :Ho * kh, :Wo * kw] = 0
        want_rem[:, :Ho * kh, :Wo * kw] = 0
        assert torch.equal(rem, want_rem), what + ": the remainder rows / columns receive zero (stay untouched under accumulate)"


@gpu
@pytest.mark.parametrize("case", AVGPOOLS, ids=lambda c: "x".join(map(str, c[:6])))
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_avgpool(engine, dtype, off, case):
    N, H, W, Cc, kh, kw, want = case
    Ho, Wo = H // kh, W // kw
    dt, g = sgdt(dtype), gen(f"avgpool{case}{dtype}{off}")
    x, dy, prior = rnd(g, N, H, W, Cc, dtype=dtype), rnd(g, N, Ho, Wo, Cc, dtype=dtype), rnd(g, N, H, W, Cc, dtype=dtype)
    what = f"avgpool {case} {dtype} off={off}"
    nws, nseg, cus = engine.lib.sg_avgpool_ws_bytes(engine.h, N, H, W, Cc, kh, kw), N * Ho * Wo, engine.lib.sg_num_cus(engine.h)
    assert (nws - 256) % (nseg * Cc * 4) == 0
    S_q = (nws - 256) // (nseg * Cc * 4)
    S_vec, S_sc = seg_plan_s(cus, kh * kw, Cc, True), seg_plan_s(cus, kh * kw, Cc, False)
    assert S_q == max(S_vec, S_sc) and regime(S_q) == want and regime(S_vec if (Cc % 4 == 0 and not off) else S_sc) == want, \
        (what, S_q, S_vec, S_sc, cus)
    X, Y, Wk = G(x, off), GO((N, Ho, Wo, Cc), dtype, off), Guarded.ws(nws, DEV)
    done(engine, call(engine, "sg_avgpool_fwd", dt, N, H, W, Cc, kh, kw, X.ptr(), Y.ptr(), Wk.ptr(), nws), what, X, Y, Wk)
    assert_written(Y.read(), what)
    close(Y.read(), avgpool_ref(x.double(), kh, kw), tol(dtype, True), what + " fwd")     # the remainder contributes nothing
    _avgpool_bwd_case(engine, dtype, off, N, H, W, Cc, kh, kw, dy, prior, what)


@gpu
def test_avgpool_wrapped(engine):
    # scalar backward kernel (C = 5): N H W C = 917 * 917 * 5 = 4 204 445 > 16384 * 256 input elements; H % kh = W % kw = 1
    N, H, W, Cc, kh, kw = 1, 917, 917, 5, 2, 2
    g = gen("avgpool wrapped")
    dy, prior = rnd(g, N, H // kh, W // kw, Cc, dtype=F32), rnd(g, N, H, W, Cc, dtype=F32)
    _avgpool_bwd_case(engine, F32, False, N, H, W, Cc, kh, kw, dy, prior, "avgpool wrapped")


# ------------------------------------------------------------------------------------------------ up-sampling
def _up_fwd_case(engine, dtype, off, N, H, W, Cc, sh, sw, ld, mid):
    dt, g = sgdt(dtype), gen(f"upf{N}{H}{W}{Cc}{sh}{sw}{ld}{mid}{dtype}{off}")
    x = rnd(g, N, H, W, Cc, dtype=dtype)
    wide = rnd(g, N, H * sh, W * sw, ld, dtype=dtype)
    start = wide.clone()
    start[..., mid:mid + Cc] = float("nan")
    what = f"upsample_fwd {N}x{H}x{W}x{Cc} s={sh}x{sw} ld={ld}+{mid} {dtype} off={off}"
    X, Y = G(x, off), G(start, off, role="out")
    done(engine, call(engine, "sg_upsample_nearest_fwd", dt, N, H, W, Cc, sh, sw, X.ptr(), Y.ptr(mid), ld if ld != Cc else 0), what, X, Y)
    got = Y.read()
    same_outside(got, start, slice(mid, mid + Cc), what)
    assert torch.equal(got[..., mid:mid + Cc], upsample_ref(x, sh, sw)), what + ": nearest up-sampling is a copy"


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_upsample_fwd(engine, dtype, off):
    _up_fwd_case(engine, dtype, off, 2, 3, 5, 8, 2, 3, 8, 0)     # sh != sw, dense (y_ld = 0): V = 4 when aligned
    _up_fwd_case(engine, dtype, off, 2, 3, 5, 8, 2, 3, 24, 8)    # y_ld = 24 > C, 8 channels into the wider buffer: V = 4
    _up_fwd_case(engine, dtype, off, 2, 3, 5, 8, 3, 2, 13, 3)    # y_ld % 4 = 1: V = 1 although C % 4 = 0
    _up_fwd_case(engine, dtype, off, 2, 3, 5, 5, 2, 3, 11, 4)    # C % 4 = 1: V = 1
    _up_fwd_case(engine, dtype, off, 1, 2, 2, 4, 1, 4, 12, 4)    # sh = 1; bf16: 4 channels in = 8 bytes, not 16-byte aligned: V = 1


def _up_bwd_case(engine, dtype, off, N, H, W, Cc, sh, sw, ld):
    dt, g = sgdt(dtype), gen(f"upb{N}{H}{W}{Cc}{sh}{sw}{ld}{dtype}{off}")
    wide, prior = rnd(g, N, H * sh, W * sw, ld, dtype=dtype), rnd(g, N, H, W, Cc, dtype=dtype)
    ref = upsample_bwd_ref(wide[..., :Cc].double(), sh, sw)
    for acc in (0, 1):
        what = f"upsample_bwd {N}x{H}x{W}x{Cc} s={sh}x{sw} ld={ld} acc={acc} {dtype} off={off}"
        DY, DX = G(wide, off), out_or_prior(prior, acc, off)
        done(engine, call(engine, "sg_upsample_nearest_bwd", dt, N, H, W, Cc, sh, sw, DY.ptr(), ld if ld != Cc else 0, DX.ptr(), acc), what, DY, DX)
        assert_written(DX.read(), what)
        close(DX.read(), ref + prior.double() if acc else ref, tol(dtype), what)


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_upsample_bwd(engine, dtype, off):
    _up_bwd_case(engine, dtype, off, 2, 2, 3, 36, 8, 8, 40)   # window kernel: vector, sh * sw = 64, C / 4 = 9 > 8 chunks: grid.x = 2; dy_ld > C
    _up_bwd_case(engine, dtype, off, 2, 2, 3, 36, 8, 8, 36)   # ... dense
    _up_bwd_case(engine, dtype, off, 2, 3, 5, 8, 2, 3, 12)    # V = 4 kernel (sh * sw = 6 < 64), dy_ld > C
    _up_bwd_case(engine, dtype, off, 2, 3, 5, 5, 2, 3, 7)     # scalar kernel
    _up_bwd_case(engine, dtype, off, 2, 2, 3, 5, 8, 8, 6)     # scalar kernel with sh * sw = 64: C % 4 != 0 keeps it off the window kernel
    _up_bwd_case(engine, dtype, off, 2, 2, 3, 8, 8, 8, 10)    # dy_ld % 4 = 2 does the same


@gpu
def test_upsample_wrapped(engine):
    # scalar backward kernel: N H W C = 917 * 917 * 5 = 4 204 445 > 16384 * 256 output elements, each the sum of 1 x 2 cells
    _up_bwd_case(engine, F32, False, 1, 917, 917, 5, 1, 2, 5)
    # scalar forward kernel: N (H sh) (W sw) C = 917 * 2 * 459 * 5 = 4 209 030 > 16384 * 256
    _up_fwd_case(engine, F32, False, 1, 917, 459, 5, 1, 2, 5, 0)


@gpu
def test_upsample_wrapped_vector(engine):
    # the V = 4 form's second trip, through the cheapest op with an exact reference (a copy: sh = sw = 1): N H W C / 4 =
    # 1025 * 1025 * 4 = 4 202 500 > 16384 * 256 = 4 194 304 chunks (67 MB in fp32, aligned, dense)
    _up_fwd_case(engine, F32, False, 1, 1025, 1025, 16, 1, 1, 16, 0)


# ================================================================================================ loss / metrics
def _loss_inputs(rows, y_cols, tag, lead=0):
    g = gen(f"loss{rows}{y_cols}{tag}")
    p = torch.softmax(rnd(g, rows + lead, 2, lo=-4, hi=4).double(), dim=1).float()
    fg = (torch.rand(rows + lead, generator=g) > 0.6).float()
    cols = [1 - fg, fg]
    if y_cols == 4:
        cols += [1 + (torch.rand(rows + lead, generator=g) > 0.7).float(), 1 + (torch.rand(rows + lead, generator=g) > 0.8).float()]
    return p, torch.stack(cols, 1).contiguous()


def _loss_case(engine, rows, y_cols, kinds, scales, off=False, p=None, yt=None, fwd=True):
    lead = 1 if off else 0
    if p is None:
        p, yt = _loss_inputs(rows, y_cols, "x", lead)
    for kind in kinds:
        what = f"loss kind={kind} rows={rows} y_cols={y_cols} off={off}"
        bad = kind == 2 and y_cols == 2
        nws = engine.lib.sg_loss_ws_bytes(engine.h, rows)
        if fwd:
            P, Y, L, W = G(p), G(yt), GO((1,), F32), Guarded.ws(nws, DEV)
            rc = call(engine, "sg_loss_fwd", kind, rows, y_cols, P.ptr(2 * lead), Y.ptr(y_cols * lead), L.ptr(), W.ptr(), nws)
            if bad:   # edge_focal_loss needs the two weight columns: refused, nothing launched, nothing written
                assert rc == SG_EINVAL, what
                check_all((P, Y, L, W), what)
                assert torch.isnan(L.read()).all() and (W.fetch().after == 0xFF).all(), what
            else:
                done(engine, rc, what, P, Y, L, W)
                close(L.read(), loss_ref(kind, p[lead:].double(), yt[lead:].double()).reshape(1), tol(F32, True), what + " fwd")
        for gs in scales:
            P, Y, DP = G(p), G(yt), GO((rows + lead, 2), F32)
            rc = call(engine, "sg_loss_bwd", kind, rows, y_cols, P.ptr(2 * lead), Y.ptr(y_cols * lead), DP.ptr(2 * lead), gs)
            if bad:
                assert rc == SG_EINVAL, what
                check_all((P, Y, DP), what)
                assert torch.isnan(DP.read()).all(), what
                continue
            done(engine, rc, what, P, Y, DP)
            dp = DP.read()
            assert torch.isnan(dp[:lead]).all()
            assert_written(dp[lead:], what)
            close(dp[lead:], loss_bwd_ref(kind, p[lead:].double(), yt[lead:].double(), gs), tol(F32), what + f" bwd scale={gs}")


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("y_cols", (2, 4))
def test_loss(engine, y_cols, off):
    for rows in (1, 255, 1025):      # 1 block with 1 / 255 live threads; 2 blocks, each thread up to 4 rows
        _loss_case(engine, rows, y_cols, (0, 1, 2), (1.0, 0.25), off)


@gpu
def test_loss_wrapped(engine):
    _loss_case(engine, 600001, 4, (0, 1, 2), (1.0,))                 # loss_parts = 586 blocks of 256 threads x 4+ rows each
    _loss_case(engine, 600001, 2, (1,), (0.25,))
    _loss_case(engine, EW_CAP + 1027, 2, (1,), (0.25,), fwd=False)   # sg_loss_bwd's grid caps at 8192 blocks: rows > 8192 * 256
    _loss_case(engine, 2048 * 1024 + 1027, 2, (0,), ())               # loss_parts itself caps at 2048 blocks of 1024 rows


@gpu
@pytest.mark.parametrize("y_cols", (2, 4))
def test_loss_at_probabilities_zero_and_one(engine, y_cols):
    # 64 rows of p = (0, 1) / (1, 0) exactly, both label values on each: log(0 + 1e-7), 1 / (0 + 1e-7) and (1 - 1)^2 stay finite
    rows = 64
    p = torch.zeros(rows, 2)
    p[torch.arange(rows), torch.arange(rows) % 2] = 1.0
    _, yt = _loss_inputs(rows, y_cols, "edge")
    yt[:, 1] = ((torch.arange(rows) // 2) % 2).float()
    yt[:, 0] = 1 - yt[:, 1]
    _loss_case(engine, rows, y_cols, (0, 1, 2) if y_cols == 4 else (0, 1), (1.0, 0.25), p=p, yt=yt)


def _confusion_inputs(rows, y_cols, tag):
    g = gen(f"conf{rows}{y_cols}{tag}")
    p, yt = _loss_inputs(rows, y_cols, tag)
    near = (p[:, 0] - p[:, 1]).abs() < 1e-3      # no pair closer than 1e-3 ...
    p[near] = torch.tensor([0.25, 0.75])
    r = torch.rand(rows, generator=g)
    p[r < 0.1] = 0.5                             # ... except exact ties p0 == p1 -> class 0
    yt[(r > 0.3) & (r < 0.4), :2] = 1.0          # y0 == y1 == 1 -> class 0
    yt[(r > 0.6) & (r < 0.7), :2] = 0.0          # y0 == y1 == 0 -> class 0
    d32, d64 = p[:, 1] - p[:, 0], p[:, 1].double() - p[:, 0].double()
    assert torch.equal(d32 > 0, d64 > 0) and ((d64 == 0) | (d64.abs() >= 1e-3)).all()
    return p, yt.contiguous()


@gpu
@pytest.mark.parametrize("y_cols", (2, 4))
def test_confusion_counts(engine, y_cols):
    for rows in (1, 255, 1025, 600001):
        start = torch.tensor([5, 7, 11, 13], dtype=torch.int64)     # a non-zero `out`: the counts are accumulated
        want, O = start.clone(), G(start, role="out")
        for call_no in range(2):                                    # two calls into the same out
            p, yt = _confusion_inputs(rows, y_cols, f"c{call_no}")
            if rows >= 255:
                assert (p[:, 0] == p[:, 1]).any() and (yt[:, 0] == yt[:, 1]).any()
            want += confusion_ref(p, yt)
            P, Y = G(p), G(yt)
            done(engine, call(engine, "sg_confusion_counts", rows, y_cols, P.ptr(), Y.ptr(), O.ptr()), f"confusion rows={rows}", P, Y, O)
            assert torch.equal(O.read(), want), (rows, y_cols, call_no, O.read(), want)
        assert int(want.sum()) == int(start.sum()) + 2 * rows


# ================================================================================================ Adam
def _adam_case(engine, n, gs, lr_dev):
    g = gen(f"adam{n}{gs}")
    w, m, gr = rnd(g, n), rnd(g, n, lo=-0.1, hi=0.1), rnd(g, n)
    v = rnd(g, n, lo=0.0, hi=0.01)
    cold = torch.arange(n) % 7 == 3          # elements with v = g = 0: the step is lr_t * b1 * m / eps
    v[cold], gr[cold] = 0.0, 0.0
    m[cold] *= 1e-6                          # (m small there, or 1 / eps = 1e7 would make the step the largest number of the tensor)
    lr_t, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-7
    what = f"adam n={n} grad_scale={gs} lr_dev={lr_dev}"
    Wt, M, V, Gr = G(w, role="out"), G(m, role="out"), G(v, role="out"), G(gr)
    if lr_dev:
        LR = G(torch.tensor([lr_t]))
        rc = call(engine, "sg_adam_step_lr", n, Wt.ptr(), M.ptr(), V.ptr(), Gr.ptr(), LR.ptr(), b1, b2, eps, gs)
        done(engine, rc, what, Wt, M, V, Gr, LR)
    else:
        done(engine, call(engine, "sg_adam_step", n, Wt.ptr(), M.ptr(), V.ptr(), Gr.ptr(), lr_t, b1, b2, eps, gs), what, Wt, M, V, Gr)
    f = lambda t: t.double()
    w2, m2, v2 = adam_ref(f(w), f(m), f(v), f(gr), float(torch.tensor(lr_t)), float(torch.tensor(b1)), float(torch.tensor(b2)),
                          float(torch.tensor(eps)), gs)
    for name, got, ref in (("w", Wt.read(), w2), ("m", M.read(), m2), ("v", V.read(), v2)):
        close(got, ref, tol(F32), f"{what} {name}")
        if cold.any():   # the cold elements once more on their own scale (m there is 1e-6 of the others)
            close(got[cold], ref[cold], tol(F32), f"{what} {name} (v = g = 0)")
    return Wt.read(), M.read(), V.read()


@gpu
@pytest.mark.parametrize("gs", (1.0, 0.5))
def test_adam(engine, gs):
    for n in (1, 2, 3, 4, 5, 1023):          # n < 4: tail only; 4: one vector item; 5, 1023: vector items + 1 / 3 tail elements
        a = _adam_case(engine, n, gs, False)
        b = _adam_case(engine, n, gs, True)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"sg_adam_step_lr differs from sg_adam_step at n={n}"


@gpu
def test_adam_wrapped(engine):
    n = 4 * EW_CAP + 7                       # n / 4 > 8192 * 256 vector items and a 3-element tail (34 MB per arena)
    a = _adam_case(engine, n, 0.5, False)
    b = _adam_case(engine, n, 0.5, True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


@gpu
def test_adam_refuses_unaligned_arenas(engine):
    n = 8
    t = [torch.ones(n) for _ in range(4)]
    for which in range(4):
        ops = [G(x, off=(i == which), role="in") for i, x in enumerate(t)]
        LR = G(torch.tensor([1e-3]))
        assert call(engine, "sg_adam_step", n, *[o.ptr() for o in ops], 1e-3, 0.9, 0.999, 1e-7, 1.0) == SG_EINVAL
        assert call(engine, "sg_adam_step_lr", n, *[o.ptr() for o in ops], LR.ptr(), 0.9, 0.999, 1e-7, 1.0) == SG_EINVAL
        check_all(ops + [LR], "adam unaligned")


# ================================================================================================ inference tail
@gpu
def test_argmax_accumulate_overhang(engine):
    TH, TW, CH, CW = 20, 30, 32, 40          # 600 tile pixels: three blocks, the last one partly live
    g = gen("argmax")
    p, _ = _confusion_inputs(TH * TW, 2, "tile")
    mask = (p[:, 1] > p[:, 0]).reshape(TH, TW).to(torch.int8)
    canvas = torch.randint(0, 5, (CH, CW), generator=g).to(torch.int8)
    # inside; over the top, bottom, left and right edge; over a corner; wholly outside
    for y0, x0 in ((3, 4), (-7, 4), (CH - 9, 4), (3, -11), (3, CW - 13), (-7, -11), (CH - 9, CW - 13), (CH, 0), (0, -TW)):
        want = canvas.clone()
        ys, xs = max(y0, 0), max(x0, 0)
        ye, xe = min(y0 + TH, CH), min(x0 + TW, CW)
        if ye > ys and xe > xs:
            want[ys:ye, xs:xe] += mask[ys - y0:ye - y0, xs - x0:xe - x0]
        P, Cv = G(p), G(canvas, role="out")
        what = f"argmax_accumulate at ({y0}, {x0})"
        done(engine, call(engine, "sg_argmax_accumulate_i8", P.ptr(), TH, TW, Cv.ptr(), CH, CW, y0, x0), what, P, Cv)
        assert torch.equal(Cv.read(), want), what + ": only the overlap changes"


def _vote_case(engine, nm, k, n, fill):
    g = gen(f"vote{nm}{k}{n}")
    vals = torch.tensor([0, 255, 128, 254, 255, 0], dtype=torch.uint8)      # only 255 votes (mask // 255)
    masks = [vals[torch.randint(0, 6, (n,), generator=g)] for _ in range(nm)]
    want = torch.where(sum((m == 255).to(torch.int32) for m in masks) >= k, 255, 0).to(torch.uint8)
    MS = [G(m, off=(i % 2 == 1)) for i, m in enumerate(masks)]
    O = Guarded.out((n,), torch.uint8, DEV, off=True, fill=fill)
    arr = (C.c_void_p * nm)(*[m.ptr() for m in MS])
    what = f"vote nmasks={nm} k={k} n={n}"
    done(engine, call(engine, "sg_vote_ge", nm, arr, n, k, O.ptr()), what, O, *MS)
    if fill != 0xFF:
        assert_written(O.read(), what, fill=fill)
    assert torch.equal(O.read(), want), what


@gpu
def test_vote_ge(engine):
    for nm in (1, 5, 8):
        for k in (1, nm):
            # 255 is both the prefill and a legitimate result: the exact comparison finds an unwritten element where the vote
            # fails, a second run from a prefill the kernel never produces (0x01) finds it where the vote passes
            _vote_case(engine, nm, k, 1027, 0xFF)
            _vote_case(engine, nm, k, 1027, 0x01)
    _vote_case(engine, 5, 3, EW_CAP + 1027, 0x01)       # n > 8192 * 256 bytes: the grid-stride loop's second trip
