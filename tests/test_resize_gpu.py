"""sg_resize_fwd / _bwd (csrc/resample.hip, csrc/resize_coords.h) through the C ABI, in tests/_guarded.py arenas, against the
float64 restatement tests/_resize_ref.py (which tests/test_resize_cpu.py holds to torch's float64 interpolate and autograd).

Tolerances are those of tests/test_upsample_bilinear_gpu.py, as max|got - ref| <= tol * max|ref|: 2e-5 fp32 forward, 1e-4 fp32
backward (a reduction), 2^-7 for bf16 storage; bf16 references start from the same bf16-rounded inputs (and, on an accumulate,
the bf16-rounded prior output).  Nearest is a gather forward and a sum of few terms in a stated order backward: bit for bit
in fp32 (and the forward in bf16 as well).  Every shape runs with C in {1, 3, 8, 12}, 16-byte aligned and one-element-offset
operands, a dense and a wider pixel stride, both methods, both dtypes, accumulate 0 and 1.

The wrapped grid: the case N = 2, (64, 64) -> (160, 176), C = 48 has 675 840 chunk work items, fewer than the 16384 * 256 =
4 194 304 after which pixel_kernel's loop takes a second trip, so it runs as a plain large case and the wrap is taken by
(160, 176) -> (400, 440) forward and its reverse backward at the same N and C (4 224 000 items each)."""
import zlib

import numpy as np
import pytest
import torch

import _resize_ref as R
from _guarded import Guarded, assert_written, check_all, close, same_outside

gpu = pytest.mark.gpu

SG_F32, SG_BF16, SG_EINVAL = 0, 1, -1
BILINEAR, NEAREST = 0, 1
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
OFFS = [pytest.param(False, id="aligned"), pytest.param(True, id="offset")]
METHODS = [pytest.param(BILINEAR, id="bilinear"), pytest.param(NEAREST, id="nearest")]
NAMES = {BILINEAR: "bilinear", NEAREST: "nearest"}
SP_CAP = 16384 * 256     # work items after which resample.hip's grid-stride loops take a second trip
SHAPES = [(5, 7, 8, 5),       # up on one axis, down on the other
          (8, 8, 3, 3),       # source pixels that no output touches
          (1, 1, 4, 6), (4, 6, 1, 1),
          (6, 6, 6, 6),       # the identity
          (6, 9, 9, 6),       # the exact-tie pair of nearest
          (3, 4, 12, 16),     # the integer factor 4
          (16, 16, 40, 24)]
CHANNELS = (1, 3, 8, 12)


def sgdt(dtype):
    return SG_BF16 if dtype == BF16 else SG_F32


def tol(dtype, reduced=False):
    return 2.0 ** -7 if dtype == BF16 else (1e-4 if reduced else 2e-5)


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) % (2 ** 31))


def rnd(g, *shape, dtype=F32):
    return (torch.rand(*shape, generator=g) * 2 - 1).float().to(dtype)


def call(engine, name, *args):
    return getattr(engine.lib, name)(engine.h, engine.stream, *args)


def done(engine, rc, what, *ops):
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    check_all(ops, what)


def bits(t):
    return t.contiguous().view(torch.uint8)


def ref_fwd(x, oh, ow, method):
    return torch.from_numpy(R.resize_fwd(x.double().numpy(), oh, ow, NAMES[method]))


def ref_bwd(dy, h, w, method):
    return torch.from_numpy(R.resize_bwd(dy.double().numpy(), h, w, NAMES[method]))


def untouched(n, m, method):
    """bool [n]: input positions of one axis that no output reads."""
    hit = np.zeros(n, dtype=bool)
    if method == NEAREST:
        hit[R.nearest_src(n, m)] = True
    else:
        lo, hi, _, _ = R.taps(n, m)
        hit[lo] = True
        hit[hi] = True
    return torch.from_numpy(~hit)


# ------------------------------------------------------------------------------------------------ forward
def _fwd_launch(engine, dtype, off, method, x, start, Cc, ld, mid, what):
    N, H, W, _ = x.shape
    OH, OW = start.shape[1:3]
    X, Y = Guarded(x, DEV, off=off), Guarded(start, DEV, off=off, role="out")
    done(engine, call(engine, "sg_resize_fwd", sgdt(dtype), method, N, H, W, Cc, OH, OW, X.ptr(), Y.ptr(mid), ld if ld != Cc else 0),
         what, X, Y)
    return Y.read()


def _fwd_case(engine, dtype, off, method, N, H, W, OH, OW, Cc, ld=None, mid=0):
    ld = Cc if ld is None else ld
    g = gen(f"rsf{N}{H}{W}{OH}{OW}{Cc}{ld}{mid}{dtype}{off}{method}")
    x = rnd(g, N, H, W, Cc, dtype=dtype)
    start = rnd(g, N, OH, OW, ld, dtype=dtype)
    before = start.clone()
    start[..., mid:mid + Cc] = float("nan")
    what = f"resize_fwd {NAMES[method]} {N}x{H}x{W}x{Cc} -> {OH}x{OW} ld={ld}+{mid} {dtype} off={off}"
    ref = ref_fwd(x, OH, OW, method)
    got = _fwd_launch(engine, dtype, off, method, x, start, Cc, ld, mid, what)
    same_outside(got, before, slice(mid, mid + Cc), what)
    y = got[..., mid:mid + Cc].contiguous()
    assert_written(y, what)
    err = close(y, ref, tol(dtype), what)
    print(f"{what}: max err {err:.3e} (bound {tol(dtype) * ref.abs().max().item():.3e})")
    if method == NEAREST:
        assert torch.equal(bits(y), bits(ref.to(dtype))), f"{what}: a gather returns its source's bits"
    if (H, W) == (OH, OW):
        assert torch.equal(bits(y), bits(x)), f"{what}: equal sizes are the identity, bit for bit"
    return x, y


@gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_fwd(engine, dtype, off, method):
    for (H, W, OH, OW) in SHAPES:
        for Cc in CHANNELS:
            _fwd_case(engine, dtype, off, method, 2, H, W, OH, OW, Cc)
            _fwd_case(engine, dtype, off, method, 2, H, W, OH, OW, Cc, Cc + 4, 2)     # y_ld > C, a slice in the middle
    _fwd_case(engine, dtype, off, method, 2, 5, 7, 8, 5, 8, 13, 3)                    # y_ld % 4 = 1: scalar although C % 4 = 0


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_fwd_at_an_integer_factor_against_the_integer_factor_kernel(engine, dtype):
    """(3, 4) -> (12, 16): within tolerance of sg_upsample_bilinear_fwd (whether the bits agree is printed, not asserted: that
    kernel forms f as (2p + 1 - s) / (2s), this one as r / (2m), the same rational from other integers)."""
    for Cc in CHANNELS:
        x, y = _fwd_case(engine, dtype, False, BILINEAR, 2, 3, 4, 12, 16, Cc)
        X, Y = Guarded(x, DEV), Guarded.out((2, 12, 16, Cc), dtype, DEV)
        done(engine, call(engine, "sg_upsample_bilinear_fwd", sgdt(dtype), 2, 3, 4, Cc, 4, 4, X.ptr(), Y.ptr(), 0), "integer factor", X, Y)
        other = Y.read()
        close(y, other.double(), tol(dtype), f"general against integer-factor forward, C={Cc} {dtype}")
        print(f"(3,4)->(12,16) C={Cc} {dtype}: bits equal to sg_upsample_bilinear_fwd: {torch.equal(bits(y), bits(other))}")


# ------------------------------------------------------------------------------------------------ backward
def _bwd_launch(engine, dtype, off, method, wide, prior, Cc, ld, acc, what):
    N, H, W, _ = prior.shape
    OH, OW = wide.shape[1:3]
    DY = Guarded(wide, DEV, off=off)
    DX = Guarded(prior, DEV, off=off, role="out") if acc else Guarded.out(prior.shape, prior.dtype, DEV, off=off)
    done(engine, call(engine, "sg_resize_bwd", sgdt(dtype), method, N, H, W, Cc, OH, OW, DY.ptr(), ld if ld != Cc else 0, DX.ptr(), acc),
         what, DY, DX)
    return DX.read()


def _bwd_case(engine, dtype, off, method, N, H, W, OH, OW, Cc, ld=None):
    ld = Cc if ld is None else ld
    g = gen(f"rsb{N}{H}{W}{OH}{OW}{Cc}{ld}{dtype}{off}{method}")
    wide, prior = rnd(g, N, OH, OW, ld, dtype=dtype), rnd(g, N, H, W, Cc, dtype=dtype)
    what = f"resize_bwd {NAMES[method]} {N}x{H}x{W}x{Cc} <- {OH}x{OW} ld={ld} {dtype} off={off}"
    dy = wide[..., :Cc].contiguous()
    ref = ref_bwd(dy, H, W, method)
    free = untouched(H, OH, method)[:, None] | untouched(W, OW, method)[None, :]      # [H,W]: pixels no output touches
    for acc in (0, 1):
        dx = _bwd_launch(engine, dtype, off, method, wide, prior, Cc, ld, acc, what + f" acc={acc}")
        assert_written(dx, what + f" acc={acc}")
        want = ref + prior.double() if acc else ref
        err = close(dx, want, tol(dtype, True), what + f" acc={acc}")
        print(f"{what} acc={acc}: max err {err:.3e} (bound {tol(dtype, True) * want.abs().max().item():.3e})")
        if free.any():
            there = dx[:, free]
            if acc:
                assert torch.equal(bits(there), bits(prior[:, free])), f"{what}: an untouched pixel keeps its prior value to the bit"
            else:
                assert (there == 0).all(), f"{what}: an untouched pixel's gradient is 0"
        if method == NEAREST and dtype == F32:
            exact = torch.from_numpy(R.nearest_bwd_f32(dy.numpy(), H, W))
            exact = exact + prior if acc else exact
            assert torch.equal(bits(dx), bits(exact)), f"{what} acc={acc}: the sums of a run in their stated order, bit for bit"
    return wide, prior


@gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_bwd(engine, dtype, off, method):
    for (H, W, OH, OW) in SHAPES:
        for Cc in CHANNELS:
            _bwd_case(engine, dtype, off, method, 2, H, W, OH, OW, Cc)
            _bwd_case(engine, dtype, off, method, 2, H, W, OH, OW, Cc, Cc + 4)        # dy_ld > C
    _bwd_case(engine, dtype, off, method, 2, 5, 7, 8, 5, 8, 13)                       # dy_ld % 4 = 1: scalar although C % 4 = 0


def test_the_shapes_hold_what_they_are_there_for():
    assert untouched(8, 3, BILINEAR).any() and untouched(8, 3, NEAREST).any()
    assert not untouched(5, 8, BILINEAR).any()
    o = np.arange(9)
    assert ((((2 * o + 1) * 6) % 18) == 0).any(), "(6 -> 9): an output whose nearest source is an exact tie"
    assert 2 * 160 * 176 * (48 // 4) < SP_CAP < 2 * 400 * 440 * (48 // 4)


# ------------------------------------------------------------------------------------------------ large grids
@gpu
def test_resize_large_case_of_the_issue(engine):
    _fwd_case(engine, F32, False, BILINEAR, 2, 64, 64, 160, 176, 48)
    _bwd_case(engine, F32, False, BILINEAR, 2, 64, 64, 160, 176, 48)


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_resize_wrapped_grid(engine, method):
    """More than 16384 * 256 chunk work items: the forward on the output grid, the backward on the input grid."""
    assert 2 * 400 * 440 * (48 // 4) > SP_CAP
    _fwd_case(engine, F32, False, method, 2, 160, 176, 400, 440, 48)
    g = gen(f"rswrapb{method}")
    wide, prior = rnd(g, 2, 160, 176, 48), rnd(g, 2, 400, 440, 48)
    dx = _bwd_launch(engine, F32, False, method, wide, prior, 48, 48, 0, "wrapped backward")
    assert_written(dx, "wrapped backward")
    close(dx, ref_bwd(wide, 400, 440, method), tol(F32, True), "wrapped backward")


# ------------------------------------------------------------------------------------------------ invariants
INVARIANT_SHAPES = [(5, 7, 8, 5, 8), (8, 8, 3, 3, 3), (16, 16, 40, 24, 12), (4, 6, 1, 1, 1)]


@gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_bwd_twice_gives_the_same_bits(engine, dtype, method):
    for (H, W, OH, OW, Cc) in INVARIANT_SHAPES:
        g = gen(f"rstwice{H}{W}{OH}{OW}{Cc}{dtype}{method}")
        wide, prior = rnd(g, 2, OH, OW, Cc, dtype=dtype), rnd(g, 2, H, W, Cc, dtype=dtype)
        for acc in (0, 1):
            a = _bwd_launch(engine, dtype, False, method, wide, prior, Cc, Cc, acc, "first")
            b = _bwd_launch(engine, dtype, False, method, wide, prior, Cc, Cc, acc, "second")
            assert torch.equal(bits(a), bits(b))


@gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_resize_image_1_of_a_batch_equals_the_single_image_launch(engine, dtype, method):
    for (H, W, OH, OW, Cc) in INVARIANT_SHAPES:
        g = gen(f"rsslice{H}{W}{OH}{OW}{Cc}{dtype}{method}")
        x, dy = rnd(g, 2, H, W, Cc, dtype=dtype), rnd(g, 2, OH, OW, Cc, dtype=dtype)
        nan_y, prior = torch.full_like(dy, float("nan")), rnd(g, 2, H, W, Cc, dtype=dtype)
        y2 = _fwd_launch(engine, dtype, False, method, x, nan_y, Cc, Cc, 0, "fwd batch 2")
        y1 = _fwd_launch(engine, dtype, False, method, x[1:2].contiguous(), nan_y[1:2].contiguous(), Cc, Cc, 0, "fwd image 1")
        assert torch.equal(bits(y2[1:2]), bits(y1))
        for acc in (0, 1):
            d2 = _bwd_launch(engine, dtype, False, method, dy, prior, Cc, Cc, acc, "bwd batch 2")
            d1 = _bwd_launch(engine, dtype, False, method, dy[1:2].contiguous(), prior[1:2].contiguous(), Cc, Cc, acc, "bwd image 1")
            assert torch.equal(bits(d2[1:2]), bits(d1))


# ------------------------------------------------------------------------------------------------ refusals
@gpu
def test_resize_refuses_before_any_launch(engine):
    x, wide = torch.zeros(1, 2, 2, 8), torch.zeros(1, 4, 4, 8)
    X, Y = Guarded(x, DEV), Guarded.out(wide.shape, F32, DEV)
    DY, DX = Guarded(wide, DEV), Guarded.out(x.shape, F32, DEV)
    ok = dict(dtype=SG_F32, method=BILINEAR, N=1, H=2, W=2, C=8, OH=4, OW=4, x=X.ptr(), y=Y.ptr(), dy=DY.ptr(), dx=DX.ptr(), ld=0)
    bad = [dict(H=0), dict(W=0), dict(OH=0), dict(OW=0), dict(H=16385), dict(W=16385), dict(OH=16385), dict(OW=16385),
           dict(x=None, dy=None), dict(y=None, dx=None), dict(method=2), dict(method=-1), dict(dtype=2), dict(ld=4),
           dict(N=2, H=16384, W=16384, C=4),              # N H W C = 2^31
           dict(N=2, OH=16384, OW=16384, C=4),            # N OH OW C = 2^31
           dict(N=2, OH=16384, OW=8192, C=4, ld=8)]       # ... with the pixel stride
    for change in bad:
        a = dict(ok, **change)
        rc = call(engine, "sg_resize_fwd", a["dtype"], a["method"], a["N"], a["H"], a["W"], a["C"], a["OH"], a["OW"], a["x"], a["y"], a["ld"])
        assert rc == SG_EINVAL, f"forward {change}: rc={rc}"
        assert engine.lib.sg_last_error().decode().startswith("sg_resize_fwd"), change
        rc = call(engine, "sg_resize_bwd", a["dtype"], a["method"], a["N"], a["H"], a["W"], a["C"], a["OH"], a["OW"], a["dy"], a["ld"], a["dx"], 0)
        assert rc == SG_EINVAL, f"backward {change}: rc={rc}"
        assert engine.lib.sg_last_error().decode().startswith("sg_resize_bwd"), change
    check_all((X, Y, DY, DX), "refused launches")
    assert torch.isnan(Y.read()).all() and torch.isnan(DX.read()).all(), "a refused launch writes nothing"
    # and the same operands are accepted
    assert call(engine, "sg_resize_fwd", SG_F32, BILINEAR, 1, 2, 2, 8, 4, 4, X.ptr(), Y.ptr(), 0) == 0
    assert call(engine, "sg_resize_bwd", SG_F32, BILINEAR, 1, 2, 2, 8, 4, 4, DY.ptr(), 0, DX.ptr(), 0) == 0
    check_all((X, DY), "accepted launches")
