"""sg_upsample_bilinear_fwd / _bwd (csrc/resample.hip) through the C ABI, in tests/_guarded.py arenas, against float64 on the CPU.

Semantics: tf.image.resize(method='bilinear'), half-pixel centres, no antialiasing, integer factor s per axis:
    in = (o + 0.5) / s - 0.5,  lo = max(floor(in), 0),  hi = min(ceil(in), n - 1),  f = in - floor(in),  y = x[lo] + (x[hi] - x[lo]) f
and the backward is its transpose.  The reference is written twice - that formula restated in float64, and torch's float64
interpolate(mode='bilinear', align_corners=False) with its autograd - and the two must agree to 1e-12 before the GPU is compared
with either.  Tolerances as max|got - ref| <= tol * max|ref|: 2e-5 fp32 forward, 1e-4 fp32 backward (a reduction), 2^-7 for bf16
storage; bf16 references start from the same bf16-rounded inputs (and, on an accumulate, the bf16-rounded prior output).
Every case runs for both dtypes and for 16-byte aligned and one-element-offset operands (the scalar kernels)."""
import zlib

import pytest
import torch

from _guarded import Guarded, assert_written, check_all, close, same_outside

gpu = pytest.mark.gpu

SG_F32, SG_BF16, SG_EINVAL = 0, 1, -1
DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
OFFS = [pytest.param(False, id="aligned"), pytest.param(True, id="offset")]
SP_CAP = 16384 * 256     # work items after which resample.hip's grid-stride loops take a second trip
REF_AGREE = 1e-12


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


# ------------------------------------------------------------------------------------------------ the two references (float64)
def axis_taps(n, s):
    o = torch.arange(n * s, dtype=F64)
    src = (o + 0.5) / s - 0.5
    fl = torch.floor(src)
    return fl.clamp(min=0).long(), torch.ceil(src).clamp(max=n - 1).long(), src - fl


def formula_fwd(x, sh, sw):
    lo, hi, f = axis_taps(x.shape[1], sh)
    x = x[:, lo] + (x[:, hi] - x[:, lo]) * f[None, :, None, None]
    lo, hi, f = axis_taps(x.shape[2], sw)
    return x[:, :, lo] + (x[:, :, hi] - x[:, :, lo]) * f[None, None, :, None]


def formula_bwd(dy, sh, sw):
    """dx[i] collects (1 - f) dy[o] from every o with lo(o) == i and f dy[o] from every o with hi(o) == i, per axis."""
    N, OH, OW, C = dy.shape
    lo, hi, f = axis_taps(OH // sh, sh)
    f = f[None, :, None, None]
    t = torch.zeros(N, OH // sh, OW, C, dtype=F64).index_add_(1, lo, dy * (1 - f)).index_add_(1, hi, dy * f)
    lo, hi, f = axis_taps(OW // sw, sw)
    f = f[None, None, :, None]
    return torch.zeros(N, OH // sh, OW // sw, C, dtype=F64).index_add_(2, lo, t * (1 - f)).index_add_(2, hi, t * f)


def torch_fwd(x, sh, sw):
    y = torch.nn.functional.interpolate(x.permute(0, 3, 1, 2), size=(x.shape[1] * sh, x.shape[2] * sw), mode="bilinear",
                                        align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous()


def torch_bwd(dy, sh, sw):
    N, OH, OW, C = dy.shape
    x = torch.zeros(N, OH // sh, OW // sw, C, dtype=F64, requires_grad=True)
    torch_fwd(x, sh, sw).backward(dy)
    return x.grad


def _agreed(a, b, what):
    assert a.dtype == F64 and b.dtype == F64 and a.shape == b.shape, what
    err = (a - b).abs().max().item()
    assert err <= REF_AGREE, f"{what}: the formula and torch's float64 interpolate differ by {err:.3e}"
    return a


def ref_fwd(x, sh, sw, what):
    return _agreed(formula_fwd(x.double(), sh, sw), torch_fwd(x.double(), sh, sw), what + " (forward references)")


def ref_bwd(dy, sh, sw, what):
    return _agreed(formula_bwd(dy.double(), sh, sw), torch_bwd(dy.double(), sh, sw), what + " (backward references)")


def test_references_agree_down_to_one_pixel_and_up_to_factor_32():
    g = gen("refs")
    for (H, W, sh, sw) in [(1, 1, 32, 32), (1, 3, 2, 7), (3, 1, 5, 4), (4, 5, 3, 2), (2, 2, 16, 8), (3, 3, 1, 1)]:
        x, dy = rnd(g, 2, H, W, 3).double(), rnd(g, 2, H * sh, W * sw, 3).double()
        y, dx = ref_fwd(x, sh, sw, f"{H}x{W} s={sh}x{sw}"), ref_bwd(dy, sh, sw, f"{H}x{W} s={sh}x{sw}")
        # the backward is the transpose: <y(x), dy> = <x, dx(dy)>
        assert abs((y * dy).sum().item() - (x * dx).sum().item()) <= 1e-10
    ones = torch.ones(1, 1, 1, 2, dtype=F64)
    assert torch.equal(formula_fwd(ones, 4, 4), torch.ones(1, 4, 4, 2, dtype=F64))            # a 1x1 source: a broadcast ...
    assert torch.equal(formula_bwd(torch.ones(1, 4, 4, 2, dtype=F64), 4, 4), 16 * ones)       # ... and a plain sum


# ------------------------------------------------------------------------------------------------ forward
def _fwd_launch(engine, dtype, off, x, start, Cc, sh, sw, ld, mid, what):
    N, H, W, _ = x.shape
    X, Y = Guarded(x, DEV, off=off), Guarded(start, DEV, off=off, role="out")
    done(engine, call(engine, "sg_upsample_bilinear_fwd", sgdt(dtype), N, H, W, Cc, sh, sw, X.ptr(), Y.ptr(mid), ld if ld != Cc else 0),
         what, X, Y)
    return Y.read()


def _fwd_case(engine, dtype, off, N, H, W, Cc, sh, sw, ld=None, mid=0):
    ld = Cc if ld is None else ld
    g = gen(f"bilf{N}{H}{W}{Cc}{sh}{sw}{ld}{mid}{dtype}{off}")
    x = rnd(g, N, H, W, Cc, dtype=dtype)
    start = rnd(g, N, H * sh, W * sw, ld, dtype=dtype)
    before = start.clone()
    start[..., mid:mid + Cc] = float("nan")
    what = f"bilinear_fwd {N}x{H}x{W}x{Cc} s={sh}x{sw} ld={ld}+{mid} {dtype} off={off}"
    ref = ref_fwd(x, sh, sw, what)
    got = _fwd_launch(engine, dtype, off, x, start, Cc, sh, sw, ld, mid, what)
    same_outside(got, before, slice(mid, mid + Cc), what)
    y = got[..., mid:mid + Cc]
    assert_written(y, what)
    err = close(y, ref, tol(dtype), what)
    print(f"{what}: max err {err:.3e} (bound {tol(dtype) * ref.abs().max().item():.3e})")
    return x, y


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bilinear_fwd(engine, dtype, off):
    _fwd_case(engine, dtype, off, 2, 3, 5, 8, 2, 3)               # dense: V = 4 when aligned
    _fwd_case(engine, dtype, off, 2, 3, 5, 8, 2, 3, 24, 8)        # into a wider buffer: the neighbouring columns stay untouched
    _fwd_case(engine, dtype, off, 2, 3, 5, 8, 3, 2, 13, 3)        # y_ld % 4 = 1: scalar although C % 4 = 0
    _fwd_case(engine, dtype, off, 1, 4, 4, 6, 2, 2)               # C % 4 != 0: scalar
    _fwd_case(engine, dtype, off, 2, 1, 1, 8, 4, 4)               # 1x1 source: both neighbours clamp on both axes
    _fwd_case(engine, dtype, off, 2, 1, 7, 4, 5, 3)               # a single row; odd, non-dyadic weights
    _fwd_case(engine, dtype, off, 2, 2, 2, 4, 8, 8)               # the edge phases outnumber the interior ones
    x, y = _fwd_case(engine, dtype, off, 1, 3, 3, 4, 1, 1)        # factor 1: the identity
    assert torch.equal(y, x), "a factor of 1 x 1 is a bit-exact copy"


# ------------------------------------------------------------------------------------------------ backward
def _bwd_launch(engine, dtype, off, wide, prior, Cc, sh, sw, ld, acc, what):
    N, H, W, _ = prior.shape
    DY = Guarded(wide, DEV, off=off)
    DX = Guarded(prior, DEV, off=off, role="out") if acc else Guarded.out(prior.shape, prior.dtype, DEV, off=off)
    done(engine, call(engine, "sg_upsample_bilinear_bwd", sgdt(dtype), N, H, W, Cc, sh, sw, DY.ptr(), ld if ld != Cc else 0, DX.ptr(), acc),
         what, DY, DX)
    return DX.read()


def _bwd_case(engine, dtype, off, N, H, W, Cc, sh, sw, ld=None):
    ld = Cc if ld is None else ld
    g = gen(f"bilb{N}{H}{W}{Cc}{sh}{sw}{ld}{dtype}{off}")
    wide, prior = rnd(g, N, H * sh, W * sw, ld, dtype=dtype), rnd(g, N, H, W, Cc, dtype=dtype)
    what = f"bilinear_bwd {N}x{H}x{W}x{Cc} s={sh}x{sw} ld={ld} {dtype} off={off}"
    ref = ref_bwd(wide[..., :Cc], sh, sw, what)
    out = []
    for acc in (0, 1):
        dx = _bwd_launch(engine, dtype, off, wide, prior, Cc, sh, sw, ld, acc, what + f" acc={acc}")
        assert_written(dx, what + f" acc={acc}")
        want = ref + prior.double() if acc else ref
        err = close(dx, want, tol(dtype, True), what + f" acc={acc}")
        print(f"{what} acc={acc}: max err {err:.3e} (bound {tol(dtype, True) * want.abs().max().item():.3e})")
        out.append(dx)
    return wide, prior, out


@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_bilinear_bwd(engine, dtype, off):
    for ld in (None, 12):
        _bwd_case(engine, dtype, off, 2, 3, 5, 8, 2, 3, ld)       # V = 4 when aligned, dense and dy_ld > C
    _bwd_case(engine, dtype, off, 2, 3, 5, 8, 3, 2)
    _bwd_case(engine, dtype, off, 2, 3, 5, 8, 3, 2, 13)           # dy_ld % 4 = 1: scalar although C % 4 = 0
    for ld in (None, 8):
        _bwd_case(engine, dtype, off, 1, 4, 4, 6, 2, 2, ld)       # C % 4 != 0: scalar
    for ld in (None, 12):
        _bwd_case(engine, dtype, off, 2, 1, 1, 8, 4, 4, ld)       # 1x1 source: a plain sum of all 16 cells
    for ld in (None, 8):
        _bwd_case(engine, dtype, off, 2, 1, 7, 4, 5, 3, ld)       # a single row; odd factors (2s - 1 taps per axis)
        _bwd_case(engine, dtype, off, 2, 2, 2, 4, 8, 8, ld)       # window kernel when aligned (sh * sw = 64), every pixel on two borders
        _bwd_case(engine, dtype, off, 1, 3, 3, 4, 1, 1, ld)       # factor 1
    _bwd_case(engine, dtype, off, 2, 2, 3, 36, 8, 8, 40)          # window kernel: C / 4 = 9 > 8 chunks: grid.x = 2; dy_ld > C
    _bwd_case(engine, dtype, off, 2, 2, 3, 36, 8, 8)              # ... dense
    for ld in (None, 12):
        _bwd_case(engine, dtype, off, 2, 1, 1, 8, 8, 8, ld)       # window kernel on a 1x1 source: every cell contributes in full


@gpu
def test_bilinear_bwd_interior_pixels_of_the_window_kernel(engine):
    # 4 x 5 source, 8 x 8: the window kernel on pixels with a full 16 x 16 span (nothing clamped) next to border pixels
    _bwd_case(engine, F32, False, 1, 4, 5, 8, 8, 8)
    _bwd_case(engine, BF16, False, 1, 4, 5, 8, 8, 8, 12)


# ------------------------------------------------------------------------------------------------ invariants
@gpu
def test_bilinear_wrapped(engine):
    # scalar backward kernel: N H W C = 917 * 917 * 5 = 4 204 445 > 16384 * 256 dx elements, each gathers 1 x 4 cells
    assert 917 * 917 * 5 > SP_CAP and 917 * 2 * 459 * 5 > SP_CAP
    _bwd_case(engine, F32, False, 1, 917, 917, 5, 1, 2)
    # scalar forward kernel: N (H sh) (W sw) C = 917 * 2 * 459 * 5 = 4 209 030 > 16384 * 256
    _fwd_case(engine, F32, False, 1, 917, 459, 5, 1, 2)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_bilinear_bwd_twice_gives_the_same_bits(engine, dtype):
    for (N, H, W, Cc, sh, sw) in [(2, 3, 5, 8, 2, 3), (2, 2, 3, 36, 8, 8), (2, 3, 5, 5, 3, 2)]:
        g = gen(f"biltwice{N}{H}{W}{Cc}{sh}{sw}{dtype}")
        wide, prior = rnd(g, N, H * sh, W * sw, Cc, dtype=dtype), rnd(g, N, H, W, Cc, dtype=dtype)
        a = _bwd_launch(engine, dtype, False, wide, prior, Cc, sh, sw, Cc, 0, "first")
        b = _bwd_launch(engine, dtype, False, wide, prior, Cc, sh, sw, Cc, 0, "second")
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_bilinear_image_0_of_a_batch_equals_the_single_image_launch(engine, dtype):
    for (H, W, Cc, sh, sw) in [(3, 5, 8, 2, 3), (2, 3, 36, 8, 8), (3, 5, 5, 3, 2)]:
        g = gen(f"bilslice{H}{W}{Cc}{sh}{sw}{dtype}")
        x, dy = rnd(g, 2, H, W, Cc, dtype=dtype), rnd(g, 2, H * sh, W * sw, Cc, dtype=dtype)
        nan_y, prior = torch.full_like(dy, float("nan")), rnd(g, 2, H, W, Cc, dtype=dtype)
        y2 = _fwd_launch(engine, dtype, False, x, nan_y, Cc, sh, sw, Cc, 0, "fwd batch 2")
        y1 = _fwd_launch(engine, dtype, False, x[:1], nan_y[:1], Cc, sh, sw, Cc, 0, "fwd batch 1")
        assert torch.equal(y2[:1].contiguous().view(torch.uint8), y1.view(torch.uint8))
        for acc in (0, 1):
            d2 = _bwd_launch(engine, dtype, False, dy, prior, Cc, sh, sw, Cc, acc, "bwd batch 2")
            d1 = _bwd_launch(engine, dtype, False, dy[:1], prior[:1], Cc, sh, sw, Cc, acc, "bwd batch 1")
            assert torch.equal(d2[:1].contiguous().view(torch.uint8), d1.view(torch.uint8))


@gpu
def test_bilinear_refuses_a_pixel_stride_below_the_channel_count(engine):
    x, wide = torch.zeros(1, 2, 2, 8), torch.zeros(1, 4, 4, 8)
    X, Y = Guarded(x, DEV), Guarded.out(wide.shape, F32, DEV)
    assert call(engine, "sg_upsample_bilinear_fwd", SG_F32, 1, 2, 2, 8, 2, 2, X.ptr(), Y.ptr(), 4) == SG_EINVAL
    check_all((X, Y), "refused forward")
    assert torch.isnan(Y.read()).all(), "a refused launch writes nothing"
    DY, DX = Guarded(wide, DEV), Guarded.out(x.shape, F32, DEV)
    assert call(engine, "sg_upsample_bilinear_bwd", SG_F32, 1, 2, 2, 8, 2, 2, DY.ptr(), 4, DX.ptr(), 0) == SG_EINVAL
    check_all((DY, DX), "refused backward")
    assert torch.isnan(DX.read()).all(), "a refused launch writes nothing"
