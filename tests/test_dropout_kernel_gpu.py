"""sg_dropout through the C ABI, bit for bit against the numpy restatement of its definition (tests/_dropout_ref.py: Philox4x32-10,
keep(), the fp32 multiply, torch's CPU round-to-nearest-even for bf16).  Operands are tests/_guarded.py arenas (NaN guard bands,
NaN-prefilled outputs), their start 16-byte aligned or one element further.  The entry point picks between two kernel forms:

    vector   x, y 16-byte aligned, first % 4 == 0, n >= 4 (fp32) / 8 (bf16) and, in the spatial form, c % 4 == 0:
             one generator call per 4 elements, one 16-byte access per thread and trip; the ragged tail goes element by element
    scalar   everything else: one call per element

and the definition admits one answer, so every case below - whatever form it lands in - is compared with the same reference."""
import numpy as np
import pytest
import torch

import _dropout_ref as R
from _guarded import Guarded, assert_written, check_all, untouched

gpu = pytest.mark.gpu

SG_F32, SG_BF16, SG_EINVAL = 0, 1, -1
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
OFFS = [pytest.param(False, id="aligned"), pytest.param(True, id="offset")]
EW_CAP = 8192 * 256                     # vectors after which the grid-stride loop takes a second trip
FIRSTS = [0, 1, 6, 2 ** 34 - 8, 2 ** 34 - 3]
SEEDS = (1103, 0, 0)                    # k0, k1, step
BIG = 4 * 256 * 3 + 2                   # three workgroups of fp32 vectors and a ragged tail


def sgdt(dtype):
    return SG_BF16 if dtype == BF16 else SG_F32


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def values(n, dtype, tag=0):
    """n values in +-[2^-7, 1): no zero, so a kept element is told from a dropped one by its value."""
    g = torch.Generator().manual_seed(1000 + tag)
    v = torch.rand(n, generator=g) * (1 - 2.0 ** -7) + 2.0 ** -7
    return (v * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)).to(dtype)


def rng_words(k0, k1, step):
    w = np.array([k0, k1, step, 0], dtype=np.uint32).view(np.int32)
    return torch.from_numpy(w.copy()).to(DEV)


def launch(engine, dtype, n, x, y, thr, scale, stream=0, seeds=SEEDS, first=0, hwc=0, c=0):
    rng = rng_words(*seeds)
    rc = engine.lib.sg_dropout(engine.h, engine.stream, sgdt(dtype), n, hwc, c, first, stream, thr, scale, rng.data_ptr(),
                               x.ptr(), y.ptr())
    torch.cuda.synchronize()
    return rc


def run(engine, x, rate=0.5, thr=None, scale=None, stream=0, seeds=SEEDS, first=0, hwc=0, c=0, off=False, inplace=False, what=""):
    """One launch on guarded operands; returns (output, reference, flat keep mask) after the byte comparison."""
    thr = R.threshold(rate) if thr is None else thr
    scale = R.scale(rate) if scale is None else scale
    ref, kept = R.reference(x, thr, seeds[0], seeds[1], stream, seeds[2], first, hwc, c, sc=scale, is_thr=True)
    if inplace:
        gx = gy = Guarded(x, DEV, off=off, role="out")
    else:
        gx, gy = Guarded(x, DEV, off=off), Guarded.out(x.shape, x.dtype, DEV, off=off)
    rc = launch(engine, x.dtype, x.numel(), gx, gy, thr, scale, stream, seeds, first, hwc, c)
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    check_all([gx, gy], what)
    y = gy.read()
    assert_written(y, what)
    assert torch.equal(bits(y), bits(ref)), f"{what}: {int((bits(y) != bits(ref)).sum())} of {y.numel()} elements differ from the reference"
    return y, ref, kept


# ------------------------------------------------------------------------------------------------------------ element form
@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 1023, BIG])
@pytest.mark.parametrize("dtype", DTYPES)
def test_element_form(engine, dtype, n, off):
    x = values(n, dtype, n)
    for first in FIRSTS:   # 0: vector form when aligned; 1, 6, 2^34 - 3: scalar form; 2^34 - 8: vector form across the counter's carry
        run(engine, x, first=first, off=off, what=f"n={n} first={first}")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_rates_streams_and_seed_words(engine, dtype):
    x = values(BIG, dtype, 7)
    base, _, kept0 = run(engine, x, what="base")
    for rate in (0.1, 0.999):
        y, _, kept = run(engine, x, rate=rate, what=f"rate {rate}")
        assert abs(kept.mean() - (1 - rate)) <= 4 * np.sqrt(rate * (1 - rate) / BIG)
    # thr = 0 keeps everything: with scale 1 the output is the input, bit for bit
    y, _, kept = run(engine, x, thr=0, scale=1.0, what="thr 0")
    assert kept.all() and torch.equal(bits(y), bits(x))
    # every seed word moves the mask
    for what, kw in {"stream": dict(stream=1), "stream 2^32-1": dict(stream=2 ** 32 - 1), "k0": dict(seeds=(1104, 0, 0)),
                     "k1": dict(seeds=(1103, 1, 0)), "step": dict(seeds=(1103, 0, 1)), "all high": dict(seeds=(2 ** 32 - 1,) * 3)}.items():
        _, _, kept = run(engine, x, what=what, **kw)
        assert 0.4 < (kept == kept0).mean() < 0.6, what


_WRAP = {}


def _wrap_mask(n):
    """The keep mask of mask indices 0 .. n - 1 at rate 0.5, computed once for both storage types."""
    if "kept" not in _WRAP or _WRAP["kept"].size < n:
        _WRAP["kept"] = R.keep(R.mask_index(n), *SEEDS[:2], 0, SEEDS[2], R.threshold(0.5))
    return _WRAP["kept"][:n]


@gpu
@pytest.mark.parametrize("dtype", [pytest.param(BF16, id="bf16"), pytest.param(F32, id="f32")])
def test_wrapped_grid(engine, dtype):
    """Just over EW_CAP * 256 vectors: the first threads take a second trip, and three elements are left for the scalar tail."""
    V = 8 if dtype == BF16 else 4
    n = V * (EW_CAP + 5) + 3
    x = values(n, dtype, 11)
    ref = R.expected(x, _wrap_mask(n), 2.0)
    gx, gy = Guarded(x, DEV), Guarded.out(x.shape, dtype, DEV)
    rc = launch(engine, dtype, n, gx, gy, R.threshold(0.5), 2.0)
    assert rc == 0, engine.lib.sg_last_error().decode("utf-8", "replace")
    check_all([gx, gy], "wrapped grid")
    y = gy.read()
    assert_written(y, "wrapped grid")
    assert torch.equal(bits(y), bits(ref))


# ------------------------------------------------------------------------------------------------------------ spatial form
@gpu
@pytest.mark.parametrize("c", [2, 4, 6, 8, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_spatial_form(engine, dtype, c):
    for hw in (1, 5):
        for N in (1, 3):
            x = values(N * hw * c, dtype, c + hw + N).reshape(N, hw, c)
            for off in (False, True):
                for first in (0, 6, 2 ** 34 - 4):   # c % 4 == 0, aligned, first % 4 == 0: vector form; else scalar
                    what = f"N={N} hw={hw} c={c} off={off} first={first}"
                    y, _, kept = run(engine, x, first=first, hwc=hw * c, c=c, off=off, what=what)
                    k = kept.reshape(N, hw, c)
                    assert (k == k[:, :1]).all(), what                       # every pixel of an image and channel shares its decision
                    assert torch.equal(y.float() != 0, torch.from_numpy(k)), what
    # the [N,1,1,C] mask is the element form's mask of an [N,C] tensor with the same seed words
    _, _, ke = run(engine, values(3 * c, dtype, 5), what="element twin")
    _, _, ks = run(engine, values(3 * 5 * c, dtype, 6).reshape(3, 5, c), hwc=5 * c, c=c, what="spatial twin")
    assert np.array_equal(ks.reshape(3, 5, c)[:, 0].reshape(-1), ke)


# ------------------------------------------------------------------------------------------- in place, backward, repeated
@gpu
@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_in_place(engine, dtype, off):
    run(engine, values(BIG, dtype, 21), off=off, inplace=True, what="element, in place")
    run(engine, values(3 * 5 * 8, dtype, 22).reshape(3, 5, 8), hwc=40, c=8, first=4, off=off, inplace=True, what="spatial, in place")


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_call_drops_the_forward_positions(engine, dtype):
    for kw in (dict(first=2 ** 34 - 8), dict(hwc=6 * 8, c=8, first=8), dict(first=3, off=True)):
        n = 4 * 6 * 8 * 9 + (0 if "hwc" in kw else 5)
        y, _, kf = run(engine, values(n, dtype, 31), rate=0.1, stream=3, seeds=(5, 2, 17), what=f"forward {kw}", **kw)
        dx, _, kb = run(engine, values(n, dtype, 32), rate=0.1, stream=3, seeds=(5, 2, 17), what=f"backward {kw}", **kw)
        assert np.array_equal(kf, kb) and torch.equal(y.float() == 0, dx.float() == 0)
        assert 0 < int((dx.float() == 0).sum()) < n


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_launches_give_equal_bytes(engine, dtype):
    for kw in (dict(), dict(off=True), dict(hwc=8 * 256, c=256)):
        x = values(3 * 8 * 256, dtype, 41)
        a, _, _ = run(engine, x, what="first", **kw)
        b, _, _ = run(engine, x, what="second", **kw)
        assert torch.equal(bits(a), bits(b))


# --------------------------------------------------------------------------------------------------------------- refusals
@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_write_nothing(engine, dtype):
    x = values(48, dtype, 51)
    for what, n, hwc, c, dt in [("n < 0", -4, 0, 0, sgdt(dtype)), ("hwc % c != 0", 48, 24, 5, sgdt(dtype)),
                                ("c == 0", 48, 24, 0, sgdt(dtype)), ("n % hwc != 0", 48, 20, 4, sgdt(dtype)),
                                ("hwc < 0", 48, -24, 4, sgdt(dtype)), ("unknown dtype", 48, 0, 0, 7)]:
        gx, gy = Guarded(x, DEV), Guarded.out(x.shape, dtype, DEV)
        rng = rng_words(*SEEDS)
        rc = engine.lib.sg_dropout(engine.h, engine.stream, dt, n, hwc, c, 0, 0, R.threshold(0.5), 2.0, rng.data_ptr(), gx.ptr(), gy.ptr())
        torch.cuda.synchronize()
        assert rc == SG_EINVAL, f"{what}: rc={rc}"
        assert engine.lib.sg_last_error().decode("utf-8", "replace").startswith("sg_dropout"), what
        untouched(gy, what)
        gx.fetch().check(what)
