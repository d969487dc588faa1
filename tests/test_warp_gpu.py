"""sg_warp_u8 (Engine.warp_u8) on the device against the numpy restatement of include/segengine.h (tests/_warp_ref.py), bit
for bit, every operand between guard bands (tests/_guarded.py); the symmetries and shifts against numpy's own flips, rot90 and
slices; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import _warp_ref as R
from _guarded import Guarded, check_all, untouched
from building_detection_amd import _lib

pytestmark = pytest.mark.gpu

NE, RE, CO = R.NEAREST, R.REFLECT, R.COLOR


def _call(engine, src, items, out_hw, luts=None, seed=0, n=None, S=None, c=None):
    """The raw ABI call on guarded operands: (rc, guarded output, [operands])."""
    s4 = src if src.ndim == 4 else src[..., None]
    gs = Guarded(torch.from_numpy(np.ascontiguousarray(src)), engine.device)
    gl = None if luts is None else Guarded(torch.from_numpy(np.ascontiguousarray(luts)), engine.device)
    out = Guarded.out((len(items), out_hw[0], out_hw[1]) + src.shape[3:], torch.uint8, engine.device)
    full = [dict(it, sh=s4.shape[1] if it["sh"] is None else it["sh"], sw=s4.shape[2] if it["sw"] is None else it["sw"]) for it in items]
    table = (_lib.WarpItem * max(len(full), 1))(*[_lib.warp_item(**it) for it in full])
    rc = engine.lib.sg_warp_u8(engine.h, engine.stream, s4.shape[0] if S is None else S, s4.shape[1], s4.shape[2],
                               s4.shape[3] if c is None else c, C.c_void_p(gs.ptr()), len(items) if n is None else n, table,
                               None if gl is None else C.c_void_p(gl.ptr()), seed, out_hw[0], out_hw[1], C.c_void_p(out.ptr()))
    torch.cuda.synchronize()
    return rc, out, [o for o in (gs, gl, out) if o is not None]


def _run(engine, src, items, out_hw, luts=None, seed=0):
    rc, out, ops = _call(engine, src, items, out_hw, luts, seed)
    assert rc == 0, engine.lib.sg_last_error().decode()
    check_all(ops, "sg_warp_u8")
    return out.read().numpy()


def _same(got, want, items):
    assert got.shape == want.shape
    for i, it in enumerate(items):
        bad = np.argwhere(got[i] != want[i])
        assert bad.size == 0, (i, it, len(bad), bad[0].tolist(), got[i][tuple(bad[0])], want[i][tuple(bad[0])])


def _two_sources(C_, seed):
    """37 x 53 and 64 x 40 in one padded [2,64,53,C] array; the padding holds 0xEE, which no tap may read."""
    rng = np.random.default_rng(seed)
    src = np.full((2, 64, 53, C_), 0xEE, np.uint8)
    src[0, :37, :53] = rng.integers(0, 256, size=(37, 53, C_), dtype=np.uint8)
    src[1, :64, :40] = rng.integers(0, 256, size=(64, 40, C_), dtype=np.uint8)
    return (src if C_ == 3 else src[..., 0]), [(37, 53), (64, 40)]


@pytest.mark.parametrize("out_hw", [(24, 20), (21, 19)])
@pytest.mark.parametrize("C_", [1, 3])
def test_kernel_matches_the_restatement(engine, C_, out_hw):
    """Rotations of 30 degrees at scale 0.7 and 1.6 with shear, windows partly and wholly outside, reflect several periods away,
    bilinear and nearest, constant and reflect - mixed in one table, so one call launches every combination."""
    src, ext = _two_sources(C_, 11 + C_)
    items = []
    for k, (angle, scale, shear, shift) in enumerate([(30, 0.7, 8, (0, 0)), (30, 1.6, -5, (0, 0)), (-30, 1.6, 0, (3.3, -2.7)),
                                                      (0, 1.0, 0, (0, 0)), (0, 1.0, 0, (30.0, 20.0)), (0, 1.0, 0, (-45.5, 10.25)),
                                                      (0, 1.0, 0, (500.0, -400.0)), (77, 0.31, 20, (0, 0)), (0, 1.0, 0, (-1000.5, 777.0))]):
        for flags in (0, NE, RE, NE | RE):
            s = (k + (flags >> 1)) % 2
            a, b = R.affine(ext[s], out_hw, angle, scale, shear, shift=shift)
            items.append(R.item(src=s, sh=ext[s][0], sw=ext[s][1], flags=flags, a=a, b=b, fill=(37 * k + 5) % 256))
    assert len(items) > _lib.SG_WARP_MAX_ITEMS
    for i0 in range(0, len(items), 12):
        part = items[i0:i0 + 12]
        _same(_run(engine, src, part, out_hw), R.warp(src, part, None, 0, out_hw), part)


@pytest.mark.parametrize("C_", [1, 3])
def test_symmetries_and_identity_reproduce_source_bytes(engine, C_):
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, size=(1, 40, 40, 3), dtype=np.uint8)
    src = src if C_ == 3 else src[..., 0]
    items, want = [], []
    for name, form, D in R.SYMMETRIES:
        a, b = R.affine((40, 40), (40, 40), D=D)
        for flags in (0, NE, RE):
            items.append(R.item(flags=flags, a=a, b=b, fill=9))
            want.append(form(src[0]))
    got = _run(engine, src, items, (40, 40))
    _same(got, np.stack(want), items)                      # numpy's own flips / rot90 / transposes, not the restatement


def test_half_pixel_and_whole_pixel_shifts(engine):
    rng = np.random.default_rng(6)
    src = rng.integers(0, 256, size=(1, 40, 40), dtype=np.uint8)
    p = src[0].astype(np.int64)
    got = _run(engine, src, [R.item(b=(32768, 0), fill=0), R.item(b=(0, 32768), fill=0)], (39, 39))
    assert np.array_equal(got[0], ((p[:39, :39] + p[:39, 1:] + 1) >> 1).astype(np.uint8))
    assert np.array_equal(got[1], ((p[:39, :39] + p[1:, :39] + 1) >> 1).astype(np.uint8))
    shifts = [(7, 0), (-7, 0), (0, 9), (0, -9), (39, 39), (-39, -39), (40, 0), (0, -40), (12345, -5)]
    items = [R.item(b=(dx * 65536, dy * 65536), fill=200, flags=f) for dx, dy in shifts for f in (0, NE)]
    got = _run(engine, src, items, (40, 40))
    k = 0
    for dx, dy in shifts:
        want = np.full((40, 40), 200, np.uint8)
        ys, xs = np.arange(40) + dy, np.arange(40) + dx
        oky, okx = (ys >= 0) & (ys < 40), (xs >= 0) & (xs < 40)
        want[np.ix_(oky, okx)] = src[0][np.ix_(ys[oky], xs[okx])]
        for _ in range(2):
            assert np.array_equal(got[k], want), (dx, dy, k)
            k += 1


def test_tiny_sources_and_the_stated_bounds(engine):
    """A 2 x 2 and a 1 x 1 source, coefficients at +-2^24 and offsets at +-(2^46 - 1), and the widest row (2^14)."""
    rng = np.random.default_rng(8)
    src = np.full((2, 5, 6, 3), 0xEE, np.uint8)
    src[0, :2, :2] = rng.integers(0, 256, size=(2, 2, 3), dtype=np.uint8)
    src[1, :1, :1] = 77
    A_, B_ = R.A_MAX, R.B_LIM - 1
    items = []
    for flags in (0, NE, RE, NE | RE):
        a, b = R.affine((2, 2), (24, 20), 30, 3.0, 4)
        items.append(R.item(src=0, sh=2, sw=2, flags=flags, a=a, b=b, fill=3))
        items.append(R.item(src=0, sh=2, sw=2, flags=flags, a=(A_, -A_, -A_, A_), b=(B_, -B_), fill=4))
        items.append(R.item(src=0, sh=2, sw=2, flags=flags, a=(-A_, -A_, A_, A_), b=(-B_, B_), fill=5))
        items.append(R.item(src=0, sh=2, sw=2, flags=flags, a=(21845, 0, 0, 21845), b=(-40 * 65536 - 1, 65536 * 1000 + 3), fill=6))
        if not flags & RE:                                   # reflect needs an extent of 2
            items.append(R.item(src=1, sh=1, sw=1, flags=flags, a=(9000, 100, -100, 9000), b=(-30000, -30000), fill=250))
    _same(_run(engine, src, items, (24, 20)), R.warp(src, items, None, 0, (24, 20)), items)
    wide = [R.item(src=0, sh=2, sw=2, flags=f, a=(A_, A_, A_, A_), b=(B_, B_), fill=1) for f in (RE, 0)]
    wide += [R.item(src=0, sh=2, sw=2, flags=RE, a=(17, 0, 0, 40000), b=(-3, 0), fill=1)]
    g = src[..., 0].copy()
    _same(_run(engine, g, wide, (2, R.OUT_MAX)), R.warp(g, wide, None, 0, (2, R.OUT_MAX)), wide)


def test_nearest_keeps_a_class_map_valid(engine):
    rng = np.random.default_rng(9)
    lab = rng.integers(0, 6, size=(1, 37, 53), dtype=np.uint8)
    items = []
    for angle, scale in ((30, 0.7), (30, 1.6), (-115, 1.0)):
        a, b = R.affine((37, 53), (21, 19), angle, scale, 6)
        items += [R.item(flags=NE, a=a, b=b, fill=255), R.item(flags=NE | RE, a=a, b=b, fill=255)]
    got = _run(engine, lab, items, (21, 19))
    _same(got, R.warp(lab, items, None, 0, (21, 19)), items)
    assert set(np.unique(got[0::2])) <= set(range(6)) | {255} and 255 in got[0::2]
    assert set(np.unique(got[1::2])) <= set(range(6))


def _colour_cases(rng):
    sat = (5000, -500, -404, -300, 4700, -304, 123, -4000, 7973)      # rows need not sum to 4096; negative sums clamp at 0
    lut = rng.integers(0, 256, size=(3, 256), dtype=np.uint8)
    ident = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
    return [("matrix", dict(m=sat, off=(40960, -81920, 0)), ident), ("swap", dict(m=(0, 0, 4096, 0, 4096, 0, 4096, 0, 0)), ident),
            ("lut", dict(), lut), ("noise", dict(noise_q12=300, sample=2 ** 40 + 3), ident),
            ("all", dict(m=sat, off=(-3000, 2000, 100000), noise_q12=150, sample=17), lut)]


@pytest.mark.parametrize("out_hw", [(24, 20), (21, 19)])
def test_colour_steps(engine, out_hw):
    rng = np.random.default_rng(12)
    src, ext = _two_sources(3, 13)
    cases = _colour_cases(rng)
    a, b = R.affine(ext[0], out_hw, 30, 1.6, 3)
    items, luts = [], []
    for name, kw, lut in cases:
        for flags, (aa, bb) in ((CO, ((65536, 0, 0, 65536), (0, 0))), (CO | RE, (a, b)), (CO | NE, (a, b))):
            items.append(R.item(src=0, sh=37, sw=53, flags=flags, a=aa, b=bb, fill=128, **kw))
            luts.append(lut)
    items.append(R.item(src=1, sh=64, sw=40, flags=0, a=a, b=b, fill=128, m=(0,) * 9, noise_q12=4096))   # no COLOR: all ignored
    luts.append(rng.integers(0, 256, size=(3, 256), dtype=np.uint8))
    luts = np.stack(luts)
    seed = 0xDEADBEEF12345678
    got = _run(engine, src, items, out_hw, luts, seed)
    _same(got, R.warp(src, items, luts, seed, out_hw), items)
    assert np.array_equal(got[3], src[0, :out_hw[0], :out_hw[1], ::-1])               # the R-B swap, against numpy
    assert np.array_equal(got[6], np.stack([luts[6][c][src[0, :out_hw[0], :out_hw[1], c]] for c in range(3)], -1))
    # the same table without tone tables: step 2 is skipped
    plain = [it for it, (name, _, _) in zip(items[0:15:3], cases) if name != "lut"]
    _same(_run(engine, src, plain, out_hw, None, seed), R.warp(src, plain, None, seed, out_hw), plain)


def test_noise_depends_on_seed_sample_pixel_and_channel_only(engine):
    src = np.full((2, 16, 16, 3), 128, np.uint8)
    mk = lambda sample, s=0: R.item(src=s, flags=CO, noise_q12=900, sample=sample, fill=0)
    seed = 2 ** 33 + 7
    base = _run(engine, src, [mk(5), mk(6), mk(2 ** 32 + 5)], (16, 16), None, seed)
    assert not np.array_equal(base[0], base[1]) and not np.array_equal(base[0], base[2])         # another sample, low or high word
    assert not np.array_equal(base[0][..., 0], base[0][..., 1])                                   # channels draw apart
    moved = _run(engine, src, [mk(9), R.item(flags=NE, fill=0), mk(6, 1), mk(5, 1)], (16, 16), None, seed)
    assert np.array_equal(moved[3], base[0]) and np.array_equal(moved[2], base[1])                # another slot, other neighbours
    alone = _run(engine, src, [mk(5)], (16, 16), None, seed)                                      # another split into calls
    assert np.array_equal(alone[0], base[0])
    for other in (seed + 1, seed + 2 ** 32):
        assert not np.array_equal(_run(engine, src, [mk(5)], (16, 16), None, other)[0], base[0])  # another seed, low or high word
    # a pixel's noise goes with its number oy * OW + ox: the same rows of a narrower tile draw other numbers
    assert not np.array_equal(_run(engine, src, [mk(5)], (16, 12), None, seed)[0][1], base[0][1, :12])


def test_noise_statistics(engine):
    """64 x 64 x 3 grey-128 pixels, 12 288 draws.  noise_q12 = 4096 adds t itself (standard deviation 147.80, so the clipped mean
    has a standard error below 147.80 / sqrt(12288) = 1.33: within 7 = five of them of 128, by symmetry of t and of the clip
    about 127.5 +- 0.5); noise_q12 = 512 adds t / 8 (|t / 8| <= 64: nothing clips), whose standard deviation times 8 must lie
    within 5 % of 147.80 (its standard error is 147.80 / sqrt(2 * 12288) = 0.9, i.e. 0.6 %)."""
    src = np.full((1, 64, 64, 3), 128, np.uint8)
    got = _run(engine, src, [R.item(flags=CO, noise_q12=4096, sample=3), R.item(flags=CO, noise_q12=512, sample=3)], (64, 64),
               None, 99).astype(np.float64)
    mean, std = got[0].mean(), (got[1] - 128).std() * 8
    print(f"noise: mean {mean:.3f} (128 +- 7), std {std:.2f} ({R.T_STD:.2f} +- 5 %)")
    assert abs(mean - 128) <= 7
    assert got[1].min() > 0 and got[1].max() < 255
    assert abs(std / R.T_STD - 1) <= 0.05


def test_more_items_than_the_cap_take_several_calls(engine):
    rng = np.random.default_rng(14)
    src = rng.integers(0, 256, size=(1, 12, 12, 3), dtype=np.uint8)
    n = 2 * _lib.SG_WARP_MAX_ITEMS + 3
    items = [R.item(flags=CO | (RE if i % 3 == 0 else 0), a=(65536 + 700 * i, 300, -300, 65536), b=(-i * 9000, i * 5000), fill=128,
                    noise_q12=200, sample=1000 + i) for i in range(n)]
    luts = rng.integers(0, 256, size=(n, 3, 256), dtype=np.uint8)
    got = engine.warp_u8(torch.from_numpy(src).to(engine.device), items, torch.from_numpy(luts).to(engine.device), seed=5,
                         out_hw=(8, 8)).cpu().numpy()
    _same(got, R.warp(src, items, luts, 5, (8, 8)), items)
    # extents= fills the items' sh / sw
    bare = [{k: v for k, v in R.item(a=(40000, 0, 0, 40000), b=(-70000, -70000), fill=1).items() if k not in ("sh", "sw")}]
    got = engine.warp_u8(torch.from_numpy(src).to(engine.device), bare, out_hw=(8, 8), extents=[(7, 5)]).cpu().numpy()
    _same(got, R.warp(src, [dict(bare[0], sh=7, sw=5)], None, 0, (8, 8)), bare)
    rc, out, _ = _call(engine, src, [R.item()] * (_lib.SG_WARP_MAX_ITEMS + 1), (8, 8))
    assert rc == -1 and "N = 33" in engine.lib.sg_last_error().decode()
    untouched(out, "over the cap")


def test_refused_calls_name_the_item_and_write_nothing(engine):
    src3 = np.zeros((2, 8, 10, 3), np.uint8)
    good = R.item(fill=128)
    cases = [
        ("src at S", [good, R.item(src=2)], {}, "item 1: source 2"),
        ("sh > H", [good, good, R.item(sh=9, sw=10)], {}, "item 2: extent 9 x 10"),
        ("sw > W", [R.item(sh=8, sw=11)], {}, "item 0: extent 8 x 11"),
        ("unknown flag", [good, R.item(flags=8)], {}, "item 1: unknown flags"),
        ("colour with C = 1", [R.item(flags=CO)], dict(grey=True), "item 0: colour needs C = 3"),
        ("reflect with extent 1", [good, R.item(flags=RE, sh=1, sw=10)], {}, "item 1: reflect"),
        ("a out of bounds", [good, R.item(a=(R.A_MAX + 1, 0, 0, 65536))], {}, "item 1: a coefficient"),
        ("b out of bounds", [R.item(b=(0, -R.B_LIM))], {}, "item 0: an offset"),
        ("m out of bounds", [R.item(flags=CO, m=(R.M_MAX + 1,) + (0,) * 8)], {}, "item 0: m[0]"),
        ("noise out of bounds", [R.item(flags=CO, noise_q12=R.NOISE_MAX + 1)], {}, "item 0: noise_q12"),
        ("N = 0", [good], dict(n=0), "N = 0"),
        ("fill = 256", [good, R.item(fill=256)], {}, "item 1: fill = 256"),
        ("output too large", [good], dict(out_hw=(1, R.OUT_MAX + 1)), "output of"),
    ]
    for what, items, kw, msg in cases:
        src = src3[..., 0].copy() if kw.get("grey") else src3
        rc, out, ops = _call(engine, src, items, kw.get("out_hw", (8, 12)), n=kw.get("n"))
        err = engine.lib.sg_last_error().decode()
        assert rc == -1 and msg in err and "sg_warp_u8" in err, (what, rc, err)
        untouched(out, what)
        check_all(ops, what)
    with pytest.raises(_lib.SgError, match="sg_warp_u8.*item 0: source 3"):
        engine.warp_u8(torch.from_numpy(src3).to(engine.device), [dict(src=3)])
