"""sg_sort_pairs_u32 on the GPU, bit for bit against np.argsort(..., kind="stable"): every operand between guard bands
(tests/_guarded.py), outputs prefilled, the workspace exactly as long as the query says and filled with 0xFF (the call may
assume nothing about it), at the 16-byte aligned start and ONE ELEMENT further.  T and W mirror SG_SORT_TILE and
SG_SORT_DIGIT_BITS of include/segengine.h."""
import re
import os
import zlib

import numpy as np
import pytest
import torch

from _guarded import Guarded, assert_written, check_all, untouched

pytestmark = pytest.mark.gpu

SG_EINVAL, SG_EWORKSPACE = -1, -2
DEV = "cuda"
T, W = 2048, 8
OFFS = [pytest.param(False, id="aligned"), pytest.param(True, id="offset")]
LENS = (1, 63, 64, 65, 255, 257, T - 1, T, T + 1, 3 * T + 17)
SEGMENTS = (1, 3)
KEY_BITS = (1, W, W + 1, 30, 32)
KEYSETS = ("equal", "two_values", "random30", "top_digit", "low_digit", "junk_above", "sorted", "reversed")


def test_constants_mirror_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segengine.h")).read()
    assert int(re.search(r"#define SG_SORT_TILE (\d+)", hdr).group(1)) == T
    assert int(re.search(r"#define SG_SORT_DIGIT_BITS (\d+)", hdr).group(1)) == W


def rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def passes(key_bits):
    return -(-key_bits // W)


def ws_formula(segments, n, key_bits):
    tiles = -(-n // T)
    return 4 * (segments * 256 * (tiles + 1) + (2 * segments * n if passes(key_bits) > 1 else 0))


def make_keys(name, r, n, key_bits):
    top = (passes(key_bits) - 1) * W
    x = r.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if name == "equal":
        return np.full(n, 0x2A5A5A5A, np.uint32)
    if name == "two_values":
        return np.where(x & 1, np.uint32(0x00000001), np.uint32(0x20000100)).astype(np.uint32)
    if name == "random30":
        return x & np.uint32(0x3FFFFFFF)
    if name == "top_digit":                                           # differ in the highest compared digit only
        return (((x & np.uint32(0xFF)) << np.uint32(top)) | np.uint32(0x15)).astype(np.uint32)
    if name == "low_digit":
        return (np.uint32(0x12345600) | (x & np.uint32(0xFF))).astype(np.uint32)
    if name == "junk_above":                                          # 32 random bits: those above key_bits must not be compared
        return x
    if name == "sorted":
        return np.arange(n, dtype=np.uint32)
    assert name == "reversed"
    return np.arange(n, dtype=np.uint32)[::-1].copy()


def as_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32))


def expected(keys, vals, segments, n, key_bits):
    mask = np.uint32(0xFFFFFFFF if key_bits == 32 else (1 << key_bits) - 1)
    ko, vo = np.empty_like(keys), np.empty_like(vals)
    for s in range(segments):
        sl = slice(s * n, (s + 1) * n)
        o = np.argsort(keys[sl] & mask, kind="stable")
        ko[sl], vo[sl] = keys[sl][o], vals[sl][o]
    return ko, vo


def call(engine, segments, n, key_bits, KI, VI, KO, VO, WS, nws):
    return engine.lib.sg_sort_pairs_u32(engine.h, engine.stream, segments, n, key_bits, KI.ptr(), VI.ptr(), KO.ptr(), VO.ptr(),
                                        WS.ptr(), nws)


def run(engine, keys, vals, segments, n, key_bits, off, what):
    nws = engine.lib.sg_sort_pairs_ws_bytes(engine.h, segments, n, key_bits)
    assert nws == ws_formula(segments, n, key_bits), what
    KI, VI = Guarded(as_i32(keys), DEV, off=off), Guarded(as_i32(vals), DEV, off=off)
    KO, VO = Guarded.out((segments * n,), torch.int32, DEV, off=off), Guarded.out((segments * n,), torch.int32, DEV, off=off)
    WS = Guarded.ws(nws, DEV)
    rc = call(engine, segments, n, key_bits, KI, VI, KO, VO, WS, nws)
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    check_all((KI, VI, KO, VO, WS), what)
    return KO.read().numpy().view(np.uint32), VO.read().numpy().view(np.uint32)


@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("key_bits", KEY_BITS)
def test_sort_is_stable_and_exact(engine, key_bits, off):
    for n in LENS:
        for segments in SEGMENTS:
            for name in KEYSETS:
                what = f"sort len={n} segments={segments} key_bits={key_bits} {name} off={off}"
                r = rng(what)
                keys = make_keys(name, r, segments * n, key_bits)
                vals = r.permutation(segments * n).astype(np.uint32) | np.uint32(0x80000000)     # distinct: a place is a witness
                ko, vo = run(engine, keys, vals, segments, n, key_bits, off, what)
                ek, ev = expected(keys, vals, segments, n, key_bits)
                assert np.array_equal(vo, ev), f"{what}: {int((vo != ev).sum())} values out of place"
                assert np.array_equal(ko, ek), f"{what}: keys differ (the bits above key_bits travel with the key)"
                if name in ("equal", "random30") and n in (T + 1, 3 * T + 17):
                    ko2, vo2 = run(engine, keys, vals, segments, n, key_bits, off, what + " again")
                    assert np.array_equal(ko2, ko) and np.array_equal(vo2, vo), what + ": the call is not reproducible"


def test_a_segment_never_reads_its_neighbour(engine):
    """Three segments whose keys would interleave if they were sorted together."""
    n = T + 1
    keys = np.concatenate([np.full(n, 7, np.uint32), np.arange(n, dtype=np.uint32)[::-1], np.full(n, 3, np.uint32)])
    vals = np.arange(3 * n, dtype=np.uint32)
    ko, vo = run(engine, keys, vals, 3, n, 32, False, "neighbours")
    assert np.array_equal(vo[:n], vals[:n]) and np.array_equal(vo[n:2 * n], vals[n:2 * n][::-1]) and np.array_equal(vo[2 * n:], vals[2 * n:])
    assert np.array_equal(ko[n:2 * n], np.arange(n, dtype=np.uint32))


def test_refusals_write_nothing(engine):
    segments, n, bits = 3, 65, 30
    r = rng("refuse")
    keys, vals = make_keys("random30", r, segments * n, bits), np.arange(segments * n, dtype=np.uint32)
    nws = ws_formula(segments, n, bits)
    KI, VI = Guarded(as_i32(keys), DEV), Guarded(as_i32(vals), DEV)
    KO, VO, WS = Guarded.out((segments * n,), torch.int32, DEV), Guarded.out((segments * n,), torch.int32, DEV), Guarded.ws(nws, DEV)
    lib, h = engine.lib, engine.h
    for s, l, b in ((0, n, bits), (-1, n, bits), (segments, 0, bits), (segments, -5, bits), (segments, n, 0), (segments, n, 33),
                    (segments, n, -1), (2, 2 ** 30, bits), (1, 2 ** 31, bits), (2 ** 31, 1, bits)):
        assert lib.sg_sort_pairs_ws_bytes(h, s, l, b) == 0, (s, l, b)
        assert call(engine, s, l, b, KI, VI, KO, VO, WS, nws) == SG_EINVAL, (s, l, b)
    null = type("Null", (), {"ptr": staticmethod(lambda: None)})
    for i in range(5):                                                        # a null pointer in every position
        ops = [KI, VI, KO, VO, WS]
        ops[i] = null
        assert call(engine, segments, n, bits, *ops, nws) == (SG_EWORKSPACE if i == 4 else SG_EINVAL), i
    for ops in ((KI, VI, KI, VO), (KI, VI, KO, VI), (KI, VI, KO, KO), (KI, VI, VI, VO), (KI, VI, KO, KI)):      # aliased operands
        assert call(engine, segments, n, bits, *ops, WS, nws) == SG_EINVAL
    assert call(engine, segments, n, bits, KI, VI, KO, VO, WS, nws - 1) == SG_EWORKSPACE      # one byte short
    torch.cuda.synchronize()
    for o in (KO, VO, WS):
        untouched(o, "refusals")
    check_all((KI, VI), "refusals")
    # ... and the same operands are taken once the arguments are right
    assert call(engine, segments, n, bits, KI, VI, KO, VO, WS, nws) == 0
    check_all((KI, VI, KO, VO, WS), "good")
    ek, ev = expected(keys, vals, segments, n, bits)
    assert np.array_equal(KO.read().numpy().view(np.uint32), ek) and np.array_equal(VO.read().numpy().view(np.uint32), ev)
    assert_written(VO.read(), "good")


def test_engine_wrapper(engine):
    r = rng("wrap")
    n = 3 * T + 17
    keys, vals = make_keys("random30", r, 2 * n, 30), np.arange(2 * n, dtype=np.uint32)
    kd, vd = as_i32(keys).reshape(2, n).to(DEV), as_i32(vals).reshape(2, n).to(DEV)
    ko, vo = engine.sort_pairs(kd, vd, key_bits=30)
    ek, ev = expected(keys, vals, 2, n, 30)
    assert ko.shape == kd.shape and np.array_equal(ko.cpu().numpy().view(np.uint32).ravel(), ek)
    assert np.array_equal(vo.cpu().numpy().view(np.uint32).ravel(), ev) and np.array_equal(kd.cpu().numpy().view(np.uint32).ravel(), keys)
    ko, vo = engine.sort_pairs(kd[0], vd[0])                                  # one segment, all 32 bits
    ek, ev = expected(keys[:n], vals[:n], 1, n, 32)
    assert np.array_equal(ko.cpu().numpy().view(np.uint32), ek) and np.array_equal(vo.cpu().numpy().view(np.uint32), ev)
    for bad in ((kd.float(), vd), (kd, vd[:1]), (kd.cpu(), vd.cpu()), (kd[:, ::2], vd[:, ::2]), (kd.reshape(2, 1, n), vd.reshape(2, 1, n))):
        with pytest.raises(ValueError):
            engine.sort_pairs(*bad)
