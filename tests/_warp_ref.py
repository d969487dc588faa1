"""numpy restatement of sg_warp_u8 as include/segengine.h states it (not of the kernel): the integer geometry, the reflect-101
index, the 8-bit bilinear blend, the Q12 colour matrix, the tone table and the Philox noise (the generator of
tests/_dropout_ref.py), plus a float64 item builder for the tests' own maps.  Everything is int64 numpy; an item is a mapping
with every field of sg_warp_item spelled out (`item()` fills the defaults)."""
import math

import numpy as np

from _dropout_ref import philox4x32_10

NEAREST, REFLECT, COLOR = 1, 2, 4                       # SG_WARP_*
NOISE_STREAM, NOISE_KEY = 0x6E6F6973, 0x77617270        # SG_WARP_NOISE_STREAM, SG_WARP_NOISE_KEY
T_STD = math.sqrt(4 * (256 ** 2 - 1) / 12)              # 147.80
A_MAX, B_LIM, OUT_MAX, M_MAX, OFF_MAX, NOISE_MAX = 1 << 24, 1 << 46, 1 << 14, 1 << 18, 1 << 24, 1 << 16
IDENTITY_M = (4096, 0, 0, 0, 4096, 0, 0, 0, 4096)


def item(src=0, sh=None, sw=None, flags=0, a=(65536, 0, 0, 65536), b=(0, 0), sample=0, fill=0, noise_q12=0, m=IDENTITY_M,
         off=(0, 0, 0)):
    return dict(src=src, sh=sh, sw=sw, flags=flags, a=tuple(int(v) for v in a), b=tuple(int(v) for v in b), sample=int(sample),
                fill=fill, noise_q12=noise_q12, m=tuple(int(v) for v in m), off=tuple(int(v) for v in off))


def reflect101(i, n):
    """j = i mod 2 (n - 1), non-negative; r = j < n ? j : 2 (n - 1) - j."""
    p = 2 * (n - 1)
    j = np.mod(i, p)
    return np.where(j < n, j, p - j)


def _tap(img, x, y, sh, sw, fill, reflect):
    """img [H,W,C] int64; x, y [OH,OW] int64 -> [OH,OW,C]."""
    if reflect:
        return img[reflect101(y, sh), reflect101(x, sw)]
    inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
    v = img[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)]
    return np.where(inside[..., None], v, np.int64(fill))


def noise_t(pixels, sample, seed):
    """t_c (c = 0, 1, 2) of the given pixel numbers: [n, 3] int64."""
    w = philox4x32_10((pixels.astype(np.uint64), sample & 0xFFFFFFFF, sample >> 32, NOISE_STREAM),
                      (seed & 0xFFFFFFFF, (seed >> 32) ^ NOISE_KEY))
    out = []
    for c in range(3):
        wc = np.broadcast_to(w[c], pixels.shape).astype(np.int64)
        out.append((wc & 255) + ((wc >> 8) & 255) + ((wc >> 16) & 255) + (wc >> 24) - 510)
    return np.stack(out, -1)


def warp_one(src, it, lut, seed, out_hw):
    """One output tile [OH,OW,C] (uint8) of sources src [S,H,W,C]."""
    oh, ow = out_hw
    C = src.shape[3]
    sh = src.shape[1] if it["sh"] is None else it["sh"]
    sw = src.shape[2] if it["sw"] is None else it["sw"]
    img = src[it["src"]].astype(np.int64)
    oy, ox = np.meshgrid(np.arange(oh, dtype=np.int64), np.arange(ow, dtype=np.int64), indexing="ij")
    a00, a01, a10, a11 = it["a"]
    X = a00 * ox + a01 * oy + it["b"][0]
    Y = a10 * ox + a11 * oy + it["b"][1]
    refl, fill = bool(it["flags"] & REFLECT), it["fill"]
    if it["flags"] & NEAREST:
        v = _tap(img, (X + 32768) >> 16, (Y + 32768) >> 16, sh, sw, fill, refl)
    else:
        x0, y0 = X >> 16, Y >> 16
        wx, wy = ((X & 0xFFFF) >> 8)[..., None], ((Y & 0xFFFF) >> 8)[..., None]
        p00, p01 = _tap(img, x0, y0, sh, sw, fill, refl), _tap(img, x0 + 1, y0, sh, sw, fill, refl)
        p10, p11 = _tap(img, x0, y0 + 1, sh, sw, fill, refl), _tap(img, x0 + 1, y0 + 1, sh, sw, fill, refl)
        v = ((256 - wx) * (256 - wy) * p00 + wx * (256 - wy) * p01 + (256 - wx) * wy * p10 + wx * wy * p11 + 32768) >> 16
    if it["flags"] & COLOR:
        assert C == 3
        m = np.array(it["m"], np.int64).reshape(3, 3)
        u = np.clip((v @ m.T + np.array(it["off"], np.int64) + 2048) >> 12, 0, 255)
        if lut is not None:
            u = np.stack([lut[c].astype(np.int64)[u[..., c]] for c in range(3)], -1)
        if it["noise_q12"] > 0:
            t = noise_t((oy * ow + ox).reshape(-1), it["sample"], seed).reshape(oh, ow, 3)
            u = np.clip(u + ((it["noise_q12"] * t + 2048) >> 12), 0, 255)
        v = u
    return v.astype(np.uint8)


def warp(src, items, luts=None, seed=0, out_hw=None):
    """sg_warp_u8: src uint8 [S,H,W,C] or [S,H,W] -> [N,OH,OW(,C)]; luts uint8 [N,3,256] or None."""
    grey = src.ndim == 3
    s4 = src[..., None] if grey else src
    out_hw = s4.shape[1:3] if out_hw is None else out_hw
    out = np.stack([warp_one(s4, it, None if luts is None else luts[i], seed, out_hw) for i, it in enumerate(items)])
    return out[..., 0] if grey else out


# ---- the tests' own float64 item builder --------------------------------------------------------------------------------------
# symmetry k of the square as (numpy form, integer matrix D of output offset -> source offset in (x, y))
SYMMETRIES = [
    ("identity", lambda s: s, ((1, 0), (0, 1))),
    ("flipud", lambda s: s[::-1], ((1, 0), (0, -1))),
    ("fliplr", lambda s: s[:, ::-1], ((-1, 0), (0, 1))),
    ("rot180", lambda s: np.rot90(s, 2), ((-1, 0), (0, -1))),
    ("transpose", lambda s: np.swapaxes(s, 0, 1), ((0, 1), (1, 0))),
    ("rot90cw", lambda s: np.rot90(s, -1), ((0, 1), (-1, 0))),
    ("rot90ccw", lambda s: np.rot90(s, 1), ((0, -1), (1, 0))),
    ("antitranspose", lambda s: np.swapaxes(np.rot90(s, 2), 0, 1), ((0, -1), (-1, 0))),
]


def affine(src_hw, out_hw, angle=0.0, scale=1.0, shear=0.0, D=((1, 0), (0, 1)), shift=(0.0, 0.0)):
    """(a, b) of p_src = c_src + shift + M (p_out - c_out), M = R(angle) Sh(shear) D / scale in float64, rounded once to Q16;
    R = [[cos, -sin], [sin, cos]], Sh = [[1, tan], [0, 1]], c = ((w - 1) / 2, (h - 1) / 2), shift in source pixels (x, y)."""
    (sh, sw), (oh, ow) = src_hw, out_hw
    c, s = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    M = np.array([[c, -s], [s, c]]) @ np.array([[1.0, math.tan(math.radians(shear))], [0.0, 1.0]]) @ np.array(D, np.float64) / scale
    t = np.array([(sw - 1) / 2 + shift[0], (sh - 1) / 2 + shift[1]]) - M @ np.array([(ow - 1) / 2, (oh - 1) / 2])
    return tuple(int(round(float(v) * 65536)) for v in M.reshape(-1)), tuple(int(round(float(v) * 65536)) for v in t)
