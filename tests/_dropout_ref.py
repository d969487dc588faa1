"""Host reference of Dropout / SpatialDropout2D (include/segengine.h: sg_dropout), written from the definition and
not from the kernel: Philox4x32-10 and keep() in numpy on uint64, and the expected output in fp32 and - through torch's CPU
bfloat16, which rounds to nearest even - in bf16.

    keep(idx; k0, k1, stream, step, thr):  q = idx >> 2;  words = Philox4x32-10(counter (q mod 2^32, q >> 32, stream, step),
                                           key (k0, k1));  kept iff words[idx & 3] >= thr
    thr = min(floor(rate * 2^32), 2^32 - 1);  scale = float32(1 / (1 - rate));  kept: x * scale in fp32, dropped: +0
    mask index of element i (flat NHWC):  first + i  |  first + (i div HWC) * C + i mod C  (noise shape [N,1,1,C])
"""
import math

import numpy as np
import torch

U64 = np.uint64
MASK32 = U64(0xFFFFFFFF)
M0, M1 = U64(0xD2511F53), U64(0xCD9E8D57)
W0, W1 = U64(0x9E3779B9), U64(0xBB67AE85)
S32 = U64(32)


def _u(v, like=None):
    a = np.asarray(v, dtype=U64)
    return a if like is None else np.broadcast_to(a, like.shape)


def philox4x32_10(counter, key):
    """counter: four uint32 values or arrays, key: two.  Returns the four output words as uint64 arrays (values < 2^32)."""
    c0, c1, c2, c3 = (_u(c) for c in counter)
    k0, k1 = (_u(k) for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2            # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK32, (p0 >> S32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def words(idx, k0, k1, stream, step):
    """The 32-bit mask word of every mask index in `idx` (uint64 array)."""
    idx = np.asarray(idx, dtype=U64)
    q = idx >> U64(2)
    if idx.ndim == 1 and idx.size > 4096 and bool(np.all(q[1:] >= q[:-1])):
        # a long ascending run (the element form): one generator call per distinct q instead of one per index - the same function
        new = np.concatenate(([True], q[1:] != q[:-1]))
        w = np.stack(philox4x32_10((q[new] & MASK32, q[new] >> S32, stream, step), (k0, k1)))
        return w[(idx & U64(3)).astype(np.int64), np.cumsum(new) - 1]
    w = np.stack([np.broadcast_to(x, idx.shape) for x in philox4x32_10((q & MASK32, q >> S32, stream, step), (k0, k1))])
    return np.take_along_axis(w, (idx & U64(3)).astype(np.int64)[None], 0)[0]


def keep(idx, k0, k1, stream, step, thr):
    return words(idx, k0, k1, stream, step) >= U64(thr)


def threshold(rate):
    return min(int(math.floor(float(rate) * 2.0 ** 32)), 2 ** 32 - 1)


def scale(rate):
    return float(np.float32(1.0 / (1.0 - float(rate))))


def mask_index(n, first=0, hwc=0, c=0):
    """Mask indices of the flat NHWC elements 0 .. n - 1 (uint64, wrapping like the kernel's arithmetic)."""
    i = np.arange(n, dtype=U64)
    first = U64(int(first) % 2 ** 64)
    with np.errstate(over="ignore"):
        if hwc == 0:
            return first + i
        return first + (i // U64(hwc)) * U64(c) + i % U64(c)


def expected(x, kept, sc):
    """x (torch fp32 or bf16, any shape) with the flat boolean mask `kept`: x * sc in fp32 where kept, +0 elsewhere, in x's type."""
    k = torch.from_numpy(np.ascontiguousarray(kept)).reshape(x.shape)
    y = torch.where(k, x.float() * torch.tensor(sc, dtype=torch.float32), torch.zeros((), dtype=torch.float32))
    return y.to(x.dtype)


def reference(x, rate_or_thr, k0, k1, stream, step, first=0, hwc=0, c=0, sc=None, is_thr=False):
    """Expected sg_dropout output of tensor x and the flat mask that produced it."""
    thr = rate_or_thr if is_thr else threshold(rate_or_thr)
    if sc is None:
        sc = scale(rate_or_thr)
    kept = keep(mask_index(x.numel(), first, hwc, c), k0, k1, stream, step, thr)
    return expected(x, kept, sc), kept
