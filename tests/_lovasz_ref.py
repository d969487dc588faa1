"""numpy restatement of the Lovasz-Softmax loss of include/segengine.h (sg_loss_lovasz_*), written from the definition.
The clamped probabilities, the errors m and the sort keys are float32 / uint32 to the bit; the order is
np.argsort(key, kind="stable"); everything after that is float64.

g_k here is the CLOSED form, 1 / U_k or I_k / (U_k (U_k - 1)), one or two float64 roundings.  The difference form J_k - J_(k-1)
loses up to 2^-53 / g_k relative to cancellation (1e-6 at 70001 rows, where g_k reaches 2e-10): gk_diff() states it, and
tests/test_lovasz_cpu.py holds the two against each other in exact rational arithmetic."""
from fractions import Fraction

import numpy as np

ONE = np.uint32(0x3F800000)


def clamp_bits(p32):
    """The bits of p with NaN, negative and -0 -> +0 and above 1 -> 1 (row_key of csrc/hard_mining.hip)."""
    b = np.ascontiguousarray(p32, np.float32).view(np.uint32)
    return np.where(b > np.uint32(0x7F800000), np.uint32(0), np.where(b < ONE, b, ONE)).astype(np.uint32)


def truth(yt, C):
    """argmax y_true[:, :C], ties to the lowest index."""
    return np.argmax(np.asarray(yt)[:, :C], axis=1)


def errors_and_keys(p32, t, c):
    """(f, m float32 of the clamped p, key uint32) of class c."""
    f = t == c
    q = clamp_bits(p32[:, c])
    m = np.where(f, (np.float32(1.0) - q.view(np.float32)).astype(np.float32), q.view(np.float32)).astype(np.float32)
    key = (ONE - m.view(np.uint32)).astype(np.uint32)
    assert (key < 2 ** 30).all()
    return f, m, key


def gk_closed(f_sorted):
    """g_k along the order, float64, from the integer counts."""
    n = len(f_sorted)
    G = int(f_sorted.sum())
    if G == 0:
        g = np.zeros(n)
        g[0] = 1.0
        return g
    F = np.cumsum(f_sorted.astype(np.int64))
    k = np.arange(1, n + 1, dtype=np.int64)
    I, U = (G - F).astype(np.float64), (G + k - F).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(f_sorted, 1.0 / U, I / (U * (U - 1.0)))


def gk_diff(f_sorted, exact=False):
    """J_k - J_(k-1), J_k = 1 - I_k / U_k, J_0 = 0: float64, or Fractions with `exact`."""
    n = len(f_sorted)
    G = int(f_sorted.sum())
    F = np.cumsum(f_sorted.astype(np.int64))
    out, prev = [], Fraction(0) if exact else 0.0
    for k in range(1, n + 1):
        I, U = G - int(F[k - 1]), G + k - int(F[k - 1])
        J = 1 - Fraction(I, U) if exact else 1.0 - I / U
        out.append(J - prev)
        prev = J
    return out if exact else np.array(out)


def gk_closed_exact(f_sorted):
    n = len(f_sorted)
    G = int(f_sorted.sum())
    if G == 0:
        return [Fraction(1)] + [Fraction(0)] * (n - 1)
    F = np.cumsum(f_sorted.astype(np.int64))
    out = []
    for k in range(1, n + 1):
        I, U = G - int(F[k - 1]), G + k - int(F[k - 1])
        out.append(Fraction(1, U) if f_sorted[k - 1] else Fraction(I, U * (U - 1)))
    return out


def lovasz_ref(p32, yt, images=1, classes_all=False, p64=None):
    """dict(loss, l [groups, C], used [groups, C] bool, n_c [groups], g [rows, C] = dL/dp, order {(group, class): pixel indices})
    of p32 [rows, C] float32 and y_true [rows, C or 2C].  p64: evaluate the sum at these float64 probabilities instead (the
    ranks still come from p32): for finite differences."""
    p32 = np.ascontiguousarray(p32, np.float32)
    rows, C = p32.shape
    assert rows % images == 0
    n = rows // images
    t = truth(yt, C)
    l = np.zeros((images, C))
    used = np.zeros((images, C), bool)
    g = np.zeros((rows, C))
    order = {}
    for grp in range(images):
        sl = slice(grp * n, (grp + 1) * n)
        for c in range(C):
            f, m, key = errors_and_keys(p32[sl], t[sl], c)
            used[grp, c] = classes_all or f.any()
            o = np.argsort(key, kind="stable")
            order[(grp, c)] = o + grp * n
            if not used[grp, c]:
                continue
            gk = gk_closed(f[o])
            pc = p32[sl, c].astype(np.float64) if p64 is None else np.asarray(p64)[sl, c]
            mu = np.where(f, (np.float32(1.0) - p32[sl, c]).astype(np.float64) if p64 is None else 1.0 - pc, pc)   # unclamped
            with np.errstate(invalid="ignore"):
                l[grp, c] = float(np.sum(mu[o] * gk))
            g[grp * n + o, c] = np.where(f[o], -gk, gk)
    n_c = used.sum(1)
    with np.errstate(invalid="ignore"):
        loss = float(np.sum(np.where(used, l, 0.0).sum(1) / n_c) / images)
    g = g / (images * np.repeat(n_c, n))[:, None]
    return dict(loss=loss, l=l, used=used, n_c=n_c, g=g, order=order)
