"""The arbitrary-size resize (csrc/resize_coords.h, sg_resize_fwd / _bwd, sg_prob_resize_accumulate) restated in numpy: the
taps in integers, the blend in float64, the transpose as an explicit scatter.  Per axis, input extent n, output extent m:
    num = (2o + 1) n - m    den = 2m    fl = floor(num / den)    r = num - fl den
    bilinear:  lo = max(fl, 0)   hi = min(max(fl + (r != 0), 0), n - 1)   f = r / den     y = x[lo] + (x[hi] - x[lo]) f
    nearest:   src = min(floor((2o + 1) n / (2m)), n - 1)
tests/test_resize_cpu.py holds these to torch's float64 interpolate(align_corners=False) and its autograd."""
import numpy as np


def taps(n, m):
    """(lo, hi, r, den) of every output index of one axis: int64 arrays [m] and the integer den."""
    o = np.arange(m, dtype=np.int64)
    num, den = (2 * o + 1) * n - m, 2 * m
    fl = num // den                         # numpy's // floors
    r = num - fl * den
    assert ((0 <= r) & (r < den)).all()
    lo = np.maximum(fl, 0)
    hi = np.minimum(np.maximum(fl + (r != 0), 0), n - 1)
    return lo, hi, r, den


def frac(n, m, dtype=np.float64):
    """f of every output index: float64 for the references, float32 (one correctly rounded division) as the kernels form it."""
    _, _, r, den = taps(n, m)
    return (r.astype(dtype) / dtype(den)).astype(dtype)


def nearest_src(n, m):
    o = np.arange(m, dtype=np.int64)
    return np.minimum(((2 * o + 1) * n) // (2 * m), n - 1)


def first(k, n, m):
    """clamp(ceil(((2k + 1) m - n) / (2n)), 0, m): the smallest o with fl(o) >= k."""
    return int(min(max(-((-((2 * k + 1) * m - n)) // (2 * n)), 0), m))


def span(i, n, m):
    """[o0, o1): the outputs that can touch input i (the bilinear backward's gather range)."""
    return (0 if i == 0 else first(i - 1, n, m)), (m if i == n - 1 else first(i + 1, n, m))


def span_brute(i, n, m):
    """(first, last) output with lo == i or hi == i, or None."""
    lo, hi, _, _ = taps(n, m)
    hit = np.nonzero((lo == i) | (hi == i))[0]
    return (int(hit[0]), int(hit[-1])) if hit.size else None


def _axis_fwd(x, axis, m, method):
    n = x.shape[axis]
    if method == "nearest":
        return np.take(x, nearest_src(n, m), axis=axis)
    lo, hi, _, _ = taps(n, m)
    shape = [1] * x.ndim
    shape[axis] = m
    f = frac(n, m).reshape(shape)
    a, b = np.take(x, lo, axis=axis), np.take(x, hi, axis=axis)
    return a + (b - a) * f


def resize_fwd(x, oh, ow, method="bilinear"):
    """x [N,H,W,C] -> float64 [N,oh,ow,C]; columns first, then rows."""
    x = np.asarray(x, dtype=np.float64)
    return _axis_fwd(_axis_fwd(x, 2, ow, method), 1, oh, method)


def _axis_bwd(dy, axis, n, method):
    """The transpose along one axis by an explicit scatter, output by output."""
    m = dy.shape[axis]
    dy = np.moveaxis(dy, axis, 0)
    dx = np.zeros((n,) + dy.shape[1:], dtype=np.float64)
    if method == "nearest":
        for o, s in enumerate(nearest_src(n, m)):
            dx[s] += dy[o]
    else:
        lo, hi, _, _ = taps(n, m)
        f = frac(n, m)
        for o in range(m):
            dx[lo[o]] += (1.0 - f[o]) * dy[o]
            dx[hi[o]] += f[o] * dy[o]
    return np.moveaxis(dx, 0, axis)


def resize_bwd(dy, h, w, method="bilinear"):
    """dy [N,OH,OW,C] -> float64 dx [N,h,w,C]."""
    dy = np.asarray(dy, dtype=np.float64)
    return _axis_bwd(_axis_bwd(dy, 1, h, method), 2, w, method)


def nearest_bwd_f32(dy, h, w):
    """The nearest backward as the kernel sums it, in float32: per dx element the dy of its run, rows outer, columns inner,
    ascending, starting from 0 (bit-exact reference)."""
    dy = np.asarray(dy, dtype=np.float32)
    N, OH, OW, C = dy.shape
    sh, sw = nearest_src(h, OH), nearest_src(w, OW)
    dx = np.zeros((N, h, w, C), dtype=np.float32)
    for a in range(OH):
        for b in range(OW):
            dx[:, sh[a], sw[b]] = dx[:, sh[a], sw[b]] + dy[:, a, b]
    return dx


def fold(acc_s, wsum_s, acc, wsum, weight):
    """sg_prob_resize_accumulate in float64 from the given canvases: (acc + weight * resize(acc_s / wsum_s), wsum + weight);
    every tap normalised before the blend, 0 where wsum_s is not positive."""
    acc_s, wsum_s = np.asarray(acc_s, dtype=np.float64), np.asarray(wsum_s, dtype=np.float64)
    q = np.where(wsum_s[..., None] > 0, acc_s / np.where(wsum_s > 0, wsum_s, 1.0)[..., None], 0.0)
    ch, cw = np.asarray(wsum).shape
    v = resize_fwd(q[None], ch, cw)[0]
    return np.asarray(acc, dtype=np.float64) + float(weight) * v, np.asarray(wsum, dtype=np.float64) + float(weight)
