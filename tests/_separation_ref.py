"""Brute-force restatement of sg_object_distances / sg_separation_weights for tests/test_separation_cpu.py and
tests/test_separation_gpu.py: exact integers for the distances, float64 for the weight.  Nothing here imports the package.

    label8(mask)                    int32 [H, W]: 8-connected objects of a binary mask numbered from 0, -1 elsewhere (scipy)
    distances_ref(labels)           labels int [N, H, W] or [H, W] (>= 0 object, < 0 none) -> (d1sq, d2sq) int64 of that shape
    weight_ref(d1sq, d2sq, w0, s)   float64 term of the same shape, 0 where it does not apply

distances_ref takes, per object, the minimum over ITS pixels of dy^2 + dx^2 at every pixel of the image, and keeps the two
smallest of these per-object minima per pixel - no row / column decomposition, no distance transform."""
import numpy as np

INF = 0x7fffffff


def label8(mask, connectivity=8):
    from scipy import ndimage
    st = np.ones((3, 3), np.int8) if connectivity == 8 else None
    lab, _ = ndimage.label(np.asarray(mask) != 0, structure=st)
    return (lab - 1).astype(np.int32)


def _one(labels):
    h, w = labels.shape
    ys, xs = np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64)
    d1 = np.full((h, w), INF, np.int64)
    d2 = np.full((h, w), INF, np.int64)
    for k in np.unique(labels[labels >= 0]):
        py, px = np.nonzero(labels == k)
        d = np.full((h, w), INF, np.int64)
        for a in range(0, len(py), 256):   # the object's pixels, 256 at a time: dd[p, y, x] = (y - py)^2 + (x - px)^2
            dd = ((ys[None] - py[a:a + 256, None]) ** 2)[:, :, None] + ((xs[None] - px[a:a + 256, None]) ** 2)[:, None, :]
            d = np.minimum(d, dd.min(0))
        d2 = np.minimum(d2, np.maximum(d1, d))
        d1 = np.minimum(d1, d)
    return d1, d2


def distances_ref(labels):
    labels = np.asarray(labels)
    if labels.ndim == 2:
        return _one(labels)
    outs = [_one(l) for l in labels]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


def weight_ref(d1sq, d2sq, w0, sigma):
    d1sq, d2sq = np.asarray(d1sq, np.int64), np.asarray(d2sq, np.int64)
    on = (d1sq > 0) & (d2sq != INF)
    s = np.sqrt(np.where(on, d1sq, 0).astype(np.float64)) + np.sqrt(np.where(on, d2sq, 0).astype(np.float64))
    return np.where(on, float(w0) * np.exp(-(s * s) / (2.0 * float(sigma) ** 2)), 0.0)
