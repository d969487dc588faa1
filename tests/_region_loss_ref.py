"""Plain float64 restatement of the region-overlap losses (tests/test_region_loss_cpu.py, tests/test_region_loss_gpu.py):
Dice / Jaccard / Tversky terms, alone or added to one of the three pointwise losses of tests/_multiclass_ref.py.  Everything
takes torch tensors in the dtype it is to compute in (float64 for a reference) and needs no GPU.

A descriptor is a dict: a, b, smooth, gamma, class_w (C floats), images, point_kind (-1: none), point_alpha (C floats or None),
point_weight, region_weight.  p is [rows, C], y_true [rows, C or 2C]; group g is rows g * rows/images ... of both."""
import torch

import _multiclass_ref as MR


def desc(C, a=0.5, b=0.5, smooth=1.0, gamma=1.0, class_w=None, images=1, point_kind=-1, point_alpha=None, point_weight=1.0,
         region_weight=1.0):
    return dict(a=a, b=b, smooth=smooth, gamma=gamma, class_w=tuple(class_w) if class_w is not None else (1.0,) * C, images=images,
                point_kind=point_kind, point_alpha=point_alpha, point_weight=point_weight, region_weight=region_weight)


def sums(d, p, yt):
    """I, P, Y as [images, C]."""
    C = p.shape[-1]
    G = d["images"]
    pg, yg = p.reshape(G, -1, C), yt[..., :C].reshape(G, -1, C)
    return (pg * yg).sum(1), pg.sum(1), yg.sum(1)


def region_terms(d, p, yt):
    """(L_region, A, B): the loss of the region term on its own (no region_weight) and the coefficients [images, C] of its
    gradient dL_region/dp[r, c] = A[g, c] y[r, c] + B[g, c]."""
    a, b, s, gamma = d["a"], d["b"], d["smooth"], d["gamma"]
    w = torch.as_tensor(d["class_w"], dtype=p.dtype)
    G, sw = d["images"], float(sum(d["class_w"]))
    I, P, Y = sums(d, p, yt)
    D = I + a * (P - I) + b * (Y - I) + s
    u = (1 - (I + s) / D).clamp_min(0)
    L = (w * u ** gamma).sum() / (G * sw)
    du = torch.ones_like(u) if gamma == 1 else gamma * u ** (gamma - 1)      # (1 - T)^0 = 1 also at T = 1
    k = -w * du / (G * sw * D ** 2)
    return L, k * (D - (I + s) * (1 - a - b)), -k * (I + s) * a


def point_loss(d, p, yt):
    if d["point_kind"] < 0:
        return torch.zeros((), dtype=p.dtype)
    return MR.loss_ref(d["point_kind"], p, yt, d["point_alpha"])


def loss_ref(d, p, yt):
    """[3] = {L, L_point, L_region}; L_point is 0 without a pointwise term."""
    Lr = region_terms(d, p, yt)[0]
    Lp = point_loss(d, p, yt)
    L = d["region_weight"] * Lr + (d["point_weight"] * Lp if d["point_kind"] >= 0 else 0.0)
    return torch.stack([L, Lp, Lr])


def coef_ref(d, p, yt):
    """[images, 2C] = {A[C], B[C]} with region_weight folded in: what the backward pass reads."""
    _, A, B = region_terms(d, p, yt)
    return d["region_weight"] * torch.cat([A, B], 1)


def grad_ref(d, p, yt, scale=1.0):
    """scale * dL/dp, [rows, C]."""
    C = p.shape[-1]
    G = d["images"]
    AB = coef_ref(d, p, yt)
    y = yt[..., :C].reshape(G, -1, C)
    g = (AB[:, None, :C] * y + AB[:, None, C:]).reshape(p.shape)
    if d["point_kind"] >= 0:
        g = g + d["point_weight"] * MR.loss_bwd_ref(d["point_kind"], p, yt, d["point_alpha"], 1.0)
    return scale * g
