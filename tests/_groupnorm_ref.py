"""GroupNormalization in plain float64 torch formulas, for tests/test_groupnorm_cpu.py (which holds them to
torch.nn.functional.group_norm and its autograd) and the GPU tests.

Layout as in the engine: x [N][HW][C], G groups of Cg = C / G adjacent channels, statistics per (n, g) over HW * Cg elements,
biased variance, invstd = 1 / sqrt(var + eps).  gamma / beta None: 1 / 0.  Nothing here needs a GPU."""
import torch

EPS = 1e-3

# (N, HW, C, G): where the kernels can break (tests/test_groupnorm_gpu.py says why for each)
SHAPES = [(2, 25, 12, 3), (2, 25, 12, 4), (3, 25, 12, 1), (3, 25, 12, 12), (2, 9, 26, 2), (2, 9, 7, 7), (2, 9, 16, 2), (2, 9, 12, 3),
          (1, 1, 16, 2), (4, 1, 8, 8), (2, 2100, 8, 2), (2, 2101, 8, 2), (2, 16400, 8, 2)]


def _per_channel(t, G):
    """[N][G] -> [N][1][C]"""
    return lambda C: t.repeat_interleave(C // G, dim=1).unsqueeze(1)


def stats(x, G):
    """mean, biased variance [N][G] of x [N][HW][C]"""
    N, HW, C = x.shape
    v = x.reshape(N, HW, G, C // G)
    mean = v.mean(dim=(1, 3))
    var = ((v - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, var


def affine(x, gamma, beta, mean, invstd, G):
    """gamma_c (x - mean_ng) invstd_ng + beta_c, before any ReLU, and xhat"""
    C = x.shape[-1]
    xhat = (x - _per_channel(mean, G)(C)) * _per_channel(invstd, G)(C)
    t = xhat if gamma is None else xhat * gamma
    return (t if beta is None else t + beta), xhat


def fwd(x, gamma, beta, G, eps=EPS, relu=False):
    """-> y, mean [N][G], invstd [N][G]"""
    mean, var = stats(x, G)
    invstd = 1.0 / torch.sqrt(var + eps)
    t, _ = affine(x, gamma, beta, mean, invstd, G)
    return (torch.relu(t) if relu else t), mean, invstd


def bwd(x, dy, gamma, beta, mean, invstd, G, relu=False):
    """-> dx, dgamma [C], dbeta [C] from the given (saved) statistics; the fused ReLU masks dy where the forward's value is <= 0"""
    N, HW, C = x.shape
    m = HW * (C // G)
    t, xhat = affine(x, gamma, beta, mean, invstd, G)
    g = dy * (t > 0) if relu else dy
    s1, s2 = g.sum(1), (g * xhat).sum(1)                     # [N][C]
    gm = torch.ones(C, dtype=x.dtype) if gamma is None else gamma
    a = (gm * s1).reshape(N, G, C // G).sum(-1)              # [N][G]
    b = (gm * s2).reshape(N, G, C // G).sum(-1)
    dx = _per_channel(invstd, G)(C) * (gm * g - _per_channel(a, G)(C) / m - xhat * _per_channel(b, G)(C) / m)
    return dx, s2.sum(0), s1.sum(0)


def off_boundary(x, gamma, beta, G, store, need_rel=1e-3, eps=EPS):
    """x (float64, already representable in `store`) moved so that no gamma * xhat + beta lies within need_rel * max|.| of the fused
    ReLU's boundary: the offending elements are stepped across or away from it (by at least one unit of the storage type) and
    the statistics taken again, until none is left.  Returns the new x (float64 values of `store` numbers) and the margin."""
    C = x.shape[-1]
    for _ in range(20):
        t = fwd(x, gamma, beta, G, eps)[0]
        ymax = float(t.abs().max())
        need = need_rel * max(ymax, 1e-30)
        bad = t.abs() < need
        if not bad.any():
            return x, float(t.abs().min()) / max(ymax, 1e-30)
        _, var = stats(x, G)
        invstd = 1.0 / torch.sqrt(var + eps)
        slope = _per_channel(invstd, G)(C) * (1.0 if gamma is None else gamma)        # dt / dx
        step = (4 * need / slope.abs()) * torch.where((t >= 0) == (slope >= 0), 1.0, -1.0)   # away from the boundary
        unit = x.abs() * 2.0 ** -6 if store == torch.bfloat16 else x.abs() * 2.0 ** -21
        step = torch.where(step >= 0, torch.maximum(step, unit), torch.minimum(step, -unit))
        x = torch.where(bad, x + step, x).to(store).double()
    raise AssertionError("could not move the inputs off the ReLU boundary")
