"""Float64 reference of hard-pixel mining (sg_loss_mined_*) for tests/test_hard_mining_cpu.py and
tests/test_hard_mining_gpu.py.  Needs no GPU.

The keys are taken from the fp32 p by indexing (no arithmetic: the device's keys to the bit), T from np.partition on float32,
the kept set is key <= T (every tie kept), loss and gradient are float64 on the same fp32 inputs."""
import numpy as np
import torch

import _multiclass_ref as MR

K_EPS = MR.K_EPS


def keys_ref(p32, yt, C):
    """float32 numpy [rows]: p at the first maximum of y_true[:, :C], clamped to [0, 1]; a NaN (and -0) counts as +0."""
    p32 = p32.detach().cpu().reshape(-1, C)
    assert p32.dtype == torch.float32
    t = MR.argmax_low(yt.detach().cpu().reshape(p32.shape[0], -1)[:, :C])
    q = p32.gather(1, t.reshape(-1, 1)).reshape(-1).numpy().copy()
    out = np.where(q > 0, np.minimum(q, np.float32(1.0)), np.float32(0.0)).astype(np.float32)   # NaN > 0 is False
    return out


def select_ref(keys, thresh, k):
    """(T as float32, kept mask) for the k-th smallest key, 1 <= k <= rows."""
    assert keys.dtype == np.float32 and 1 <= k <= keys.size
    qk = np.partition(keys, k - 1)[k - 1]
    T = max(np.float32(thresh), qk)
    return np.float32(T), keys <= T


def bits(v):
    return int(np.asarray(v, np.float32).reshape(1).view(np.uint32)[0])


def row_terms(kind, p, yt, alpha=None):
    """l_i [rows] in the dtype of p: -(sum_c a_c f(p_c) log(p_c + eps))."""
    C = p.shape[-1]
    a = MR.loss_coeffs(kind, yt, C, alpha)
    f = torch.ones_like(p) if kind == 0 else (1 - p) ** 2
    return -(a * f * torch.log(p + K_EPS)).sum(-1)


def mined_ref(kind, p32, yt32, alpha, thresh, k, scale=1.0, p64=None):
    """dict(T, T_bits, kept (bool tensor), n_kept, loss (float64 [1]), grad (float64 [rows, C])).  p64: evaluate loss and
    gradient at these float64 probabilities instead of p32.double() (central differences); the kept set stays that of p32."""
    C = p32.shape[-1]
    keys = keys_ref(p32, yt32, C)
    T, keep = select_ref(keys, thresh, k)
    keep = torch.from_numpy(keep)
    n = int(keep.sum())
    p = p32.double() if p64 is None else p64
    yt = yt32.double()
    loss = row_terms(kind, p, yt, alpha)[keep].sum().reshape(1) / n
    a = MR.loss_coeffs(kind, yt, C, alpha)
    g = 1 / (p + K_EPS) if kind == 0 else -2 * (1 - p) * torch.log(p + K_EPS) + (1 - p) ** 2 / (p + K_EPS)
    grad = -(scale / n) * a * g * keep.reshape(-1, 1)
    return dict(T=T, T_bits=bits(T), kept=keep, n_kept=n, loss=loss, grad=grad)
