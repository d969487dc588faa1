"""Plain references for the C-class head (tests/test_multiclass_cpu.py, tests/test_multiclass_gpu.py): last-axis softmax, the
three losses with per-class weights, the C x C confusion matrix, the class-map canvas and the matrix metrics.  Everything
takes torch tensors in the dtype it is to compute in (float64 for a reference) and needs no GPU."""
import numpy as np
import torch

K_EPS = 1e-7   # tf.keras.backend.epsilon()


def softmax_ref(z):
    return torch.softmax(z, dim=-1)


def softmax_bwd_ref(p, dp):
    return p * (dp - (dp * p).sum(-1, keepdim=True))


def loss_coeffs(kind, yt, C, alpha):
    """a_c: kind 0 y_c; kind 1 alpha_c y_c; kind 2 alpha_c w_c y_c with w = y_true[..., C:2C]."""
    y = yt[..., :C]
    if kind == 0:
        return y
    a = torch.as_tensor(alpha, dtype=yt.dtype)
    if kind == 1:
        return a * y
    return a * yt[..., C:2 * C] * y


def loss_ref(kind, p, yt, alpha=None):
    """L = -(1/rows) sum_rows sum_c a_c f(p_c) log(p_c + eps), rows = every axis but the last."""
    C = p.shape[-1]
    a = loss_coeffs(kind, yt, C, alpha)
    f = torch.ones_like(p) if kind == 0 else (1 - p) ** 2
    return -(a * f * torch.log(p + K_EPS)).sum() / (p.numel() // C)


def loss_bwd_ref(kind, p, yt, alpha, scale):
    C = p.shape[-1]
    a = loss_coeffs(kind, yt, C, alpha)
    if kind == 0:
        g = 1 / (p + K_EPS)
    else:
        g = -2 * (1 - p) * torch.log(p + K_EPS) + (1 - p) ** 2 / (p + K_EPS)
    return -(scale / (p.numel() // C)) * a * g


def argmax_low(t):
    """Index of the FIRST maximum of the last axis (strict '>' while scanning upwards, as tf.argmax)."""
    C = t.shape[-1]
    idx = torch.arange(C).expand(t.shape)
    top = t.max(-1, keepdim=True).values
    return torch.where(t == top, idx, torch.full_like(idx, C)).min(-1).values


def confusion_matrix_ref(p, yt):
    """int64 [C * C]: cell t * C + q counts the rows whose truth is class t and prediction class q."""
    C = p.shape[-1]
    cell = argmax_low(yt[..., :C]).reshape(-1) * C + argmax_low(p).reshape(-1)
    return torch.bincount(cell, minlength=C * C).to(torch.int64)


def argmax_max_ref(canvas, p, y0, x0):
    """canvas[y0 + r, x0 + c] = max(canvas, argmax p[r, c]) clipped to the canvas; returns a new uint8 canvas."""
    out = canvas.clone()
    CH, CW = out.shape
    TH, TW = p.shape[:2]
    q = argmax_low(p).to(torch.uint8)
    r0, r1, c0, c1 = max(0, -y0), min(TH, CH - y0), max(0, -x0), min(TW, CW - x0)
    if r1 > r0 and c1 > c0:
        win = out[y0 + r0:y0 + r1, x0 + c0:x0 + c1]
        out[y0 + r0:y0 + r1, x0 + c0:x0 + c1] = torch.maximum(win, q[r0:r1, c0:c1])
    return out


def metrics_ref64(M):
    """The matrix metrics restated in float64: PA, per-class IoU / F1, IoU and F1_score over the foreground classes, MIoU."""
    M = np.asarray(M, np.float64)
    C, e = M.shape[0], K_EPS
    row, col, diag = M.sum(1), M.sum(0), np.diag(M)
    iou = diag / (row + col - diag + e)
    rec, prec = diag / (row + e), diag / (col + e)
    f1 = 2 * prec * rec / (prec + rec + e)
    return {"PA": diag.sum() / (M.sum() + e), "IoU": iou[1:].mean(), "MIoU": iou.mean(), "F1_score": f1[1:].mean(),
            "IoU_per_class": list(iou), "F1_per_class": list(f1)}


def class_probs(g, rows, C, lo=-4.0, hi=4.0):
    """fp32 probabilities of random logits in [lo, hi] (rows of them sum to 1 within fp32 rounding)."""
    z = torch.rand(rows, C, generator=g, dtype=torch.float64) * (hi - lo) + lo
    return torch.softmax(z, dim=1).float()


def class_labels(g, rows, C, y_cols):
    """One-hot truth of random classes and, with y_cols = 2C, per-class weights in {1, 2}."""
    t = torch.randint(0, C, (rows,), generator=g)
    y = torch.nn.functional.one_hot(t, C).float()
    if y_cols == 2 * C:
        y = torch.cat([y, 1 + (torch.rand(rows, C, generator=g) > 0.7).float()], 1)
    return y.contiguous()
