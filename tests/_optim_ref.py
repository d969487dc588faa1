"""The optimizers' update rules restated in float64 torch on the CPU (building_detection_amd/optimizers.py states them in words;
csrc/optim.hip computes them in fp32).  One flat arena per operand, as the engine keeps them: `segs` = [(offset, size, decayed)],
one entry per trainable parameter; elements between two parameters (padding) are never read and come back as they went in.
"""
import math
from dataclasses import dataclass
from typing import Optional

import torch


@dataclass
class Cfg:
    kind: str = "adam"                 # "adam" | "sgd"
    beta_1: float = 0.9
    beta_2: float = 0.999
    epsilon: float = 1e-7
    amsgrad: bool = False
    momentum: float = 0.0
    nesterov: bool = False
    weight_decay: float = 0.0
    clip: Optional[str] = None         # None | "value" | "norm" | "global"
    clip_c: float = 0.0
    ema_momentum: Optional[float] = None
    grad_scale: float = 1.0


def adam_lr_t(lr, b1, b2, t):
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def norms_ref(segs, g, grad_scale=1.0):
    """(sum over all parameter elements, [sum per parameter]) of (grad_scale * g)^2, float64."""
    per = [((g[o:o + n].double() * grad_scale) ** 2).sum() for o, n, _ in segs]
    return torch.stack(per).sum(), torch.stack(per)


def new_state(cfg, w):
    """Zero moments; the average starts as a copy of the weights."""
    z = torch.zeros_like(w, dtype=torch.float64)
    return dict(m=z.clone(), v=z.clone(), vhat=z.clone(), ema=w.double().clone())


def step_ref(cfg, segs, w, g, st, lr, lr_t=None):
    """One step: returns (w', state') as new float64 tensors.  lr_t: Adam's bias-corrected rate (adam_lr_t); ignored by SGD."""
    w = w.double().clone()
    st = {k: v.double().clone() for k, v in st.items()}
    total, per = norms_ref(segs, g, cfg.grad_scale)
    for s, (o, n, decayed) in enumerate(segs):
        sl = slice(o, o + n)
        gk = g[sl].double() * cfg.grad_scale
        if cfg.clip == "value":
            gk = gk.clamp(-cfg.clip_c, cfg.clip_c)
        elif cfg.clip in ("norm", "global"):
            nrm = math.sqrt(float(per[s] if cfg.clip == "norm" else total))
            gk = gk * (cfg.clip_c / max(nrm, cfg.clip_c))
        ws = w[sl]
        if decayed and cfg.weight_decay:
            ws = ws - lr * cfg.weight_decay * ws
        if cfg.kind == "adam":
            m = cfg.beta_1 * st["m"][sl] + (1 - cfg.beta_1) * gk
            v = cfg.beta_2 * st["v"][sl] + (1 - cfg.beta_2) * gk * gk
            st["m"][sl], st["v"][sl] = m, v
            d = v
            if cfg.amsgrad:
                d = torch.maximum(st["vhat"][sl], v)
                st["vhat"][sl] = d
            ws = ws - lr_t * m / (torch.sqrt(d) + cfg.epsilon)
        elif cfg.momentum == 0.0:
            ws = ws - lr * gk
        else:
            m = cfg.momentum * st["m"][sl] - lr * gk
            st["m"][sl] = m
            ws = ws + (cfg.momentum * m - lr * gk if cfg.nesterov else m)
        w[sl] = ws
        if cfg.ema_momentum is not None:
            st["ema"][sl] = cfg.ema_momentum * st["ema"][sl] + (1 - cfg.ema_momentum) * ws
    return w, st
