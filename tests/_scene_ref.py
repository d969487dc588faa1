"""numpy float64 restatement of sg_scene_tiles_u8, sg_prob_accumulate and sg_prob_finalize (include/segengine.h), written from
the formulas with explicit index arithmetic (no flip / transpose helper), for tests/test_scene_cpu.py and
tests/test_scene_gpu.py.

The tile <-> window map: for tile coordinate (r, c) of a T x T tile
    (a, b) = (sym & 4) ? (c, r) : (r, c);  u = (sym & 1) ? T-1-a : a;  v = (sym & 2) ? T-1-b : b
and tile element (r, c) corresponds to scene / canvas pixel (y0+u, x0+v)."""
import numpy as np


def sym_map(sym, T):
    """Index arrays (r, c, u, v), each [T,T]: tile element (r, c) <-> window position (u, v)."""
    r = np.repeat(np.arange(T), T).reshape(T, T)
    c = np.tile(np.arange(T), T).reshape(T, T)
    a, b = (c, r) if sym & 4 else (r, c)
    u = T - 1 - a if sym & 1 else a
    v = T - 1 - b if sym & 2 else b
    return r, c, u, v


def scene_tiles_ref(scene, items, T):
    """uint8 [H,W,3] -> float32 [N,T,T,3]: np.float32(np.float64(s) / 127.5 - 1), 0 outside the scene."""
    H, W = scene.shape[:2]
    out = np.zeros((len(items), T, T, 3), np.float32)
    for n, (y0, x0, sym) in enumerate(items):
        r, c, u, v = sym_map(sym, T)
        y, x = y0 + u, x0 + v
        m = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        out[n, r[m], c[m], :] = np.float32(np.float64(scene[y[m], x[m], :]) / 127.5 - 1)
    return out


def prob_accumulate_ref(p, items, win, scale, acc, wsum, state=None):
    """acc [CH,CW,C] and wsum [CH,CW] (float64, updated in place) take the items in order.  `state` = (mag, wmag, cnt) carries
    what the error bound needs across calls: mag = |acc0| + sum w |p|, wmag = |wsum0| + sum w, cnt = contributions per
    pixel; it is created from the canvases when None and returned."""
    CH, CW = wsum.shape
    T = p.shape[1]
    if state is None:
        state = (np.abs(acc).copy(), np.abs(wsum).copy(), np.zeros((CH, CW), np.int64))
    mag, wmag, cnt = state
    p = np.asarray(p, np.float64)
    win = np.asarray(win, np.float64)
    scale = float(np.float32(scale))          # the entry point takes a C float
    for n, (y0, x0, sym) in enumerate(items):
        r, c, u, v = sym_map(sym, T)
        y, x = y0 + u, x0 + v
        m = (y >= 0) & (y < CH) & (x >= 0) & (x < CW)
        ym, xm = y[m], x[m]                   # distinct pixels: the map is a bijection of the window
        w = scale * win[u[m]] * win[v[m]]
        contrib = w[:, None] * p[n, r[m], c[m], :]
        acc[ym, xm, :] += contrib
        wsum[ym, xm] += w
        mag[ym, xm, :] += np.abs(contrib)
        wmag[ym, xm] += w
        cnt[ym, xm] += 1
    return state


def prob_finalize_ref(acc, wsum, out_scale):
    """(uint8 map, float64 probabilities): first maximum (ties -> lowest index) of acc, acc / wsum; 0 and 0 where wsum == 0."""
    C = acc.shape[-1]
    best, arg = acc[..., 0].copy(), np.zeros(acc.shape[:2], np.int64)
    for k in range(1, C):
        take = acc[..., k] > best
        best = np.where(take, acc[..., k], best)
        arg = np.where(take, k, arg)
    reached = wsum != 0
    safe = np.where(reached, wsum, 1.0)
    probs = np.where(reached[..., None], np.asarray(acc, np.float64) / np.asarray(safe, np.float64)[..., None], 0.0)
    return np.where(reached, out_scale * arg, 0).astype(np.uint8), probs
