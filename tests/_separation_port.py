"""A plain Python port of csrc/separation.hip's algorithm - the row-state merge scanned in tiles of 64 with a carry, the
left / right merge into two signed column offsets, the outward column walk with its early stop - for tests/test_separation_cpu.py:
it holds the ALGORITHM (two candidates per row suffice; the merges; the stop rule) to the brute force where there is no GPU.
The kernels are held to the same brute force by tests/test_separation_gpu.py."""
import numpy as np

INF = 0x7fffffff
NONE = -32768
WAVE = 64


def merge(a, b, second):
    if b[0] < 0:
        return a
    r = list(b)
    if second and b[2] < 0:
        if a[0] >= 0 and a[1] != b[1]:
            r[2], r[3] = a[0], a[1]
        elif a[2] >= 0 and a[3] != b[1]:
            r[2], r[3] = a[2], a[3]
    return tuple(r)


def scan_tile(us, labs, carry, second):
    s = [(u if l >= 0 else -1, l, -1, 0) for u, l in zip(us, labs)]
    off = 1
    while off < WAVE:
        o = [s[i - off] if i >= off else None for i in range(WAVE)]
        s = [merge(o[i], s[i], second) if i >= off else s[i] for i in range(WAVE)]
        off *= 2
    s = [merge(carry, x, second) for x in s]
    return s, s[-1]


def dist(c):
    return abs(c[0])


def nearer(a, b):
    return b if dist(b) < dist(a) else a


def other(c1, c2, obj):
    return c2 if (c1[0] != NONE and c1[1] == obj) else c1


def row_pass(L, second):
    W = len(L)
    tiles = (W + WAVE - 1) // WAVE
    c = [None] * W
    carry = (-1, 0, -1, 0)
    for t in range(tiles):
        xs = [t * WAVE + l for l in range(WAVE)]
        s, carry = scan_tile(xs, [L[x] if x < W else -1 for x in xs], carry, second)
        for l, x in enumerate(xs):
            if x < W:
                c[x] = (s[l][0] - x if s[l][0] >= 0 else NONE, s[l][2] - x if (second and s[l][2] >= 0) else NONE)
    carry = (-1, 0, -1, 0)
    out = [None] * W
    for t in range(tiles):
        us = [t * WAVE + l for l in range(WAVE)]
        xs = [W - 1 - u for u in us]
        s, carry = scan_tile(us, [L[x] if x >= 0 else -1 for x in xs], carry, second)
        for l, (u, x) in enumerate(zip(us, xs)):
            if x < 0:
                continue
            l1 = [c[x][0], 0]
            l2 = [c[x][1], 0]
            r1 = (u - s[l][0] if s[l][0] >= 0 else NONE, s[l][1])
            r2 = (u - s[l][2] if s[l][2] >= 0 else NONE, s[l][3])
            if not second:
                out[x] = (nearer(l1, r1)[0], NONE)
                continue
            if l1[0] != NONE:
                l1[1] = L[x + l1[0]]
            if l2[0] != NONE:
                l2[1] = L[x + l2[0]]
            if dist(l1) <= dist(r1):
                first = l1
                sec = nearer(l2, other(r1, r2, l1[1]))
            else:
                first = r1
                sec = nearer(r2, other(l1, l2, r1[1]))
            out[x] = (first[0], sec[0])
    return out


def col_pass(lab, cand, second):
    H, W = lab.shape
    d1 = np.zeros((H, W), np.int64)
    d2 = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            st = dict(b1=INF, b2=INF, o1=-1)

            def take(d, o):
                if d < st["b1"]:
                    if o != st["o1"]:
                        st["b2"] = st["b1"]
                    st["b1"] = d
                    st["o1"] = o
                elif o != st["o1"]:
                    st["b2"] = d

            def visit(r, dy2):
                o1, o2 = cand[r][x]
                if o1 == NONE:
                    return
                da = o1 * o1 + dy2
                if not second:
                    st["b1"] = min(st["b1"], da)
                    return
                if da < st["b2"]:
                    take(da, lab[r, x + o1])
                if o2 == NONE:
                    return
                db = o2 * o2 + dy2
                if db < st["b2"]:
                    take(db, lab[r, x + o2])

            for dy in range(H):
                dy2 = dy * dy
                if dy2 >= (st["b2"] if second else st["b1"]):
                    break
                up, down = y - dy >= 0, dy > 0 and y + dy < H
                if not up and not down:
                    break
                if up:
                    visit(y - dy, dy2)
                if down:
                    visit(y + dy, dy2)
            d1[y, x], d2[y, x] = st["b1"], st["b2"]
    return d1, d2


def run(lab, second=True):
    cand = [row_pass(list(r), second) for r in lab]
    return col_pass(lab, cand, second)
