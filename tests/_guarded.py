"""Guarded device operands and plain float64 references for tests/test_bandwidth_variants_gpu.py,
tests/test_batchnorm_variants_gpu.py and tests/test_depthwise_variants_gpu.py.

Every operand of a launch lives in its own uint8 arena: BAND bytes of 0xFF, the operand, BAND bytes of 0xFF.  0xFF.. is a NaN
in fp32 and in bf16, so a read outside an operand that reaches the arithmetic poisons the result, and a write outside it changes
a band.  The arena's bytes as uploaded are kept on the host; after the launch the bands (and, for an input, the operand) must be
byte-identical.  Nothing here needs a GPU: `device` may be "cpu" (the self-checks of the harness run there).
"""
import math

import torch

BAND = 1024   # bytes in front of and behind every operand (a multiple of 16: the operand starts 16-byte aligned)
INF = float("inf")


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


class Guarded:
    """One device operand between two guard bands.  role: "in" (bits must survive the launch), "out" (anything may be written
    inside the operand) or "ws" (a workspace: only the bands are looked at)."""

    def __init__(self, host, device, off=False, role="in"):
        host = host.detach().cpu()
        self.shape, self.dtype, self.role = tuple(host.shape), host.dtype, role
        self.es = host.element_size()
        self.nb = host.numel() * self.es
        # 16-byte aligned, or one element further: the dispatch code promises its scalar kernels for such tensors
        self.start = BAND + (self.es if off else 0)
        arena = torch.full((self.start + self.nb + BAND,), 0xFF, dtype=torch.uint8)
        arena[self.start:self.start + self.nb] = _bits(host)
        self.before = arena
        self.dev = arena.clone().to(device)
        assert self.dev.data_ptr() % 16 == 0, "allocator returned a block that is not 16-byte aligned"
        self.after = None

    @classmethod
    def out(cls, shape, dtype, device, off=False, role="out", fill=0xFF):
        """A non-accumulating output: every byte `fill` (0xFF = NaN for float types) before the launch."""
        shape = tuple(shape)
        n = math.prod(shape)
        es = torch.empty((), dtype=dtype).element_size()
        host = torch.full((n * es,), fill, dtype=torch.uint8).view(dtype).reshape(shape)
        return cls(host, device, off=off, role=role)

    @classmethod
    def ws(cls, nbytes, device):
        """A workspace of exactly `nbytes` bytes (16-byte aligned), NaN-filled, a band right behind its last byte."""
        return cls.out((max(int(nbytes), 1),), torch.uint8, device, role="ws")

    def ptr(self, elem_off=0):
        return self.dev.data_ptr() + self.start + elem_off * self.es

    def fetch(self):
        self.after = self.dev.cpu()
        return self

    def read(self):
        if self.after is None:
            self.fetch()
        return self.after[self.start:self.start + self.nb].clone().view(self.dtype).reshape(self.shape)

    def check(self, what=""):
        if self.after is None:
            self.fetch()
        a, b, s, e = self.after, self.before, self.start, self.start + self.nb
        assert torch.equal(a[:s], b[:s]), f"{what}: the band in front of a {self.role} operand {self.shape} changed"
        assert torch.equal(a[e:], b[e:]), f"{what}: the band behind a {self.role} operand {self.shape} changed"
        if self.role == "in":
            assert torch.equal(a[s:e], b[s:e]), f"{what}: an input operand {self.shape} changed"


def check_all(ops, what=""):
    for o in ops:
        o.fetch().check(what)


def assert_written(t, what="", fill=0xFF):
    """No prefill value may remain inside a non-accumulating output (float: NaN; integer: the fill byte)."""
    if t.dtype.is_floating_point:
        bad = torch.isnan(t.float())
    else:
        bad = _bits(t) == fill
    assert not bad.any(), f"{what}: {int(bad.sum())} of {t.numel()} output elements still hold the prefill value"


def close(got, ref, tol, what=""):
    """max|got - ref| <= tol * max|ref| over the whole tensor; nothing masked."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite values in the result"
    scale = ref.abs().max().item() if ref.numel() else 0.0
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    assert err <= tol * scale, f"{what}: max err {err:.3e} > {tol:.3e} * {scale:.3e} (rel {err / max(scale, 1e-300):.2e})"
    return err


def close_cols(got, ref, tol, what="", extra=None, apart=(), report=None):
    """close() for a [..][C] tensor: |got - ref| <= tol * max|ref| + extra[c].  `extra` is a per-channel absolute allowance
    (None: 0).  The channels listed in `apart` are compared on their own max|ref| and lend it to nobody else (a channel of zero
    variance has invstd = 1 / sqrt(eps), thirty times everyone else's).  `report(rel)` receives the largest error / scale
    BEFORE anything is asserted; the same number is returned."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got).all(), f"{what}: non-finite values in the result"
    C = ref.shape[-1]
    got, ref = got.reshape(-1, C), ref.reshape(-1, C)
    over = (got - ref).abs()
    if extra is not None:
        over = (over - extra.detach().cpu().double().reshape(1, C)).clamp_min(0.0)
    rest = torch.ones(C, dtype=torch.bool)
    groups = []
    for c in apart:
        rest[c] = False
        groups.append(torch.arange(C) == c)
    groups.append(rest)
    worst, fails = 0.0, []
    for sel in groups:
        if not sel.any() or not ref.numel():
            continue
        scale, err = ref[:, sel].abs().max().item(), over[:, sel].max().item()
        worst = max(worst, err / scale if scale > 0 else (0.0 if err == 0 else INF))
        if not err <= tol * scale:
            fails.append(f"max err {err:.3e} > {tol:.3e} * {scale:.3e} (rel {err / max(scale, 1e-300):.2e})")
    if report is not None:
        report(worst)
    assert not fails, f"{what}: " + "; ".join(fails)
    return worst


def same_outside(after, before, sl, what=""):
    """Channels outside the written slice `sl` (last axis) keep their exact prior bits."""
    keep = torch.ones(before.shape[-1], dtype=torch.bool)
    keep[sl] = False
    a = after[..., keep].contiguous()
    b = before[..., keep].contiguous()
    assert torch.equal(_bits(a), _bits(b)), f"{what}: channels outside the slice changed"


# ------------------------------------------------------------------------------------------------ references (float64)
def sigmoid(v):
    return 1.0 / (1.0 + torch.exp(-v))


def seg_plan(cus, rows, C, vec, wide8=False, nout=1):
    """seg_plan<NOUT> (csrc/sg_reduce.h) for one segment of `rows` rows and C channels: V, TX, TY, gx, S, part_bytes.
    wide8: the reduced tensor is bf16 - a lane takes 8 channels when C % 8 == 0 and NOUT <= 2.
    Held to the engine's own answer (sg_seg_plan) by tests/_bn_cases.py: checked_seg_plan before the column-sum launches, and
    test_plan_queries_equal_the_mirrors over every shape of its tables."""
    V = 4 if (vec and C % 4 == 0) else 1
    if V == 4 and wide8 and C % 8 == 0 and nout <= 2:
        V = 8
    chunks = C // V
    tx = 1
    while tx < chunks and tx < 16:
        tx <<= 1
    ty = 256 // tx
    gx = -(-chunks // tx)
    S = min(-(-4 * cus // gx), -(-rows // (ty * 4)))
    if rows <= ty * 16:
        S = 1
    S = max(1, min(S, 1024))
    return dict(V=V, TX=tx, TY=ty, gx=gx, S=S, part_bytes=S * nout * C * 4)


def seg_plan_s(cus, rows, C, vec, wide8=False, nout=1):
    """The row split S of seg_plan<NOUT> (csrc/sg_reduce.h) for one segment of `rows` rows and C channels."""
    return seg_plan(cus, rows, C, vec, wide8, nout)["S"]


def regime(S):
    return "one" if S == 1 else ("few" if S < 32 else "many")


def short_last_slab(rows, S):
    """The S row slabs of seg_reduce_kernel are ceil(rows / S) long: is the last one shorter?"""
    return S > 1 and -(-rows // S) * S != rows


def bn_cols_grid(cus, rows, cv, unroll):
    """bn_cols_grid (csrc/norm.hip) for cv chunks per row: (prow, b0, k) = rows per period, blocks per period (grid.x), groups of
    `unroll` periods walked in parallel (grid.y); None where the flat kernels take the launch.  Held to the engine's plan
    (sg_bn_plan: prow, gx, gy) by tests/_bn_cases.checked_plan before every BatchNormalization launch."""
    g = math.gcd(256, cv)
    b0 = cv // g
    if b0 > 16384:
        return None
    prow = 256 // g
    k = min(-(-8 * cus // b0), -(-rows // (unroll * prow)), 65535)
    return prow, b0, max(k, 1)


def pool_geom(H, k, s, same):
    """(Ho, pad_before) of MaxPooling2D: TF 'same' / 'valid'."""
    if same:
        Ho = -(-H // s)
        return Ho, max((Ho - 1) * s + k - H, 0) // 2
    return (H - k) // s + 1, 0


def _pool_slices(a, b, s, Ho, Wo):
    return slice(a, a + (Ho - 1) * s + 1, s), slice(b, b + (Wo - 1) * s + 1, s)


def maxpool_ref(x, k, s, pt, pl, Ho, Wo):
    """Window max with -inf padding and the cell (a * k + b, scan order) of the FIRST maximum (strict '>')."""
    N, H, W, C = x.shape
    Hp, Wp = max((Ho - 1) * s + k, pt + H), max((Wo - 1) * s + k, pl + W)
    xp = torch.full((N, Hp, Wp, C), -INF, dtype=x.dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    inside = torch.zeros(Hp, Wp, dtype=torch.bool)
    inside[pt:pt + H, pl:pl + W] = True
    best = torch.full((N, Ho, Wo, C), -INF, dtype=x.dtype)
    idx = torch.full((N, Ho, Wo, C), 255, dtype=torch.int64)
    for a in range(k):
        for b in range(k):
            sa, sb = _pool_slices(a, b, s, Ho, Wo)
            v = xp[:, sa, sb]
            take = inside[sa, sb][None, :, :, None] & ((v > best) | (idx == 255))
            best = torch.where(take, v, best)
            idx = torch.where(take, torch.full_like(idx, a * k + b), idx)
    return best, idx.to(torch.uint8)


def maxpool_bwd_ref(dy, idx, k, s, pt, pl, H, W):
    """dy routed to the recorded cell of every window, summed per input element."""
    N, Ho, Wo, C = dy.shape
    Hp, Wp = max((Ho - 1) * s + k, pt + H), max((Wo - 1) * s + k, pl + W)
    dxp = torch.zeros((N, Hp, Wp, C), dtype=dy.dtype)
    for a in range(k):
        for b in range(k):
            sa, sb = _pool_slices(a, b, s, Ho, Wo)
            dxp[:, sa, sb] += dy * (idx == a * k + b)
    return dxp[:, pt:pt + H, pl:pl + W].contiguous()


def avgpool_ref(x, kh, kw):
    N, H, W, C = x.shape
    Ho, Wo = H // kh, W // kw
    return x[:, :Ho * kh, :Wo * kw].reshape(N, Ho, kh, Wo, kw, C).mean(dim=(2, 4))


def avgpool_bwd_ref(dy, H, W, kh, kw):
    N, Ho, Wo, C = dy.shape
    dx = torch.zeros((N, H, W, C), dtype=dy.dtype)
    dx[:, :Ho * kh, :Wo * kw] = dy.repeat_interleave(kh, 1).repeat_interleave(kw, 2) / (kh * kw)
    return dx


def upsample_ref(x, sh, sw):
    return x.repeat_interleave(sh, 1).repeat_interleave(sw, 2)


def upsample_bwd_ref(dy, sh, sw):
    N, OH, OW, C = dy.shape
    return dy.reshape(N, OH // sh, sh, OW // sw, sw, C).sum(dim=(2, 4))


K_EPS = 1e-7   # tf.keras.backend.epsilon()


def loss_coeffs(kind, yt):
    y = yt[:, :2]
    if kind == 0:
        return y
    if kind == 1:
        return 0.5 * y
    return torch.tensor([0.35, 0.65], dtype=yt.dtype) * yt[:, 2:4] * y


def loss_ref(kind, p, yt):
    a = loss_coeffs(kind, yt)
    f = torch.ones_like(p) if kind == 0 else (1 - p) ** 2
    return -(a * f * torch.log(p + K_EPS)).sum() / p.shape[0]


def loss_bwd_ref(kind, p, yt, scale):
    a = loss_coeffs(kind, yt)
    if kind == 0:
        g = 1 / (p + K_EPS)
    else:
        g = -2 * (1 - p) * torch.log(p + K_EPS) + (1 - p) ** 2 / (p + K_EPS)
    return -(scale / p.shape[0]) * a * g


def confusion_ref(p, yt):
    """{TP, TN, FP, FN}; argmax ties go to class 0 on both sides."""
    pred, truth = p[:, 1] > p[:, 0], yt[:, 1] > yt[:, 0]
    return torch.tensor([(pred & truth).sum(), (~pred & ~truth).sum(), (pred & ~truth).sum(), (~pred & truth).sum()],
                        dtype=torch.int64)


def adam_ref(w, m, v, g, lr_t, b1, b2, eps, gs):
    g = g * gs
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return w - lr_t * m / (torch.sqrt(v) + eps), m, v


# ------------------------------------------------------------------------------ BatchNormalization / column sums (float64)
def ulp32(v):
    """The spacing of fp32 numbers at |v| (float64 in, float64 out)."""
    a = v.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def bn_stats_ref(x):
    """(mean, biased variance) of x[rows][C] per channel."""
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def bn_fwd_ref(x, gamma, beta, mm, mv, momentum, eps, relu, unbiased):
    """Training forward: y, mean, invstd, new moving mean, new moving variance (Keras: the moving variance takes the batch
    variance, n / (n - 1) times it with `unbiased` and more than one row)."""
    n = x.shape[0]
    mean, var = bn_stats_ref(x)
    invstd = 1.0 / torch.sqrt(var + eps)
    y = gamma * ((x - mean) * invstd) + beta
    var_u = var * (n / (n - 1.0)) if (unbiased and n > 1) else var
    return (torch.relu(y) if relu else y), mean, invstd, mm * momentum + mean * (1 - momentum), mv * momentum + var_u * (1 - momentum)


def bn_apply_ref(x, gamma, beta, mean, invstd, relu):
    y = gamma * ((x - mean) * invstd) + beta
    return torch.relu(y) if relu else y


def bn_bwd_ref(x, dy, gamma, mean, invstd, mask=None, dgamma=None, dbeta=None):
    """dx, dgamma, dbeta of the training forward from the saved mean / invstd; mask: the fused ReLU's [y > 0].  With dgamma and
    dbeta given, dx is formed from them (the apply pass on its own)."""
    n = x.shape[0]
    g = dy if mask is None else dy * mask
    xhat = (x - mean) * invstd
    if dgamma is None:
        dgamma, dbeta = (g * xhat).sum(0), g.sum(0)
    return gamma * invstd * (g - dbeta / n - xhat * dgamma / n), dgamma, dbeta


def add2_bn_ref(a, b, pa, pb, relu, infer, eps, a_relu, b_relu):
    """relu?(f(a) + f(b)); p = (mean, invstd or moving variance, gamma, beta) or None (identity, and no operand ReLU)."""
    def f(t, p, r):
        if p is None:
            return t
        mean, s, gamma, beta = p
        u = gamma * ((t - mean) * (1.0 / torch.sqrt(s + eps) if infer else s)) + beta
        return torch.relu(u) if r else u
    y = f(a, pa, a_relu) + f(b, pb, b_relu)
    return torch.relu(y) if relu else y


def colsum_ref(dy):
    return dy.sum(0)


def tile_stats_ref(x, bm=128):
    """[tiles][2][C]: per tile of bm rows (the last one ragged) the sum and the sum of squares about the tile's own mean."""
    rows, C = x.shape
    out = []
    for r0 in range(0, rows, bm):
        t = x[r0:r0 + bm]
        out.append(torch.stack([t.sum(0), ((t - t.mean(0)) ** 2).sum(0)]))
    return torch.stack(out)


# ------------------------------------------------------------------------------------ depthwise convolution (float64), ld views
def dw_geom(H, W, KH, KW, s, d, same):
    """(Ho, Wo, pad_t, pad_b, pad_l, pad_r) of a TF 'same' / 'valid' convolution with a dilated KH x KW window."""
    def one(n, k):
        eff = (k - 1) * d + 1
        if not same:
            return (n - eff) // s + 1, 0, 0
        o = -(-n // s)
        total = max((o - 1) * s + eff - n, 0)
        return o, total // 2, total - total // 2
    Ho, pt, pb = one(H, KH)
    Wo, pl, pr = one(W, KW)
    return Ho, Wo, pt, pb, pl, pr


def dw_input_ref(x, pre_relu=False, bn=None):
    """What the window multiplies: relu?(x), or z = ((x - mean) * invstd) * gamma + beta [ReLU] with bn = (mean, invstd, gamma,
    beta, relu).  The zero padding comes AFTER this (BN(0) != 0)."""
    if bn is not None:
        mean, invstd, gamma, beta, relu = bn
        z = ((x - mean) * invstd) * gamma + beta
        return torch.relu(z) if relu else z
    return torch.relu(x) if pre_relu else x


def dw_conv_ref(x, w, geom, s, d, pre_relu=False, bn=None):
    """y[N][Ho][Wo][C] of the depthwise convolution of x[N][H][W][C] with w[KH][KW][C]: F.conv2d(groups = C) on the explicitly
    padded tensor.  geom: dw_geom()."""
    import torch.nn.functional as F
    Ho, Wo, pt, pb, pl, pr = geom
    C = x.shape[-1]
    zp = F.pad(dw_input_ref(x, pre_relu, bn).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(zp, w.permute(2, 0, 1).unsqueeze(1), stride=s, dilation=d, groups=C).permute(0, 2, 3, 1)
    assert y.shape[1:3] == (Ho, Wo), (tuple(y.shape), Ho, Wo)
    return y


def dw_grads_ref(x, w, dy, geom, s, d, pre_relu=False, bn=None, want="dx"):
    """dx or dw of dw_conv_ref by autograd (dx never has a BatchNormalization in front)."""
    x = x.detach().clone().requires_grad_(want == "dx")
    w = w.detach().clone().requires_grad_(want == "dw")
    y = dw_conv_ref(x, w, geom, s, d, pre_relu, bn)
    (g,) = torch.autograd.grad(y, x if want == "dx" else w, dy)
    return g.detach()


def bn_sums_ref(g, bsx, mean, invstd, gamma, beta, relu):
    """(dgamma, dbeta) = (sum g * xhat, sum g) per channel, g masked by z > 0 under a fused ReLU; all [..][C] float64."""
    C = g.shape[-1]
    xhat = ((bsx - mean) * invstd).reshape(-1, C)
    g = g.reshape(-1, C)
    if relu:
        g = g * ((xhat * gamma + beta) > 0)
    return (g * xhat).sum(0), g.sum(0)


def widen(t, ld, mid=0):
    """t[..][C] as the columns [mid, mid + C) of a [pixels][ld] tensor whose other bytes are 0xFF (NaN)."""
    C = t.shape[-1]
    t = t.detach().cpu().reshape(-1, C)
    wide = torch.full((t.shape[0] * ld * t.element_size(),), 0xFF, dtype=torch.uint8).view(t.dtype).reshape(t.shape[0], ld)
    wide[:, mid:mid + C] = t
    return wide


def gaps_keep_prefill(wide, C, mid, what="", fill=0xFF):
    """The columns outside [mid, mid + C) of a strided output keep every prefill byte."""
    keep = torch.ones(wide.shape[-1], dtype=torch.bool)
    keep[mid:mid + C] = False
    bad = _bits(wide[:, keep]) != fill
    assert not bad.any(), f"{what}: {int(bad.sum())} bytes of the gap columns of a strided output were overwritten"


def untouched(o, what=""):
    """A refused launch: every byte of the output arena keeps its prefill (bands included)."""
    o.fetch()
    assert torch.equal(o.after, o.before), f"{what}: a refused launch wrote into an output {o.shape}"
