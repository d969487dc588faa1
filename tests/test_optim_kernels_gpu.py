"""sg_optim_grad_norms and sg_optim_step (csrc/optim.hip) through the C ABI against the float64 restatement of the update rules
(tests/_optim_ref.py).

Every operand is a tests/_guarded.py arena between NaN guard bands; the padding elements between two parameters of an arena hold
NaN as well, in every arena, so a kernel that reads padding poisons a result and one that writes it changes its bits.  Parameter
sizes 1, 3, 4, 5, L, L + 1, 2L + 3 (L = the chunk bound: tail-only chunks, one vector item, vector items with a 1- and a 3-element
tail, full chunks, a parameter of two and of three chunks), and one table of more chunks than the launch's grid cap (8192
workgroups) so that the chunk loop takes a second trip.  The step is held to the tolerance test_adam holds sg_adam_step to:
max|got - ref| <= 2e-5 * max|ref| per arena (close(), tol(F32) of tests/test_bandwidth_variants_gpu.py).  The norms are
accumulated in fp64, so once rounded to fp32 they sit within 2 ulp of the float64 sum whatever the reduction's shape."""
import ctypes as C
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _optim_ref as R
from _guarded import Guarded, check_all, close, ulp32
from building_detection_amd import _lib, optimizers as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
SG_EINVAL = -1
TOL_F32 = 2e-5          # tol(F32) of tests/test_bandwidth_variants_gpu.py: what test_adam uses
L = O.CHUNK
GRID_CAP = 8192         # OPT_GRID_CAP of csrc/optim.hip
SIZES = [1, 3, 4, 5, L, L + 1, 2 * L + 3]
KINDS = ["bias", "gamma", "kernel", "beta", "depthwise_kernel", "bias", "kernel"]   # decayed: segments 2, 4, 6


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) % (2 ** 31))


def G(t, off=False, role="in"):
    return Guarded(t, DEV, off=off, role=role)


class Table:
    """A parameter list laid out like the trainable arena, its chunk table in host and (guarded) device memory."""

    def __init__(self, sizes, kinds):
        params, off = [], 0
        for i, (n, k) in enumerate(zip(sizes, kinds)):
            params.append(SimpleNamespace(name=f"p{i}/{k}", size=n, kind=k, trainable=True, offset=off))
            off += (n + 3) // 4 * 4
        self.n = off
        self.chunks, self.segs, _ = O.chunk_table(params)
        self.ref_segs = [(p.offset, p.size, p.kind in O.DEFAULT_DECAY_KINDS) for p in params]
        self.live = torch.zeros(off, dtype=torch.bool)
        for p in params:
            self.live[p.offset:p.offset + p.size] = True
        self.upload(self.chunks)

    def upload(self, chunks):
        self.host_chunks = np.ascontiguousarray(chunks)
        self.CH = G(torch.from_numpy(self.host_chunks.view(np.uint8).reshape(-1).copy()))
        self.SG = G(torch.from_numpy(self.segs.view(np.uint8).reshape(-1).copy()))
        self.c = _lib.OptimTable(self.host_chunks.ctypes.data, self.segs.ctypes.data, self.CH.ptr(), self.SG.ptr(),
                                 len(self.host_chunks), len(self.segs), self.n)

    def arena(self, g, lo=-1.0, hi=1.0, zero=False):
        """fp32 values on the parameters' elements, NaN on the padding."""
        t = torch.zeros(self.n) if zero else (torch.rand(self.n, generator=g) * (hi - lo) + lo).float()
        t[~self.live] = float("nan")
        return t

    def guards(self):
        return [self.CH, self.SG]


@pytest.fixture(scope="module")
def table():
    return Table(SIZES, KINDS)


@pytest.fixture(scope="module")
def long_table():
    sizes = [(1, 3, 4, 5, 7, 8)[i % 6] for i in range(GRID_CAP + 101)]   # one chunk each: more chunks than workgroups
    return Table(sizes, [("kernel", "bias")[i % 2] for i in range(len(sizes))])


def call(engine, name, *args):
    return getattr(engine.lib, name)(engine.h, engine.stream, *args)


def err(engine):
    return engine.lib.sg_last_error().decode("utf-8", "replace")


def padding_kept(tab, got, what):
    assert torch.isnan(got[~tab.live]).all(), f"{what}: a padding element was written"


# ================================================================================================ norms
def _norms(engine, tab, g, gs):
    Gr = G(g)
    ws = Guarded.ws(engine.lib.sg_optim_norms_ws_bytes(len(tab.chunks)), DEV)
    N = Guarded.out((1 + len(tab.segs),), torch.float64, DEV)
    rc = call(engine, "sg_optim_grad_norms", C.byref(tab.c), Gr.ptr(), gs, N.ptr(), ws.ptr(), ws.nb)
    assert rc == 0, err(engine)
    check_all([Gr, ws, N] + tab.guards(), "grad norms")
    return N.read()


@pytest.mark.parametrize("which", ["sizes", "beyond_grid_cap"])
@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_grad_norms(engine, table, long_table, which, gs):
    tab = table if which == "sizes" else long_table
    assert which == "sizes" or len(tab.chunks) > GRID_CAP
    g = tab.arena(gen(f"norms{which}"))
    got = _norms(engine, tab, g, gs)
    total, per = R.norms_ref(tab.ref_segs, g, gs)
    ref = torch.cat([total.reshape(1), per])
    assert torch.isfinite(got).all(), "a padding NaN reached a sum"
    d = (got.float().double() - ref.float().double()).abs()
    print(f"grad norms {which} gs={gs}: worst distance {float((d / ulp32(ref)).max()):.2f} ulp32")
    assert (d <= 2 * ulp32(ref)).all(), (got, ref)
    again = _norms(engine, tab, g, gs)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64)), "two launches, two results"


def test_grad_norms_short_workspace_is_refused(engine, table):
    Gr = G(table.arena(gen("short")))
    need = engine.lib.sg_optim_norms_ws_bytes(len(table.chunks))
    assert need == 8 * len(table.chunks)
    ws = Guarded.ws(need - 8, DEV)
    N = Guarded.out((1 + len(table.segs),), torch.float64, DEV)
    assert call(engine, "sg_optim_grad_norms", C.byref(table.c), Gr.ptr(), 1.0, N.ptr(), ws.ptr(), ws.nb) == -2   # SG_EWORKSPACE
    check_all([Gr, ws, N], "short workspace")
    assert torch.isnan(N.read()).all()


# ================================================================================================ step
KIND_CASES = {
    "adam": dict(kind="adam"),
    "amsgrad": dict(kind="adam", amsgrad=True),
    "sgd": dict(kind="sgd"),
    "sgd_momentum": dict(kind="sgd", momentum=0.9),
    "sgd_nesterov": dict(kind="sgd", momentum=0.9, nesterov=True),
}
C_ON, C_OFF = 0.04, 1e4        # below every parameter's gradient norm (|g| >= 0.1 on each element, times grad_scale 0.5) / above all
OPTION_CASES = {
    "none": dict(),
    "decay": dict(weight_decay=0.05),
    "clipvalue_on": dict(clip="value", clip_c=0.2),
    "clipvalue_off": dict(clip="value", clip_c=C_OFF),
    "clipnorm_on": dict(clip="norm", clip_c=C_ON),
    "clipnorm_off": dict(clip="norm", clip_c=C_OFF),
    "global_on": dict(clip="global", clip_c=C_ON),
    "global_off": dict(clip="global", clip_c=C_OFF),
    "ema": dict(ema_momentum=0.9),
    "all": dict(weight_decay=0.05, clip="global", clip_c=C_ON, ema_momentum=0.9),
}
CLIP_MODE = {None: _lib.SG_OPT_CLIP_NONE, "value": _lib.SG_OPT_CLIP_VALUE, "norm": _lib.SG_OPT_CLIP_NORM,
             "global": _lib.SG_OPT_CLIP_GLOBAL}
LRS = (1e-3, 3e-3, 5e-4)       # a different learning rate at each of the three steps
F = lambda v: float(torch.tensor(v, dtype=torch.float32))   # the fp32 value the kernel is handed


def _desc(cfg):
    flags = ((_lib.SG_OPT_AMSGRAD if cfg.amsgrad else 0) | (_lib.SG_OPT_NESTEROV if cfg.nesterov else 0) |
             (_lib.SG_OPT_EMA if cfg.ema_momentum is not None else 0))
    return _lib.OptimDesc(_lib.SG_OPT_ADAM if cfg.kind == "adam" else _lib.SG_OPT_SGD, flags, CLIP_MODE[cfg.clip], cfg.beta_1,
                          cfg.beta_2, cfg.epsilon, cfg.momentum, cfg.weight_decay, cfg.clip_c,
                          0.0 if cfg.ema_momentum is None else cfg.ema_momentum, cfg.grad_scale)


def _f32cfg(cfg):
    """The same configuration with every constant rounded to fp32, as the descriptor carries it."""
    return R.Cfg(cfg.kind, F(cfg.beta_1), F(cfg.beta_2), F(cfg.epsilon), cfg.amsgrad, F(cfg.momentum), cfg.nesterov,
                 F(cfg.weight_decay), cfg.clip, F(cfg.clip_c), None if cfg.ema_momentum is None else F(cfg.ema_momentum),
                 F(cfg.grad_scale))


def _inputs(tab, tag):
    g = gen(tag)
    w = tab.arena(g)
    grads = []
    for _ in LRS:
        gr = tab.arena(g)
        gr = torch.where(gr.abs() < 0.1, torch.where(gr >= 0, 0.1, -0.1).float(), gr)   # every parameter's norm is >= 0.1
        grads.append(gr)
    m = tab.arena(g, -0.1, 0.1)
    v = tab.arena(g, 1e-4, 1e-2)
    vhat = tab.arena(g, 1e-4, 1e-2)     # above v on some elements and below it on others
    return w, grads, m, v, vhat


def _run_steps(engine, tab, cfg, tag, lr_form):
    """Three steps through the ABI from the state of _inputs; lr_form "args" | "dev".  Returns the final arenas (host)."""
    w, grads, m, v, vhat = _inputs(tab, tag)
    adam, mom = cfg.kind == "adam", cfg.kind == "sgd" and cfg.momentum != 0.0
    by_norm = cfg.clip in ("norm", "global")
    Wt = G(w, role="out")
    M = G(m, role="out") if adam or mom else None
    V = G(v, role="out") if adam else None
    H = G(vhat, role="out") if cfg.amsgrad else None
    E = G(w, role="out") if cfg.ema_momentum is not None else None     # the average starts as a copy of the weights
    N = Guarded.out((1 + len(tab.segs),), torch.float64, DEV) if by_norm else None
    ws = Guarded.ws(engine.lib.sg_optim_norms_ws_bytes(len(tab.chunks)), DEV) if by_norm else None
    d = _desc(cfg)
    ptr = lambda o: None if o is None else o.ptr()
    for t, (lr, gr) in enumerate(zip(LRS, grads), 1):
        Gr = G(gr)
        lr_t = R.adam_lr_t(lr, cfg.beta_1, cfg.beta_2, t) if adam else lr
        if by_norm:
            rc = call(engine, "sg_optim_grad_norms", C.byref(tab.c), Gr.ptr(), cfg.grad_scale, N.ptr(), ws.ptr(), ws.nb)
            assert rc == 0, err(engine)
        LR = G(torch.tensor([lr_t, lr, float("nan"), float("nan")])) if lr_form == "dev" else None
        args = (float("nan"), float("nan")) if lr_form == "dev" else (lr_t, lr)
        rc = call(engine, "sg_optim_step", C.byref(d), C.byref(tab.c), Wt.ptr(), Gr.ptr(), ptr(M), ptr(V), ptr(H), ptr(E), ptr(N),
                  *args, ptr(LR))
        assert rc == 0, err(engine)
        for o in (Wt, M, V, H, E, N, ws, Gr, LR):
            if o is not None:
                o.after = None
                o.fetch().check(f"{tag} step {t}")
    check_all(tab.guards(), tag)
    out = dict(w=Wt.read(), m=None if M is None else M.read(), v=None if V is None else V.read(),
               vhat=None if H is None else H.read(), ema=None if E is None else E.read())
    for k, a in out.items():
        if a is not None:
            padding_kept(tab, a, f"{tag} {k}")
    return out


def _ref_steps(tab, cfg, tag):
    w, grads, m, v, vhat = _inputs(tab, tag)
    c = _f32cfg(cfg)
    st = dict(m=m.double(), v=v.double(), vhat=vhat.double(), ema=w.double())
    wd = w.double()
    for t, (lr, gr) in enumerate(zip(LRS, grads), 1):
        lr_t = R.adam_lr_t(lr, cfg.beta_1, cfg.beta_2, t)
        wd, st = R.step_ref(c, tab.ref_segs, wd, gr, st, F(lr), F(lr_t))
    return dict(st, w=wd), grads


def _clip_is(tab, cfg, grads, on):
    """The case is what its name says: every norm the clip mode looks at is above / below the constant at every step."""
    for gr in grads:
        total, per = R.norms_ref(tab.ref_segs, gr, cfg.grad_scale)
        if cfg.clip == "value":
            a = (gr[tab.live].abs() * cfg.grad_scale)
            assert (a.max() > cfg.clip_c) if on else (a.max() < cfg.clip_c)
            continue
        nrm = (per if cfg.clip == "norm" else total.reshape(1)).sqrt()
        assert (nrm > cfg.clip_c).all() if on else (nrm < cfg.clip_c).all()


@pytest.mark.parametrize("options", list(OPTION_CASES))
@pytest.mark.parametrize("kind", list(KIND_CASES))
def test_step(engine, table, kind, options):
    cfg = R.Cfg(grad_scale=0.5, **KIND_CASES[kind], **OPTION_CASES[options])
    tag = f"step-{kind}-{options}"
    ref, grads = _ref_steps(table, cfg, tag)
    if cfg.clip is not None:
        _clip_is(table, cfg, grads, options.endswith("_on") or options == "all")
    a = _run_steps(engine, table, cfg, tag, "args")
    b = _run_steps(engine, table, cfg, tag, "dev")
    for k in a:
        if a[k] is None:
            continue
        e = close(a[k][table.live], ref[k][table.live], TOL_F32, f"{tag} {k}")
        print(f"{tag} {k}: max err {e:.3e}")
        assert torch.equal(a[k][table.live].view(torch.int32), b[k][table.live].view(torch.int32)), \
            f"{tag} {k}: learning rates from device memory give other bits than the arguments"


def test_step_beyond_the_grid_cap(engine, long_table):
    cfg = R.Cfg(grad_scale=0.5, amsgrad=True, weight_decay=0.05, clip="norm", clip_c=0.3, ema_momentum=0.9)
    tag = "step-long"
    ref, _ = _ref_steps(long_table, cfg, tag)
    a = _run_steps(engine, long_table, cfg, tag, "args")
    b = _run_steps(engine, long_table, cfg, tag, "dev")
    for k in a:
        close(a[k][long_table.live], ref[k][long_table.live], TOL_F32, f"{tag} {k}")
        assert torch.equal(a[k][long_table.live].view(torch.int32), b[k][long_table.live].view(torch.int32))


@pytest.mark.parametrize("kind", list(KIND_CASES))
def test_undecayed_parameters_have_the_bits_of_a_run_without_decay(engine, table, kind):
    tag = f"decay-bits-{kind}"
    with_wd = _run_steps(engine, table, R.Cfg(grad_scale=0.5, weight_decay=0.05, **KIND_CASES[kind]), tag, "args")
    without = _run_steps(engine, table, R.Cfg(grad_scale=0.5, **KIND_CASES[kind]), tag, "args")
    changed = 0
    for o, n, decayed in table.ref_segs:
        for k in with_wd:
            if with_wd[k] is None:
                continue
            same = torch.equal(with_wd[k][o:o + n].view(torch.int32), without[k][o:o + n].view(torch.int32))
            if not decayed:
                assert same, f"{tag}: {k} of an undecayed parameter at {o} differs"
            elif k == "w":
                changed += not same
    assert changed == sum(1 for s in table.ref_segs if s[2]), "the decay reached every decayed parameter"


# ================================================================================================ refusals
def _all_operands(tab, off_which=None):
    g = gen("refuse")
    ops = [G(tab.arena(g), off=(i == off_which), role="in") for i in range(6)]     # w, g, m, v, vhat, ema: must stay as they are
    N = G(torch.ones(1 + len(tab.segs), dtype=torch.float64))
    return ops, N


FULL = dict(kind=_lib.SG_OPT_ADAM, flags=_lib.SG_OPT_AMSGRAD | _lib.SG_OPT_EMA, clip=_lib.SG_OPT_CLIP_GLOBAL)


def _full_desc(**kw):
    f = dict(FULL, **kw)
    return _lib.OptimDesc(f["kind"], f["flags"], f["clip"], 0.9, 0.999, 1e-7, f.get("momentum", 0.0), f.get("weight_decay", 0.01),
                          f.get("clip_c", 1.0), 0.99, 1.0)


def _refused(engine, tab, d, ops, N, what):
    rc = call(engine, "sg_optim_step", C.byref(d), C.byref(tab.c), *[o.ptr() for o in ops], N.ptr(), 1e-3, 1e-3, None)
    assert rc == SG_EINVAL, f"{what}: rc={rc}"
    check_all(ops + [N] + tab.guards(), what)


def test_unaligned_arenas_are_refused(engine, table):
    for which in range(6):
        ops, N = _all_operands(table, which)
        _refused(engine, table, _full_desc(), ops, N, f"arena {which} one element off")
    ops, N = _all_operands(table)
    Goff = G(table.arena(gen("goff")), off=True)
    ws = Guarded.ws(engine.lib.sg_optim_norms_ws_bytes(len(table.chunks)), DEV)
    No = Guarded.out((1 + len(table.segs),), torch.float64, DEV)
    assert call(engine, "sg_optim_grad_norms", C.byref(table.c), Goff.ptr(), 1.0, No.ptr(), ws.ptr(), ws.nb) == SG_EINVAL
    check_all([Goff, ws, No], "norms of an unaligned arena")
    assert torch.isnan(No.read()).all()


def test_malformed_tables_are_refused(engine):
    def broken(edit):
        tab = Table(SIZES, KINDS)
        chunks = tab.chunks.copy()
        edit(chunks, tab)
        tab.upload(chunks)
        return tab

    def off_boundary(ch, tab):
        ch["start"][4] += 1               # a chunk that starts off a 16-byte boundary
        ch["length"][4] -= 1

    def overlapping(ch, tab):
        ch["start"][6] -= 4

    def beyond(ch, tab):
        ch["length"][-1] += 8             # past the arena's end

    def empty(ch, tab):
        ch["length"][2] = 0

    def wrong_segment(ch, tab):
        ch["segment"][5] = 6              # not the segment whose chunk range holds it

    def bad_range(ch, tab):
        tab.segs["chunk_end"][3] += 1     # the segments no longer tile the table

    for edit in (off_boundary, overlapping, beyond, empty, wrong_segment, bad_range):
        tab = broken(edit)
        ops, N = _all_operands(tab)
        _refused(engine, tab, _full_desc(), ops, N, edit.__name__)
        ws = Guarded.ws(engine.lib.sg_optim_norms_ws_bytes(len(tab.chunks)), DEV)
        No = Guarded.out((1 + len(tab.segs),), torch.float64, DEV)
        rc = call(engine, "sg_optim_grad_norms", C.byref(tab.c), ops[1].ptr(), 1.0, No.ptr(), ws.ptr(), ws.nb)
        assert rc == SG_EINVAL, edit.__name__
        check_all([ws, No, ops[1]], edit.__name__)


def test_descriptors_outside_the_domain_are_refused(engine, table):
    ops, N = _all_operands(table)
    for what, d in (("kind", _full_desc(kind=2)), ("flags", _full_desc(flags=8)), ("clip", _full_desc(clip=4)),
                    ("amsgrad on SGD", _full_desc(kind=_lib.SG_OPT_SGD)), ("nesterov on Adam", _full_desc(flags=_lib.SG_OPT_NESTEROV)),
                    ("negative decay", _full_desc(weight_decay=-0.1)), ("NaN clip", _full_desc(clip_c=float("nan"))),
                    ("zero clip", _full_desc(clip_c=0.0)), ("infinite momentum", _full_desc(momentum=float("inf")))):
        _refused(engine, table, d, ops, N, what)
    d = _full_desc()
    for missing in (2, 3, 4, 5):      # m, v, vhat, ema: each is needed by this configuration
        ptrs = [None if i == missing else o.ptr() for i, o in enumerate(ops)]
        assert call(engine, "sg_optim_step", C.byref(d), C.byref(table.c), *ptrs, N.ptr(), 1e-3, 1e-3, None) == SG_EINVAL
    assert call(engine, "sg_optim_step", C.byref(d), C.byref(table.c), *[o.ptr() for o in ops], None, 1e-3, 1e-3, None) == SG_EINVAL
    check_all(ops + [N], "missing arenas")
