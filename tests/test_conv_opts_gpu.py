"""The convolution entry points with optional operands (include/segengine.h: sg_conv_opts, the trailing operands of
sg_dwconv2d_*, sg_conv2d_caps), through the raw C ABI.

What is held here is the boundary, not the arithmetic (test_ops_gpu.py has that): the ways to spell "no option" are one launch, a
combination no kernel takes is refused with its documented code before anything is written, and sg_conv_caps.thin is the rule the
Python host used to restate.

Two facts of the library this file has to respect, both older than sg_conv_opts and unchanged by it:
  - the forward's workspace selects its arithmetic on fp32 storage: with one the six-pass bf16 kernels run, without one the fp32
    MFMA kernel.  NULL opts, zeroed opts and opts carrying only `ws` are therefore compared on operands for which both are exact
    (small integers: every product and every partial sum is an integer below 2^24, and an integer below 2^8 is its own first bf16
    plane), so that any differing bit is an operand that went astray and not a rounding; on random operands NULL is compared with
    zeroed opts, and `ws` alone with the host's own call.
  - the input gradient and the filter gradient have no launch without a workspace (the transposed kernel / the split-K partials
    live there): NULL and zeroed opts both return SG_EWORKSPACE and write nothing, as their ws = NULL call always did.
"""
import ctypes as C
import itertools

import pytest
import torch

from oracle import tfops as T

pytestmark = pytest.mark.gpu

SG_EINVAL, SG_EWORKSPACE, SG_EUNSUPPORTED = -1, -2, -3
SENTINEL = 123.0
# the smallest geometry of test_ops_gpu.py's conv2d_dgrad(res=...) cases whose input gradient is known to take the slab kernels
# (test_dgrad_kernel_choice_does_not_depend_on_a_collected_gradient asserts kind 1 for it): 3x3, dilation 2, 64 -> 96
SLAB = dict(n=2, h=16, w=32, cin=64, cout=96, k=3, stride=1, dil=2)


def _lib():
    from building_detection_amd import _lib as L
    return L


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ints(gen, *shape, amp):
    return torch.randint(-amp, amp + 1, shape, generator=gen).float()


def _rnd(gen, *shape):
    return (torch.rand(*shape, generator=gen) * 2 - 1).float()


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device="cuda")


def _untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t == SENTINEL).all()) for t in tensors)


@pytest.fixture(scope="module")
def slab(engine):
    """The slab-family convolution: descriptor, integer-valued and random operands, a workspace that serves all three launches."""
    L = _lib()
    s = SLAB
    d = engine.conv_desc((s["n"], s["h"], s["w"], s["cin"]), s["cout"], s["k"], s["k"], s["stride"], s["dil"], "same")
    job, nbytes = L.PlanesJob(), C.c_size_t(0)
    L.check(engine.lib.sg_conv2d_planes_job(engine.h, L.SG_F32, C.byref(d), 1, C.byref(job), C.byref(nbytes)), "sg_conv2d_planes_job")
    assert int(job.kind) == 1, f"the input gradient of this geometry no longer takes the slab kernels (kind {job.kind})"
    g = torch.Generator().manual_seed(20261018)
    xs, ys, ws_ = (s["n"], s["h"], s["w"], s["cin"]), (s["n"], d.Ho, d.Wo, s["cout"]), (s["k"], s["k"], s["cin"], s["cout"])
    ops = {}
    for kind, mk in (("int", lambda *sh: _ints(g, *sh, amp=3)), ("rnd", lambda *sh: _rnd(g, *sh))):
        ops[kind] = dict(x=mk(*xs).cuda(), dy=mk(*ys).cuda(), w=mk(*ws_).cuda(), b=mk(s["cout"]).cuda(), bt=mk(s["cin"]).cuda())
    need = max(engine.lib.sg_conv2d_fwd_ws_bytes(C.byref(d)), engine.lib.sg_conv2d_dgrad_ws_bytes(C.byref(d)),
               engine.lib.sg_conv2d_wgrad_ws_bytes(engine.h, C.byref(d)))
    ws = torch.empty(int(need) + 256, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    return dict(d=d, ops=ops, ws=ws, xs=xs, ys=ys, wshape=ws_)


def _opts_forms(S):
    """NULL, zeroed, `ws` alone: (name, the pointer to pass, the object that keeps it alive)"""
    L = _lib()
    zero, only_ws = L.ConvOpts(), L.ConvOpts(S["ws"].data_ptr(), S["ws"].numel())
    return [("null", None, None), ("zeroed", C.byref(zero), zero), ("ws", C.byref(only_ws), only_ws)]


def _fwd(engine, S, o, opts):
    L = _lib()
    y = _sentinel(*S["ys"])
    rc = engine.lib.sg_conv2d_fwd(engine.h, engine.stream, L.SG_F32, C.byref(S["d"]), _p(o["x"]), _p(o["w"]), _p(o["b"]), _p(y),
                                  L.SG_EPI_BIAS, opts)
    return int(rc), y


def _dgrad(engine, S, o, opts, bias=None, flags=0):
    L = _lib()
    dx = _sentinel(*S["xs"])
    rc = engine.lib.sg_conv2d_dgrad(engine.h, engine.stream, L.SG_F32, C.byref(S["d"]), _p(o["dy"]), _p(o["w"]), _p(bias), _p(dx), flags,
                                    opts)
    return int(rc), dx


def _wgrad(engine, S, o, opts):
    L = _lib()
    dw, db = _sentinel(*S["wshape"]), _sentinel(S["d"].Cout)
    rc = engine.lib.sg_conv2d_wgrad(engine.h, engine.stream, L.SG_F32, C.byref(S["d"]), _p(o["x"]), _p(o["dy"]), _p(dw), _p(db), opts)
    return int(rc), dw, db


# ------------------------------------------------------------------------------------------- plain-launch equivalence
def test_forward_null_zeroed_and_ws_only_opts_are_one_launch(engine, slab):
    S = slab
    o = S["ops"]["int"]
    outs = {}
    for name, ptr, _keep in _opts_forms(S):
        rc, y = _fwd(engine, S, o, ptr)
        assert rc == 0, (name, rc)
        outs[name] = y
    want = T.conv2d(o["x"].cpu().double(), o["w"].cpu().double(), o["b"].cpu().double(), SLAB["stride"], SLAB["dil"], "same")
    assert torch.equal(outs["null"].cpu().double(), want), "the integer operands are not exact after all"
    assert torch.equal(outs["null"], outs["zeroed"]) and torch.equal(outs["null"], outs["ws"])
    # random operands: the two spellings of "no workspace" are one launch, and `ws` alone is the host's plain call
    o = S["ops"]["rnd"]
    (rn, yn), (rz, yz), (rw, yw) = (_fwd(engine, S, o, ptr) for _n, ptr, _k in _opts_forms(S))
    assert (rn, rz, rw) == (0, 0, 0)
    assert torch.equal(yn, yz)
    assert torch.equal(yw, engine.conv2d_fwd(o["x"], o["w"], o["b"], desc=S["d"]))


@pytest.mark.parametrize("kind", ["int", "rnd"])
def test_dgrad_and_wgrad_null_and_zeroed_opts_are_one_answer(engine, slab, kind):
    S = slab
    o = S["ops"][kind]
    forms = _opts_forms(S)
    for name, ptr, _keep in forms[:2]:   # no launch without a workspace: the same refusal, nothing written
        rc, dx = _dgrad(engine, S, o, ptr)
        assert rc == SG_EWORKSPACE and _untouched(dx), (name, rc)
        rc, dw, db = _wgrad(engine, S, o, ptr)
        assert rc == SG_EWORKSPACE and _untouched(dw, db), (name, rc)
    ptr = forms[2][1]
    rc, dx = _dgrad(engine, S, o, ptr)
    rc2, dx2 = _dgrad(engine, S, o, ptr)
    assert (rc, rc2) == (0, 0)
    assert torch.equal(dx, dx2) and torch.equal(dx, engine.conv2d_dgrad(o["dy"], o["w"], S["d"]))
    rc, dw, db = _wgrad(engine, S, o, ptr)
    assert rc == 0
    gw, gb = engine.conv2d_wgrad(o["x"], o["dy"], S["d"])
    assert torch.equal(dw, gw) and torch.equal(db, gb)
    if kind == "int":   # exact operands: the bits of the fp64 oracle
        xr = o["x"].cpu().double().requires_grad_()
        wr = o["w"].cpu().double().requires_grad_()
        T.conv2d(xr, wr, None, SLAB["stride"], SLAB["dil"], "same").backward(o["dy"].cpu().double())
        assert torch.equal(dx.cpu().double(), xr.grad) and torch.equal(dw.cpu().double(), wr.grad)


@pytest.fixture(scope="module")
def dw(engine):
    """Depthwise N = 1, 8 x 8 x 16, 3x3 stride 1, and the same with stride 2."""
    g = torch.Generator().manual_seed(816)
    n, h, w, c = 1, 8, 8, 16
    d = engine.conv_desc((n, h, w, c), c, 3, 3, 1, 1, "same")
    d2 = engine.conv_desc((n, h, w, c), c, 3, 3, 2, 1, "same")
    t = dict(x=_rnd(g, n, h, w, c).cuda(), dy=_rnd(g, n, h, w, c).cuda(), w=_rnd(g, 3, 3, c, 1).cuda(),
             dy2=_rnd(g, n, d2.Ho, d2.Wo, c).cuda())
    vec = {k: (_rnd(g, c) + (2.0 if k == "invstd" else 0.0)).cuda() for k in ("gamma", "beta", "mean", "invstd")}
    need = max(engine.lib.sg_dwconv2d_wgrad_ws_bytes(engine.h, C.byref(d)), engine.lib.sg_dwconv2d_dgrad_bnsums_ws_bytes(engine.h, C.byref(d)),
               engine.lib.sg_dwconv2d_dgrad_bnsums_ws_bytes(engine.h, C.byref(d2)))
    ws = torch.empty(int(need) + 256, dtype=torch.uint8, device="cuda")
    return dict(d=d, d2=d2, t=t, vec=vec, ws=ws, shape=(n, h, w, c))


@pytest.mark.parametrize("pre_relu", [0, 1])
def test_depthwise_trailing_nulls_are_the_plain_launch(engine, dw, pre_relu):
    L, t, d = _lib(), dw["t"], dw["d"]
    lib, dt = engine.lib, L.SG_F32
    y = _sentinel(*dw["shape"])
    assert lib.sg_dwconv2d_fwd(engine.h, engine.stream, dt, C.byref(d), _p(t["x"]), _p(t["w"]), _p(y), pre_relu, None) == 0
    assert torch.equal(y, engine.dwconv_fwd(t["x"], t["w"], pre_relu=bool(pre_relu), desc=d))
    xin = torch.relu(t["x"]) if pre_relu else t["x"]
    want = T.depthwise_conv2d(xin.cpu().double(), t["w"].cpu().double(), 1, "same")
    assert float((y.cpu().double() - want).abs().max()) <= 2e-5 * float(want.abs().max())
    dx = _sentinel(*dw["shape"])
    assert lib.sg_dwconv2d_dgrad(engine.h, engine.stream, dt, C.byref(d), _p(t["dy"]), _p(t["w"]), _p(t["x"]), _p(dx), pre_relu, None,
                                 None) == 0
    assert torch.equal(dx, engine.dwconv_dgrad(t["dy"], t["w"], d, x=t["x"], pre_relu=bool(pre_relu)))
    gw = _sentinel(3, 3, dw["shape"][3], 1)
    assert lib.sg_dwconv2d_wgrad(engine.h, engine.stream, dt, C.byref(d), _p(t["x"]), _p(t["dy"]), _p(gw), pre_relu, None, _p(dw["ws"]),
                                 dw["ws"].numel()) == 0
    assert torch.equal(gw, engine.dwconv_wgrad(t["x"], t["dy"], d, pre_relu=bool(pre_relu)))
    assert not _untouched(y) and not _untouched(dx) and not _untouched(gw)


# ------------------------------------------------------------------------------------------------ refused combinations
def _bn_in(L, vec, infer=0):
    return L.BnIn(_p(vec["mean"]), _p(vec["invstd"]), _p(vec["gamma"]), _p(vec["beta"]), 1, infer, 1e-3)


def test_conv_opts_refuse_what_no_kernel_takes(engine, slab):
    """Every refusal returns before any launch; the output keeps its sentinel."""
    L, S = _lib(), slab
    o = S["ops"]["rnd"]
    d = S["d"]
    ws, wsn = S["ws"].data_ptr(), S["ws"].numel()
    g = torch.Generator().manual_seed(3)
    cin, cout = d.Cin, d.Cout
    bn_vec = {k: (_rnd(g, cin) + (2.0 if k == "invstd" else 0.0)).cuda() for k in ("gamma", "beta", "mean", "invstd")}
    bq = _bn_in(L, bn_vec)
    rows = d.N * d.Ho * d.Wo
    bx, bdz = _rnd(g, *S["ys"]).cuda(), _sentinel(*S["ys"])
    cv = {k: (_rnd(g, cout) + 2.0).cuda() for k in ("mean", "invstd", "gamma", "beta", "dgamma", "dbeta")}
    bnb = L.BnBwdIn(_p(bx), _p(cv["mean"]), _p(cv["invstd"]), _p(cv["gamma"]), _p(cv["beta"]), _p(cv["dgamma"]), _p(cv["dbeta"]), _p(bdz), 1, rows)
    xpl, dypl = engine.split_planes(o["x"]), engine.split_planes(o["dy"])
    res = _rnd(g, *S["xs"]).cuda()
    stats = torch.empty(int(engine.lib.sg_conv2d_fwd_stats_bytes(C.byref(d))) // 4 + 4, device="cuda")
    tiles = C.c_int(7)
    assert not engine.conv2d_caps(d).bn_in and not engine.conv2d_caps(d, dgrad=True).bnb

    def opts(**kw):
        return L.ConvOpts(ws, wsn, **kw)

    fwd_cases = [
        ("res", opts(res=_p(res)), SG_EINVAL), ("bnb", opts(bnb=C.pointer(bnb)), SG_EINVAL),
        ("bn_in + a_planes", opts(bn_in=C.pointer(bq), a_planes=_p(xpl)), SG_EINVAL),
        ("bn_in on a geometry caps.bn_in denies", opts(bn_in=C.pointer(bq)), SG_EUNSUPPORTED),
    ]
    for name, oo, code in fwd_cases:
        rc, y = _fwd(engine, S, o, C.byref(oo))
        assert rc == code and _untouched(y), ("fwd", name, rc)
    dgrad_cases = [
        ("res + a_planes", opts(res=_p(res), a_planes=_p(dypl)), SG_EINVAL, None, 0),
        ("bnb + res", opts(bnb=C.pointer(bnb), res=_p(res)), SG_EINVAL, None, 0),
        ("bnb + a_planes", opts(bnb=C.pointer(bnb), a_planes=_p(dypl)), SG_EINVAL, None, 0),
        ("bnb + bias", opts(bnb=C.pointer(bnb)), SG_EINVAL, o["bt"], 0),
        ("bnb + flags", opts(bnb=C.pointer(bnb)), SG_EINVAL, None, L.SG_EPI_RELU),
        ("stats", opts(stats=_p(stats)), SG_EINVAL, None, 0), ("tiles_out", opts(tiles_out=C.pointer(tiles)), SG_EINVAL, None, 0),
        ("bn_in", opts(bn_in=C.pointer(bq)), SG_EINVAL, None, 0),
        ("bnb on a geometry caps.bnb denies", opts(bnb=C.pointer(bnb)), SG_EUNSUPPORTED, None, 0),
    ]
    for name, oo, code, bias, flags in dgrad_cases:
        rc, dx = _dgrad(engine, S, o, C.byref(oo), bias=bias, flags=flags)
        assert rc == code and _untouched(dx, bdz), ("dgrad", name, rc)
    wgrad_cases = [
        ("stats", opts(stats=_p(stats)), SG_EINVAL), ("tiles_out", opts(tiles_out=C.pointer(tiles)), SG_EINVAL),
        ("a_planes", opts(a_planes=_p(xpl)), SG_EINVAL), ("res", opts(res=_p(res)), SG_EINVAL), ("bnb", opts(bnb=C.pointer(bnb)), SG_EINVAL),
        ("bn_in on a geometry caps.bn_in denies", opts(bn_in=C.pointer(bq)), SG_EUNSUPPORTED),
    ]
    for name, oo, code in wgrad_cases:
        rc, gw, gb = _wgrad(engine, S, o, C.byref(oo))
        assert rc == code and _untouched(gw, gb), ("wgrad", name, rc)
    assert tiles.value == 7, "a refused launch wrote tiles_out"


def test_depthwise_options_refuse_what_no_kernel_takes(engine, dw):
    L, t, d, d2 = _lib(), dw["t"], dw["d"], dw["d2"]
    lib, dt, c = engine.lib, L.SG_F32, dw["shape"][3]
    wsp, wsn = _p(dw["ws"]), dw["ws"].numel()
    for infer, pre_relu in ((0, 1), (1, 0)):   # bn->relu has pre_relu's role; the fused BatchNormalization is the training form
        bq = _bn_in(L, dw["vec"], infer=infer)
        y = _sentinel(*dw["shape"])
        rc = lib.sg_dwconv2d_fwd(engine.h, engine.stream, dt, C.byref(d), _p(t["x"]), _p(t["w"]), _p(y), pre_relu, C.byref(bq))
        assert rc == SG_EINVAL and _untouched(y), (infer, pre_relu, rc)
        gw = _sentinel(3, 3, c, 1)
        rc = lib.sg_dwconv2d_wgrad(engine.h, engine.stream, dt, C.byref(d), _p(t["x"]), _p(t["dy"]), _p(gw), pre_relu, C.byref(bq), wsp, wsn)
        assert rc == SG_EINVAL and _untouched(gw), (infer, pre_relu, rc)
    # sums on a stride-2 descriptor: only the stride-1 run kernels sum for the BatchNormalization
    dgamma, dbeta, dx = _sentinel(c), _sentinel(c), _sentinel(*dw["shape"])
    v = dw["vec"]
    sums = L.DwBnSums(_p(t["x"]), _p(v["mean"]), _p(v["invstd"]), _p(v["gamma"]), _p(v["beta"]), 1, _p(dgamma), _p(dbeta), wsp, wsn)
    rc = lib.sg_dwconv2d_dgrad(engine.h, engine.stream, dt, C.byref(d2), _p(t["dy2"]), _p(t["w"]), None, _p(dx), 0, None, C.byref(sums))
    assert rc == SG_EUNSUPPORTED and _untouched(dx, dgamma, dbeta), rc
    # ... and the same operands on the stride-1 descriptor are taken (the refusal above is the geometry's)
    rc = lib.sg_dwconv2d_dgrad(engine.h, engine.stream, dt, C.byref(d), _p(t["dy"]), _p(t["w"]), None, _p(dx), 0, None, C.byref(sums))
    assert rc == 0 and not _untouched(dx) and not _untouched(dgamma) and not _untouched(dbeta)


# ------------------------------------------------------------------------------- caps.thin against the rule it replaces
def test_caps_thin_is_the_rule_the_host_restated(engine):
    from building_detection_amd import switches
    for k, stride, filters, cin in itertools.product((1, 3), (1, 2), (1, 2, 4, 8), (8, 16, 18, 64)):
        x_shape = (1, 8, 8, cin)
        d = engine.conv_desc(x_shape, filters, k, k, stride, 1, "same")
        thin = (k == 1 and stride == 1 and filters <= 4 and x_shape[-1] % 4 == 0 and x_shape[-1] >= 16
                and not switches.get("SG_CONV_NOTHIN"))
        for dgrad in (False, True):
            assert bool(engine.conv2d_caps(d, dgrad=dgrad).thin) == thin, (k, stride, filters, cin, dgrad)
