"""Prepared weight planes at every convolution site of the five models ("who chooses the kernel").

The product lays out every layer's bf16 weight planes once per optimiser step (sg_conv2d_planes_job, ONE sg_prepare_planes launch,
then launches with ws_bytes = SG_WS_PREPARED); the op tests convert per launch into a plain workspace.  The two routes meet in one
plan, plan_conv(), and both bugs this path has had were a query and a launch reading that plan differently.  This file runs the
product's route at the layer geometries and batch sizes the models really have (tests/_plane_sites.py enumerates them), under the
three arithmetic modes of fp32 storage and under bf16 storage, and holds it to three things:

  bits     the launch on prepared planes equals the launch that converts for itself, output and BatchNormalization statistics;
  bounds   a launch stays inside the workspace its own *_ws_bytes query returned, sg_prepare_planes and a prepared launch stay
           inside the bytes sg_conv2d_planes_job reported (guard bands of a fixed byte pattern behind every slot);
  oracle   one representative of every plan class (what the ABI reveals of the plan) against oracle.tfops in float64 - two engine
           paths that agree bit for bit may still both be wrong.

Oracle references and bounds are the ones the op tests apply to each arithmetic (test_ops_gpu.close, test_bf16_gpu.close_bf16,
test_bf16_compute_mode_on_fp32_storage, test_conv_transpose_and_head_bf16); the oracle sees images 0 and N - 1 of a representative,
every image takes part in the bit comparison.  One sweep (module fixture) collects every finding; the tests below assert on it, so
a failure lists all offending sites at once.  Run with -s for the report (profiles/plane_sites_gpu.txt is one).
"""
import collections
import ctypes as C
import time
import zlib

import numpy as np
import pytest
import torch

import _plane_sites as PS
from oracle import tfops as T

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ULP = 2.0 ** -8          # 1 bf16 ulp (test_bf16_gpu.ULP)
RTOL = 2e-5              # test_ops_gpu.RTOL
RTOL_MODE2 = 1e-5        # test_bf16_compute_mode_on_fp32_storage
GUARD, PATTERN = 1024, 0xA5
SG_EINVAL, SG_EWORKSPACE = -1, -2
BIAS, RELU = 1, 2
NAN = float("nan")


def rb(t):
    return t.to(BF).float()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _pad256(n):
    return (n + 255) // 256 * 256


def _seed(*what):
    return zlib.crc32(repr(what).encode()) % (2 ** 31)


def _mode_name(mode):
    return "bf16" if mode is None else f"m{mode}"


def _shapes(s, d):
    """(activation shape, activation dtype, output shape, output dtype) of a site's launch"""
    bf = s.policy != "float32"
    act = BF if bf else torch.float32
    if not s.dgrad:
        return (d.N, d.H, d.W, d.Cin), act, (d.N, d.Ho, d.Wo, d.Cout), (torch.float32 if (bf and s.head) else act)
    return (d.N, d.Ho, d.Wo, d.Cout), (torch.float32 if (bf and s.head) else act), (d.N, d.H, d.W, d.Cin), act


def _launch(e, s, d, a, w, bias, flags, wsp, wsn, want_stats=False, a_planes=None, out=None):
    """One raw library launch of site `s` -> (rc, output, statistics, tiles).  Output and statistics are pre-filled with NaN, so an
    element no kernel wrote can never compare equal."""
    lib = e.lib
    _, _, oshape, odt = _shapes(s, d)
    if out is None:
        out = torch.full(oshape, NAN, dtype=odt, device=e.device)
    st, tiles = None, C.c_int(0)
    bp = _p(bias) if (flags & BIAS) else None
    if not s.dgrad:
        if want_stats:
            st = torch.full((lib.sg_conv2d_fwd_stats_bytes(C.byref(d)) // 4,), NAN, dtype=torch.float32, device=e.device)
        o = PS_lib().ConvOpts(wsp, wsn, _p(st), C.pointer(tiles) if want_stats else None, _p(a_planes))
        rc = lib.sg_conv2d_fwd(e.h, e.stream, PS.abi_dtype(s), C.byref(d), _p(a), _p(w), bp, _p(out), flags, C.byref(o))
    else:
        o = PS_lib().ConvOpts(wsp, wsn, a_planes=_p(a_planes))
        rc = lib.sg_conv2d_dgrad(e.h, e.stream, PS.abi_dtype(s), C.byref(d), _p(a), _p(w), bp, _p(out), flags, C.byref(o))
    return int(rc), out, st, int(tiles.value)


def _activation(e, s, d, key):
    shape, dt, _, _ = _shapes(s, d)
    g = torch.Generator(device=e.device).manual_seed(_seed("act", key))
    a = torch.randn(shape, generator=g, device=e.device, dtype=torch.float32)
    return a if dt == torch.float32 else a.to(dt)


def _bias(e, s, d, key):
    g = torch.Generator(device=e.device).manual_seed(_seed("bias", key))
    return torch.randn(d.Cin if s.dgrad else d.Cout, generator=g, device=e.device, dtype=torch.float32)


_W_CACHE = {}


def _weights(e, group):
    """The model's weight arena: seeded random kernels at the model's own offsets, each scaled to its fan-in."""
    got = _W_CACHE.get("w")
    if got is not None and got[0] == (group.model, group.n_train):
        return got[1]
    _W_CACHE.clear()
    g = torch.Generator().manual_seed(_seed("weights", group.model))
    host = torch.rand(max(group.n_train, 64), generator=g) * 2 - 1
    done = set()
    for s in group.sites:
        if s.w_off in done:
            continue
        done.add(s.w_off)
        n = int(np.prod(s.w_shape))
        host[s.w_off:s.w_off + n] *= 1.0 / np.sqrt(s.w_shape[0] * s.w_shape[1] * s.w_shape[2])
    w = host.to(e.device)
    _W_CACHE["w"] = ((group.model, group.n_train), w)
    return w


def _w_of(arena, s):
    n = int(np.prod(s.w_shape))
    return arena[s.w_off:s.w_off + n].view(s.w_shape)


class _Table:
    """The job table of one (model, batch, storage, mode) as the header describes it: out_off 256-byte aligned and non-zero for the
    first job, block0 the running sum of nblocks, the whole table prepared in ONE launch; a guard band behind every slot (the pad
    up to 256 belongs to it) and in front of the first."""

    def __init__(self, e, group, w_arena):
        self.e, self.slots, self.first = e, [], {}
        jobs, off, blocks = [], 256, 0
        for s in group.sites:
            job, nbytes = PS.planes_job(e, s)
            if job.kind == 0:
                continue
            job.w_off, job.out_off, job.block0 = s.w_off, off, blocks
            self.first.setdefault(PS.site_key(s), len(self.slots))
            self.slots.append((off, nbytes, s))
            off += _pad256(nbytes) + GUARD
            blocks += job.nblocks
            jobs.append(job)
        self.njobs, self.blocks, self.size = len(jobs), blocks, off
        self.arena = None
        if not jobs:
            return
        self.arena = torch.full((off,), PATTERN, dtype=torch.uint8, device=e.device)
        arr = (PS_lib().PlanesJob * len(jobs))(*jobs)
        self.jobs_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(e.device)
        bands = [(0, 256)] + [(o + n, o + _pad256(n) + GUARD) for o, n, _ in self.slots]
        self._bands = bands
        self._idx = torch.from_numpy(np.concatenate([np.arange(a, b, dtype=np.int64) for a, b in bands])).to(e.device)
        PS_lib().check(e.lib.sg_prepare_planes(e.h, e.stream, _p(w_arena), _p(self.arena), _p(self.jobs_dev), self.njobs, self.blocks),
                       "sg_prepare_planes")

    def slot(self, key):
        i = self.first.get(key)
        return None if i is None else self.slots[i]

    def touched(self):
        """descriptions of the guard bands that no longer hold the pattern"""
        if self.arena is None:
            return []
        bad = (self.arena[self._idx] != PATTERN)
        if not bool(bad.any()):
            return []
        bad = bad.cpu().numpy()
        out, pos = [], 0
        for bi, (a, b) in enumerate(self._bands):
            n = int(bad[pos:pos + (b - a)].sum())
            if n:
                first = int(np.argmax(bad[pos:pos + (b - a)]))
                who = "front band" if bi == 0 else PS.describe(self.slots[bi - 1][2])
                out.append(f"{n} guard bytes of the band behind [{who}] (the first {first} bytes past the slot's end)")
            pos += b - a
        return out


def PS_lib():
    from building_detection_amd import _lib
    return _lib


def _oracle(s, mode, d, a, w, bias, outs):
    """fp64 reference of images 0 and N - 1 -> [(what, error, scale, bound)] for the outputs {flags: tensor} of one launch path.
    Reference operands and bound by arithmetic: see the module docstring."""
    f32 = s.policy == "float32"
    idx = [0] if d.N == 1 else [0, d.N - 1]
    a_s = a[idx].float().cpu()
    w_s, b_s = w.detach().float().cpu(), bias.detach().cpu().double()
    if f32 and mode == 2:
        a_s, w_s = rb(a_s), rb(w_s)
    elif not f32 and not s.head:
        w_s = rb(w_s)       # (the activation is bf16 already; the thin head multiplies the fp32 kernel itself)
    a64, w64 = a_s.double(), w_s.double()
    padding = "same" if (d.Ho, d.Wo) == (-(-d.H // d.stride), -(-d.W // d.stride)) else "valid"
    assert T.same_pad(d.H, d.KH, d.stride, d.dilation)[1] == d.pad_t or padding == "valid"
    if not s.dgrad:
        ref = T.conv2d(a64, w64, None, d.stride, d.dilation, padding)
    else:
        xr = torch.zeros(len(idx), d.H, d.W, d.Cin, dtype=torch.float64, requires_grad=True)
        y = T.conv2d(xr, w64, None, d.stride, d.dilation, padding)
        assert tuple(y.shape) == tuple(a64.shape), (tuple(y.shape), tuple(a64.shape))
        y.backward(a64)
        ref = xr.grad
    rows = []
    for flags, out in outs.items():
        r = ref
        if flags & BIAS:
            r = r + b_s
        if flags & RELU:
            r = torch.relu(r)
        got = out[idx].float().cpu().double()
        assert got.shape == r.shape, (got.shape, r.shape)
        err = float((got - r).abs().max())
        if got.isnan().any():
            err = float("inf")
        scale = float(r.abs().max())
        if f32:
            bound = (RTOL_MODE2 if mode == 2 else RTOL) * max(scale, 1e-6 if mode != 2 else 0.0)
        elif s.head and not s.dgrad:
            bound = 1e-5 * scale          # fp32 logits of the softmax head (test_conv_transpose_and_head_bf16)
        else:
            bound = ULP * max(scale, 1e-30)
        rows.append((f"flags={flags}", err, scale, bound))
    return rows


class Sweep:
    def __init__(self, e):
        self.e = e
        self.report = []          # the lines of profiles/plane_sites_gpu.txt
        self.bit, self.rc, self.guards, self.pin, self.oracle_fail = [], [], [], [], []
        self.oracle_rows = []
        self.launched = 0
        self.oracle_seconds = 0.0
        t0 = time.time()
        self.groups = PS.enumerate_groups()
        self.uniq, self.owner = PS.unique_sites(self.groups)
        self.info = PS.survey(e, self.uniq)
        self.reps = PS.representatives(self.uniq, self.info)
        self.pinned = self.pin_wide_pointwise_mode2()
        self.rep_set = set(self.reps.values()) | set(self.pinned)
        self.diagnosed = 0
        self.say(f"unique sites: {len(self.uniq)} (of {sum(len(g.sites) for g in self.groups)} in {len(self.groups)} "
                 "(model, size, batch, storage) tables)")
        kinds = collections.Counter()
        for (k, mode), i in self.info.items():
            kinds[(self.uniq[k].policy, _mode_name(mode), "dgrad" if self.uniq[k].dgrad else "fwd", i.kind)] += 1
        for key in sorted(kinds):
            self.say(f"kind count: storage {key[0]:15s} {key[1]:5s} {key[2]:5s} kind {key[3]}: {kinds[key]}")
        self.kinds = kinds
        self.say(f"plan classes: {len(self.reps)}")
        prev = e.lib.sg_get_conv_x6()
        try:
            for gi, g in enumerate(self.groups):
                owned = [k for k, o in self.owner.items() if o == gi]
                if not owned:
                    continue
                for mode in PS.modes_of(g.policy):
                    tg = time.time()
                    with PS.mode_set(e, mode):
                        self.run_group(g, mode, owned)
                    torch.cuda.empty_cache()
                    print(f"  .. {g.model}/{g.size}/b{g.batch}/{g.policy}/{_mode_name(mode)}: {len(owned)} sites, {time.time() - tg:.1f} s "
                          f"(oracle {self.oracle_seconds:.1f} s so far)", flush=True)
        finally:
            e.lib.sg_set_conv_x6(prev)
            _W_CACHE.clear()
        self.seconds = time.time() - t0
        for cls, (k, mode) in self.reps.items():
            rows = [r for r in self.oracle_rows if r[0] == (k, mode)]
            i = self.info[(k, mode)]
            txt = "; ".join(f"{what} err {err:.3e} bound {bound:.3e} ({err / bound if bound else float('inf'):.2f})" for _, what, err, scale, bound in rows)
            self.say(f"class {_mode_name(mode):5s} {'dgrad' if cls[2] else 'fwd  '} kind {i.kind} npl {i.npl} kd {i.kd:2d} vpad {int(cls[6])} "
                     f"npad {int(cls[7])} planes_in {cls[8]} s{cls[9]} dil {int(cls[10])} head {int(cls[11])} | {PS.describe(self.uniq[k])} | "
                     f"{txt or ('not checked' if i.kind >= 1 or (cls[0] == 'float32' and mode in (0, 1)) else 'no prepared path; counted only')}")
        for k, mode in self.pinned:
            rows = [r for r in self.oracle_rows if r[0] == (k, mode)]
            txt = "; ".join(f"{what} err {err:.3e} bound {bound:.3e} ({err / bound if bound else float('inf'):.2f})" for _, what, err, scale, bound in rows)
            self.say(f"pinned {_mode_name(mode)} kind {self.info[(k, mode)].kind} (wide-pointwise geometry, batch >= 8) | {PS.describe(self.uniq[k])} | "
                     f"{txt or 'not checked'}")
        self.say(f"launch pairs compared: {self.launched}; sweep wall time {self.seconds:.1f} s, of which the fp64 oracle {self.oracle_seconds:.1f} s")

    def pin_wide_pointwise_mode2(self):
        """Beside the class representatives (which tend to be the smallest shapes a model has) the oracle always sees the case the
        shared plan was introduced for: fp32 storage with bf16 products (mode 2) at the wide pointwise geometry - 1x1, stride 1,
        728 -> 728, >= 6144 rows - at batch >= 8, forward and input gradient, the site with the fewest multiply-adds each."""
        best = {}
        for (k, mode), i in self.info.items():
            s = self.uniq[k]
            f = dict(zip(PS.desc_fields(), s.desc))
            if (mode == 2 and i.kind >= 1 and f["KH"] == 1 and f["KW"] == 1 and f["stride"] == 1 and f["Cin"] == 728 and f["Cout"] == 728
                    and f["N"] >= 8 and f["N"] * f["Ho"] * f["Wo"] >= 6144):
                if s.dgrad not in best or PS.macs(s) < PS.macs(self.uniq[best[s.dgrad][0]]):
                    best[s.dgrad] = (k, mode)
        return [best[dg] for dg in sorted(best)]

    def say(self, line):
        self.report.append(line)
        print(line, flush=True)

    # ------------------------------------------------------------------------------------------------------------------
    def run_group(self, g, mode, owned):
        e = self.e
        w_arena = _weights(e, g)
        table = _Table(e, g, w_arena)
        torch.cuda.synchronize()
        tag = f"{g.model}/{g.size}/b{g.batch}/{g.policy}/{_mode_name(mode)}"
        for t in table.touched():
            self.guards.append(f"{tag}: sg_prepare_planes wrote {t}")
        for k in owned:
            s, i = self.uniq[k], self.info[(k, mode)]
            rep = (k, mode) in self.rep_set
            if i.kind == 0 and not (rep and s.policy == "float32" and mode in (0, 1)):
                continue
            try:
                self.run_site(table, w_arena, k, s, mode, i, rep)
            except AssertionError:
                raise
            except Exception as ex:   # a library error at one site is a finding, the sweep goes on
                self.rc.append(f"{_mode_name(mode)} {PS.describe(s)}: {type(ex).__name__}: {ex}")
        torch.cuda.synchronize()
        for t in table.touched():
            self.guards.append(f"{tag}: after the launches, {t}")

    def run_site(self, table, w_arena, k, s, mode, i, rep):
        e = self.e
        d = PS.make_desc(s)
        name = f"{_mode_name(mode)} kind {i.kind} {PS.describe(s)}"
        a, w, bias = _activation(e, s, d, k), _w_of(w_arena, s), _bias(e, s, d, k)
        # the per-launch route: a private workspace of EXACTLY the query's size, a guard band behind it
        need = i.ws
        wsbuf = torch.full((need + GUARD,), PATTERN, dtype=torch.uint8, device=e.device)
        plain = (_p(wsbuf), C.c_size_t(need))
        epi = [0, BIAS, BIAS | RELU] if (not s.dgrad or s.convt) else [0]
        keep = {}
        if i.kind == 0:   # no prepared path: the representative's per-launch result against the oracle
            for flags in ([0, BIAS | RELU] if len(epi) > 1 else [0]):
                rc, o, _, _ = _launch(e, s, d, a, w, bias, flags, *plain)
                if rc:
                    self.rc.append(f"{name} flags={flags}: per-launch rc={rc} ({e.lib.sg_last_error().decode()})")
                else:
                    keep[flags] = o
        else:
            off, nbytes, _ = table.slot(k)
            assert nbytes == i.bytes
            prepared = (C.c_void_p(table.arena.data_ptr() + off), C.c_size_t(PS_lib().SG_WS_PREPARED))
            runs = [(f, False) for f in epi] + ([(BIAS, True)] if not s.dgrad else [])
            for flags, stats in runs:
                rc1, o1, st1, t1 = _launch(e, s, d, a, w, bias, flags, *prepared, want_stats=stats)
                rc2, o2, st2, t2 = _launch(e, s, d, a, w, bias, flags, *plain, want_stats=stats)
                what = f"{name} flags={flags}{' +stats' if stats else ''}"
                if rc1 or rc2:
                    self.rc.append(f"{what}: prepared rc={rc1}, per-launch rc={rc2} ({e.lib.sg_last_error().decode()})")
                    continue
                self.launched += 1
                if not torch.equal(o1, o2):
                    df = (o1.float() - o2.float()).abs()
                    nn = int(torch.isnan(o1).sum()) + int(torch.isnan(o2).sum())
                    self.bit.append(f"{what}: prepared != per-launch: {int((o1 != o2).sum())} of {o1.numel()} elements, max |diff| "
                                    f"{float(torch.nan_to_num(df).max()):.3e} of max |y| {float(torch.nan_to_num(o2.float()).abs().max()):.3e}, {nn} NaN")
                    del df
                    if flags == 0 and not stats and self.diagnosed < 8:   # which of the two is wrong?  (the first few sites only)
                        self.diagnosed += 1
                        for route, o in (("prepared", o1), ("per-launch", o2)):
                            for _, err, scale, bound in _oracle(s, mode, d, a, w, bias, {0: o}):
                                self.bit.append(f"{what}: {route} against the fp64 oracle: max error {err:.3e}, bound {bound:.3e}")
                if stats:
                    n = t1 * 2 * (d.Cout)
                    if t1 != t2:
                        self.bit.append(f"{what}: statistics tiles {t1} (prepared) != {t2} (per-launch)")
                    elif t1 > 0 and not torch.equal(st1[:n], st2[:n]):
                        self.bit.append(f"{what}: statistics differ ({int((st1[:n] != st2[:n]).sum())} of {n})")
                elif rep and flags in (0, BIAS | RELU):
                    keep[flags] = o1
                if flags == 0 and not stats and i.pin:
                    # planes-in launches: the caller's split_planes(x) gives the bits of the launch that splits for itself,
                    # with prepared weight planes and without them
                    pl = e.split_planes(a)
                    for route, ws in (("prepared", prepared), ("per-launch", plain)):
                        rc, o, _, _ = _launch(e, s, d, a, w, bias, 0, *ws, a_planes=pl)
                        if rc or not torch.equal(o, o1):
                            self.pin.append(f"{name}: activation planes handed in ({route}): rc={rc}, "
                                            f"{'bits differ' if not rc else e.lib.sg_last_error().decode()}")
                    del pl
                del o1, o2, st1, st2
        torch.cuda.synchronize()
        if not bool((wsbuf[need:] == PATTERN).all()):
            self.guards.append(f"{name}: a launch wrote behind the {need} bytes sg_conv2d_{'dgrad' if s.dgrad else 'fwd'}_ws_bytes returned "
                               f"({int((wsbuf[need:] != PATTERN).sum())} guard bytes)")
        if rep and keep:
            to = time.time()
            rows = _oracle(s, mode, d, a, w, bias, keep)
            self.oracle_seconds += time.time() - to
            for what, err, scale, bound in rows:
                self.oracle_rows.append(((k, mode), what, err, scale, bound))
                if not err <= bound:
                    self.oracle_fail.append(f"{name} {what}: max error {err:.3e} > bound {bound:.3e} (max |ref| {scale:.3e})")


@pytest.fixture(scope="module")
def sweep(engine):
    return Sweep(engine)


def _none(findings, what):
    assert not findings, f"{len(findings)} {what}:\n  " + "\n  ".join(findings[:400])


def test_enumeration_still_covers_every_plan_family(sweep):
    """The sweep is only as good as the sites it meets.  Which kind a given layer takes is a performance choice and is not pinned;
    that every family is still met is."""
    sw = sweep
    have = collections.defaultdict(int)
    for (k, mode), i in sw.info.items():
        s = sw.uniq[k]
        f = dict(zip(PS.desc_fields(), s.desc))
        if s.policy == "float32" and mode == 1:
            have[("fp32 mode 1", "dgrad" if s.dgrad else "fwd", i.kind)] += 1
        if s.policy != "float32":
            have[("bf16", i.kind)] += 1
        if (mode == 2 and i.kind >= 1 and f["KH"] == 1 and f["KW"] == 1 and f["stride"] == 1 and f["N"] * f["Ho"] * f["Wo"] >= 6144
                and i.N == 728):
            have["wide-pointwise geometry in mode 2"] += 1
        if i.kind >= 1 and i.Ckp != i.Ck:
            have["Ckp != Ck"] += 1
        if i.pin == 1 and i.kind >= 1:
            have["planes_in == 1"] += 1
        if s.dgrad and f["stride"] == 2 and i.kind >= 1:
            have["stride-2 dgrad"] += 1
    wanted = [("fp32 mode 1", dr, kd) for dr in ("fwd", "dgrad") for kd in (1, 2, 3)] + [("bf16", 1), ("bf16", 3)] + [
        "wide-pointwise geometry in mode 2", "Ckp != Ck", "planes_in == 1", "stride-2 dgrad"]
    missing = [str(c) for c in wanted if not have[c]]
    assert not missing, "the enumerated sites no longer include: " + "; ".join(missing)
    assert len(sw.uniq) > 0 and sw.launched > 0


def test_prepared_planes_equal_per_launch_conversion_bit_for_bit(sweep):
    _none(sweep.bit, "launches whose result depends on who converted the weights")


def test_no_launch_is_refused_on_its_own_workspace_query(sweep):
    """no SG_EWORKSPACE (or any other error) on a workspace of exactly *_ws_bytes, nor on the prepared planes"""
    _none(sweep.rc, "refused launches")


def test_guard_bands_behind_slots_and_workspaces_are_untouched(sweep):
    _none(sweep.guards, "writes outside the reported sizes")


def test_activation_planes_handed_in_give_the_same_bits(sweep):
    _none(sweep.pin, "planes-in launches that depend on who split the activation")


def test_every_plan_class_meets_the_fp64_oracle(sweep):
    sw = sweep
    unchecked = [f"{cls}: {PS.describe(sw.uniq[k])}" for cls, (k, mode) in sw.reps.items()
                 if not any(r[0] == (k, mode) for r in sw.oracle_rows)
                 and (sw.info[(k, mode)].kind >= 1 or (sw.uniq[k].policy == "float32" and mode in (0, 1)))]
    _none(unchecked, "plan classes without an oracle check")
    missing = [PS.describe(sw.uniq[k]) for k, mode in sw.pinned if not any(r[0] == (k, mode) for r in sw.oracle_rows)]
    assert len(sw.pinned) == 2 and not missing, f"the pinned mode-2 wide-pointwise sites were not checked: {sw.pinned} {missing}"
    _none(sw.oracle_fail, "representatives outside their bound")


def _one_job_table(e, s, w_arena):
    job, nbytes = PS.planes_job(e, s)
    job.w_off, job.out_off, job.block0 = s.w_off, 256, 0
    arena = torch.full((256 + _pad256(nbytes) + GUARD,), PATTERN, dtype=torch.uint8, device=e.device)
    jd = torch.frombuffer(bytearray(bytes((PS_lib().PlanesJob * 1)(job))), dtype=torch.uint8).to(e.device)
    PS_lib().check(e.lib.sg_prepare_planes(e.h, e.stream, _p(w_arena), _p(arena), _p(jd), 1, job.nblocks), "sg_prepare_planes")
    return arena, jd


def test_misaligned_activation_is_refused_on_prepared_planes_and_runs_on_a_plain_workspace(sweep):
    """An activation pointer 4 bytes off a 16-byte boundary: with SG_WS_PREPARED the launch returns SG_EINVAL and leaves the output
    untouched (the planes are laid out for a kernel it cannot take); with a plain workspace it runs (on the any-shape kernels) and
    meets the oracle bound of its arithmetic.  One site of each kind per storage type, the one with the fewest multiply-adds."""
    sw, e = sweep, sweep.e
    picks = {}
    for (k, mode), i in sw.info.items():
        s = sw.uniq[k]
        if mode not in (1, None) or i.kind == 0 or s.head:
            continue
        key = (s.policy, i.kind)
        if key not in picks or PS.macs(s) < PS.macs(sw.uniq[picks[key][0]]):
            picks[key] = (k, mode)
    for want in (("float32", 1), ("float32", 2), ("float32", 3), ("mixed_bfloat16", 1), ("mixed_bfloat16", 3)):
        assert want in picks, f"no site of kind {want[1]} on {want[0]} storage"
    by_group = {(g.model, g.size, g.batch, g.policy): g for g in sw.groups}
    try:
        for (policy, kind), (k, mode) in sorted(picks.items()):
            s, i = sw.uniq[k], sw.info[(k, mode)]
            d = PS.make_desc(s)
            w_arena = _weights(e, by_group[(s.model, s.size, s.batch, s.policy)])
            w, bias = _w_of(w_arena, s), _bias(e, s, d, k)
            arena, jd = _one_job_table(e, s, w_arena)
            ashape, adt, oshape, odt = _shapes(s, d)
            n = int(np.prod(ashape))
            shift = 4 // torch.empty(0, dtype=adt).element_size()
            g = torch.Generator(device=e.device).manual_seed(_seed("shifted", k))
            buf = torch.randn(n + 8, generator=g, device=e.device, dtype=torch.float32).to(adt)
            a = buf[shift:shift + n].view(ashape)
            assert a.data_ptr() % 16 == 4 and a.is_contiguous()
            out = torch.full(oshape, 123.0, dtype=odt, device=e.device)
            rc, _, _, _ = _launch(e, s, d, a, w, bias, 0, C.c_void_p(arena.data_ptr() + 256), C.c_size_t(PS_lib().SG_WS_PREPARED), out=out)
            torch.cuda.synchronize()
            name = f"kind {kind} {PS.describe(s)}"
            assert rc == SG_EINVAL, f"{name}: misaligned activation on prepared planes returned rc={rc}, not SG_EINVAL"
            assert bool((out == 123.0).all()), f"{name}: a refused launch wrote into its output"
            wsbuf = torch.full((i.ws + GUARD,), PATTERN, dtype=torch.uint8, device=e.device)
            rc, o, _, _ = _launch(e, s, d, a, w, bias, 0, _p(wsbuf), C.c_size_t(i.ws))
            torch.cuda.synchronize()
            assert rc == 0, f"{name}: misaligned activation on a plain workspace: rc={rc} ({e.lib.sg_last_error().decode()})"
            assert bool((wsbuf[i.ws:] == PATTERN).all()), f"{name}: wrote behind its workspace"
            for what, err, scale, bound in _oracle(s, mode, d, a, w, bias, {0: o}):
                print(f"misaligned, plain workspace: {_mode_name(mode)} {name}: err {err:.3e} bound {bound:.3e} ({err / bound:.2f})", flush=True)
                assert err <= bound, f"{name}: max error {err:.3e} > bound {bound:.3e}"
            del arena, jd, buf, a, out, o, wsbuf
    finally:
        _W_CACHE.clear()
