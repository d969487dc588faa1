"""Every launch-time variant of the depthwise convolution kernels (csrc/spatial.hip: sg_dwconv2d_fwd / _dgrad / _wgrad) against plain
float64 torch on the CPU, through the C ABI itself.  The companion of tests/test_bandwidth_variants_gpu.py and
tests/test_batchnorm_variants_gpu.py, with their machinery: operands are tests/_guarded.py arenas (NaN guard bands, NaN-prefilled
outputs, inputs whose bits must survive, workspaces of exactly the queried size).  The cases themselves are tests/_dw_cases.py
(also run as a program, for the forms behind the process-wide switches SG_DW_FSTRIP, SG_DW_FSTRIP_HS, SG_DW_STRIP, SG_DW_RR).

Reference: F.conv2d(groups = C, dilation) on the explicitly padded tensor, autograd for dx and dw; pre-ReLU before the padding; a
BatchNormalization in the gather as z = ((x - mean) invstd) gamma + beta [ReLU], padded with zeros AFTER that; the sums as
dbeta = sum g, dgamma = sum g xhat with g the complete dx (res included), masked by z > 0 under the layer's fused ReLU, beta placed by
_bn_cases.gap_beta so that the whole tensor is compared.  bf16 references start from the bf16-rounded inputs (and res).
Inputs: N >= 2 (257 and 9 in two cap cases), uniform in [-1, 1] on every border, H != W, nine distinct random taps per channel.
Tolerances, as max|got - ref| <= tol * max|ref| over the whole tensor: 2e-5 fp32 y / dx, 1e-4 fp32 dw / dgamma / dbeta (fp32 for
either storage), 2^-7 bf16-stored y / dx; refusals and gap columns exact.

Every case id ends in the kernel the launch takes at 256 CUs (the case asserts the same for this device before launching, and that
the engine's own plan, sg_dwconv2d_plan, equals the mirror of the rules it was named from, tests/_dw_cases.plan_mirror):
    fwd|dgrad.V<1|4>[.cap]                                      dw_fwd_kernel / dw_dgrad_kernel; .cap: past ew_blocks' 16384 workgroups
    fwd|dgrad.run.RR<1|2>lc<lanes per run>gx<column blocks>gy<workgroup rows>.dead<lanes past the last chunk>[.trip2]
    fwd|dgrad.strip.HS<band>[+short]r<last band's rows % 3>gx..gy...dead..[.trip2]          .trip2: the run / strip loop's second trip
    wgrad.seg.V<1|4>tx..gx...<one|few|many>                       DwWgradOp on the segment reducer
    wgrad.run.RR<1|2>.V4tx..gx...<one|few|many>                   DwWgradRunOp
    wgrad.strip.HS<band>[+short]gx...<one|few|many>[.capped]      dw_wgrad_strip_kernel; .capped: S = 256 and a slot walks a second strip
and inside a case every template form runs: forward plain / RELU / BN / BN+RELU; dgrad plain / MASK / +res / MASK+res / res == dx /
SUMS / MASK+SUMS / res+SUMS / SUMS under a fused ReLU / all of them at once; wgrad <PRE, BN> in its four forms.

Out of reach of a test this size and left out: the second trip of the non-SUMS run and strip loops (above ~0.5 GB per operand; the
same loop is walked twice by the SUMS cap cases), and the uint32 index arithmetic near 2^32."""
import ctypes as CT
import os
import subprocess
import sys

import pytest
import torch

import _dw_cases as D
from _dw_cases import BF16, F32, Geom
from _guarded import (Guarded, assert_written, bn_sums_ref, dw_conv_ref, dw_geom, dw_grads_ref, dw_input_ref, gaps_keep_prefill,
                      widen)

gpu = pytest.mark.gpu
DT = (F32, BF16)


def _ids(g, dtype, tail):
    return f"{g.tag}-{D.dname(dtype)}-{tail}"


def _stencil_params(shapes):
    return [pytest.param(g, d, id=_ids(g, d, D.stencil_name(g, D.esize(d), g.C, False))) for g in shapes for d in DT]


def _wgrad_params(shapes):
    return [pytest.param(g, d, id=_ids(g, d, D.wgrad_name(D.REF_CUS, g, True, g.C, g.C))) for g in shapes for d in DT]


# ================================================================================================ self-checks (CPU)
def test_dispatch_mirrors_agree_with_hand_computed_values_at_256_cus():
    run = lambda *a, sums=False: D.plan_dw_stencil_run(Geom(*a), sums)
    # lc: the power of two that covers C / 4 chunks, at most 64; a workgroup holds 256 / lc runs
    assert run(2, 6, 8, 4) == (2, 1, 1, 1, 12)            # 2 images x 3 row pairs x 2 runs per row
    assert run(2, 6, 8, 20) == (2, 8, 1, 1, 12)           # 5 chunks on 8 lanes: 3 dead
    assert run(2, 62, 12, 260) == (2, 64, 2, 47, 186)     # 65 chunks: two column blocks, the second with one live lane
    assert run(2, 3, 8, 20) == (1, 8, 1, 1, 12)           # odd H: one row per run
    assert run(2, 62, 268, 132) == (2, 64, 1, 1039, 4154) and run(2, 62, 268, 132, sums=True)[3] == 1024
    assert D.dw_rows_per_run(66, 33792, True) == 2 and D.dw_rows_per_run(64, 32768, True) == 1 and D.dw_rows_per_run(9, 10 ** 6, True) == 1
    assert D.dw_rows_per_run(1, 8, False) == 1 and D.dw_rows_per_run(2, 8, False) == 2
    # the strips of the stencil: HS 16 from 64 rows on; gy = ceil(strips / 16)
    assert D.plan_dw_stencil_strip(Geom(2, 64, 8, 4), False) == (16, 16, 1, 1) and D.plan_dw_stencil_strip(Geom(2, 68, 12, 68), False) == (16, 30, 2, 2)
    assert D.plan_dw_stencil_strip(Geom(257, 64, 64, 4), False) == (16, 16448, 1, 1028) and D.plan_dw_stencil_strip(Geom(257, 64, 64, 4), True)[3] == 1024
    assert D.dw_stencil_strips_ok(Geom(2, 64, 8, 4), 4, 4) and not D.dw_stencil_strips_ok(Geom(2, 66, 8, 4), 4, 4) and not D.dw_stencil_strips_ok(Geom(2, 60, 8, 4), 4, 4)
    assert not D.dw_stencil_strips_ok(Geom(64, 1024, 1024, 4), 4, 4)      # 1 GiB: bit 30 is a flag
    # the strips of the filter gradient: HS = H below 16 rows, 8 below 128, 16 from there; S = min(ceil(strips / 16), 1024 / gx, 256)
    P = lambda *a: D.plan_dw_wgrad_strip(256, Geom(*a))
    assert P(2, 12, 8, 4) == (12, 1, 4, 1, 1) and P(2, 20, 12, 68) == (8, 3, 18, 2, 2) and P(2, 128, 128, 4) == (16, 8, 512, 1, 32)
    assert P(2, 132, 8, 20) == (16, 9, 36, 1, 3) and P(9, 64, 256, 4) == (8, 8, 4608, 1, 256)
    assert D.dw_wgrad_strips_ok(Geom(2, 8, 8, 4), 4, 4) and not D.dw_wgrad_strips_ok(Geom(2, 6, 8, 4), 4, 4) and not D.dw_wgrad_strips_ok(Geom(2, 8, 8, 4, s=2), 4, 4)
    assert D.dw_run_ok(Geom(2, 5, 8, 4)) and not D.dw_run_ok(Geom(2, 5, 6, 4)) and not D.dw_run_ok(Geom(2, 5, 8, 5))
    assert not D.dw_run_ok(Geom(2, 5, 8, 4, d=2)) and not D.dw_run_ok(Geom(2, 5, 8, 4, KH=5)) and not D.dw_run_ok(Geom(2, 5, 8, 4, same=False))
    # geometry: stride 2 'same' pads (0, 1) on even and (1, 1) on odd maps; dilation 3 on three rows: (3, 3)
    assert dw_geom(6, 8, 3, 3, 2, 1, True) == (3, 4, 0, 1, 0, 1) and dw_geom(7, 5, 3, 3, 2, 1, True) == (4, 3, 1, 1, 1, 1)
    assert dw_geom(7, 8, 3, 3, 2, 1, False) == (3, 3, 0, 0, 0, 0) and dw_geom(3, 6, 3, 3, 1, 3, True) == (3, 6, 3, 3, 3, 3)
    assert dw_geom(6, 7, 5, 3, 1, 1, True) == (6, 7, 2, 2, 1, 1)
    # names
    assert D.stencil_name(Geom(2, 62, 12, 260), 4, 260, False) == "run.RR2lc64gx2gy47.dead63"
    assert D.stencil_name(Geom(2, 72, 8, 68), 2, 68, True) == "strip.HS16+shortr2gx2gy2.dead15"     # 2 x 5 bands x 2 = 20 strips
    assert D.stencil_name(Geom(2, 66, 8, 20), 4, 20, False) == "run.RR2lc8gx1gy5.dead3"
    assert D.stencil_name(Geom(257, 64, 64, 4), 4, 4, True) == "strip.HS16r1gx1gy1024.dead15.trip2"
    assert D.wgrad_name(256, Geom(9, 64, 256, 4), True, 4, 4) == "wgrad.strip.HS8gx1.many.capped"
    assert D.wgrad_name(256, Geom(2, 66, 256, 4), True, 4, 4) == "wgrad.run.RR2.V4tx1gx1.few"
    assert D.wgrad_name(256, Geom(2, 8, 8, 8), False, 8, 8) == "wgrad.seg.V1tx8gx1.one"
    assert D.wgrad_ws_query(256, Geom(2, 8, 8, 8)) == 9 * 8 * 4 + 256


def test_case_tables_contain_every_form_by_name():
    st = {D.stencil_name(g, 4, g.C, s) for g in D.RUN_SHAPES + D.STRIP_SHAPES + D.SUMS_CAP for s in (False, True)}
    have = lambda *parts: any(all(p in n for p in parts) for n in st)
    for rr in ("RR1", "RR2"):
        for lc in ("lc1gx1", "lc8gx1", "lc64gx2"):
            assert have("run." + rr + lc), (rr, lc)
    assert have("run.", "lc8", "dead3") and have("run.", "gx2", "dead63") and have("strip.", "gx2", "dead15") and have("strip.", "dead11")
    for r in ("HS16r1", "HS16+shortr1", "HS16+shortr2"):
        assert have("strip." + r), r
    assert have("run.", "gy1024", ".trip2") and have("strip.", "gy1024", ".trip2")
    assert D.stencil_name(Geom(2, 66, 8, 20), 4, 20, False).startswith("run.RR2")
    gen = {D.generic_name(g, F32, gap, off) for g, gap, off in D.GENERIC}
    assert any("fwd.V1+dgrad.V1+wgrad.seg.V1" in n for n in gen) and any("fwd.V4+dgrad.V4+wgrad.seg.V4" in n for n in gen)
    assert any("wgrad.refused" in n for n in gen)
    v1 = {(g.C, gap, off) for g, gap, off in D.GENERIC if "fwd.V1" in D.generic_name(g, F32, gap, off)}
    assert {(1, 0, False), (5, 0, False), (45, 0, False), (8, 0, True), (8, 1, False)} <= v1                  # V = 1 three ways
    v4 = {(g.s, g.d, g.W % 4) for g, gap, off in D.GENERIC if "fwd.V4" in D.generic_name(g, F32, gap, off)}
    assert {(2, 1, 0), (1, 2, 1), (1, 1, 2)} <= v4                                                          # V = 4 three ways
    caps = {(fn(g, BF16, g.C % 4 == 0, g.C)) for k, g in D.CAPS for fn in ((D.fwd_name,) if k == "fwd" else (D.dgrad_name,))}
    assert caps == {"fwd.V1.cap", "fwd.V4.cap", "dgrad.V1.cap", "dgrad.V4.cap"}
    for _, g in D.CAPS:
        assert g.N * g.H * g.W * g.C <= 17 * 10 ** 6
    wg = {D.wgrad_name(256, g, True, g.C, g.C) for g in D.WSTRIP_SHAPES + D.WSTRIP_MORE + D.WRUN_SHAPES + D.WRUN_MORE}
    for part in ("strip.HS4gx1.one", "strip.HS12gx", "strip.HS8+short", "strip.HS16gx", "strip.HS16+short", "gx2.few", ".many", ".many.capped",
                 "run.RR1.V4tx1gx1", "run.RR1.V4tx8gx1", "run.RR1.V4tx16gx2", "run.RR2."):
        assert any(part in n for n in wg), part
    # the forms a case runs: every <RELU, MASK, BN, SUMS> instantiation launch_dw_stencil can launch (DwForm), every <PRE, BN>
    assert {(bool(p), b is not None) for _, p, b in D.FWD_FORMS} == {(False, False), (True, False), (False, True)}
    assert {b for _, p, b in D.FWD_FORMS if b is not None} == {0, 1}
    assert {(bool(m), bool(s)) for m, r, s, q in D.DGRAD_FORMS} == {(False, False), (True, False), (False, True), (True, True)}
    assert {r for m, r, s, q in D.DGRAD_FORMS} == {0, 1, "inplace"} and any(s and q for m, r, s, q in D.DGRAD_FORMS)
    assert [n for n, _, _ in D.WGRAD_FORMS] == ["PRE0BN0", "PRE1BN0", "PRE0BN1", "PRE1BN1"]
    # behind the switches
    names = {D.env_label(e): D.child_names(e) for e in D.CHILD_ENVS}
    assert any("run.RR2" in n and "gy4" in n for n in names["SG_DW_FSTRIP=0 SG_DW_STRIP=0"])               # the run stencil at H = 64
    assert any(n.startswith("wgrad.run.RR2") for n in names["SG_DW_FSTRIP=0 SG_DW_STRIP=0"])
    assert all(".RR1" in n for n in names["SG_DW_FSTRIP=0 SG_DW_STRIP=0 SG_DW_RR=1"])
    assert all(n.startswith("wgrad.run.RR2") for n in names["SG_DW_STRIP=0 SG_DW_RR=2"])
    assert any("strip.HS8+shortr1" in n for n in names["SG_DW_FSTRIP=2"]) and any("strip.HS12r0" in n for n in names["SG_DW_FSTRIP=2"])
    assert any("strip.HS12r0" in n for n in names["SG_DW_FSTRIP=2 SG_DW_FSTRIP_HS=12"])
    assert any("strip.HS12+shortr1" in n for n in names["SG_DW_FSTRIP=2 SG_DW_FSTRIP_HS=12"])
    assert all("strip.HS4" in n for n in names["SG_DW_FSTRIP=2 SG_DW_FSTRIP_HS=6"])
    assert D.SW == D.switches_of(os.environ)


def _shifted(zp, w, H, W, flip=False):
    """The stride-1 3x3 stencil written out as nine shifted products (a restatement; the reference is F.conv2d)."""
    y = 0
    for a in range(3):
        for b in range(3):
            y = y + zp[:, a:a + H, b:b + W, :] * (w[2 - a, 2 - b] if flip else w[a, b])
    return y


def _pad1(z):
    return torch.nn.functional.pad(z, (0, 0, 1, 1, 1, 1))


def _restatement_inputs(C=8):
    g = Geom(2, 5, 8, C)
    x, dy, w = D.tensor(g, F32, "x").double(), D.tensor(g, F32, "dy").double(), D.taps(g).double()
    return g, x, dy, w


def test_planted_unflipped_taps_fail_the_dgrad_comparison():
    g, x, dy, w = _restatement_inputs()
    ref = dw_grads_ref(x, w, dy, g.geom, 1, 1, False, None, "dx")
    D.cmp(_shifted(_pad1(dy), w, g.H, g.W, flip=True).float(), ref, 2e-5, "cpu", "selfcheck", "dx", F32)
    with pytest.raises(AssertionError, match="max err"):
        D.cmp(_shifted(_pad1(dy), w, g.H, g.W, flip=False).float(), ref, 2e-5, "cpu planted", "selfcheck", "dx", F32)
    # ... and the filter gradient of the restatement agrees with autograd's
    dw = torch.stack([torch.stack([(_pad1(x)[:, a:a + g.H, b:b + g.W] * dy).sum((0, 1, 2)) for b in range(3)]) for a in range(3)])
    D.cmp(dw.float(), dw_grads_ref(x, w, dy, g.geom, 1, 1, False, None, "dw"), 1e-4, "cpu", "selfcheck", "dw", F32)


def test_planted_halo_row_from_the_neighbouring_image_fails_the_forward_comparison():
    g, x, dy, w = _restatement_inputs()
    ref = dw_conv_ref(x, w, g.geom, 1, 1)
    D.cmp(_shifted(_pad1(x), w, g.H, g.W).float(), ref, 2e-5, "cpu", "selfcheck", "y", F32)
    # the planted error: the two images stacked into one tall map, so the row above image 1 is the last row of image 0
    tall = _pad1(x.reshape(1, 2 * g.H, g.W, g.C))
    with pytest.raises(AssertionError, match="max err"):
        D.cmp(_shifted(tall, w, 2 * g.H, g.W).reshape(2, g.H, g.W, g.C).float(), ref, 2e-5, "cpu planted", "selfcheck", "y", F32)


def test_planted_padding_before_the_batchnorm_fails_the_forward_comparison():
    g, x, dy, w = _restatement_inputs()
    for relu in (0, 1):
        bn = D.bn_ref(g.C, relu)
        ref = dw_conv_ref(x, w, g.geom, 1, 1, False, bn)
        D.cmp(_shifted(_pad1(dw_input_ref(x, False, bn)), w, g.H, g.W).float(), ref, 2e-5, "cpu", "selfcheck", "y", F32)
        with pytest.raises(AssertionError, match="max err"):     # z = BN(0) at the border instead of 0
            D.cmp(_shifted(dw_input_ref(_pad1(x), False, bn), w, g.H, g.W).float(), ref, 2e-5, "cpu planted", "selfcheck", "y", F32)


def test_planted_dead_lane_in_the_sums_fails_the_comparison():
    g = Geom(2, 6, 8, 20)
    S = D.sums_inputs(g, F32)
    assert S.margin >= 1e-4 * S.zmax and 0.1 < S.on < 0.9          # the mask cuts through the data
    dx = D.dx_ref(g, F32, False)
    args = (S.bsx.double(), S.mean.double(), S.invstd.double(), S.gamma.double(), S.beta.double())
    for relu in (0, 1):
        dg, db = bn_sums_ref(dx, *args, relu)
        for ref in (dg, db):
            D.cmp(ref.float(), ref, 1e-4, "cpu", "selfcheck", "sums", F32)
            bad = ref.clone()
            bad[:4] *= 2          # the planted error: a lane past the last chunk walked chunk 0 and its sums were added as well
            with pytest.raises(AssertionError, match="max err"):
                D.cmp(bad.float(), ref, 1e-4, "cpu planted", "selfcheck", "sums", F32)


def test_checks_fire_on_a_strided_output():
    for dtype in DT:
        g = Geom(2, 3, 4, 8)
        y = D.tensor(g, dtype, "x")

        def fresh():
            o = D.vout(y.shape, dtype, gap=4, device="cpu")
            s, m, ld = o.start, o.mid, g.C + 4
            wide = o.dev[s:s + o.nb].view(dtype).reshape(-1, ld)
            wide[:, m:m + g.C] = y.reshape(-1, g.C)               # what a correct kernel leaves: the C columns written, nothing else
            return o, wide

        o, wide = fresh()
        o.check("clean")
        assert torch.equal(D.vread(o, "clean"), y)
        o, wide = fresh()
        wide[5, (o.mid + g.C) % (g.C + 4)] = 1.0                  # the planted error: one gap element overwritten
        with pytest.raises(AssertionError, match="gap columns"):
            D.vread(o, "planted")
        o, wide = fresh()
        wide[7, o.mid + 3] = float("nan")                         # ... one element of the operand left unwritten
        with pytest.raises(AssertionError, match="prefill"):
            D.vread(o, "planted")
        o, wide = fresh()
        o.dev[o.start + o.nb + 2] = 0                             # ... one byte behind the last row
        with pytest.raises(AssertionError, match="band behind"):
            o.fetch().check("planted")
    # an input view: NaN in the gap columns, the operand's own columns intact
    i = D.vin(torch.ones(2, 3, 4, 8), gap=4, device="cpu")
    w = i.read()
    assert torch.isnan(w[:, 8:]).all() and (w[:, :8] == 1).all() and w.shape == (24, 12)
    assert torch.equal(widen(torch.ones(3, 2), 5, 2)[:, 2:4], torch.ones(3, 2))
    gaps_keep_prefill(widen(torch.ones(3, 2), 5, 2), 2, 2)
    r = Guarded.out((4,), F32, "cpu")
    D.untouched(r, "clean")
    r.dev[r.start + 1] = 0
    with pytest.raises(AssertionError, match="refused"):
        D.untouched(r, "planted")


# ================================================================================================ the entry points (GPU)
@gpu
@pytest.mark.parametrize("g,gap,off,dtype", [pytest.param(g, gap, off, d, id=_ids(g, d, f"ld+{gap}{'-off' if off else ''}-" + D.generic_name(g, d, gap, off)))
                                             for g, gap, off in D.GENERIC for d in DT])
def test_generic_kernels(engine, g, gap, off, dtype):
    names = D.generic_case(engine, g, dtype, gap, off)
    want = D.generic_name(g, dtype, gap, off).split("+")
    assert {n.split(".PRE")[0] for n in names} == set(want), (names, want)


@gpu
@pytest.mark.parametrize("g,dtype", _stencil_params(D.RUN_SHAPES))
def test_run_stencil(engine, g, dtype):
    names = D.stencil_case(engine, g, dtype)
    assert all(".run.RR" in n for n in names), names


@gpu
@pytest.mark.parametrize("g,dtype", _stencil_params(D.STRIP_SHAPES))
def test_strip_stencil(engine, g, dtype):
    names = D.stencil_case(engine, g, dtype)
    assert all((".run.RR2" if g.H == 66 else ".strip.HS16") in n for n in names), names


@gpu
@pytest.mark.parametrize("g,dtype", [pytest.param(g, d, id=_ids(g, d, D.stencil_name(g, D.esize(d), g.C, True))) for g in D.SUMS_CAP for d in DT])
def test_sums_past_the_row_cap(engine, g, dtype):
    (name,) = D.stencil_case(engine, g, dtype, views=False, fwd_forms=(), dgrad_forms=D.SUMS_CAP_FORMS)
    assert "gy1024" in name and ".trip2" in name, name


@gpu
@pytest.mark.parametrize("g,dtype", _wgrad_params(D.WSTRIP_SHAPES + D.WSTRIP_MORE))
def test_wgrad_strips(engine, g, dtype):
    names = D.wgrad_case(engine, g, dtype)
    assert all(n.startswith("wgrad.strip.") for n in names), names


@gpu
@pytest.mark.parametrize("g,dtype", _wgrad_params(D.WRUN_SHAPES + D.WRUN_MORE))
def test_wgrad_run_reducer(engine, g, dtype):
    names = D.wgrad_case(engine, g, dtype)
    assert all(n.startswith("wgrad.run.RR") for n in names), names


@gpu
@pytest.mark.parametrize("kind,g", [pytest.param(k, g, id=f"{g.tag}-bf16-" + (D.fwd_name if k == "fwd" else D.dgrad_name)(g, BF16, g.C % 4 == 0, g.C))
                                    for k, g in D.CAPS])
def test_grid_cap_of_the_generic_kernels(engine, kind, g):
    assert D.cap_case(engine, kind, g).endswith(".cap")


@gpu
def test_plan_query_equals_the_mirrors(engine):
    """No launch: sg_dwconv2d_plan against plan_mirror over every shape of the case tables, both storages, the three directions,
    operands aligned or not, the dgrad with and without sums; and the two workspace queries against the plan's bytes."""
    shapes = [(g, 0) for g in D.RUN_SHAPES + D.STRIP_SHAPES + D.SUMS_CAP + D.WSTRIP_SHAPES + D.WSTRIP_MORE + D.WRUN_SHAPES + D.WRUN_MORE]
    shapes += [(g, gap) for g, gap, _ in D.GENERIC] + [(g, 0) for _, g in D.CAPS]
    families = set()
    for g, gap in dict.fromkeys(shapes):
        d = g.desc(gap, gap)
        wq = engine.lib.sg_dwconv2d_wgrad_ws_bytes(engine.h, CT.byref(d))
        sq = engine.lib.sg_dwconv2d_dgrad_bnsums_ws_bytes(engine.h, CT.byref(d))
        for dtype in DT:
            for direction in (D.FWD, D.DGRAD, D.WGRAD):
                for aligned in (0, 1):
                    for sums in ((0, 1) if direction == D.DGRAD else (0,)):
                        plan = D.checked_plan(engine, g, dtype, direction, aligned, sums, gap, gap)
                        families.add((direction, plan["family"]))
                        if direction == D.WGRAD and (g.KH, g.KW) == (3, 3):
                            assert wq >= plan["ws_bytes"] + 256, (g.tag, gap, aligned, wq, plan)
                        if sums:
                            assert sq == plan["ws_bytes"] + 256, (g.tag, gap, aligned, sq, plan)
    assert families == {(k, f) for k in (D.FWD, D.DGRAD, D.WGRAD) for f in (D.K_GENERIC, D.K_RUN, D.K_STRIP)}
    # a descriptor the entry points refuse: all-zero with their code
    rc, got = D.plan_query(engine, Geom(2, 6, 8, 8, KH=5), F32, D.WGRAD, 1)
    assert rc == D.SG_EINVAL and not any(got.values())


@gpu
@pytest.mark.parametrize("dtype", DT, ids=D.dname)
def test_refusals_leave_every_output_untouched(engine, dtype):
    D.refusal_case(engine, dtype)


@gpu
def test_forms_behind_switches_in_child_processes(engine):
    """SG_DW_FSTRIP, SG_DW_FSTRIP_HS, SG_DW_STRIP and SG_DW_RR are read once per process: fresh children run tests/_dw_cases.py, one
    environment after the other, against the same float64 references; the first child that fails ends the test."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dw_cases.py")
    for e in D.CHILD_ENVS:
        env = {k: v for k, v in os.environ.items() if k not in D.SWITCH_NAMES}
        env.update(e)
        label = D.env_label(e)
        try:
            r = subprocess.run([sys.executable, script], env=env, timeout=180, capture_output=True, text=True)
        except subprocess.TimeoutExpired as exc:
            pytest.fail(f"{label}: the child ran into its time limit: {exc}")
        assert r.returncode == 0, f"{label}: child exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-4000:]}"
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
        want = D.child_cases(e)
        assert len(lines) == len(want) and all(ln.startswith("CASE ok ") for ln in lines), f"{label}\n{r.stdout[-4000:]}"
        for ln, (lab, _, _, must) in zip(lines, want):
            assert lab in ln and must in ln, (label, ln, must)
        for ln in r.stdout.splitlines():
            if ln.startswith("REC "):
                _, form, qty, dn, rel, n = ln.split()
                key = (form + "@switch", qty, dn)
                D.RECORDS[key] = max(D.RECORDS.get(key, 0.0), float(rel.split("=")[1]))
                D.COUNTS[key] = D.COUNTS.get(key, 0) + int(n.split("=")[1])
        print("\n".join(f"{label}: {ln}" for ln in lines))


@gpu
def test_records_table(engine, capsys):
    """Not a check: the largest observed error / scale per kernel form of this run (tests/_dw_cases.RECORDS), printed."""
    with capsys.disabled():
        print("\n" + D.records_table())
