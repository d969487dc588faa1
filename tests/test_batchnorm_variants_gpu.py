"""Every variant of the BatchNormalization kernels (csrc/norm.hip) and of the column sums built on csrc/sg_reduce.h in
csrc/conv_thin.hip (sg_bias_grad, sg_bn_train_fwd_tiles) against plain float64 torch on the CPU, through the C ABI itself.
The companion of tests/test_bandwidth_variants_gpu.py, with its machinery: operands are tests/_guarded.py arenas (NaN guard
bands, NaN-prefilled outputs, inputs whose bits must survive, workspaces of exactly the queried size), their start 16-byte
aligned or one element further.  The cases themselves are tests/_bn_cases.py (also run as a program, for the forms behind
process-wide switches).

Every case id ends in the kernels the launch takes at 256 CUs, from the mirrors of plan_bn, seg_plan and bn_cols_grid:
    V<lanes' channels>tx<TX>gx<column blocks>.<one|few|many row slabs>[+short last slab].<fused|fin4|fin16 finalize>
    .<cols|flat><V of the apply pass>[p<rows per period>b<blocks per period>k<period groups>]
and before it launches the case asserts (B.checked_plan) that the ENGINE's plan for this device's CU count - sg_bn_plan, or
sg_seg_plan for the column sums - equals the mirror in every field and spells the same string.  Where to find what:
    V = 1 / 4 / 8 in reduce and apply          c45 / c64-f32 / c64-bf16, c72-bf16; bf16 V = 4-not-8: c20-bf16
    column and flat apply forms                 cols*: every C % 4 == 0 case; flat1: c1, c45, every "-off"; flat4 / flat8: the child
    mask modes 0 / 1 / 2                        every test_train_bwd case runs the three (1 and 2 bit-identical)
    row-split regimes, 4- and 16-lane finalize  .one.fused / .few.fin4 / .many.fin16; 4 lanes behind S >= 32: the child
    offset operands                             "-off" ids; one operand only: test_one_unaligned_operand_of_several
    ld forms of the bias gradient               test_bias_grad[dense | slice | odd | offset]
    tile regimes                                test_train_fwd_tiles (rows < 128, ragged, one / few / many tiles, offset)

Inputs: one constant channel everywhere (C >= 2); x = 1000 + N(0, 1) ("mean1000") beside an ordinary one; the pivot row at 4 and
16 sigma; beta in the widest gap of -gamma * xhat so that the whole tensor is compared under a fused ReLU.
Tolerances, as max|got - ref| <= tol * max|ref|: 2e-5 fp32 element-wise and statistics, 1e-4 fp32 reduced (dx, dgamma, dbeta,
bias gradient, tile statistics, everything at the 16-sigma pivot), 2^-7 bf16-stored; y of the training forward may add
|gamma| invstd ulp32(mean) / 2 per channel (save_mean is an fp32 number).  The constant channel (invstd = 1 / sqrt(eps)) is
compared on its own scale where it would otherwise set everyone's."""
import ctypes as CT
import os
import subprocess
import sys

import pytest
import torch

import _bn_cases as B
from _bn_cases import BF16, F32
from _guarded import bn_cols_grid, close_cols, regime, seg_plan, seg_plan_s, short_last_slab, tile_stats_ref, bn_stats_ref

gpu = pytest.mark.gpu


def _params(shapes, off, **kw):
    out = []
    for C, rows in shapes:
        for dtype in (F32, BF16):
            name = B.plan(B.REF_CUS, rows, C, dtype, off, **kw)
            out.append(pytest.param(C, rows, dtype, off, id=f"c{C}r{rows}-{B.dname(dtype)}{'-off' if off else ''}-{name}"))
    return out


FWD = _params(B.SHAPES, False) + _params(B.OFF_SHAPES, True)
BWD = _params(B.SHAPES, False, pass_=B.BWD) + _params(B.OFF_SHAPES, True, pass_=B.BWD)


# ================================================================================================ harness self-checks (CPU)
def test_plan_mirrors_agree_with_hand_computed_values_at_256_cus():
    P = lambda rows, C, vec, w8=False, nout=2: tuple(seg_plan(256, rows, C, vec, w8, nout)[k] for k in ("V", "TX", "TY", "gx", "S"))
    # C = 64 fp32: 16 chunks, TX = TY = 16, one column block; S = ceil(rows / 64) once rows > 16 TY = 256
    assert P(256, 64, True) == (4, 16, 16, 1, 1) and P(130, 64, True)[4] == 1
    assert P(520, 64, True) == (4, 16, 16, 1, 9) and short_last_slab(520, 9)        # 8 slabs of 58 rows and one of 56
    assert P(4100, 64, True) == (4, 16, 16, 1, 65) and short_last_slab(4100, 65)    # 64 slabs of 64 rows and one of 4
    # ... bf16: 8 chunks, TX = 8, TY = 32; S = ceil(rows / 128) once rows > 512
    assert P(256, 64, True, True) == (8, 8, 32, 1, 1) and P(520, 64, True, True)[4] == 5 and P(4100, 64, True, True)[4] == 33
    # ... through offset pointers: 64 chunks, four column blocks
    assert P(520, 64, False) == (1, 16, 16, 4, 9)
    assert P(67, 1, False) == (1, 1, 256, 1, 1) and P(67, 4, True) == (4, 1, 256, 1, 1)
    assert P(67, 20, True, True) == (4, 8, 32, 1, 1)          # bf16, C % 8 = 4: four channels per lane
    assert P(67, 45, False) == (1, 16, 16, 3, 1)
    assert P(67, 68, True) == (4, 16, 16, 2, 1)               # 17 chunks: the second column block has one live lane
    assert P(67, 72, True, True) == (8, 16, 16, 1, 1)         # 9 chunks in a block of 16
    assert P(1992, 728, True) == (4, 16, 16, 12, 32) and P(1992, 728, True, True)[3] == 6
    assert P(4100, 64, True, True, 9)[0] == 4                 # NOUT > 2 never takes eight
    assert seg_plan(256, 520, 64, True, nout=2)["part_bytes"] == 9 * 2 * 64 * 4
    assert seg_plan_s(256, 4100, 64, True) == 65 and seg_plan_s(256, 4100, 64, True, True, 2) == 33
    assert [regime(s) for s in (1, 2, 31, 32)] == ["one", "few", "few", "many"]
    # bn_cols_grid: (prow, b0, k)
    assert bn_cols_grid(256, 520, 16, 4) == (16, 1, 9)        # C = 64 fp32: gcd(256, 16) = 16; k = ceil(520 / (4 * 16))
    assert bn_cols_grid(256, 67, 5, 4) == (256, 5, 1)         # C = 20
    assert bn_cols_grid(256, 1992, 182, 4) == (128, 91, 4)    # C = 728 fp32
    assert bn_cols_grid(256, 1992, 91, 1) == (256, 91, 8)     # C = 728 bf16, the backward's grid
    assert bn_cols_grid(256, 1 << 20, 16, 1) == (16, 1, 2048) and bn_cols_grid(256, 10, 16385 * 3, 1) is None
    # every row of the tables, by name
    for C, rows in B.SHAPES:
        for dtype in (F32, BF16):
            assert B.plan(256, rows, C, dtype, False).count(".") == 3
    names = {(B.dname(d), B.plan(256, r, C, d, off)) for C, r in B.SHAPES for d in (F32, BF16) for off in (False,)}
    names |= {(B.dname(d), B.plan(256, r, C, d, True)) for C, r in B.OFF_SHAPES for d in (F32, BF16)}
    have = lambda dn, *parts: any(n == dn and all(p in s for p in parts) for n, s in names)
    for v, dn in (("V1tx", "f32"), ("V4tx", "f32"), ("V1tx", "bf16"), ("V4tx", "bf16"), ("V8tx", "bf16")):
        for reg in (".one.fused", ".few", ".many"):
            assert have(dn, v, reg), (v, dn, reg)
    assert have("f32", "+short.fin4") and have("f32", "+short.fin16") and have("bf16", ".cols8") and have("bf16", ".cols4")
    assert have("f32", ".cols4p16b1") and have("f32", "cols4p256b5") and have("f32", "cols4p128b91") and have("f32", ".flat1")


def test_planted_unpivoted_variance_fails_the_forward_comparison():
    """Statistics from the un-pivoted single-pass fp32 formula on x = 1000 + N(0, 1) must fail compare_forward; the pivoted form in
    the same fp32 arithmetic passes it."""
    for rows in (520, 4100):
        I = B.inputs(64, rows, F32, "mean1000")
        x = I.x                                               # fp32
        n = torch.tensor(float(rows))

        def run(mean, var):
            invstd = (1.0 / torch.sqrt(var.double() + B.EPS)).float()
            y = ((x - mean) * invstd) * I.gamma + I.beta
            mm = I.mm * B.MOMENTUM + mean * (1 - B.MOMENTUM)
            mv = I.mv * B.MOMENTUM + var * (1 - B.MOMENTUM)
            B.compare_forward(I, y, mean, invstd, mm, mv, 0, 0, "cpu", entry="selfcheck")

        d = x - x[0]                                          # pivot = row 0, fp32 throughout
        m1 = d.sum(0) / n
        run(x[0] + m1, ((d * d).sum(0) / n - m1 * m1).clamp_min(0))
        m = x.sum(0) / n                                      # the planted error: E[x^2] - E[x]^2 in fp32
        with pytest.raises(AssertionError, match="max err"):
            run(m, ((x * x).sum(0) / n - m * m).clamp_min(0))


def test_mask_gap_construction_yields_its_margin():
    for C, rows, dtype, kind in ((64, 4100, F32, "plain"), (64, 4100, F32, "mean1000"), (64, 520, BF16, "plain"),
                                 (64, 520, BF16, "mean1000"), (1, 31752, F32, "plain"), (64, 1, F32, "plain"),
                                 (64, 3, BF16, "plain"), (72, 264, F32, "pivot16")):
        I = B.inputs(C, rows, dtype, kind)                    # (asserts the margin itself)
        assert I.margin >= 1e-4 * I.ymax
        if I.cc is not None:
            assert abs(float(I.beta[I.cc])) >= 2.0 ** -7 and float(I.var[I.cc]) == 0.0
        if rows >= 100:
            on = I.mask.double().mean(0)
            keep = torch.ones(C, dtype=torch.bool)
            if I.cc is not None:
                keep[I.cc] = False
            assert ((on[keep] > 0) & (on[keep] < 1)).float().mean() > 0.8    # the masks cut through the data, not past it
    # a beta ON a value fails the same assertion
    v = torch.tensor([0.0, 1.0, 1.5, 4.0], dtype=torch.float64)
    assert B.gap_beta(v, 1.2, 1e-3) == 1.25 and B.gap_beta(v, 2.9, 1e-3) == 2.75 and B.gap_beta(v, 1.2, 0.3) == 0.5


def test_column_comparison_and_tile_statistics_helpers():
    ref = torch.tensor([[1.0, 30.0, -2.0], [0.5, -30.0, 1.0]], dtype=torch.float64)
    bad = ref.clone()
    bad[0, 0] += 1e-3                                         # inside 1e-4 * 30, outside 1e-4 * 2
    close_cols(bad, ref, 1e-4, "one scale")
    with pytest.raises(AssertionError, match="max err"):
        close_cols(bad, ref, 1e-4, "apart", apart=(1,))
    close_cols(bad, ref, 1e-4, "allowance", apart=(1,), extra=torch.tensor([1e-3, 0.0, 0.0]))
    seen = []
    with pytest.raises(AssertionError):
        close_cols(bad, ref, 1e-4, "report", apart=(1,), report=seen.append)
    assert len(seen) == 1 and abs(seen[0] - 1e-3 / 2.0) < 1e-12
    with pytest.raises(AssertionError, match="non-finite"):
        close_cols(torch.tensor([[float("nan")]]), torch.tensor([[1.0]]), 1.0)
    # per-tile (sum, centred sum of squares) combine to the statistics of the whole: Chan's formula in float64
    x = torch.randn(300, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) + 7
    st = tile_stats_ref(x, 128)
    assert st.shape == (3, 2, 5)
    cnt = torch.tensor([128.0, 128.0, 44.0], dtype=torch.float64)[:, None]
    mean, var = bn_stats_ref(x)
    m = st[:, 0].sum(0) / 300
    assert torch.allclose(m, mean, rtol=1e-14, atol=0)
    assert torch.allclose((st[:, 1] + cnt * (st[:, 0] / cnt - m) ** 2).sum(0) / 300, var, rtol=1e-12, atol=0)
    s32, m64, v64 = B.tile_inputs(45, 3 * B.BM + 1, "mean1000")
    assert s32.shape == (4, 2, 45) and s32.dtype == torch.float32 and abs(float(m64[0]) - 1000) < 0.5 and abs(float(v64[0]) - 1) < 0.3


def test_child_subset_takes_the_switched_forms():
    # what the child asserts for itself, here from the mirrors with the switches as the child sees them
    assert len(B.child_cases()) == len(B.CHILD_SHAPES) * 2 * 4
    assert any(seg_plan_s(256, r, C, True, True, 2) >= 32 for C, r in B.CHILD_SHAPES)
    assert all(C % 4 == 0 for C, _ in B.CHILD_SHAPES) and {C % 8 for C, _ in B.CHILD_SHAPES} == {0, 4}


# ================================================================================================ the entry points (GPU)
@gpu
@pytest.mark.parametrize("C,rows,dtype,off", FWD)
def test_train_fwd(engine, C, rows, dtype, off):
    for kind in B.kinds_for(C, dtype):
        B.fwd_case(engine, C, rows, dtype, off, kind)


PIVOT_SHAPES = [(64, 17), (64, 256), (64, 520), (64, 4100), (45, 264), (72, 264), (72, 1992)]


@gpu
@pytest.mark.parametrize("k", (4, 16))
@pytest.mark.parametrize("C,rows,dtype,off", _params(PIVOT_SHAPES, False) + _params([(64, 520)], True))
def test_train_fwd_pivot_row_is_an_outlier(engine, C, rows, dtype, off, k):
    """Row 0 - the pivot of the single-pass variance - at k sigma: k = 4 at the element-wise tolerance, k = 16 at the reduced one."""
    B.fwd_case(engine, C, rows, dtype, off, f"pivot{k}")


@gpu
@pytest.mark.parametrize("C,rows,dtype,off", BWD)
def test_train_bwd(engine, C, rows, dtype, off):
    for kind in B.kinds_for(C, dtype):
        B.bwd_case(engine, C, rows, dtype, off, kind)


@gpu
@pytest.mark.parametrize("C,rows,dtype,off", BWD)
def test_train_bwd_apply(engine, C, rows, dtype, off):
    for kind in B.kinds_for(C, dtype):
        B.bwd_apply_case(engine, C, rows, dtype, off, kind)


@gpu
@pytest.mark.parametrize("C,rows,dtype,off", FWD)
def test_apply_and_infer(engine, C, rows, dtype, off):
    for kind in B.kinds_for(C, dtype):
        B.apply_case(engine, C, rows, dtype, off, kind)


@gpu
@pytest.mark.parametrize("dtype", (F32, BF16), ids=B.dname)
def test_one_unaligned_operand_of_several(engine, dtype):
    # C % 8 == 0 and every tensor but ONE aligned: `vec` must fall to the scalar kernels for all of them
    for which in ("x", "y"):
        B.fwd_case(engine, 64, 130, dtype, True, "plain", off_only=which)
    for which in ("x", "dy", "dx", "y"):
        B.bwd_case(engine, 64, 130, dtype, True, "plain", off_only=which)


def _add2_params():
    return [pytest.param(C, rows, d, id=f"c{C}r{rows}-{B.dname(d)}-{B.add2_plan(B.REF_CUS, rows, C, d)}")
            for C, rows in B.ADD2_SHAPES for d in (F32, BF16)]


@gpu
@pytest.mark.parametrize("C,rows,dtype", _add2_params())
def test_add2_bn(engine, C, rows, dtype):
    for kind in B.kinds_for(C, dtype):
        B.add2_case(engine, C, rows, dtype, kind)


@gpu
@pytest.mark.parametrize("dtype", (F32, BF16), ids=B.dname)
def test_add2_bn_refuses_what_it_has_no_kernel_for(engine, dtype):
    B.add2_refusal_case(engine, dtype)


@gpu
@pytest.mark.parametrize("form", ("dense", "slice", "odd", "offset"))
@pytest.mark.parametrize("dtype", (F32, BF16), ids=B.dname)
def test_bias_grad(engine, dtype, form):
    seen = {B.bias_case(engine, C, rows, dtype, form) for C, rows in B.BIAS_SHAPES}
    want = {"dense": ("V4", "V1"), "slice": ("V4", "V1"), "odd": ("V1",), "offset": ("V1",)}[form]
    assert {n[:2] for n in seen} == set(want), seen
    assert {n.split(".")[1].split("+")[0] for n in seen} == {"one", "few", "many"}, seen


def _tile_params():
    out = []
    for C, rows in B.TILE_SHAPES:
        for off in (False, True):
            tiles = -(-rows // B.BM)
            name = B.seg_name(seg_plan(B.REF_CUS, tiles, C, C % 4 == 0 and not off, nout=2), tiles)
            out.append(pytest.param(C, rows, off, id=f"c{C}r{rows}{'-off' if off else ''}-{name}"))
    return out


@gpu
@pytest.mark.parametrize("C,rows,off", _tile_params())
def test_train_fwd_tiles(engine, C, rows, off):
    for dtype in (F32, BF16):          # names the activations' storage; the statistics are fp32 either way
        for kind in ("plain", "mean1000"):
            B.tiles_case(engine, C, rows, dtype, off, kind)


@gpu
def test_forms_behind_switches_in_a_child_process(engine):
    """SG_BN_COLS=0 (the flat V = 4 / V = 8 apply and backward-apply kernels on shapes the column forms would take) and
    SG_FINALIZE_LANES=4 (four finalize lanes behind S >= 32) are read once per process: a fresh child runs tests/_bn_cases.py,
    the aligned vectorisable subset against the same float64 references, one line per case."""
    env = dict(os.environ)
    env.update(B.CHILD_ENV)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_bn_cases.py")
    try:
        r = subprocess.run([sys.executable, script], env=env, timeout=240, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"the child ran into its time limit: {e}")
    assert r.returncode == 0, f"child exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
    assert len(lines) == len(B.child_cases()) and all(ln.startswith("CASE ok ") for ln in lines), r.stdout[-4000:]
    assert any(".flat4" in ln for ln in lines) and any(".flat8" in ln for ln in lines) and any(".many" in ln and ".fin4" in ln for ln in lines)


@gpu
def test_plan_queries_equal_the_mirrors(engine):
    """sg_bn_plan and sg_seg_plan against the mirrors over every shape of the tables, both storage types, every pass, aligned or not;
    the three workspace queries against what the engine's own plans add up to; the refusals.  Launches nothing."""
    cus, lib, h = B.num_cus(engine), engine.lib, engine.h
    tiles = [(C, -(-rows // B.BM)) for C, rows in B.TILE_SHAPES]
    shapes = sorted(set(B.SHAPES + B.OFF_SHAPES + B.ADD2_SHAPES + B.BIAS_SHAPES + B.TILE_SHAPES + tiles + PIVOT_SHAPES))
    for C, rows in shapes:
        bn_need = 0
        for dtype in (F32, BF16):
            for aligned in (False, True):
                for pass_ in (B.FWD, B.APPLY, B.BWD, B.BWD_APPLY, B.ADD2):
                    what = f"sg_bn_plan rows={rows} C={C} {B.dname(dtype)} pass={pass_} aligned={int(aligned)}"
                    rc, got = B.plan_query(engine, rows, C, dtype, pass_, aligned)
                    want = B.plan_mirror(cus, rows, C, dtype, pass_, aligned)
                    if want is None:          # sg_add2_bn refuses: all-zero with its code
                        assert pass_ == B.ADD2 and (C % 4 != 0 or not aligned), what
                        assert rc == B.SG_EUNSUPPORTED and not any(got.values()), (what, rc, got)
                        continue
                    assert rc == 0, (what, rc)
                    B._same(what, got, want)
                    if pass_ == B.FWD:
                        bn_need = max(bn_need, got["ws_bytes"])
                    assert (got["ws_bytes"] > 0) == (pass_ in (B.FWD, B.BWD)), (what, got)
        assert lib.sg_bn_ws_bytes(h, rows, C) == bn_need + 256, (rows, C)
        part = {}
        for nout in (1, 2, 9):
            for vec in (False, True):
                for wide8 in (False, True):
                    what = f"sg_seg_plan nout={nout} rows={rows} C={C} vec={int(vec)} wide8={int(wide8)}"
                    rc, got = B.seg_query(engine, nout, rows, C, vec, wide8)
                    assert rc == 0, (what, rc)
                    B._same(what, got, seg_plan(cus, rows, C, vec, wide8, nout))
                    part[nout, vec, wide8] = got["part_bytes"]
        assert lib.sg_bias_grad_ws_bytes(h, rows, C) == max(part[1, True, False], part[1, False, False]) + 256, (rows, C)
        assert lib.sg_bn_tiles_ws_bytes(h, rows, C) == part[2, True, False] + part[2, False, False], (rows, C)
        rc, got = B.seg_query(engine, 2, rows, C, True, nseg=3)
        assert rc == 0 and got["part_bytes"] == 3 * seg_plan(cus, rows, C, True, nout=2)["part_bytes"]
    # what the entry points answer SG_EINVAL to: all-zero with that code
    p = B.BnPlan()
    bad = [(h, 0, 0, 64, B.FWD), (h, 0, 130, 0, B.BWD), (h, 0, -1, 64, B.APPLY), (h, 7, 130, 64, B.FWD), (h, 0, 130, 64, 5),
           (h, 0, 130, 64, -1), (None, 0, 130, 64, B.FWD), (h, 0, 1 << 25, 64, B.FWD), (h, 1, 1 << 25, 64, B.BWD_APPLY)]
    for ctx, dt, rows, C, pass_ in bad:
        CT.memset(CT.byref(p), 0xFF, CT.sizeof(p))
        assert lib.sg_bn_plan(ctx, dt, rows, C, pass_, 1, CT.byref(p)) == B.SG_EINVAL, (dt, rows, C, pass_)
        assert not any(getattr(p, n) for n in B.BN_FIELDS), (dt, rows, C, pass_)
    # ... which sg_add2_bn walks in row chunks: the plan of one full chunk (an even number of rows below 2^31 elements)
    rc, got = B.plan_query(engine, 1 << 25, 64, F32, B.ADD2, True)
    assert rc == 0
    B._same("add2 chunk", got, B.plan_mirror(cus, (((1 << 31) - 1) // 64) & ~1, 64, F32, B.ADD2, True))
    assert lib.sg_bn_plan(h, 0, 130, 64, B.FWD, 1, None) == B.SG_EINVAL
    s = B.SegPlan()
    for ctx, nout, nseg, rows, C in ((None, 1, 1, 130, 64), (h, 0, 1, 130, 64), (h, 1, 0, 130, 64), (h, 1, 1, 0, 64), (h, 1, 1, 130, 0)):
        CT.memset(CT.byref(s), 0xFF, CT.sizeof(s))
        assert lib.sg_seg_plan(ctx, nout, nseg, rows, C, 1, 0, CT.byref(s)) == B.SG_EINVAL
        assert not any(getattr(s, n) for n in B.SEG_FIELDS)
