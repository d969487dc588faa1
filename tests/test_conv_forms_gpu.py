"""Every kernel form of the forward convolution and of the input gradient (sg_conv2d_fwd, sg_conv2d_dgrad: csrc/conv_igemm.hip with
conv_native.hip, conv_thin.hip, conv_x6.h, conv_x6p.h, conv_x6w.h, conv_b16.h, conv_b16w.h and the forward / dgrad half of conv_pw.h) against float64, through the C
ABI on guarded operands.  The tables, the mirror of the dispatch rules, the reference and the runner are tests/_conv_cases.py; a
case id ends in the name of the form its launch takes, asserted against the mirror and against sg_conv2d_plan before anything
is launched.

The first tests need no GPU: the mirror against values worked out by hand, the tables against the mirror at 256 CUs, and the list
of forms that must keep a case.  The process-wide switches run in child processes, one after another."""
import os
import subprocess
import sys
import time

import pytest
import torch

import _conv_cases as CC
from _conv_cases import CASES, SLICE_CASES, SUB_CASES, Geom, View

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240     # seconds per child process (its cases take well under a minute on an MI355X)


# ================================================================================================ CPU self-checks
def test_pick_bn_by_hand():
    # pick_bn's own example at 256 CUs: M = 16384, N = 728.  128-wide: 128 x 6 = 768 tiles = 3 rounds exactly, columns 728 / 768;
    # 64-wide: 128 x 12 = 1536 tiles = 6 rounds exactly, columns 728 / 768, times 0.93 -> 128
    assert CC.pick_bn(16384, 728, 256) == 128
    assert CC.pick_bn(10 ** 6, 32, 256) == 32 and CC.pick_bn(10 ** 6, 33, 256) == 64 and CC.pick_bn(10 ** 6, 64, 256) == 64
    # fewer tiles than CUs: eff = tiles / 256 * fill, so the 64-wide tile's doubled count wins unless its fill is under 1 / 1.86
    assert CC.pick_bn(1920, 96, 256) == 64          # 15 x 1 x (96/128) = 11.25 against 15 x 2 x (96/128) x 0.93 = 20.9
    assert CC.pick_bn(16384, 256, 256) == 128       # 256 tiles = one round against 512 = two rounds at 0.93
    assert CC.pick_bn(16384 - 128, 256, 256) == 128 # 254 / 256 of a round against 508 / 512 at 0.93
    assert CC.pick_bn(8192, 192, 256) == 64         # 128-wide: 128 tiles / 256 x 192 / 256 = 0.375; 64-wide: 192 / 256 x 1 x 0.93 = 0.70
    assert CC.pick_bn(16384, 192, 256) == 128       # 256 / 256 x 0.75 = 0.75 against 384 / 512 x 1 x 0.93 = 0.70


def _view(g, dgrad=False, eb=4):
    return View(g, dgrad, eb)


def test_share_rules_by_hand():
    # x6w: 32 x 64 map, 256 -> 256 3x3: K = 2304 >= 2048, one column tile, 2048 / 128 = 16 workgroups -> one share
    assert CC.x6w_shares(_view(Geom(1, 32, 64, 256, 256))) == 1
    # 32 x 32 map, 512 -> 256: 8 workgroups, K / 2 = 2304 >= 2048 -> two shares; at 256 channels K / 2 = 1152 -> none
    assert CC.x6w_shares(_view(Geom(1, 32, 32, 512, 256))) == 2
    assert CC.x6w_shares(_view(Geom(1, 32, 32, 256, 256))) == 0
    assert CC.x6w_shares(_view(Geom(1, 32, 64, 256, 160))) == 0      # 160 / 256 < 0.75
    assert CC.x6w_shares(_view(Geom(1, 32, 64, 2304, 256, k=1))) == 0   # one tap
    assert CC.x6w_shares(_view(Geom(1, 24, 24, 256, 256))) == 0      # 576 pixels: no whole 128-pixel tiles


def test_share_rules_b16w_by_hand():
    # workgroups per image = column tiles x pixels / 256; shares = 16 / workgroups, at most 4, each at least 2048 deep, 16 in all
    b = lambda g: CC.b16w_shares(_view(g, eb=2))
    assert b(Geom(1, 64, 64, 64, 256)) == 0          # K = 576 < 1024
    assert b(Geom(1, 64, 64, 128, 256)) == 1         # 16 workgroups
    assert b(Geom(1, 32, 64, 512, 256)) == 2         # 8 workgroups, 2 shares of 2304
    assert b(Geom(1, 32, 32, 768, 256)) == 0         # 4 workgroups: 4 shares would be 1728 deep, 3 are 2304 - but 4 x 3 = 12 < 16
    assert b(Geom(1, 32, 32, 1024, 256)) == 4        # 4 shares of 2304, 4 x 4 = 16
    assert b(Geom(1, 32, 32, 256, 256)) == 0         # K = 2304: one share only
    assert b(Geom(1, 24, 24, 1024, 64)) == 0         # 64 / 256 columns; 576 pixels


def test_three_shares_are_out_of_the_rules_reach():
    """b16w_S = 3 cannot occur: 16 // workgroups = 3 only at 5 workgroups (15 < 16), and 4 shares cut back to 3 by the 2048-deep
    rule leave 4 x 3 = 12 < 16.  Swept here so that a change of the rule that makes 3 reachable also asks for its case."""
    seen = set()
    for hw in ((16, 16), (16, 32), (32, 32), (32, 48), (32, 64), (48, 48), (64, 64), (16, 80), (16, 96), (16, 112)):
        for cin in (64, 128, 256, 512, 768, 1024, 2048):
            for cout in (192, 256, 448, 512, 768):
                for k in (1, 3):
                    seen.add(CC.b16w_shares(_view(Geom(1, hw[0], hw[1], cin, cout, k=k), eb=2)))
    assert seen == {0, 1, 2, 4}


def test_pw_wide_width_by_hand():
    w = lambda rows, k, n: CC.pw_wide_width(_view(Geom(1, rows // 64, 64, k, n, k=1)))
    assert w(16384, 728, 728) == 384       # 128 x 2 = 256 tiles: one round of 384; 256-wide: 384 tiles = 2 rounds of 256 = 512
    assert w(16384, 1024, 1024) == 256     # 384-wide: 1024 / 1152 fill ok, 384 tiles = 2 rounds x 384 = 768; 256-wide: 512 tiles = 2 x 256
    assert w(16384, 256, 256) == 0         # 384: 256 / 384 < 0.75; 256: 128 tiles < 192
    assert w(6144, 256, 384) == 384 and w(6144 - 64, 256, 384) == 0
    assert w(6144, 248, 384) == 0          # K < 256


def test_small_rules_by_hand():
    assert CC.b16_ks(64, False) == 4 and CC.b16_ks(96, False) == 2 and CC.b16_ks(32, False) == 2 and CC.b16_ks(200, True) == 4
    assert CC.b16_pd(_view(Geom(1, 24, 24, 1024, 64), eb=2)) == 2          # forward, K = 9216
    assert CC.b16_pd(_view(Geom(1, 24, 24, 64, 1024), True, eb=2)) == 1    # the same layer's dgrad
    assert CC.b16_pd(_view(Geom(1, 24, 24, 512, 64), eb=2)) == 1           # K = 4608
    assert CC.x6_var(768, 256) == 1 and CC.x6_var(769, 256) == 0
    with CC.switched({"SG_X6_VARIANT": "0"}):
        assert CC.x6_var(1, 256) == 0
    assert CC.thin_ok(Geom(2, 9, 7, 32, 2, k=1)) and not CC.thin_ok(Geom(2, 9, 7, 12, 2, k=1)) and not CC.thin_ok(Geom(2, 9, 7, 32, 5, k=1))
    g = Geom(3, 32, 32, 192, 192)
    assert CC.images_per_2gib(g, 4, 4) == 3
    with CC.switched({"SG_CONV_MAX_BYTES": str(2 << 20)}):
        assert CC.images_per_2gib(g, 4, 4) == 2        # 786432 bytes per image: two fit 2 MiB
        assert CC.images_per_2gib(Geom(1, 64, 64, 256, 256), 4, 4) == 0
    # plan_common: the grouped order from four column tiles on, 16 rows per group up to 16 MiB of A, the K order above 2 MiB per image
    v = _view(Geom(1, 64, 64, 256, 200))
    assert CC.plan_common(v, True, 64, True, 4) == (0, 16, 4)
    v = _view(Geom(1, 32, 32, 256, 200))
    assert CC.plan_common(v, True, 64, True, 4) == (0, 16, 0)
    v = _view(Geom(1, 128, 96, 512, 256, k=1))
    assert CC.plan_common(v, True, 64, True, 4) == (0, 8, 0)


def _all_cases():
    return CASES + SLICE_CASES


@pytest.mark.parametrize("c", _all_cases(), ids=[c.id for c in _all_cases()])
def test_tables_name_what_the_mirror_names(c):
    assert c.mirror_name() == c.name
    r = c.mirror_res_name()
    assert r == (c.name if c.res == "" else c.res)


def test_sub_batch_table_names_what_the_mirror_names():
    with CC.switched(CC.CHILD_ENVS["sub"]):
        for c in SUB_CASES:
            assert c.mirror_name() == c.name, c.id


def test_tables_contain_every_form_by_name():
    assert CC.missing_forms() == []
    # the condition bites: names are matched whole (up to the modifiers), so a form is not covered by a longer one
    names = CC.all_case_names()
    assert CC.missing_forms([n for n in names if ".PD2" not in n]) == ["fwd.slab.b16.BN64.KS4.PD2"]
    assert CC.missing_forms([n for n in names if ".gm8" not in n]) == [".gm8"]
    assert CC.missing_forms([n for n in names if CC.base_of(n) != "fwd.thin.CO2.b16"]) == ["fwd.thin.CO2.b16"]      # (b16>f32 stays)
    assert CC.missing_forms([n for n in names if CC.base_of(n) != "fwd.native.BN64.vec"]) == ["fwd.native.BN64.vec"]
    assert CC.missing_forms([n for n in names if CC.base_of(n) != "dgrad.patch.C64m.BN128"]) == ["dgrad.patch.C64m.BN128"]
    assert "bnb" in CC.missing_forms(extras={"pin"})
    ids = [c.id for c in _all_cases() + SUB_CASES]
    assert len(ids) == len(set(ids)), "two cases share an id"


def test_child_tables():
    with CC.switched(CC.CHILD_ENVS["v0"]):
        v0 = CC.child_cases("v0")
        assert len(v0) >= 20 and all(".v0" in c.name or (c.res and ".v0" in c.res) for c in v0)
    with CC.switched(CC.CHILD_ENVS["ab"]):
        ab = CC.child_cases("ab")
        names = [c.name for c in ab]
        assert not any(".mf16" in n or ".perm2" in n or ".slab.b16" in n for n in names)
        assert any(".npl1" in n for n in names)      # bf16 storage on the one-plane x6 kernel


# ================================================================================================ GPU cases
CHILD_RECORDS = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """With CONV_FORMS_RECORD=<path> in the environment: every record of this run (RECORDS of this process, then each child's), one
    line per launch and output with its bound, written when the module's tests are over (profiles/conv_forms_gpu.txt)."""
    yield
    path = os.environ.get("CONV_FORMS_RECORD")
    if path and CC.RECORDS:
        with open(path, "w") as f:
            f.write(CC.records_table() + "\n")
            for child, lines in CHILD_RECORDS.items():
                env = " ".join(f"{k}={v}" for k, v in CC.CHILD_ENVS[child].items())
                f.write(f"# child {child}: {env}\n" + "\n".join(lines) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("c", _all_cases(), ids=[c.id for c in _all_cases()])
def test_every_form_against_fp64(engine, c):
    CC.run_case(engine, c)


@pytest.mark.gpu
def test_refused_combinations_leave_everything_untouched(engine):
    """What the header says is refused: its documented code, and y / dx, statistics and workspace bands untouched (the runner checks
    the latter for every refused call)."""
    assert not CC.FAULTED, CC.FAULTED
    by = {c.name: c for c in CASES}
    for name in ("dgrad.patch.C32.BN32", "dgrad.wide.x6.W384", "dgrad.native.BN64.ut"):      # res outside the slab and thin families
        c = by[name]
        prev = engine.lib.sg_set_conv_x6(c.mode)
        try:
            o_m, pl = CC.assert_plan(engine, c, c.id)
            assert o_m["with_res"]["kernel"] == 0
            o = CC.operands(c, False)
            assert CC.launch(engine, c, o, pl, 0, c.id, "res refused", res=o["res"], expect=CC.SG_EUNSUPPORTED) is None
        finally:
            engine.lib.sg_set_conv_x6(prev)
    g = torch.Generator().manual_seed(5)

    def refused(c, what, **kw):
        prev = engine.lib.sg_set_conv_x6(c.mode)
        try:
            o_m, pl = CC.assert_plan(engine, c, c.id)
            o = dict(CC.operands(c, False))
            if "up2" in kw:
                o["x_src"] = CC.rnd(g, c.g.N, c.g.H // 2, c.g.W // 2, c.g.Cin)
            assert CC.launch(engine, c, o, pl, 0, c.id, what, expect=CC.SG_EUNSUPPORTED, **kw) is None
            return o_m
        finally:
            engine.lib.sg_set_conv_x6(prev)

    c = by["fwd.slab.x6.BN64.v1.mf16"]           # a launch that is neither thin nor patch: no bn_in, no fused up-sampling forward
    o_m = refused(c, "bn refused", bn=CC._bn_params(c.g.Cin, 1) + (1, 0))
    assert o_m["bn_in"] == 0 and o_m["up2"] == 0
    refused(c, "up2 refused", up2=True)
    c = by["dgrad.slab.x6.BN64.v1.mf16"]         # the slab family's dgrad: no 2 x 2 sum in its epilogue, no BatchNormalization backward
    o_m = refused(c, "down2 refused", down2=True)
    assert o_m["up2"] == 0 and o_m["bnb"] == 0
    rows, co = c.g.N * c.g.Ho * c.g.Wo, c.g.Cout
    one, zero = torch.ones(co), torch.zeros(co)
    refused(c, "bnb refused", bnb=(CC.rnd(g, rows, co), zero, one, one, zero, zero, zero, False))


@pytest.mark.gpu
def test_process_wide_switches_in_child_processes(engine):
    """SG_X6_VARIANT=0 (the benchmark's structure for every slab.x6 case), SG_CONV_MAX_BYTES (sub-batches with N % nb != 0) and the
    A/B environment, each in a fresh process under its own time limit, one after another; after a fault, an abort or a time limit
    none follows."""
    assert not CC.FAULTED, f"no child is started: {CC.FAULTED}"
    torch.cuda.synchronize()
    for child, env in CC.CHILD_ENVS.items():
        with CC.switched(env):
            want = [c.id for c in CC.child_cases(child)]
        e = {k: v for k, v in os.environ.items() if k not in CC.SWITCH_DEFAULTS}
        e.update(env)
        t0 = time.time()
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_conv_cases.py"), child], env=e, cwd=ROOT, timeout=CHILD_TIMEOUT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(f"child {child}: rc {p.returncode}, {time.time() - t0:.1f} s")
        print("\n".join(l for l in p.stdout.splitlines() if l.startswith(("REC", "CASE", "DONE"))))
        CHILD_RECORDS[child] = [l for l in p.stdout.splitlines() if l.startswith("REC ")]
        assert p.returncode in (0, 1), f"child {child} ended with {p.returncode}: no further child is started\n{p.stdout[-4000:]}"
        ok = [l.split()[2] for l in p.stdout.splitlines() if l.startswith("CASE ok ")]
        assert p.returncode == 0 and ok == want, f"child {child}:\n{p.stdout[-6000:]}"
