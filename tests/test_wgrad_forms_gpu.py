"""Every kernel form of the filter gradient (sg_conv2d_wgrad, sg_conv2d_wgrad_planes: plan_wgrad / plan_wgrad_launch in
csrc/conv_igemm.hip with the kernels of conv_native.hip, conv_thin.hip, conv_x6.h, conv_x6p.hip and the filter-gradient half of
conv_pw.h) against float64, through the C ABI on guarded operands.  The tables, the mirror of the plan, the reference and the runner
are tests/_wgrad_cases.py; a case id ends in the name of the form its launch takes, asserted against the mirror and against
sg_conv2d_wgrad_plan before anything is launched.

The first tests need no GPU: the mirror against the fields tests/test_wgrad_plan_gpu.py wrote down by hand and against share counts
worked out by hand, the mirror against the recorded plans of profiles/plan_table.txt, the tables against the mirror at 256 CUs, the
list of forms that must keep a case, the form the rules cannot reach, and the sensitivity of every case's inputs to its last slab.
The process-wide switches run in child processes, one after another."""
import ctypes as CT
import os
import subprocess
import sys
import time

import pytest
import torch

import _wgrad_cases as WC
from _conv_cases import Geom
from _wgrad_cases import CASES, PW2_CASES, SUB_CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240     # seconds per child process (its cases take well under a minute on an MI355X)
NAMES = {1: "thin", 2: "wide", 3: "patch", 4: "slab-x6", 5: "slab-native", 6: "head32", 7: "planes-in"}


# ================================================================================================ CPU self-checks
def test_mirror_reproduces_the_fields_of_the_plan_test():
    """tests/test_wgrad_plan_gpu.py wrote its CASES' and FALLBACKS' plan fields down by hand, from the rules; the mirror must say
    the same (the tables are restated here: that module imports a GPU test module)."""
    shapes = {
        "thin": (2, 9, 7, 48, 2, 1, 1, 1), "wide": (1, 96, 64, 256, 384, 1, 1, 1), "patch": (2, 20, 48, 32, 32, 3, 1, 1),
        "x6_s1_d3": (1, 64, 32, 48, 80, 3, 1, 3), "x6_s2": (2, 64, 64, 64, 128, 3, 2, 1), "native": (2, 17, 19, 64, 64, 3, 2, 1),
        "stem_c3": (2, 24, 20, 3, 32, 3, 2, 1), "planes": (2, 32, 32, 256, 256, 3, 1, 6), "head": (2, 12, 12, 64, 2, 3, 1, 1),
    }
    cases = [
        ("thin", "f32", "thin", dict(bn=0, S=1)),
        ("wide", "f32", "wide", dict(planes=3, step_px=16, S=48, steps=8)),
        ("patch", "f32", "patch", dict(planes=3, S=30)),
        ("x6_s1_d3", "f32", "slab-x6", dict(bn=128, vec=4, planes=3, skip_slabs=1, tap_inner=0)),
        ("x6_s2", "f32", "slab-x6", dict(bn=128, vec=4, planes=3, skip_slabs=0)),
        ("native", "f32", "slab-native", dict(bn=64, vec=4, fast=0, planes=0)),
        ("stem_c3", "f32", "slab-native", dict(bn=32, vec=0, fast=0, planes=0)),
        ("planes", "f32", "slab-x6", dict(bn=128, vec=4, planes=3, skip_slabs=1, tap_inner=1)),
        ("thin", "bf16", "thin", dict(S=1)),
        ("wide", "bf16", "wide", dict(planes=1, step_px=32, S=24, steps=8)),
        ("patch", "bf16", "patch", dict(planes=1, S=30)),
        ("x6_s1_d3", "bf16", "slab-x6", dict(bn=128, vec=8, planes=1, skip_slabs=1)),
        ("x6_s2", "bf16", "slab-x6", dict(bn=128, vec=8, planes=1)),
        ("native", "bf16", "slab-native", dict(bn=64, vec=4, planes=0, skip_slabs=0)),
        ("head", "head32", "head32", dict(bn=32, vec=0)),
    ]
    fallbacks = [
        ("thin", "slab-native", dict(bn=32, vec=0, S=1, steps=4)),
        ("wide", "slab-native", dict(bn=128, vec=0, S=48, steps=4)),
        ("patch", "slab-native", dict(bn=32, vec=0, S=30, steps=2)),
    ]
    dts = {"f32": WC.F32, "bf16": WC.BF16, "head32": WC.BF16 | WC.HEAD}

    def geom(tag):
        n, h, w, cin, cout, k, s, d = shapes[tag]
        return Geom(n, h, w, cin, cout, k=k, s=s, d=d)

    def check(o, family, fields, what):
        assert NAMES[o["main"]["family"]] == family, (what, o["main"])
        for k, v in fields.items():
            assert o["main"][k] == v, f"{what}: the mirror's main.{k} = {o['main'][k]}, written down by hand: {v}"
        assert o["chunks"] == 1 and o["max_parts"] == o["main"]["S"]
        assert o["bias_off"] % 256 == 0 and o["bias_off"] >= o["dw_part_bytes"] and o["bias_off"] + o["bias_part_bytes"] <= o["ws_bytes"]

    for tag, st, family, fields in cases:
        check(WC.plan_mirror(256, 1, dts[st], geom(tag)), family, fields, f"{tag} {st}")
    for tag, family, fields in fallbacks:
        o = WC.plan_mirror(256, 1, WC.F32, geom(tag), 0, 0)
        check(o, family, fields, f"{tag} x+4")
        assert o["bn_in"] == 0 and o["up2"] == 0
        assert o["ws_bytes"] <= WC.plan_mirror(256, 1, WC.F32, geom(tag))["ws_bytes"]
    o = WC.plan_mirror(256, 1, WC.F32, geom("planes"), planes=True)
    check(o, "planes-in", dict(bn=128, vec=8, planes=3, skip_slabs=1, tap_inner=1), "planes-in")
    of = WC.plan_mirror(256, 1, WC.F32, geom("planes"))
    assert (o["main"]["S"], o["main"]["steps"]) == (of["main"]["S"], of["main"]["steps"]) and o["bias_part_bytes"] == 0
    assert WC.plan_mirror(256, 1, WC.F32, geom("patch"), planes=True)["main"]["family"] == 0
    # the fused operands: BatchNormalization where forward and filter gradient both take it, the up-sampling on its own layer
    assert WC.plan_mirror(256, 1, WC.F32, Geom(2, 24, 48, 32, 32))["bn_in"] == 1 and WC.plan_mirror(256, 1, WC.F32, geom("thin"))["bn_in"] == 1
    assert WC.plan_mirror(256, 1, WC.F32, geom("patch"))["bn_in"] == 0 and WC.plan_mirror(256, 1, WC.F32, geom("x6_s1_d3"))["bn_in"] == 0
    assert WC.plan_mirror(256, 1, WC.F32 | WC.UP2, Geom(1, 16, 32, 64, 32))["up2"] == 1
    assert WC.plan_mirror(256, 1, WC.F32 | WC.UP2, geom("x6_s1_d3"))["up2"] == 0


def test_share_rules_by_hand():
    # wgrad_slab_split, the source comment's own example: the ASPP 3x3 at 2048 -> 256 on a 32 x 32 map at the benchmark's batch 16.
    # K = 18432: 144 row tiles x 2 column tiles of 128 = 288 tiles; 7 shares make 2016 workgroups = 3.94 waves of 512 slots.  In
    # numbers: the padded work is 2 x 288 x 128 x 128 x 16384 flop = 1406 us at 110 TFLOP/s, a partial slab 18 MiB = 12.6 us both
    # ways.  S = 7: 1406 / 0.984 + 88 + 3 = 1519 us; S = 5 (1440 of 1536 slots): 1500 + 63 + 3 = 1566; S = 16 (4608 = 9 whole
    # waves): 1406 + 201 + 3 = 1610.  At batch 2 the work is an eighth of that and the slabs weigh more: S = 3 (864 of 1024 slots).
    assert WC.wgrad_slab_split(256, Geom(16, 32, 32, 2048, 256, d=6), False) == 7
    assert WC.wgrad_slab_split(256, Geom(2, 32, 32, 2048, 256, d=6), False) == 3
    # few tiles: the split is bounded by 8 slabs per share.  8 x 32 pixels = 8 slabs -> one share; 63 x 63 at stride 2 = 32 slabs -> 4
    assert WC.wgrad_slab_split(256, Geom(1, 8, 32, 48, 48), False) == 1
    assert WC.wgrad_slab_split(256, Geom(1, 63, 63, 32, 48, s=2), False) == 4
    # 60 slabs, one tile: 7 shares at most (60 // 8), and with one tile every added share models faster (a slab of 16 KiB: 11 ns)
    assert WC.wgrad_slab_split(256, Geom(3, 20, 32, 64, 64, k=1), False) == 7
    # the 0.999 hysteresis: 16 x 32 = 512 tiles fill the 512 slots exactly, so S = 2 has the same efficiency and only adds its
    # slabs' traffic: S stays 1
    assert WC.wgrad_slab_split(256, Geom(1, 64, 64, 2048, 4096, k=1), False) == 1
    # the 384 MiB break: 1024 -> 3968 channels 3x3 is 72 x 31 = 2232 tiles and 139.5 MiB per partial slab.  Five shares would fill
    # 11160 of 11264 slots (0.991, against 0.969 for two and 0.872 for one) and model fastest on 65536 pixels, but three slabs
    # are already 418 MiB: the search ends at S = 2
    assert WC.wgrad_slab_split(256, Geom(16, 64, 64, 1024, 3968), False) == 2
    # wgrad_pw_wide_plan: 6144 pixels, 256 -> 384: 2 tiles -> 128 shares wanted, capped at 384 k-steps / 8 = 48 (bf16: 192 / 8 = 24)
    wide = Geom(1, 96, 64, 256, 384, k=1)
    assert WC.wgrad_pw_wide_plan(256, wide, 16) == (48, 8) and WC.wgrad_pw_wide_plan(256, wide, 32) == (24, 8)
    # 16384 pixels, 728 -> 728: 6 x 2 = 12 tiles -> 21 shares of ceil(1024 / 21) = 49 k-steps
    assert WC.wgrad_pw_wide_plan(256, Geom(1, 128, 128, 728, 728, k=1), 16) == (21, 49)
    # x6wp_grid: 2 x 5 x 3 = 30 tiles < 512 slots; 3 x 24 x 8 = 576 tiles -> 512
    assert WC.x6wp_grid(256, Geom(2, 20, 48, 32, 32)) == 30 and WC.x6wp_grid(256, Geom(3, 96, 128, 64, 64)) == 512
    # the fallbacks keep S <= S0: 60 slabs in the patch plan's 30 shares, 192 slabs in the wide plan's 48
    assert WC.launch_mirror(256, 1, WC.F32, Geom(2, 20, 48, 32, 32), 2, 0, 16)["S"] == 30
    assert WC.launch_mirror(256, 1, WC.F32, wide, 1, 0, 16)["S"] == 48


def test_small_rules_by_hand():
    assert [WC.wgrad_bn(c) for c in (16, 32, 33, 64, 65, 136)] == [32, 32, 64, 64, 128, 128]
    assert WC.wgrad_x6_geom(Geom(1, 63, 63, 32, 48, s=2)) and not WC.wgrad_x6_geom(Geom(1, 8, 32, 48, 8)) and not WC.wgrad_x6_geom(Geom(1, 8, 24, 48, 48))
    assert WC.wgrad_pw_wide_geom(Geom(1, 96, 64, 256, 384, k=1), 4) and not WC.wgrad_pw_wide_geom(Geom(1, 95, 64, 256, 384, k=1), 4)
    assert not WC.wgrad_pw_wide_geom(Geom(1, 96, 64, 256, 256, k=1), 4)          # 256 / 384 columns
    assert not WC.wgrad_pw_wide_geom(Geom(1, 96, 64, 260, 384, k=1), 2)          # bf16: channels % 8
    with WC.switched({"SG_PW_WIDE": "2"}):
        assert WC.wgrad_pw_wide_geom(Geom(1, 5, 10, 36, 388, k=1), 4)
    g = Geom(3, 32, 32, 96, 64)
    assert WC.images_per_2gib(g) == 3
    with WC.switched({"SG_CONV_MAX_BYTES": str(1 << 20)}):
        assert WC.images_per_2gib(g) == 2          # 393216 bytes per image at 4 bytes per element, bf16 too
        o = WC.plan_mirror(256, 1, WC.BF16, g)
        assert (o["chunks"], o["nb"], o["tail_n"]) == (2, 2, 1) and o["max_parts"] == o["main"]["S"] + o["tail"]["S"]
        assert o["dw_part_bytes"] == 2 * o["main"]["S"] * 9 * 96 * 64 * 4
    assert WC.conv_l2(True) == 7 and WC.conv_l2(False) == 2
    with WC.switched({"SG_CONV_L2": "0"}):
        assert WC.conv_l2(True) == 0
    assert WC.align_class(0) == 16 and WC.align_class(8) == 8 and WC.align_class(4) == 0 and WC.align_class(2) == 0
    # fast 2 needs whole rows per slab and one tap per row tile; fast 1 is what is left of stride 1 SAME with 16-byte runs
    f = lambda g, mode=1: WC.launch_mirror(256, mode, WC.F32, g, g.N, 16, 16)["fast"]
    assert f(Geom(1, 8, 32, 40, 8, k=1)) == 2 and f(Geom(1, 8, 32, 128, 72), 0) == 2 and f(Geom(1, 8, 32, 40, 48), 0) == 1
    assert f(Geom(3, 2, 24, 8, 32)) == 1 and f(Geom(2, 17, 19, 8, 32, s=2)) == 0 and f(Geom(1, 8, 32, 128, 72)) == 0      # (x6 takes the last)


def test_more_than_1024_slabs_per_share_is_out_of_an_affordable_tests_reach():
    """The slab kernels build their list of live slabs only for shares of at most 1024 slabs (conv_x6.h, conv_native.hip: `nslab <=
    1024`); a longer share walks every slab.  A share that long needs more than 32768 pixels per share.  Within what a case may cost
    here - at most about 40 k pixels x 9 * 64 * 64 products - the split rule never leaves one: above 32768 pixels the budget holds
    K * Cout to about 45000, a handful of tiles, and with so few tiles every added share models faster, so S reaches at least 2.
    Swept so that a change of the rule that brings such a share within reach also asks for its case."""
    worst = 0
    for hw in ((128, 256), (160, 256), (192, 192), (200, 200), (128, 320), (104, 320)):
        for cin in (8, 16, 32, 64):
            for cout in (16, 32, 48, 64, 128):
                if hw[0] * hw[1] * 9 * cin * cout > 41000 * 9 * 64 * 64:
                    continue
                for d in (2, 6, 36):
                    for dt in (WC.F32, WC.BF16):
                        la = WC.plan_mirror(256, 1, dt, Geom(1, hw[0], hw[1], cin, cout, d=d))["main"]
                        if la["skip_slabs"]:      # (the mixed-storage native form has no slab list)
                            worst = max(worst, la["steps"])
    assert 0 < worst <= 1024, worst


def test_the_wide_tail_clamp_by_hand():
    """plan_wgrad_launch cuts a last, smaller sub-batch of a wide layer back to the shares of a full one (`if (f.S > S0)`).  It bites
    where the full sub-batch's own rounding loses a share: 45 images of 32 pixels are 90 k-steps, 11 shares wanted (90 // 8), 9
    k-steps each, which makes 10 shares; the last 44 images are 88 k-steps, 11 shares of exactly 8.  Clamped: 88 k-steps in 10
    shares of 9.  (SUB_CASES holds the layer: 180 channels x 32 pixels x 4 bytes = 23040 bytes per image, 45 per MiB.)"""
    with WC.switched(WC.CHILD_ENVS["sub"]):
        g = Geom(89, 4, 8, 180, 36, k=1)
        assert WC.wgrad_pw_wide_plan(256, g.with_n(45), 16) == (10, 9) and WC.wgrad_pw_wide_plan(256, g.with_n(44), 16) == (11, 8)
        o = WC.plan_mirror(256, 1, WC.F32, g)
        assert (o["chunks"], o["nb"], o["tail_n"]) == (2, 45, 44)
        assert (o["main"]["S"], o["main"]["steps"]) == (10, 9) and (o["tail"]["S"], o["tail"]["steps"]) == (10, 9)
        assert o["max_parts"] == 20 and o["dw_part_bytes"] == 2 * 10 * 180 * 36 * 4


_FAM = {"thin": 1, "wide": 2, "patch": 3, "slab-x6": 4, "slab-native": 5, "head32": 6, "planes-in": 7}


def test_mirror_reproduces_the_recorded_plan_table():
    """profiles/plan_table.txt holds sg_conv2d_wgrad_plan's answers on an MI355X for every convolution of the five models at four
    batch sizes, three arithmetic modes and both storage types (2048 plans, sub-batched ones included): family, tile width, vec,
    fast, planes, skip, tap order, shares, steps, parts, workspace, the fused operands and the planes-in plan.  The mirror must say
    the same for each."""
    import re
    head_re = re.compile(r"wgrad (head )?(\d+)x(\d+)x(\d+)>(\d+) k(\d+)s(\d+)d(\d+) o(\d+)x(\d+) b([\d,]+)$")
    plan_re = re.compile(r"(\S+) bn(\d+) v(\d+) f(\d+) pl(\d+) skip(\d+) tap(\d+) stag(\d+) S(\d+)x(\d+)/(\d+)px"
                         r"(?: chunks(\d+)x(\d+)\+(\d+) tailS(\d+)x(\d+))? parts(\d+) ws(\d+) q(\d+) sup(\d)(\d) pin (?:-|S(\d+)x(\d+) ws(\d+))$")
    count = 0
    for line in open(os.path.join(ROOT, "profiles", "plan_table.txt")):
        if not line.startswith("wgrad "):
            continue
        parts = [p.strip() for p in line.rstrip("\n").split(" | ")]
        m = head_re.match(parts[0])
        assert m, parts[0]
        H, W, Cin, Cout, k, s, d, Ho, Wo = map(int, m.groups()[1:10])
        batches = [int(b) for b in m.group(11).split(",")]
        for part in parts[1:]:
            modes, rest = part.split(": ", 1)
            plans = {}
            for item in rest.split("; "):
                mm = re.match(r"b([\d,]+): (.*)$", item)
                for b in (mm.group(1).split(",") if mm else batches):
                    plans[int(b)] = mm.group(2) if mm else item
            for mode in modes.split(","):
                for b, text in plans.items():
                    f = plan_re.match(text).groups()
                    g = Geom(b, H, W, Cin, Cout, k=k, s=s, d=d)
                    assert (g.Ho, g.Wo) == (Ho, Wo)
                    dt = WC.F32 if mode != "b16" else (WC.BF16 | WC.HEAD if m.group(1) else WC.BF16)      # (head: the softmax head)
                    md = 1 if mode == "b16" else int(mode[1])
                    o = WC.plan_mirror(256, md, dt, g)
                    la = o["main"]
                    got = [la[x] for x in ("family", "bn", "vec", "fast", "planes", "skip_slabs", "tap_inner", "S", "steps", "step_px")]
                    got += [o["max_parts"], o["ws_bytes"], o["up2"], o["bn_in"]]
                    want = [_FAM[f[0]]] + [int(v) for v in f[1:7] + f[8:11] + f[16:18] + f[19:21]]
                    if f[11]:
                        got += [o["chunks"], o["nb"], o["tail_n"], o["tail"]["S"], o["tail"]["steps"]]
                        want += [int(v) for v in f[11:16]]
                    else:
                        got, want = got + [o["chunks"]], want + [1]
                    if dt == WC.F32:
                        op = WC.plan_mirror(256, md, WC.F32, g, planes=True)
                        if f[21]:
                            got += [op["main"]["S"], op["main"]["steps"], op["ws_bytes"]]
                            want += [int(v) for v in f[21:24]]
                        else:
                            got, want = got + [op["main"]["family"]], want + [0]
                    assert got == want, f"{parts[0]} {mode} b{b}: the mirror says {got}, the table {want}"
                    count += 1
    assert count == 2048


def _main_ids():
    return [c.id for c in CASES]


@pytest.mark.parametrize("c", CASES, ids=_main_ids())
def test_tables_name_what_the_mirror_names(c):
    assert c.mirror_name() == c.name
    assert (c.mirror_pin_name() if c.pin else None) == c.pin


def test_tables_contain_every_form_by_name():
    assert WC.missing_forms() == []
    # the condition bites: names are matched whole (up to the modifiers), so a form is not covered by a longer one
    names = WC.all_case_names()
    for gone in ("wgrad.native.BN64.fast2", "wgrad.thin.CO2.b16", "wgrad.slab.x6.BN32.b16", "wgrad.patch.C64x32.npl1", "wgrad.planes.BN64",
                 "wgrad.native.BN32.vec.b16>f32", "wgrad.wide.b16"):
        assert WC.missing_forms([n for n in names if WC.base_of(n) != gone]) == [gone]
    assert WC.missing_forms([n for n in names if ".tapin" not in n]) == [".tapin"]
    assert WC.missing_forms([n for n in names if ".wv0" not in n]) == [".wv0"]
    assert WC.missing_forms([n for n in names if ".sub" not in n]) == [".sub"]
    assert WC.missing_forms([n for n in names if ".up2" not in n]) == [".up2"]
    ids = [c.id for c in CASES + PW2_CASES + SUB_CASES]
    assert len(ids) == len(set(ids)), "two cases share an id"


def test_child_tables():
    with WC.switched(WC.CHILD_ENVS["sub"]):
        sub = WC.child_cases("sub")
        assert all(c.mirror_name() == c.name for c in sub), [c.id for c in sub if c.mirror_name() != c.name]
        plans = [c.mirror() for c in sub]
        assert all(o["chunks"] > 1 and o["tail_n"] != o["nb"] for o in plans)
        assert {NAMES[o["main"]["family"]] for o in plans} >= {"slab-x6", "patch", "wide"}
    with WC.switched(WC.CHILD_ENVS["pw2"]):
        pw2 = WC.child_cases("pw2")
        assert all(c.mirror_name() == c.name for c in pw2), [c.id for c in pw2 if c.mirror_name() != c.name]
        steps = {(c.dt, c.mirror()["main"]["steps"]) for c in pw2 if ".wide." in c.name}
        assert {s for dt, s in steps if dt == "f32"} >= {1, 2, 3, 4} and {s for dt, s in steps if dt == "b16"} >= {1, 2}
        assert any(c.g.N * c.g.H * c.g.W % 16 for c in pw2) and any(c.g.Cin % 128 for c in pw2) and any(c.g.Cout % 384 for c in pw2)
    with WC.switched(WC.CHILD_ENVS["ab"]):
        ab = WC.child_cases("ab")
        names = [c.name for c in ab]
        assert len(ab) >= 30 and not any(".skip" in n or ".tapin" in n or ".fast2" in n or ".thin." in n or ".patch." in n for n in names)
        assert any(n.endswith(".wv0") for n in names) and any(".fast1" in n for n in names)
    assert not any(".wv0" in c.name for c in CASES)


def _all_tables():
    out = [(None, c) for c in CASES]
    for child in ("pw2", "sub"):
        out += [(child, c) for c in WC.child_cases(child)]
    return out


@pytest.mark.parametrize("child,c", _all_tables(), ids=[("" if ch is None else ch + ":") + c.id for ch, c in _all_tables()])
def test_inputs_are_sensitive_to_the_last_slab(child, c):
    """On the CPU in float64: without the contribution of the reduction's last slab (the last P % 32 pixels or the last 32; wide: the
    last k-step; patch: the last tile row) dw moves by more than four times the case's bound - a kernel that drops or repeats that
    slab cannot pass.  A condition on the chosen inputs and shapes."""
    with WC.switched(WC.CHILD_ENVS[child] if child else {}):
        la = c.mirror()["main"]
    full, db = WC.references(c, la)
    less, _ = WC.references(c, la, without_last=True)
    move = (full - less).abs().max().item()
    assert move > 4 * WC.BOUND * full.abs().max().item(), (c.id, move, full.abs().max().item())
    # ... and the bias gradient is no cancelled sum: the bound is a fraction of max|ref|, which for one output channel is one number
    # (the sum of P values uniform in [-1, 1] has the standard deviation sqrt(P / 3))
    P = c.g.N * c.g.Ho * c.g.Wo
    assert db.abs().max().item() > 0.25 * (P / 3) ** 0.5, (c.id, db.abs().max().item())


# ================================================================================================ GPU cases
CHILD_RECORDS = {}


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    """With WGRAD_FORMS_RECORD=<path> in the environment: every record of this run (RECORDS of this process, then each child's), one
    line per launch and output with its bound, written when the module's tests are over (profiles/wgrad_forms_gpu.txt)."""
    yield
    path = os.environ.get("WGRAD_FORMS_RECORD")
    if path and WC.RECORDS:
        with open(path, "w") as f:
            f.write(WC.records_table() + "\n")
            for child, lines in CHILD_RECORDS.items():
                env = " ".join(f"{k}={v}" for k, v in WC.CHILD_ENVS[child].items())
                f.write(f"# child {child}: {env}\n" + "\n".join(lines) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=_main_ids())
def test_every_form_against_fp64(engine, c):
    WC.run_case(engine, c)


@pytest.mark.gpu
def test_refused_combinations_leave_everything_untouched(engine):
    """What the header says is refused: its documented code, and dw, dbias and the workspace untouched (the runner checks the latter
    for every refused call)."""
    assert not WC.FAULTED, WC.FAULTED
    by = {c.name: c for c in CASES if not (c.bn or c.up2 or c.xoff or c.yoff or c.g.xgap)}

    def refused(c, what, expect, **kw):
        prev = engine.lib.sg_set_conv_x6(c.mode)
        try:
            o = WC.assert_plan(engine, c, c.id)
            ws = kw.pop("ws_bytes", o["ws_bytes"])
            assert WC.launch(engine, c, ws, c.id, what, expect=expect, **kw) is None
            return o
        finally:
            engine.lib.sg_set_conv_x6(prev)

    # bn_in and SG_X_UP2 outside the thin and patch families
    c = by["wgrad.slab.x6.BN64.x6"]
    o = refused(c, "bn refused", WC.SG_EUNSUPPORTED, bn=WC.bn_params(c.g.Cin))
    assert o["bn_in"] == 0 and o["up2"] == 0
    src = WC.rnd(torch.Generator().manual_seed(5), c.g.N, c.g.H // 2, c.g.W // 2, c.g.Cin)
    refused(c, "up2 refused", WC.SG_EUNSUPPORTED, dt=WC.F32 | WC.UP2, x=src)
    c = by["wgrad.native.BN64.vec"]
    refused(c, "bn refused", WC.SG_EUNSUPPORTED, bn=WC.bn_params(c.g.Cin))
    # ... and inside them where the forward does not take the operand (H % 8 != 0), or on bf16 storage
    c = by["wgrad.patch.C32x32.x6.S30"]
    assert refused(c, "bn refused", WC.SG_EUNSUPPORTED, bn=WC.bn_params(c.g.Cin))["bn_in"] == 0
    c = by["wgrad.thin.CO1.b16"]
    refused(c, "bn refused", WC.SG_EUNSUPPORTED, bn=WC.bn_params(c.g.Cin))
    # SG_HEAD_F32 with more than four output channels, and on fp32 storage
    c = by["wgrad.slab.x6.BN64.b16"]
    refused(c, "head refused", WC.SG_EINVAL, dt=WC.BF16 | WC.HEAD)
    refused(by["wgrad.thin.CO1.f32"], "head refused", WC.SG_EINVAL, dt=WC.F32 | WC.HEAD)
    d = c.g.desc()
    from building_detection_amd import _lib
    bad = _lib.WgradPlan()
    assert engine.lib.sg_conv2d_wgrad_plan(engine.h, WC.BF16 | WC.HEAD, CT.byref(d), 16, 0, CT.byref(bad)) == WC.SG_EINVAL
    assert bad.main.family == 0 and bad.ws_bytes == 0
    # a workspace that is not 16-byte aligned
    refused(by["wgrad.slab.x6.BN64.x6"], "ws+4 refused", WC.SG_EINVAL, ws_off=4)
    # planes-in on the other families: no plan (all-zero, the entry point's code), no launch
    for name in ("wgrad.patch.C32x32.x6.S30", "wgrad.wide.x6.S48", "wgrad.native.BN64.vec", "wgrad.native.BN32.fast2"):
        c = by[name]
        rc, none = WC.engine_plan(engine, c, 16, planes=True)
        assert rc == WC.SG_EUNSUPPORTED and none.main.family == 0 and none.ws_bytes == 0, name
        assert WC.plan_mirror(256, 1, WC.F32, c.g, planes=True)["main"]["family"] == 0
        assert engine.conv2d_caps(c.g.desc()).wgrad_planes == 0
        if "wide" not in name:
            assert WC.launch_planes(engine, c, 1 << 20, c.id, expect=WC.SG_EUNSUPPORTED) is None
    # ... and in another arithmetic mode on its own family
    c = by["wgrad.slab.x6.BN64.npl1"]
    prev = engine.lib.sg_set_conv_x6(2)
    try:
        assert WC.launch_planes(engine, c, 1 << 20, c.id, expect=WC.SG_EUNSUPPORTED) is None
    finally:
        engine.lib.sg_set_conv_x6(prev)


@pytest.mark.gpu
def test_process_wide_switches_in_child_processes(engine):
    """SG_CONV_MAX_BYTES with SG_PW_WIDE=2 (sub-batches with N % nb != 0 of the slab, patch, wide and native families, against
    float64), SG_PW_WIDE=2 (pixel tails, short shares and ragged tiles of the wide kernels) and the A/B environment, each in a fresh
    process under its own time limit, one after another; after a fault, an abort or a time limit none follows."""
    assert not WC.FAULTED, f"no child is started: {WC.FAULTED}"
    torch.cuda.synchronize()
    for child, env in WC.CHILD_ENVS.items():
        with WC.switched(env):
            want = [c.id for c in WC.child_cases(child)]
        e = {k: v for k, v in os.environ.items() if k not in WC.SWITCH_DEFAULTS}
        e.update(env)
        t0 = time.time()
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_wgrad_cases.py"), child], env=e, cwd=ROOT, timeout=CHILD_TIMEOUT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(f"child {child}: rc {p.returncode}, {time.time() - t0:.1f} s")
        print("\n".join(l for l in p.stdout.splitlines() if l.startswith(("REC", "CASE", "DONE"))))
        CHILD_RECORDS[child] = [l for l in p.stdout.splitlines() if l.startswith("REC ")]
        assert p.returncode in (0, 1), f"child {child} ended with {p.returncode}: no further child is started\n{p.stdout[-4000:]}"
        ok = [l.split()[2] for l in p.stdout.splitlines() if l.startswith("CASE ok ")]
        assert p.returncode == 0 and ok == want, f"child {child}:\n{p.stdout[-6000:]}"
