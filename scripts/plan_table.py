#!/usr/bin/env python3
"""The plan table: what the library answers about every convolution site of the five models - the planes-job fields and slot size
(sg_conv2d_planes_job), the workspace query and the planes_in / up2 / bn_in / bnb answers of sg_conv2d_caps for
every unique (site, storage, arithmetic mode, direction).  A change of plan_conv() (csrc/conv_igemm.hip) is diffed against its
parent with this: every line that moved is a launch that takes another kernel, other planes or another workspace.  The sites are the
ones tests/test_plane_sites_gpu.py sweeps (tests/_plane_sites.py enumerates them).  Needs the GPU only for the library context.

Folded so that the table can be read: one line per (direction, head, descriptor without N) with the batch sizes it occurs at and the
workspace query (which knows neither storage nor mode); behind it one group per set of arithmetics with equal answers (x0 / x1 / x2:
fp32 storage under sg_set_conv_x6 0 / 1 / 2, b16: bf16 storage); inside a group the batch sizes with equal answers share one
entry, and a value that is the same at every batch is printed once.
Behind those lines, the filter gradients: one line per (head, descriptor without N) with the batch sizes and, per arithmetic, the
plan sg_conv2d_wgrad_plan answers at 16-byte alignment - what plan_wgrad() (csrc/conv_igemm.hip) decides -, the storage-blind
sg_conv2d_wgrad_ws_bytes and the plan of sg_conv2d_wgrad_planes where it covers the layer.
Behind those, the kernel forms: one line per (direction, head, descriptor without N) and, per arithmetic, the name of the form the
launch takes at 16-byte alignment (sg_conv2d_plan, _lib.conv_form_name: kernel, tile width, structure and the launch-time choices of
the dispatchers), `res>` the form of the same launch with a collected gradient where that is another one, and the plan's workspace.
Use: python scripts/plan_table.py > profiles/plan_table.txt"""
import collections
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

Row = collections.namedtuple("Row", "arith dgrad head desc kind npl kd K Kpad N Npad Ck Ckp nblocks bytes ws pin up2 bn_in bnb")


def rows():
    """every answer of the library, unfolded (needs the GPU)"""
    import _plane_sites as PS
    from building_detection_amd import _lib
    from building_detection_amd.ops import get_engine
    e = get_engine(0)
    uniq, _ = PS.unique_sites(PS.enumerate_groups())
    info = PS.survey(e, uniq)
    out = []
    for mode in (0, 1, 2, None):
        with PS.mode_set(e, mode):
            for (k, m), i in info.items():
                if m != mode:
                    continue
                s = uniq[k]
                d = PS.make_desc(s)
                st = _lib.SG_F32 if s.policy == "float32" else _lib.SG_BF16
                out.append(Row("b16" if mode is None else f"x{mode}", s.dgrad, s.head, dict(zip(PS.desc_fields(), s.desc)), i.kind, i.npl, i.kd,
                               i.K, i.Kpad, i.N, i.Npad, i.Ck, i.Ckp, i.nblocks, i.bytes, i.ws, i.pin,
                               e.conv2d_caps(d, False, st).up2, e.conv2d_caps(d, False, st).bn_in, e.conv2d_caps(d, True, st).bnb))
    return len(uniq), out


def wgrad_rows():
    """(arith, head, desc fields, plan text) of every unique (descriptor, head, storage) under every arithmetic
    mode its storage type runs in; a layer's forward, input gradient and Conv2DTranspose share the descriptor (needs the GPU)"""
    import _plane_sites as PS
    from building_detection_amd import _lib
    from building_detection_amd.ops import get_engine
    e = get_engine(0)
    uniq, _ = PS.unique_sites(PS.enumerate_groups(geometries=tuple(g for g in PS.GEOMETRIES if g[2])))   # (training geometries)
    sites = collections.OrderedDict(((s.desc, s.head, s.policy), s) for s in uniq.values())
    out = []
    for mode in (0, 1, 2, None):
        with PS.mode_set(e, mode):
            for s in sites.values():
                if mode not in PS.modes_of(s.policy):
                    continue
                d = PS.make_desc(s)
                pl = e.conv2d_wgrad_plan(d, PS.abi_dtype(s))
                m, t = pl.main, pl.tail
                txt = (f"{_lib.WG_FAMILY_NAMES[m.family]} bn{m.bn} v{m.vec} f{m.fast} pl{m.planes} skip{m.skip_slabs} tap{m.tap_inner} "
                       f"stag{m.stagger} S{m.S}x{m.steps}/{m.step_px}px")
                if pl.chunks > 1:
                    txt += f" chunks{pl.chunks}x{pl.nb}+{pl.tail_n} tailS{t.S}x{t.steps}"
                pin = "-"
                if s.policy == "float32" and e.conv2d_caps(d).wgrad_planes:
                    pp = e.conv2d_wgrad_plan(d, _lib.SG_F32, planes=True)
                    pin = f"S{pp.main.S}x{pp.main.steps} ws{pp.ws_bytes}"
                txt += (f" parts{pl.max_parts} ws{pl.ws_bytes} q{int(e.lib.sg_conv2d_wgrad_ws_bytes(e.h, C.byref(d)))} "
                        f"sup{pl.up2}{pl.bn_in} pin {pin}")
                out.append(("b16" if mode is None else f"x{mode}", s.head, dict(zip(PS.desc_fields(), s.desc)), txt))
    return out


def form_rows():
    """(arith, dgrad, head, desc fields, form text) of every unique site under every arithmetic mode (needs the GPU)"""
    import _plane_sites as PS
    from building_detection_amd import _lib
    from building_detection_amd.ops import get_engine
    e = get_engine(0)
    uniq, _ = PS.unique_sites(PS.enumerate_groups())
    out = []
    for mode in (0, 1, 2, None):
        with PS.mode_set(e, mode):
            for s in uniq.values():
                if mode not in PS.modes_of(s.policy):
                    continue
                d = PS.make_desc(s)
                dt = PS.abi_dtype(s)
                pl = e.conv2d_plan(d, dt, dgrad=bool(s.dgrad))
                txt = _lib.conv_form_name(pl, pl.main, bool(s.dgrad), dt)
                if pl.nsub > 1 and pl.tail_n != pl.nb:
                    tail = _lib.conv_form_name(pl, pl.tail, bool(s.dgrad), dt)
                    txt += f" tail>{tail}" if tail != txt else ""
                if pl.with_res.kernel:
                    r = _lib.conv_form_name(pl, pl.with_res, bool(s.dgrad), dt)
                    txt += f" res>{r}" if r != txt else ""
                txt += f" ws{pl.ws_bytes}"
                out.append(("b16" if mode is None else f"x{mode}", s.dgrad, s.head, dict(zip(PS.desc_fields(), s.desc)), txt))
    return out


def fold_forms(rs):
    table = collections.OrderedDict()   # line -> arithmetic -> batch -> form text
    for arith, dgrad, head, f, txt in rs:
        key = (f"form {'dgrad' if dgrad else 'fwd'}{' head' if head else ''} {f['H']}x{f['W']}x{f['Cin']}>{f['Cout']} "
               f"k{f['KH']}s{f['stride']}d{f['dilation']} o{f['Ho']}x{f['Wo']}")
        table.setdefault(key, collections.OrderedDict()).setdefault(arith, {})[f["N"]] = txt
    lines = [f"# kernel forms: {len(rs)} (site, storage, mode, direction) plans on {len(table)} lines",
             "# form <direction> [head] HxWxCin>Cout k<K>s<stride>d<dilation> o<Ho>x<Wo> b<batch sizes>",
             "#   | <arithmetics with equal forms>: [b<batches>:] <form name of the main launch> [tail><last sub-batch's>] "
             "[res><with a collected gradient>] ws<plan.ws_bytes> ; ..."]
    for key, ariths in table.items():
        batches = sorted({b for per in ariths.values() for b in per})
        line = f"{key} b{','.join(map(str, batches))}"
        texts = collections.OrderedDict()
        for arith, per in ariths.items():
            by = collections.OrderedDict()
            for b in sorted(per):
                by.setdefault(per[b], []).append(b)
            parts = [(f"b{','.join(map(str, bs))}: " if (len(by) > 1 or sorted(per) != batches) else "") + t for t, bs in by.items()]
            texts.setdefault("; ".join(parts), []).append(arith)
        for txt, names in texts.items():
            line += f" | {','.join(names)}: {txt}"
        lines.append(line)
    return lines


def fold_wgrad(rs):
    table = collections.OrderedDict()   # line -> arithmetic -> batch -> plan text
    for arith, head, f, txt in rs:
        key = (f"wgrad{' head' if head else ''} {f['H']}x{f['W']}x{f['Cin']}>{f['Cout']} k{f['KH']}s{f['stride']}d{f['dilation']} "
               f"o{f['Ho']}x{f['Wo']}")
        table.setdefault(key, collections.OrderedDict()).setdefault(arith, {})[f["N"]] = txt
    lines = [f"# filter gradients: {len(rs)} (descriptor, storage, mode) plans on {len(table)} lines",
             "# wgrad [head] HxWxCin>Cout k<K>s<stride>d<dilation> o<Ho>x<Wo> b<batch sizes>",
             "#   | <arithmetics with equal plans>: [b<batches>:] family bn<tile width> v<channels per load> f<FAST> pl<bf16 planes> "
             "skip<skip_slabs> tap<tap_inner> stag<stagger> S<shares>x<steps per share>/<pixels per step> [chunks<n>x<images>+<last> "
             "tailS..] parts<max_parts> ws<plan.ws_bytes> q<sg_conv2d_wgrad_ws_bytes, which knows no storage type> sup<up2, bn_in> pin <planes-in plan or -> ; ..."]
    for key, ariths in table.items():
        batches = sorted({b for per in ariths.values() for b in per})
        line = f"{key} b{','.join(map(str, batches))}"
        texts = collections.OrderedDict()
        for arith, per in ariths.items():
            by = collections.OrderedDict()
            for b in sorted(per):
                by.setdefault(per[b], []).append(b)
            parts = [(f"b{','.join(map(str, bs))}: " if (len(by) > 1 or sorted(per) != batches) else "") + t for t, bs in by.items()]
            texts.setdefault("; ".join(parts), []).append(arith)
        for txt, names in texts.items():
            line += f" | {','.join(names)}: {txt}"
        lines.append(line)
    return lines


def once(vals):
    vals = [str(v) for v in vals]
    return vals[0] if len(set(vals)) == 1 else ",".join(vals)


def fold(n_unique, rs):
    table, ws = collections.OrderedDict(), collections.defaultdict(dict)   # line -> arithmetic -> batch -> (answer, slot bytes)
    for r in rs:
        f = r.desc
        key = (f"{'dgrad' if r.dgrad else 'fwd'}{' head' if r.head else ''} {f['H']}x{f['W']}x{f['Cin']}>{f['Cout']} "
               f"k{f['KH']}s{f['stride']}d{f['dilation']} o{f['Ho']}x{f['Wo']}")
        sup = f"sup{r.up2}{r.bn_in}{r.bnb}"
        ans = f"kind0 {sup}" if r.kind == 0 else (f"kind{r.kind} npl{r.npl} kd{r.kd} K{r.K}/{r.Kpad} N{r.N}/{r.Npad} Ck{r.Ck}/{r.Ckp} "
                                                   f"nb{r.nblocks} pin{r.pin} {sup}")
        table.setdefault(key, collections.OrderedDict()).setdefault(r.arith, {})[f["N"]] = (ans, r.bytes)
        assert ws[key].setdefault(f["N"], r.ws) == r.ws   # (the query knows neither storage nor mode)
    lines = [f"# {n_unique} unique sites, {len(rs)} (site, storage, mode, direction) answers on {len(table)} lines",
             "# <direction> [head] HxWxCin>Cout k<K>s<stride>d<dilation> o<Ho>x<Wo> b<batch sizes> ws <sg_conv2d_{fwd,dgrad}_ws_bytes per batch>",
             "#   | <arithmetics with equal answers>: [b<batches>:] kind npl kd K/Kpad N/Npad Ck/Ckp nb<nblocks> pin<planes_in> "
             "sup<up2, bn_in, dgrad_bnb supported> B<slot bytes per batch> ; ...   (an arithmetic that is absent has no such site)"]
    for key, ariths in table.items():
        batches = sorted(ws[key])
        line = f"{key} b{','.join(map(str, batches))} ws {once(ws[key][b] for b in batches)}"
        texts = collections.OrderedDict()
        for arith, per in ariths.items():
            by_ans = collections.OrderedDict()
            for b in sorted(per):
                by_ans.setdefault(per[b][0], []).append(b)
            parts = []
            for ans, bs in by_ans.items():
                size = "" if ans.startswith("kind0") else f" B{once(per[b][1] for b in bs)}"
                parts.append((f"b{','.join(map(str, bs))}: " if (len(by_ans) > 1 or sorted(per) != batches) else "") + ans + size)
            texts.setdefault("; ".join(parts), []).append(arith)
        for txt, names in texts.items():
            line += f" | {','.join(names)}: {txt}"
        lines.append(line)
    return lines


if __name__ == "__main__":
    print("\n".join(fold(*rows()) + fold_wgrad(wgrad_rows()) + fold_forms(form_rows())))
