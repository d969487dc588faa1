"""Per-building evaluation on the GPU (csrc/objects.hip through building_detection_amd/objects.py and pipeline.evaluate_objects)
against the numpy / scipy restatement of tests/_objects_ref.py.  Everything is an integer: every comparison is array equality.

Shapes are chosen where the kernels can go wrong.  The labeller works in workgroups of NT = 256 pixels and waves of 64; its
numbering scan has two levels: one workgroup per SCAN_ITEMS = 4096 block counts, then ONE workgroup over the segment totals
(by construction: 256 * 4096 * 2048 = 2^31 pixels is all the ABI admits).  So the first level runs more than one workgroup
from 256 * 4096 + 1 = 1048577 pixels on; MULTI below is the smallest two-dimensional shape with rows of 1024 that has them.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from _guarded import Guarded, check_all, untouched
from _objects_ref import evaluate_ref, label_ref, match_ref, overlaps_ref, scores_ref
from building_detection_amd import _lib

pytestmark = pytest.mark.gpu

NT, SCAN_ITEMS = 256, 4096               # csrc/objects.hip
MULTI = (1025, 1024)
assert (MULTI[0] - 1) * MULTI[1] == NT * SCAN_ITEMS < MULTI[0] * MULTI[1]
SG_EINVAL, SG_EWORKSPACE = -1, -2
FILL = 0xEE                              # prefill of every output: 0xEEEEEEEE is no label, no count, no coordinate


def vp(p):
    return C.c_void_p(p)


# ------------------------------------------------------------------------------------------------------------- patterns
def scene(rng, h, w, n_rect=14, speckle=0.002):
    """The generator of tests/test_cleanup_gpu.py (copied): rotated / overlapping rectangles, corridors, holes (left unfilled
    here), islands, speckle, objects on the image border."""
    m = np.zeros((h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_rect):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        a, b = rng.uniform(8, 70), rng.uniform(8, 70)
        t = rng.uniform(0, np.pi)
        u = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t)
        v = -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
        m |= (np.abs(u) < a) & (np.abs(v) < b)
    for _ in range(6):   # corridors between things
        y, x = rng.integers(0, h - 5), rng.integers(0, w - 5)
        if rng.random() < 0.5:
            m[y:y + rng.integers(2, 9), x:min(w, x + rng.integers(20, 120))] = True
        else:
            m[y:min(h, y + rng.integers(20, 120)), x:x + rng.integers(2, 9)] = True
    for _ in range(8):   # holes, some with islands
        y, x = rng.integers(0, h - 30), rng.integers(0, w - 30)
        m[y:y + rng.integers(4, 28), x:x + rng.integers(4, 28)] = False
        if rng.random() < 0.4:
            m[y + 5:y + 9, x + 5:x + 9] = True
    m ^= rng.random((h, w)) < speckle
    return (m * 255).astype(np.uint8)


def noise(h, w, seed=0, density=0.5):
    return ((np.random.default_rng(seed).random((h, w)) < density) * 255).astype(np.uint8)


def checkerboard(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy + xx) % 2 == 0) * 255).astype(np.uint8)


def serpentine(h, w):
    """A one-pixel-wide path through the whole image: every second row full, joined alternately at the right and left end."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 255
    for k, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if k % 2 == 0 else 0] = 255
    return m


def class_map(h, w, seed=0):
    """Values 1, 2, 3 in touching vertical stripes, with blocks of another class (and of background) set into them."""
    rng = np.random.default_rng(seed)
    m = np.zeros((h, w), np.uint8)
    sw = max(1, w // 7)
    for k in range(0, w, sw):
        m[:, k:k + sw] = (k // sw) % 4          # 0, 1, 2, 3, 0, ...: stripes of different class touch
    for _ in range(12):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[y:y + int(rng.integers(2, 14)), x:x + int(rng.integers(2, 14))] = int(rng.integers(0, 4))
    return m


PATTERNS = {
    "one_pixel_set": lambda: np.full((1, 1), 255, np.uint8),
    "one_pixel_clear": lambda: np.zeros((1, 1), np.uint8),
    "row_300": lambda: noise(1, 300, 1),
    "column_300": lambda: noise(300, 1, 2),
    "empty_37x53": lambda: np.zeros((37, 53), np.uint8),
    "full_37x53": lambda: np.full((37, 53), 255, np.uint8),
    "noise_37x53": lambda: noise(37, 53, 3),
    "noise_96x80": lambda: noise(96, 80, 4),
    "checkerboard_37x53": lambda: checkerboard(37, 53),
    "checkerboard_96x80": lambda: checkerboard(96, 80),
    "serpentine_96x80": lambda: serpentine(96, 80),
    "serpentine_37x53": lambda: serpentine(37, 53),
    "scene_300x257": lambda: scene(np.random.default_rng(1), 300, 257),
    "classes_96x80": lambda: class_map(96, 80, 5),
    "classes_37x53": lambda: class_map(37, 53, 6),
    "noise_multi_scan": lambda: noise(*MULTI, 7),
    "full_multi_scan": lambda: np.full(MULTI, 255, np.uint8),
    "scene_1024x1030": lambda: scene(np.random.default_rng(8), 1024, 1030, n_rect=60),
}
_maps, _refs = {}, {}


def pattern(name):
    """The map and its restatement at both connectivities, built once per session and never changed."""
    if name not in _maps:
        m = PATTERNS[name]()
        m.setflags(write=False)
        _maps[name] = m
        for conn in (4, 8):
            lab, tab = label_ref(m, conn)
            lab.setflags(write=False)
            tab.setflags(write=False)
            _refs[name, conn] = (lab, tab)
    return _maps[name]


def ref_of(name, conn):
    pattern(name)
    return _refs[name, conn]


# ------------------------------------------------------------------------------------------------------------- C ABI
def abi_label(engine, m, conn8, max_objs, table_rows):
    """One guarded sg_objects_label call -> (rc, map, ws, labels, table, count) operands."""
    h, w = m.shape
    dev = engine.device
    gm = Guarded(torch.from_numpy(np.array(m)), dev)
    ws = Guarded.ws(engine.lib.sg_objects_label_ws_bytes(h, w), dev)
    labels = Guarded.out((h, w), torch.int32, dev, fill=FILL)
    table = Guarded.out((table_rows, 8), torch.int32, dev, fill=FILL)
    count = Guarded.out((1,), torch.int32, dev, fill=FILL)
    rc = engine.lib.sg_objects_label(engine.h, engine.stream, h, w, vp(gm.ptr()), conn8, vp(ws.ptr()), ws.nb, vp(labels.ptr()),
                                     vp(table.ptr()), max_objs, vp(count.ptr()))
    torch.cuda.synchronize()
    return rc, gm, ws, labels, table, count


PREFILL_I32 = int(np.frombuffer(bytes([FILL] * 4), np.int32)[0])


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_label_equals_the_restatement(engine, name, conn):
    m = pattern(name)
    ref_lab, ref_tab = ref_of(name, conn)
    n = len(ref_tab)
    rc, gm, ws, labels, table, count = abi_label(engine, m, 1 if conn == 8 else 0, n + 3, n + 5)
    assert rc == 0, _lib.load().sg_last_error()
    check_all([gm, ws, labels, table, count], name)
    assert int(count.read()[0]) == n
    got = labels.read().numpy()
    assert np.array_equal(got, ref_lab), f"{int((got != ref_lab).sum())} labels differ"
    tab = table.read().numpy()
    assert np.array_equal(tab[:n], ref_tab)
    assert (tab[n:] == PREFILL_I32).all(), "table rows that belong to no object were written"
    print(f"{name} conn {conn}: {n} objects")


def test_patterns_are_what_they_are_meant_to_be():
    """The known answers the patterns were chosen for, on the restatement (the GPU is held to it above)."""
    assert len(ref_of("checkerboard_37x53", 8)[1]) == 1 and len(ref_of("checkerboard_37x53", 4)[1]) == (37 * 53 + 1) // 2
    assert len(ref_of("checkerboard_96x80", 8)[1]) == 1 and len(ref_of("checkerboard_96x80", 4)[1]) == 96 * 80 // 2
    for conn in (4, 8):
        tab = ref_of("serpentine_96x80", conn)[1]
        assert len(tab) == 1 and tab[0, 1] == 48 * 80 + 48          # one path through all of the image
        assert len(ref_of("full_37x53", conn)[1]) == 1 and len(ref_of("empty_37x53", conn)[1]) == 0
    assert len(ref_of("noise_96x80", 4)[1]) > 400 and len(ref_of("noise_96x80", 8)[1]) > 30
    assert len(ref_of("noise_multi_scan", 4)[1]) > 60000 and len(ref_of("noise_multi_scan", 8)[1]) > 3000
    # ... and the second workgroup of the first scan level has roots of its own to number
    assert (ref_of("noise_multi_scan", 4)[1][:, 0] >= NT * SCAN_ITEMS).any()
    # holes stay: the scene has background enclosed by an object, and filling would change the areas
    lab, tab = ref_of("scene_300x257", 8)
    from scipy import ndimage as ndi
    assert ndi.binary_fill_holes(lab >= 0).sum() > (lab >= 0).sum()
    # two objects of different class touch (they would be one object for a labeller that only asks "non-zero?")
    for name in ("classes_96x80", "classes_37x53"):
        m = pattern(name)
        lab, tab = ref_of(name, 4)
        a, b = m[:, :-1].astype(int), m[:, 1:].astype(int)
        touch = (a != 0) & (b != 0) & (a != b)
        assert touch.any()
        ya, xa = np.argwhere(touch)[0]
        la, lb = lab[ya, xa], lab[ya, xa + 1]
        assert la >= 0 and lb >= 0 and la != lb and tab[la, 6] != tab[lb, 6]
        assert set(tab[:, 6].tolist()) == {1, 2, 3}


@pytest.mark.parametrize("name,conn,first", [("noise_96x80", 4, 16), ("noise_96x80", 8, 1), ("classes_96x80", 8, 2),
                                             ("noise_multi_scan", 4, 1 << 14)])
def test_python_label_enlarges_its_table_and_repeats(engine, name, conn, first):
    from building_detection_amd import objects as OB
    ref_lab, ref_tab = ref_of(name, conn)
    assert len(ref_tab) > first, "the case is meant to overflow the first table"
    labels, table = OB.label(pattern(name), conn, engine, max_objs=first)
    assert labels.dtype == torch.int32 and labels.is_cuda and table.dtype == np.int32
    assert np.array_equal(labels.cpu().numpy(), ref_lab) and np.array_equal(table, ref_tab)


def test_python_label_input_forms(engine):
    from building_detection_amd import objects as OB
    m = pattern("scene_300x257")
    ref_lab, ref_tab = ref_of("scene_300x257", 8)
    for form in (torch.from_numpy(m.copy()).cuda(), np.repeat(m[:, :, None], 3, 2), m > 0, m.astype(np.float32) / 255,
                 torch.from_numpy(m > 0).cuda()):
        labels, table = OB.label(form, engine=engine)
        assert np.array_equal(labels.cpu().numpy(), ref_lab) and np.array_equal(table, ref_tab)
    cm = pattern("classes_96x80")
    labels, table = OB.label(cm, 4, engine)                       # uint8 is taken as it is: classes stay apart
    assert np.array_equal(labels.cpu().numpy(), ref_of("classes_96x80", 4)[0]) and np.array_equal(table, ref_of("classes_96x80", 4)[1])
    with pytest.raises(ValueError):
        OB.label(m, 6, engine)


def test_label_small_table_leaves_the_rest_alone(engine):
    """max_objs below the object count: labels and count are complete, rows 0 ... max_objs-1 are right, nothing behind them is
    touched."""
    m = pattern("noise_96x80")
    ref_lab, ref_tab = ref_of("noise_96x80", 8)
    n = len(ref_tab)
    for max_objs in (1, 7, n - 1):
        rc, gm, ws, labels, table, count = abi_label(engine, m, 1, max_objs, n + 2)
        assert rc == 0
        check_all([gm, ws, labels, table, count])
        assert int(count.read()[0]) == n and np.array_equal(labels.read().numpy(), ref_lab)
        tab = table.read().numpy()
        assert np.array_equal(tab[:max_objs], ref_tab[:max_objs]) and (tab[max_objs:] == PREFILL_I32).all()


def test_labelling_is_deterministic_on_a_busy_device(engine):
    from building_detection_amd import objects as OB
    m = torch.from_numpy(pattern("scene_1024x1030").copy()).cuda()
    side = torch.cuda.Stream()
    a = torch.rand(1024, 1024, device="cuda")
    runs = []
    for r in range(3):
        if r:   # other work in flight on a second stream while the labeller's atomics run
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(10):
                    b = a @ a
                    a = b / b.max()
        labels, table = OB.label(m, 8, engine)
        runs.append((labels.cpu().numpy().tobytes(), table.tobytes()))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert runs[0] == runs[1] == runs[2]
    n = noise(300, 257, 9)
    x, y = OB.label(n, 4, engine), OB.label(n, 4, engine)
    assert x[0].cpu().numpy().tobytes() == y[0].cpu().numpy().tobytes() and x[1].tobytes() == y[1].tobytes()


# ------------------------------------------------------------------------------------------------------------- overlaps
def shifted(m, dy, dx, seed):
    """A copy moved by (dy, dx) with a few blocks flipped: the other model's / the annotator's view of the same town."""
    rng = np.random.default_rng(seed)
    out = np.roll(m, (dy, dx), (0, 1)).copy()
    h, w = m.shape
    for _ in range(6):
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        out[y:y + int(rng.integers(1, 9)), x:x + int(rng.integers(1, 9))] = 0 if rng.random() < 0.5 else out.max()
    return out


def blob_over_squares():
    a = np.zeros((128, 131), np.uint8)
    a[10:115, 12:120] = 255
    b = np.zeros_like(a)
    for y in range(0, 128, 8):
        for x in range(0, 131, 8):
            b[y:y + 3, x:x + 3] = 255
    return a, b


OVERLAP_CASES = {
    "noise_37x53": lambda: (pattern("noise_37x53"), shifted(pattern("noise_37x53"), 1, 2, 0)),
    "scene_300x257": lambda: (pattern("scene_300x257"), shifted(pattern("scene_300x257"), 3, -5, 1)),
    "classes_96x80": lambda: (pattern("classes_96x80"), shifted(pattern("classes_96x80"), 0, 3, 2)),
    "classes_37x53": lambda: (pattern("classes_37x53"), shifted(pattern("classes_37x53"), 2, 0, 3)),
    "serpentine_vs_noise": lambda: (pattern("serpentine_96x80"), pattern("noise_96x80")),
    "scene_1024x1030": lambda: (pattern("scene_1024x1030"), shifted(pattern("scene_1024x1030"), 4, 7, 4)),
    "blob_over_squares": blob_over_squares,
    "row_300": lambda: (pattern("row_300"), shifted(pattern("row_300"), 0, 1, 5)),
}


def dev_labels(lab):
    return torch.from_numpy(np.array(lab)).cuda()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", list(OVERLAP_CASES))
def test_overlaps_equal_the_restatement(engine, name, conn):
    from building_detection_amd import objects as OB
    a, b = OVERLAP_CASES[name]()
    la, lb = label_ref(a, conn)[0], label_ref(b, conn)[0]
    ref = overlaps_ref(la, lb)
    got = OB.overlaps(dev_labels(la), dev_labels(lb), engine, slots=64)   # small first table: the retry runs too
    assert got.dtype == np.int32 and np.array_equal(got, ref), (got.shape, ref.shape)
    assert len(ref) > 0 and int(ref[:, 2].sum()) == int(((la >= 0) & (lb >= 0)).sum())
    if name == "blob_over_squares":
        partners = np.bincount(ref[:, 0])
        assert partners.max() >= 70, "one object is meant to meet at least 70 others"
    print(f"{name} conn {conn}: {len(ref)} pairs")


def test_overlaps_of_identical_and_disjoint_maps(engine):
    from building_detection_amd import objects as OB
    for name in ("scene_300x257", "noise_96x80", "classes_37x53"):
        lab, tab = ref_of(name, 8)
        got = OB.overlaps(dev_labels(lab), dev_labels(lab), engine)
        want = np.stack([np.arange(len(tab)), np.arange(len(tab)), tab[:, 1]], 1).astype(np.int32)
        assert np.array_equal(got, want)                          # every pair is (k, k, area)
    a = np.zeros((96, 80), np.uint8)
    b = np.zeros((96, 80), np.uint8)
    a[:, :40] = pattern("noise_96x80")[:, :40]
    b[:, 40:] = pattern("noise_96x80")[:, 40:]
    got = OB.overlaps(dev_labels(label_ref(a)[0]), dev_labels(label_ref(b)[0]), engine)
    assert got.shape == (0, 3)
    empty = dev_labels(np.full((37, 53), -1, np.int32))
    assert OB.overlaps(empty, dev_labels(ref_of("noise_37x53", 8)[0]), engine).shape == (0, 3)
    with pytest.raises(ValueError):
        OB.overlaps(empty, dev_labels(ref_of("noise_96x80", 8)[0]), engine)


def abi_overlap(engine, la, lb, slots, list_rows=None):
    h, w = la.shape
    dev = engine.device
    ga, gb = Guarded(torch.from_numpy(np.array(la)), dev), Guarded(torch.from_numpy(np.array(lb)), dev)
    ws = Guarded.ws(engine.lib.sg_objects_overlap_ws_bytes(slots), dev)
    pairs = Guarded.out((list_rows or slots, 3), torch.int32, dev, fill=FILL)
    stat = Guarded.out((2,), torch.int32, dev, fill=FILL)
    rc = engine.lib.sg_objects_overlap(engine.h, engine.stream, h, w, vp(ga.ptr()), vp(gb.ptr()), slots, vp(ws.ptr()), ws.nb,
                                       vp(pairs.ptr()), vp(stat.ptr()))
    torch.cuda.synchronize()
    return rc, ga, gb, ws, pairs, stat


def test_overlap_table_too_small_reports_lost_pixels_and_stays_in_bounds(engine):
    from building_detection_amd import objects as OB
    a, b = OVERLAP_CASES["noise_37x53"]()
    la, lb = label_ref(a, 4)[0], label_ref(b, 4)[0]
    ref = overlaps_ref(la, lb)
    for slots in (1, 16, 128):
        assert len(ref) > slots
        rc, ga, gb, ws, pairs, stat = abi_overlap(engine, la, lb, slots)
        assert rc == 0
        check_all([ga, gb, ws, pairs, stat])                      # the list has exactly `slots` rows: the band starts behind them
        n_pairs, lost = stat.read().tolist()
        assert lost > 0 and 0 < n_pairs <= slots
        rows = pairs.read().numpy()[:n_pairs]
        assert int(rows[:, 2].sum()) + lost == int(ref[:, 2].sum())   # every pixel is either counted or reported lost
    got = OB.overlaps(dev_labels(la), dev_labels(lb), engine, slots=1)
    assert np.array_equal(got, ref)
    # enough slots, exactly: the direct call is complete and the list ends where it should
    slots = 1 << int(np.ceil(np.log2(len(ref))))
    rc, ga, gb, ws, pairs, stat = abi_overlap(engine, la, lb, slots)
    check_all([ga, gb, ws, pairs, stat])
    n_pairs, lost = stat.read().tolist()
    rows = pairs.read().numpy()
    assert lost == 0, "with a slot for every pair the bounded probing must find it"
    assert n_pairs == len(ref) and (rows[n_pairs:] == PREFILL_I32).all()
    rows = rows[:n_pairs]
    assert np.array_equal(rows[np.lexsort((rows[:, 1], rows[:, 0]))], ref)


# ------------------------------------------------------------------------------------------------------------- contract
def test_refused_label_calls_write_nothing(engine):
    m = pattern("noise_37x53")
    h, w = m.shape
    dev = engine.device
    lib = engine.lib
    gm = Guarded(torch.from_numpy(m.copy()), dev)
    need = lib.sg_objects_label_ws_bytes(h, w)
    assert need >= h * w * 4 and lib.sg_objects_label_ws_bytes(0, w) == 0
    ws = Guarded.ws(need, dev)
    outs = [Guarded.out((h, w), torch.int32, dev, fill=FILL), Guarded.out((64, 8), torch.int32, dev, fill=FILL),
            Guarded.out((1,), torch.int32, dev, fill=FILL)]
    good = dict(ctx=engine.h, H=h, W=w, map=gm.ptr(), conn8=1, ws=ws.ptr(), ws_bytes=ws.nb, labels=outs[0].ptr(),
                table=outs[1].ptr(), max_objs=64, count=outs[2].ptr())

    def call(**bad):
        a = dict(good, **bad)
        return lib.sg_objects_label(a["ctx"], engine.stream, a["H"], a["W"], vp(a["map"]), a["conn8"], vp(a["ws"]), a["ws_bytes"],
                                    vp(a["labels"]), vp(a["table"]), a["max_objs"], vp(a["count"]))

    for bad in (dict(ctx=None), dict(map=None), dict(ws=None), dict(labels=None), dict(table=None), dict(count=None), dict(H=0),
                dict(W=0), dict(H=-3), dict(max_objs=0), dict(max_objs=-1), dict(conn8=2), dict(conn8=-1), dict(H=1 << 16, W=1 << 15)):
        assert call(**bad) == SG_EINVAL, bad
        assert lib.sg_last_error()
    assert call(ws_bytes=need - 1) == SG_EWORKSPACE
    assert call(ws_bytes=0) == SG_EWORKSPACE
    torch.cuda.synchronize()
    for g in [gm, ws] + outs:
        untouched(g, "refused sg_objects_label")
    assert call() == 0                                            # and the same operands are good for a real call
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].fetch().read().numpy(), ref_of("noise_37x53", 8)[0])


def test_refused_overlap_calls_write_nothing(engine):
    la = ref_of("noise_37x53", 8)[0]
    h, w = la.shape
    dev = engine.device
    lib = engine.lib
    ga, gb = Guarded(torch.from_numpy(la.copy()), dev), Guarded(torch.from_numpy(la.copy()), dev)
    slots = 1024
    need = lib.sg_objects_overlap_ws_bytes(slots)
    assert need >= slots * 12 and lib.sg_objects_overlap_ws_bytes(0) == 0
    ws = Guarded.ws(need, dev)
    outs = [Guarded.out((slots, 3), torch.int32, dev, fill=FILL), Guarded.out((2,), torch.int32, dev, fill=FILL)]
    good = dict(ctx=engine.h, H=h, W=w, a=ga.ptr(), b=gb.ptr(), slots=slots, ws=ws.ptr(), ws_bytes=ws.nb, pairs=outs[0].ptr(),
                stat=outs[1].ptr())

    def call(**bad):
        a = dict(good, **bad)
        return lib.sg_objects_overlap(a["ctx"], engine.stream, a["H"], a["W"], vp(a["a"]), vp(a["b"]), a["slots"], vp(a["ws"]),
                                      a["ws_bytes"], vp(a["pairs"]), vp(a["stat"]))

    for bad in (dict(ctx=None), dict(a=None), dict(b=None), dict(ws=None), dict(pairs=None), dict(stat=None), dict(H=0), dict(W=-1),
                dict(slots=0), dict(slots=-4), dict(slots=3), dict(slots=1000), dict(slots=(1 << 30) + 1), dict(slots=1 << 31)):
        assert call(**bad) == SG_EINVAL, bad
    assert call(ws_bytes=need - 1) == SG_EWORKSPACE
    assert call(slots=2 * slots) == SG_EWORKSPACE                 # a table of twice the slots does not fit this workspace
    torch.cuda.synchronize()
    for g in [ga, gb, ws] + outs:
        untouched(g, "refused sg_objects_overlap")
    assert call() == 0
    torch.cuda.synchronize()
    n_pairs, lost = outs[1].fetch().read().tolist()
    assert lost == 0 and n_pairs == len(ref_of("noise_37x53", 8)[1])


# ------------------------------------------------------------------------------------------------------------- surface
def binary_pair():
    truth = scene(np.random.default_rng(21), 384, 448, n_rect=12)
    pred = shifted(truth, 2, -3, 6)
    pred[100:140, 200:260] = 255                                  # a false alarm, and with the flips some misses
    return pred, truth


def class_pair():
    truth = class_map(200, 257, 11)
    pred = shifted(truth, 1, 2, 7)
    pred[50:80, 100:130] = 3
    return pred, truth


def same_result(res, matches, counts, tt, iou, **kw):
    want = scores_ref([(matches, counts, tt)], iou, **kw)
    assert (res["tp"], res["fp"], res["fn"]) == (want["tp"], want["fp"], want["fn"])
    for k in ("precision", "recall", "f1", "mean_iou"):
        assert res[k] == want[k] or (np.isnan(res[k]) and np.isnan(want[k])), k
    assert [b["tp"] for b in res["bins"]] == want["bin_tp"] and [b["fn"] for b in res["bins"]] == want["bin_fn"]


@pytest.mark.parametrize("kind", ["binary", "classes"])
@pytest.mark.parametrize("where", ["numpy", "device"])
def test_evaluate_objects_and_object_scores(engine, kind, where):
    from building_detection_amd import objects as OB, pipeline as PL
    pred, truth = binary_pair() if kind == "binary" else class_pair()
    iou = 0.5 if kind == "binary" else 0.3
    matches, counts, tp, tt = evaluate_ref(pred, truth, iou)
    assert counts["tp"] > 0 and counts["fp"] > 0 and counts["fn"] > 0, "the scene is meant to have all three"
    give = (lambda m: torch.from_numpy(m.copy()).cuda()) if where == "device" else (lambda m: m)
    res = PL.evaluate_objects(give(pred), give(truth), iou=iou, engine=engine)
    same_result(res, matches, counts, tt, iou)
    if kind == "classes":
        assert {v: (c["tp"], c["fp"], c["fn"]) for v, c in res["per_class"].items()} == \
               {v: (c["tp"], c["fp"], c["fn"]) for v, c in counts["per_class"].items()} and len(res["per_class"]) == 3
    else:
        assert "per_class" not in res
    # the accumulator over two scenes, with area limits and 4-connectivity
    s = OB.ObjectScores(iou=iou, connectivity=4, min_area_pred=30, min_area_truth=40, engine=engine)
    scenes = []
    for p, t in ((pred, truth), (truth, pred)):
        got_m, got_c = s.update(give(p), give(t))
        m, c, _, tab_t = evaluate_ref(p, t, iou, 4, 30, 40)
        assert [tuple(r) for r in got_m.tolist()] == m and got_c == c
        scenes.append((m, c, tab_t))
    res = s.result()
    want = scores_ref(scenes, iou, min_area_truth=40)
    assert (res["tp"], res["fp"], res["fn"], res["mean_iou"]) == (want["tp"], want["fp"], want["fn"], want["mean_iou"])
    assert [b["tp"] for b in res["bins"]] == want["bin_tp"] and [b["fn"] for b in res["bins"]] == want["bin_fn"]
    assert res["scenes"] == 2


def test_evaluate_objects_clean(engine):
    from building_detection_amd import cleanup as GC, pipeline as PL
    pred, truth = binary_pair()
    cleaned = GC.clean(pred, engine)
    assert not np.array_equal(cleaned, pred), "the clean-up is meant to change this prediction"
    want = PL.evaluate_objects(cleaned, truth, engine=engine)
    got = PL.evaluate_objects(pred, truth, clean=True, engine=engine)
    assert repr(got) == repr(want)
    matches, counts, _, tt = evaluate_ref(cleaned, truth, 0.5)
    same_result(got, matches, counts, tt, 0.5)
    got = PL.evaluate_objects(torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda(), clean=True, engine=engine)
    assert repr(got) == repr(want)
    cp, ct = class_pair()
    with pytest.raises(ValueError, match="a class map"):
        PL.evaluate_objects(cp, ct, clean=True, engine=engine)
    with pytest.raises(ValueError, match="a class map"):
        PL.evaluate_objects(torch.from_numpy(cp).cuda(), ct, clean=True, engine=engine)
