"""Soft scene inference on the GPU: sg_scene_tiles_u8, sg_prob_accumulate and sg_prob_finalize through the C ABI against the
float64 restatement of tests/_scene_ref.py, then pipeline.SoftScene / detection_soft on a tiny model.

Kernel operands sit in tests/_guarded.py arenas: NaN guard bands, outputs pre-filled with 0xFF (an unwritten float is a NaN);
the bands must be byte-identical after every launch and inputs unchanged.

The accumulate bound, per canvas element with K contributions: |dev - ref| <= (K + 4) * 2^-23 * (|acc0| + sum_k w_k |p_k|) -
the forward-error bound of K fused multiply-adds (K * 2^-24) plus the three roundings of the weight (float scale, two
products: 3 * 2^-24), doubled.  It is derived, not measured.  An element no item reaches keeps its bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from _guarded import Guarded, assert_written, check_all, untouched
from _scene_ref import prob_accumulate_ref, prob_finalize_ref, scene_tiles_ref, sym_map
from building_detection_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 2.0 ** -23
SCENES = ["13x17", "37x29", "ramp"]


def make_scene(name):
    if name == "ramp":                                   # 16 x 16 x 3 = 768 bytes: every byte value three times
        return (np.arange(768) % 256).astype(np.uint8).reshape(16, 16, 3)
    h, w = (int(v) for v in name.split("x"))
    return np.random.default_rng(h * 100 + w).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def table(items, reserved=0):
    return (_lib.SceneItem * len(items))(*[_lib.SceneItem(int(y), int(x), int(s), reserved) for y, x, s in items])


def vp(addr):
    return C.c_void_p(addr)


def call(engine, name, *args):
    return getattr(engine.lib, name)(engine.h, engine.stream, *args)


def ok(engine, rc, what):
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"


def G(a, off=False, role="in"):
    return Guarded(torch.from_numpy(np.ascontiguousarray(a)), DEV, off=off, role=role)


def cutter_items(H, W):
    """All 8 symmetries at an inside, an overhanging, a negative and a fully outside origin."""
    return [(y0, x0, s) for (y0, x0) in [(0, 0), (H - 3, W - 5), (-3, -2), (H + 1, 0)] for s in range(8)]


# ============================================================================================================ 1. the cutter
@pytest.mark.parametrize("off", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("T", [8, 20, 7])                # 7: a row that is no multiple of the four pixels a thread writes
@pytest.mark.parametrize("name", SCENES)
def test_cutter_is_bit_exact(engine, name, T, off):
    scene = make_scene(name)
    H, W = scene.shape[:2]
    items = cutter_items(H, W)
    ref = scene_tiles_ref(scene, items, T)
    if name == "ramp":
        assert set(np.unique(scene)) == set(range(256))
    s, o = G(scene), Guarded.out((len(items), T, T, 3), torch.float32, DEV, off=off)
    rc = call(engine, "sg_scene_tiles_u8", H, W, vp(s.ptr()), len(items), table(items), T, vp(o.ptr()))
    ok(engine, rc, "sg_scene_tiles_u8")
    check_all([s, o], f"cutter {name} T={T}")
    got = o.read()
    assert_written(got, "cutter")
    assert torch.equal(got, torch.from_numpy(ref)), f"{int((got != torch.from_numpy(ref)).sum())} tile elements differ"
    assert (ref[24:] == 0).all() and (ref[:8] != 0).any()     # the fully outside origin is all padding


def test_cutter_wrapper_takes_65_items_in_two_launches(engine):
    scene = make_scene("37x29")
    items = [((7 * i) % 40 - 4, (5 * i) % 33 - 3, i % 8) for i in range(65)]
    assert len(items) > _lib.SG_SCENE_MAX_ITEMS
    got = engine.scene_tiles(torch.from_numpy(scene).to(DEV), items, 8)
    assert got.dtype == torch.float32 and tuple(got.shape) == (65, 8, 8, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(scene_tiles_ref(scene, items, 8)))
    with pytest.raises(_lib.SgError):
        engine.scene_tiles(torch.from_numpy(scene), items, 8)             # a CPU tensor
    with pytest.raises(_lib.SgError):
        engine.scene_tiles(torch.from_numpy(scene).to(DEV).float(), items, 8)


# ===================================================================================================== 2. / 3. the soft stitch
def stitch_items(CH, CW, T):
    """12 items: one origin under three symmetries, overlapping neighbours, clipped and fully outside windows."""
    return [(0, 0, 0), (0, 0, 5), (0, 0, 3), (2, 3, 1), (2, 3, 6), (T // 2, T // 2, 2), (T // 2, 1, 7), (CH - 3, CW - 5, 4),
            (-3, -2, 0), (CH + 1, 0, 1), (-T, 0, 2), (1, CW - T // 2, 3)]


def stitch_case(C_, T, CH, CW, seed=0):
    rng = np.random.default_rng(seed + C_ * 1000 + T * 10 + CH)
    items = stitch_items(CH, CW, T)
    p = rng.random((len(items), T, T, C_), dtype=np.float32)
    win = (0.1 + 0.9 * rng.random(T)).astype(np.float32)            # strictly positive, not symmetric
    acc0 = rng.random((CH, CW, C_), dtype=np.float32)
    wsum0 = rng.random((CH, CW), dtype=np.float32)
    return items, p, win, acc0, wsum0


def launch_stitch(engine, items, p, win, acc0, wsum0, scale, splits, off=False):
    """The item list as consecutive launches of the given sizes; returns (acc, wsum) read back after the guard checks."""
    C_, T = p.shape[3], p.shape[1]
    CH, CW = wsum0.shape
    gp, gw = G(p), G(win)
    ga, gs = G(acc0, off=off, role="out"), G(wsum0, role="out")
    i0 = 0
    for n in splits:
        rc = call(engine, "sg_prob_accumulate", C_, T, vp(gp.ptr(i0 * T * T * C_)), n, table(items[i0:i0 + n]), vp(gw.ptr()),
                  C.c_float(scale), vp(ga.ptr()), vp(gs.ptr()), CH, CW)
        ok(engine, rc, "sg_prob_accumulate")
        i0 += n
    assert i0 == len(items)
    check_all([gp, gw, ga, gs], f"stitch C={C_} T={T}")
    return ga.read(), gs.read()


def check_stitch(acc, wsum, ref_acc, ref_wsum, state, acc0, wsum0, what=""):
    """The derived bound on every element; untouched elements keep their bits.  acc / wsum: float32 arrays."""
    mag, wmag, cnt = state
    acc, wsum = np.asarray(acc, np.float64), np.asarray(wsum, np.float64)
    assert np.isfinite(acc).all() and np.isfinite(wsum).all(), what
    err, bound = np.abs(acc - ref_acc), (cnt[..., None] + 4) * EPS * mag
    werr, wbound = np.abs(wsum - ref_wsum), (cnt + 4) * EPS * wmag
    print(f"{what}: K <= {int(cnt.max())}, worst acc err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}, "
          f"wsum {float((werr / np.maximum(wbound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} acc elements beyond the bound"
    assert (werr <= wbound).all(), f"{what}: {int((werr > wbound).sum())} wsum elements beyond the bound"
    none = cnt == 0
    assert np.array_equal(acc[none], np.float64(acc0)[none]) and np.array_equal(wsum[none], np.float64(wsum0)[none]), what


STITCH_CASES = [(c, t, ch, cw, False) for c in (2, 3, 5, 32) for t in (8, 20) for (ch, cw) in ((13, 17), (37, 29))]
STITCH_CASES += [(2, 8, 13, 17, True), (2, 20, 37, 29, True)]     # C = 2 off the 8-byte alignment: the one-float form


@pytest.mark.parametrize("C_,T,CH,CW,off", STITCH_CASES)
def test_accumulate_against_fp64(engine, C_, T, CH, CW, off):
    items, p, win, acc0, wsum0 = stitch_case(C_, T, CH, CW)
    ref_acc, ref_wsum = np.float64(acc0), np.float64(wsum0)
    state = prob_accumulate_ref(p, items, win, 0.37, ref_acc, ref_wsum)
    assert state[2].max() >= 5 and (state[2] == 0).any() == (CH > T + 3)     # deep overlaps; untouched pixels on the larger canvas
    acc, wsum = launch_stitch(engine, items, p, win, acc0, wsum0, 0.37, [len(items)], off=off)
    check_stitch(acc.numpy(), wsum.numpy(), ref_acc, ref_wsum, state, acc0, wsum0, f"C={C_} T={T} {CH}x{CW}")


@pytest.mark.parametrize("C_,off", [(2, False), (2, True), (3, False), (32, False)])
def test_order_does_not_depend_on_the_split_into_launches(engine, C_, off):
    items, p, win, acc0, wsum0 = stitch_case(C_, 8, 13, 17, seed=5)
    one = launch_stitch(engine, items, p, win, acc0, wsum0, 0.37, [12], off=off)
    for splits in ([1] * 12, [5, 7], [12]):
        acc, wsum = launch_stitch(engine, items, p, win, acc0, wsum0, 0.37, splits, off=off)
        assert torch.equal(acc, one[0]) and torch.equal(wsum, one[1]), f"launches of {splits} differ from one launch"
    assert not torch.equal(one[0], torch.from_numpy(acc0))


# ============================================================================================================== 4. finalize
def finalize_case(C_, CH=13, CW=17):
    rng = np.random.default_rng(40 + C_)
    acc = rng.random((CH, CW, C_), dtype=np.float32) * 3
    wsum = (0.5 + rng.random((CH, CW), dtype=np.float32)) * 2
    acc[0, :5, :] = 0.75                                  # every class ties: class 0
    acc[1, :5, :] = 0.25
    acc[1, :5, C_ - 1] = 2.0                              # the last class alone
    if C_ >= 4:
        acc[2, :5, :] = 0.25
        acc[2, :5, 1] = acc[2, :5, 3] = 2.0               # two equal maxima: the lower index
    wsum[3, :4] = 0.0                                     # no tile reached these pixels (acc keeps values: they must not show)
    acc[4, 0, :] = 0.0
    wsum[4, 0] = 0.0
    return acc, wsum


@pytest.mark.parametrize("C_,out_scale", [(2, 255), (5, 1)])
@pytest.mark.parametrize("mode", ["probs", "null", "inplace"])
def test_finalize(engine, C_, out_scale, mode):
    acc, wsum = finalize_case(C_)
    CH, CW = wsum.shape
    ref_map, ref_probs = prob_finalize_ref(acc, wsum, out_scale)
    assert ref_map[0, 0] == 0 and ref_map[1, 0] == out_scale * (C_ - 1) and (ref_map[3, :4] == 0).all()
    assert C_ < 4 or ref_map[2, 0] == out_scale
    ga, gs = G(acc, role="out" if mode == "inplace" else "in"), G(wsum)
    gm = Guarded.out((CH, CW), torch.uint8, DEV)
    gp = Guarded.out((CH, CW, C_), torch.float32, DEV) if mode == "probs" else None
    pp = {"probs": gp.ptr() if gp else None, "null": None, "inplace": ga.ptr()}[mode]
    rc = call(engine, "sg_prob_finalize", C_, vp(ga.ptr()), vp(gs.ptr()), CH, CW, vp(pp), out_scale, vp(gm.ptr()))
    ok(engine, rc, "sg_prob_finalize")
    check_all([g for g in (ga, gs, gm, gp) if g is not None], f"finalize {mode}")
    assert np.array_equal(gm.read().numpy(), ref_map)
    if mode != "null":
        probs = np.float64((gp if mode == "probs" else ga).read().numpy())
        assert np.isfinite(probs).all()
        assert (np.abs(probs - ref_probs) <= EPS * np.abs(ref_probs)).all()
        assert (probs[3, :4] == 0).all() and (probs[4, 0] == 0).all()


# ============================================================================================================= 5. arguments
def test_bad_arguments_are_refused_before_any_launch(engine):
    scene = make_scene("13x17")
    T, C_, CH, CW = 8, 3, 13, 17
    items, p, win, acc0, wsum0 = stitch_case(C_, T, CH, CW)
    gsc, gp, gw = G(scene), G(p), G(win)
    tiles = Guarded.out((12, T, T, 3), torch.float32, DEV)
    ga, gs = G(acc0, role="out"), G(wsum0, role="out")
    gm = Guarded.out((CH, CW), torch.uint8, DEV)
    big = [(0, 0, 0)] * 65
    sc, ti, pp, wi, ac, ws, mp = (vp(g.ptr()) for g in (gsc, tiles, gp, gw, ga, gs, gm))

    def cut(N=12, tab=None, T_=T, scene_ptr=sc, out=ti):
        return call(engine, "sg_scene_tiles_u8", 13, 17, scene_ptr, N, table(items) if tab is None else tab, T_, out)

    def acc(N=12, tab=None, T_=T, c=C_, p_ptr=pp):
        return call(engine, "sg_prob_accumulate", c, T_, p_ptr, N, table(items) if tab is None else tab, wi, C.c_float(1.0),
                    ac, ws, CH, CW)

    def fin(c=C_, out_scale=1, acc_ptr=ac):
        return call(engine, "sg_prob_finalize", c, acc_ptr, ws, CH, CW, None, out_scale, mp)

    bad = [("sg_scene_tiles_u8", lambda: cut(N=0)), ("sg_scene_tiles_u8", lambda: cut(N=65, tab=table(big))),
           ("sg_scene_tiles_u8", lambda: cut(N=1, tab=table([(0, 0, 8)]))),
           ("sg_scene_tiles_u8", lambda: cut(N=1, tab=table([(0, 0, 0)], reserved=1))),
           ("sg_scene_tiles_u8", lambda: cut(T_=0)), ("sg_scene_tiles_u8", lambda: cut(scene_ptr=None)),
           ("sg_scene_tiles_u8", lambda: cut(out=None)), ("sg_scene_tiles_u8", lambda: cut(tab=C.c_void_p(None))),
           ("sg_scene_tiles_u8", lambda: cut(N=1, tab=table([(1 << 30, 0, 0)]))),
           ("sg_prob_accumulate", lambda: acc(N=0)), ("sg_prob_accumulate", lambda: acc(N=65, tab=table(big))),
           ("sg_prob_accumulate", lambda: acc(N=1, tab=table([(0, 0, 8)]))),
           ("sg_prob_accumulate", lambda: acc(N=1, tab=table([(0, 0, -1)]))),
           ("sg_prob_accumulate", lambda: acc(N=1, tab=table([(0, 0, 0)], reserved=7))),
           ("sg_prob_accumulate", lambda: acc(T_=0)), ("sg_prob_accumulate", lambda: acc(c=1)),
           ("sg_prob_accumulate", lambda: acc(c=33)), ("sg_prob_accumulate", lambda: acc(p_ptr=None)),
           ("sg_prob_finalize", lambda: fin(c=1)), ("sg_prob_finalize", lambda: fin(c=33)),
           ("sg_prob_finalize", lambda: fin(out_scale=255)), ("sg_prob_finalize", lambda: fin(out_scale=0)),
           ("sg_prob_finalize", lambda: fin(acc_ptr=None))]
    for name, fn in bad:
        with pytest.raises(_lib.SgError, match=name):
            _lib.check(fn(), name)
    torch.cuda.synchronize()
    for g in (tiles, ga, gs, gm, gsc, gp, gw):           # nothing was launched
        untouched(g, "refused call")
    # ... and valid calls still work
    ok(engine, cut(), "sg_scene_tiles_u8")
    ok(engine, acc(), "sg_prob_accumulate")
    ok(engine, fin(), "sg_prob_finalize")
    assert torch.equal(tiles.fetch().read(), torch.from_numpy(scene_tiles_ref(scene, items, T)))
    ra, rw = np.float64(acc0), np.float64(wsum0)
    state = prob_accumulate_ref(p, items, win, 1.0, ra, rw)
    check_stitch(ga.fetch().read().numpy(), gs.fetch().read().numpy(), ra, rw, state, acc0, wsum0, "after refusals")
    assert np.array_equal(gm.fetch().read().numpy(), prob_finalize_ref(ga.read().numpy(), gs.read().numpy(), 1)[0])
    with pytest.raises(_lib.SgError):                    # the wrapper takes fp32 probabilities only
        engine.prob_accumulate(torch.zeros(1, 8, 8, 2, device=DEV, dtype=torch.bfloat16), [(0, 0, 0)], torch.ones(8, device=DEV),
                               torch.zeros(9, 9, 2, device=DEV), torch.zeros(9, 9, device=DEV))


# =============================================================================================================== 6. pipeline
def tiny_model(size, classes, seed):
    """Conv2D(8, 3, relu) -> Conv2D(8, 3, dilation 3, relu) -> Conv2D(classes, 1, softmax); the head bias nudged so that all
    classes occur (as tests/test_pipeline_gpu.py does)."""
    from building_detection_amd import layers as L
    from building_detection_amd.runtime import Model
    inp = L.Input((size, size, 3))
    x = L.Conv2D(8, 3, padding="same", activation="relu")(inp)
    x = L.Conv2D(8, 3, padding="same", dilation_rate=3, activation="relu")(x)
    out = L.Conv2D(classes, 1, activation="softmax")(x)
    model = Model(inp, out, name=f"tiny{size}c{classes}s{seed}", seed=seed)
    ws = model.get_weights()
    ws[5] = np.linspace(0.0, 0.02, classes).astype(np.float32)
    model.set_weights(ws)
    return model


def tiny_scene(h, w, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[h // 4:h // 2, w // 5:w // 2] //= 3               # a darker blob, so the result is not pure noise
    return img


def host_tiles(img, work, tile, stride):
    """The tiles as detection() cuts them on the host (float64 canvas, zero padding, float32 cast), then the symmetry."""
    from building_detection_amd import pipeline as PL
    h, w = img.shape[:2]
    (ch, cw), _ = PL.scene_origins(h, w, tile, stride)
    canvas = np.zeros((ch, cw, 3))
    canvas[:h, :w, :] = img.astype(np.float64) / 127.5 - 1
    out = np.empty((len(work), tile, tile, 3), np.float32)
    for n, (i, j, sym) in enumerate(work):
        base = canvas[i:i + tile, j:j + tile, :].astype(np.float32)
        r, c, u, v = sym_map(sym, tile)
        out[n, r, c, :] = base[u, v, :]
    return out


def soft_scene_checks(engine, models, weights, tta, window, batch, classes):
    """SoftScene over a 150 x 170 scene at tile 64 / stride 40 against the float64 stitch of the ENGINE'S OWN per-tile
    probabilities: no model tolerance and no near-tie exclusion enters."""
    from building_detection_amd import pipeline as PL
    tile, stride = 64, 40
    img = tiny_scene(150, 170, 11)
    scene = PL.SoftScene(img, classes, tile, stride, window, engine=engine)
    _, origins = PL.scene_origins(150, 170, tile, stride)
    syms = {8: list(range(8)), 2: [0, 2], 1: [0]}[tta]
    work = [(i, j, s) for (i, j) in origins for s in syms]           # origins-major, then symmetries
    assert len(origins) == 16 and scene.work_list(tta) == work
    tiles = engine.scene_tiles(scene.scene, work, tile)
    assert torch.equal(tiles.cpu(), torch.from_numpy(host_tiles(img, work, tile, stride))), "device tiles differ from the host cut"
    win = scene.win.cpu().numpy()
    ref_acc, ref_wsum, state = np.zeros((150, 170, classes)), np.zeros((150, 170)), None
    for m, wt in zip(models, weights):
        # the engine's own probabilities, tile batches as add() forms them
        P = torch.cat([m.predict_device(tiles[s:s + batch]).float().cpu() for s in range(0, len(work), batch)]).numpy()
        assert P.shape == (len(work), tile, tile, classes)
        state = prob_accumulate_ref(P, work, win, wt, ref_acc, ref_wsum, state)
        scene.add(m, tta=tta, weight=wt, batch=batch)
    zero = np.zeros_like
    check_stitch(scene.acc.cpu().numpy(), scene.wsum.cpu().numpy(), ref_acc, ref_wsum, state, zero(ref_acc, np.float32),
                 zero(ref_wsum, np.float32), f"SoftScene tta={tta} C={classes}")
    K = state[2]
    assert K.min() >= len(models) * len(syms)
    out, probs = scene.result(return_probs=True)
    assert out.dtype == np.uint8 and out.shape == (150, 170) and probs.dtype == np.float32 and probs.shape == (150, 170, classes)
    perr = np.abs(np.float64(probs) - ref_acc / ref_wsum[..., None])
    assert (perr <= (2 * K[..., None] + 10) * EPS).all(), f"probabilities off by up to {perr.max():.3e}"
    acc_back = scene.acc.cpu().numpy()
    assert np.array_equal(out, ((255 if classes == 2 else 1) * np.argmax(acc_back, -1)).astype(np.uint8))
    assert np.array_equal(out, scene.result())
    print(f"classes in the result: {np.unique(out).tolist()}")
    return img, out, probs


def test_soft_scene_tta8_pyramid(engine):
    _, out, _ = soft_scene_checks(engine, [tiny_model(64, 2, 4)], [1.0], 8, "pyramid", 5, 2)
    assert set(np.unique(out)) <= {0, 255}


def test_soft_scene_does_not_depend_on_the_batch(engine):
    from building_detection_amd import pipeline as PL
    model, img = tiny_model(64, 2, 4), tiny_scene(150, 170, 11)
    a = PL.SoftScene(img, 2, 64, 40, "pyramid", engine=engine).add(model, tta=8, batch=3)
    b = PL.SoftScene(img, 2, 64, 40, "pyramid", engine=engine).add(model, tta=8, batch=8)
    assert torch.equal(a.acc, b.acc) and torch.equal(a.wsum, b.wsum)


def test_soft_ensemble_of_two_models(engine, tmp_path):
    from building_detection_amd import pipeline as PL
    models = [tiny_model(64, 2, 4), tiny_model(64, 2, 9)]
    img, out, probs = soft_scene_checks(engine, models, [1.0, 0.5], 2, "flat", 8, 2)
    got, gp = PL.detection_soft(img, str(tmp_path), models, "soft", batch=8, tta=2, weights=[1.0, 0.5], stride=40,
                                return_probs=True)
    assert np.array_equal(got, out) and np.array_equal(gp, probs)
    from PIL import Image
    assert np.array_equal(np.asarray(Image.open(tmp_path / "soft.png")), out)
    with pytest.raises(ValueError):
        PL.detection_soft(img, None, models, tta=2)                       # tile 64 has no default stride


def test_soft_scene_three_classes(engine):
    _, out, _ = soft_scene_checks(engine, [tiny_model(64, 3, 4)], [1.0], 8, "pyramid", 5, 3)
    assert out.dtype == np.uint8 and set(np.unique(out)) <= {0, 1, 2}


def test_one_tile_flat_equals_the_hard_path(engine):
    """One 512-px tile of weight 1: fmaf(1, p, 0) = p and the same tie rule, so the soft mask is detection()'s."""
    from building_detection_amd import pipeline as PL
    model = tiny_model(512, 2, 4)
    img = tiny_scene(512, 512, 3)
    soft = PL.detection_soft(img, None, model, tta=1, window="flat")
    hard = PL.detection(img, None, model)
    assert soft.dtype == np.uint8 and np.array_equal(soft, hard)
    print(f"{int((soft == 255).sum())} of {soft.size} pixels are building")


def test_soft_scene_refuses_a_model_that_does_not_fit(engine):
    from building_detection_amd import pipeline as PL
    img = tiny_scene(150, 170, 11)
    with pytest.raises(ValueError, match="tile"):
        PL.SoftScene(img, 2, 64, 40, engine=engine).add(tiny_model(32, 2, 4))
    with pytest.raises(ValueError, match="classes"):
        PL.SoftScene(img, 2, 64, 40, engine=engine).add(tiny_model(64, 3, 4))
