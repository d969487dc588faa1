"""Multi-scale soft scenes on the GPU: sg_prob_resize_accumulate through the C ABI (tests/_guarded.py arenas) against the
float64 restatement tests/_resize_ref.py:fold, then detection_soft(scales=...) on a tiny model against a host composition of
input_pipeline._resize_bilinear_u8 (cv.resize's INTER_LINEAR), the float64 stitch of tests/_scene_ref.py per scale on the
model's own per-tile probabilities, and the float64 fold.

End to end the probabilities must be within 1e-5 absolute, and the class map equal wherever the reference's two largest
probabilities differ by more than 1e-4; the pixels this exempts must stay below 2 %.  Models of seed 4 (the seed of
tests/test_scene_gpu.py), scene of seed 11."""
import ctypes as C

import numpy as np
import pytest
import torch

import _resize_ref as R
from _guarded import Guarded, check_all, close, ulp32
from _scene_ref import prob_accumulate_ref
from building_detection_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODEL_SEED, SCENE_SEED = 4, 11


def vp(addr):
    return C.c_void_p(addr)


def G(a, role="in"):
    return Guarded(torch.from_numpy(np.ascontiguousarray(a)), DEV, role=role)


def fold_call(engine, C_, ga_s, gw_s, HS, WS, weight, ga, gw, CH, CW):
    return engine.lib.sg_prob_resize_accumulate(engine.h, engine.stream, C_, vp(ga_s.ptr()) if ga_s else None, vp(gw_s.ptr()), HS, WS,
                                                C.c_float(weight), vp(ga.ptr()), vp(gw.ptr()), CH, CW)


def fold_case(C_, HS, WS, CH, CW):
    rng = np.random.default_rng(C_ * 1000 + HS * 10 + CH)
    wsum_s = (0.5 + rng.random((HS, WS), dtype=np.float32)) * 3
    acc_s = rng.random((HS, WS, C_), dtype=np.float32) * wsum_s[..., None]
    wsum_s[HS // 2, :] = 0.0                      # a row the scaled pass never reached ...
    acc_s[HS // 2, :, :] = 1000.0                 # ... whose acc_s holds values that must not show
    acc0 = rng.random((CH, CW, C_), dtype=np.float32)
    wsum0 = rng.random((CH, CW), dtype=np.float32)
    return acc_s, wsum_s, acc0, wsum0


def launch_fold(engine, acc_s, wsum_s, acc0, wsum0, weight, what):
    (HS, WS, C_), (CH, CW) = acc_s.shape, wsum0.shape
    ga_s, gw_s, ga, gw = G(acc_s), G(wsum_s), G(acc0, role="out"), G(wsum0, role="out")
    rc = fold_call(engine, C_, ga_s, gw_s, HS, WS, weight, ga, gw, CH, CW)
    assert rc == 0, f"{what}: rc={rc}: {engine.lib.sg_last_error().decode('utf-8', 'replace')}"
    check_all([ga_s, gw_s, ga, gw], what)
    return ga.read(), gw.read()


FOLD_SHAPES = [(10, 13, 13, 17), (17, 21, 13, 17), (13, 17, 13, 17)]


@pytest.mark.parametrize("HS,WS,CH,CW", FOLD_SHAPES)
@pytest.mark.parametrize("C_", [2, 5])
def test_fold_against_fp64(engine, C_, HS, WS, CH, CW):
    acc_s, wsum_s, acc0, wsum0 = fold_case(C_, HS, WS, CH, CW)
    weight = 0.37
    what = f"fold C={C_} {HS}x{WS} -> {CH}x{CW}"
    ref_acc, ref_wsum = R.fold(acc_s, wsum_s, acc0, wsum0, np.float32(weight))
    acc, wsum = launch_fold(engine, acc_s, wsum_s, acc0, wsum0, weight, what)
    err = close(acc, torch.from_numpy(ref_acc), 2e-5, what)
    werr = close(wsum, torch.from_numpy(ref_wsum), 2e-5, what + " wsum")
    print(f"{what}: acc err {err:.3e}, wsum err {werr:.3e}")
    assert ref_acc.max() < 3.0, "the values beside wsum_s == 0 do not show"
    # a second run gives the same bytes
    again = launch_fold(engine, acc_s, wsum_s, acc0, wsum0, weight, what + " again")
    assert torch.equal(acc.view(torch.uint8), again[0].view(torch.uint8)) and torch.equal(wsum.view(torch.uint8), again[1].view(torch.uint8))
    if (HS, WS) == (CH, CW):
        # normalise-and-add: acc = fma(weight, acc_s / wsum_s, acc0) with the quotient rounded to fp32, to the ulp of the fma
        q = np.where(wsum_s[..., None] > 0, acc_s / np.where(wsum_s > 0, wsum_s, np.float32(1))[..., None], np.float32(0))
        assert q.dtype == np.float32
        want = torch.from_numpy(np.float64(np.float32(weight)) * np.float64(q) + np.float64(acc0))
        assert ((acc.double() - want).abs() <= ulp32(want)).all()
        assert torch.equal(wsum, torch.from_numpy(wsum0 + np.float32(weight)))
        assert torch.equal(acc[HS // 2], torch.from_numpy(acc0[HS // 2])), "fma(w, 0, a) = a where the scaled pass has no weight"


def test_fold_refuses_before_any_launch(engine):
    acc_s, wsum_s, acc0, wsum0 = fold_case(3, 10, 13, 13, 17)
    ga_s, gw_s, ga, gw = G(acc_s), G(wsum_s), G(acc0, role="out"), G(wsum0, role="out")
    ok = dict(C_=3, a=ga_s, HS=10, WS=13, weight=1.0, CH=13, CW=17)
    for change in [dict(C_=1), dict(C_=33), dict(a=None), dict(HS=0), dict(WS=16385), dict(CH=0), dict(CW=16385), dict(weight=0.0),
                   dict(weight=-1.0), dict(weight=float("inf")), dict(weight=float("nan"))]:
        a = dict(ok, **change)
        rc = fold_call(engine, a["C_"], a["a"], gw_s, a["HS"], a["WS"], a["weight"], ga, gw, a["CH"], a["CW"])
        assert rc == -1, f"{change}: rc={rc}"
        assert engine.lib.sg_last_error().decode().startswith("sg_prob_resize_accumulate"), change
    check_all([ga_s, gw_s, ga, gw], "refused folds")
    assert torch.equal(ga.read(), torch.from_numpy(acc0)) and torch.equal(gw.read(), torch.from_numpy(wsum0))
    with pytest.raises(_lib.SgError):                                        # the wrapper: canvases that do not fit each other
        engine.prob_resize_accumulate(torch.zeros(4, 4, 2, device=DEV), torch.zeros(4, 4, device=DEV), torch.zeros(5, 5, 3, device=DEV),
                                      torch.zeros(5, 5, device=DEV))


# ================================================================================================================ end to end
TILE, STRIDE, SCENE_HW = 16, 10, (37, 45)


def tiny_model(size, classes, seed):
    """As tests/test_scene_gpu.py: Conv2D(8, 3, relu) -> Conv2D(8, 3, dilation 3, relu) -> Conv2D(classes, 1, softmax)."""
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
    img[h // 4:h // 2, w // 5:w // 2] //= 3
    return img


def host_multiscale(engine, model, img, scales, scale_weights, window, tta, batch):
    """float64 probabilities [h,w,C]: per scale the host resize, the float64 stitch of the model's own tile probabilities on
    canvases of the scaled size, the float64 fold into the base canvases; sum(w P) / sum(w)."""
    from building_detection_amd import input_pipeline as IP, pipeline as PL
    h, w = img.shape[:2]
    classes = model.num_classes
    win = PL.make_window(window, TILE)
    syms = PL.tta_symmetries(tta)
    acc, wsum = np.zeros((h, w, classes)), np.zeros((h, w))
    for s, sw in zip(scales, scale_weights):
        hs, ws = PL.scaled_size(h, w, s)
        img_s = IP._resize_bilinear_u8(img, (ws, hs))
        dev_s = engine.resize_linear_u8(torch.from_numpy(img).to(DEV)[None], hs, ws)[0]
        assert np.array_equal(dev_s.cpu().numpy(), img_s), f"scale {s}: the device resize differs from the host's"
        _, origins = PL.scene_origins(hs, ws, TILE, STRIDE)
        work = [(i, j, sy) for (i, j) in origins for sy in syms]
        tiles = engine.scene_tiles(torch.from_numpy(img_s).to(DEV), work, TILE)
        P = torch.cat([model.predict_device(tiles[k:k + batch]).float().cpu() for k in range(0, len(work), batch)]).numpy()
        a_s, w_s = np.zeros((hs, ws, classes)), np.zeros((hs, ws))
        prob_accumulate_ref(P, work, win, 1.0, a_s, w_s)
        assert (w_s > 0).all()
        acc, wsum = R.fold(a_s, w_s, acc, wsum, np.float32(sw))
    return acc / wsum[..., None]


@pytest.mark.parametrize("classes", [2, 3])
def test_detection_soft_over_three_scales(engine, classes):
    from building_detection_amd import pipeline as PL
    model, img = tiny_model(TILE, classes, MODEL_SEED), tiny_scene(*SCENE_HW, SCENE_SEED)
    scales = (0.75, 1.0, 1.5)
    assert [PL.scaled_size(*SCENE_HW, s) for s in scales] == [(28, 34), (37, 45), (56, 68)]
    out, probs = PL.detection_soft(img, None, model, tta=2, window="pyramid", stride=STRIDE, return_probs=True, scales=scales, batch=8)
    ref = host_multiscale(engine, model, img, scales, (1.0, 1.0, 1.0), "pyramid", 2, 8)
    assert out.dtype == np.uint8 and out.shape == SCENE_HW and probs.dtype == np.float32 and probs.shape == SCENE_HW + (classes,)
    perr = np.abs(np.float64(probs) - ref).max()
    top = np.sort(ref, axis=-1)
    decided = (top[..., -1] - top[..., -2]) > 1e-4
    share = 1.0 - decided.mean()
    print(f"C={classes}: probabilities off by {perr:.3e}; {100 * share:.2f} % of the pixels are near-ties; classes {np.unique(out).tolist()}")
    assert perr <= 1e-5
    assert share < 0.02
    ref_map = ((255 if classes == 2 else 1) * np.argmax(ref, -1)).astype(np.uint8)
    assert np.array_equal(out[decided], ref_map[decided])
    assert np.abs(probs.sum(-1) - 1).max() <= 1e-5


def test_scale_weights_enter_as_weights_of_normalised_maps(engine):
    from building_detection_amd import pipeline as PL
    model, img = tiny_model(TILE, 2, MODEL_SEED), tiny_scene(*SCENE_HW, SCENE_SEED)
    _, probs = PL.detection_soft(img, None, model, tta=1, window="flat", stride=STRIDE, return_probs=True, scales=(0.75, 1.5),
                                 scale_weights=(2.0, 0.5), batch=3)
    ref = host_multiscale(engine, model, img, (0.75, 1.5), (2.0, 0.5), "flat", 1, 3)
    assert np.abs(np.float64(probs) - ref).max() <= 1e-5


def test_scales_none_is_the_single_scale_path_and_one_scale_of_1_matches_it(engine):
    from building_detection_amd import pipeline as PL
    model, img = tiny_model(TILE, 2, MODEL_SEED), tiny_scene(*SCENE_HW, SCENE_SEED)
    out, probs = PL.detection_soft(img, None, model, tta=2, window="pyramid", stride=STRIDE, return_probs=True)
    scene = PL.SoftScene(img, 2, TILE, STRIDE, "pyramid", engine=engine).add(model, tta=2, weight=1.0, batch=8)
    by_hand, by_hand_probs = scene.result(return_probs=True)
    assert np.array_equal(out, by_hand) and np.array_equal(probs.view(np.uint8), by_hand_probs.view(np.uint8))
    _, one = PL.detection_soft(img, None, model, tta=2, window="pyramid", stride=STRIDE, return_probs=True, scales=(1.0,))
    err = np.abs(np.float64(one) - np.float64(probs)).max()
    print(f"scales=(1.0,) against scales=None: {err:.3e}")
    assert err <= 1e-6


def test_a_scene_takes_passes_of_one_kind_only(engine):
    from building_detection_amd import pipeline as PL
    model, img = tiny_model(TILE, 2, MODEL_SEED), tiny_scene(*SCENE_HW, SCENE_SEED)
    scene = PL.SoftScene(img, 2, TILE, STRIDE, engine=engine).add(model, scale=1.0)
    with pytest.raises(ValueError, match="plain pass"):
        scene.add(model)
    with pytest.raises(ValueError, match="scales"):
        scene.add(model, scale=5.0)
