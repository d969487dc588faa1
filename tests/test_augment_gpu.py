"""data_enhancement.py on the device: sg_augment_u8 (Engine.augment_u8), device_augment_gen and Data_Enhance against the
test-side restatement of Data_Enhance.run (tests/_data_enhance_ref.py) and the oracle's train_data_gen, bit for bit."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from building_detection_amd import _lib
from building_detection_amd import augment as A
from oracle import input_pipeline as OIP

import _data_enhance_ref as R

pytestmark = pytest.mark.gpu

UD, LR, RB, THR = _lib.SG_AUG_FLIP_UD, _lib.SG_AUG_FLIP_LR, _lib.SG_AUG_SWAP_RB, _lib.SG_AUG_THRESHOLD


def _label(rng, size=512):
    """Buildings of 255 on 0 with a band of 128 (-> 255 under the threshold at s = 1.0) and scattered 0 / 128 / 255."""
    lab = np.zeros((size, size), np.uint8)
    lab[60:260, 40:300] = 255
    lab[300:340, 100:420] = 128
    lab[400:, 350:] = rng.choice(np.array([0, 128, 255], np.uint8), size=(size - 400, size - 350))
    lab[5, 7] = 128
    return lab


def _sources(tmp_path, names, seed=8):
    rng = np.random.default_rng(seed)
    from PIL import Image
    idir, ldir = tmp_path / "src_img", tmp_path / "src_lab"
    idir.mkdir()
    ldir.mkdir()
    for name in names:
        Image.fromarray(rng.integers(0, 256, size=(512, 512, 3), dtype=np.uint8)).save(idir / name)
        Image.fromarray(_label(rng)).save(ldir / name)
    return str(idir), str(ldir)


def _flip(a, ud, lr):
    return a[::-1] if ud else (a[:, ::-1] if lr else a)


def test_augment_kernel_matches_the_restatement(engine):
    """Every factor 0.6 ... 2.0 with no flip, an up-down and a left-right flip; identity, R-B swap; images (C = 3, fill 128)
    and labels (C = 1, threshold, fill 0) from two sources in one launch each."""
    rng = np.random.default_rng(1)
    imgs = rng.integers(0, 256, size=(2, 512, 512, 3), dtype=np.uint8)
    labs = np.stack([_label(rng), _label(rng)])
    xi, li, want_x, want_y = [], [], [], []
    for k in range(6, 21):
        s = k / 10
        src = k % 2
        i3, l3 = R.scale_pad_crop(imgs[src], labs[src], s)
        n, shift = A.scale_geometry(s)
        for ud, lr in ((False, False), (True, False), (False, True)):
            flags = (UD if ud else 0) | (LR if lr else 0)
            xi.append((src, n, shift, flags))
            li.append((src, n, shift, flags | THR))
            want_x.append(_flip(i3, ud, lr))
            want_y.append(_flip(l3, ud, lr))
    for src, flags in ((0, 0), (1, RB), (0, RB | UD)):       # identity, R-B swap (with a flip)
        xi.append((src, 512, 0, flags))
        li.append((src, 512, 0, flags & ~RB))
        want_x.append(_flip(imgs[src][..., ::-1] if flags & RB else imgs[src], flags & UD, False))
        want_y.append(_flip(labs[src], flags & UD, False))
    assert len(xi) <= _lib.SG_AUGMENT_MAX_ITEMS
    gx = engine.augment_u8(torch.from_numpy(imgs).cuda(), xi, 128).cpu().numpy()
    gy = engine.augment_u8(torch.from_numpy(labs).cuda(), li, 0).cpu().numpy()
    for i in range(len(xi)):
        assert np.array_equal(gx[i], want_x[i]), ("image", xi[i])
        assert np.array_equal(gy[i], want_y[i]), ("label", li[i])
    one = 3 * (10 - 6)                                  # s = 1.0: the identity resize, and still the threshold (128 -> 255)
    assert np.array_equal(gy[one], np.where(labs[0] > 125, 255, 0).astype(np.uint8)) and (labs[0] == 128).any()


def test_augment_kernel_general_geometry(engine):
    """Sizes other than the WHU tile: an exact 2x downscale (cv.resize's INTER_AREA), a pad and a crop into an output row
    that is not a multiple of four pixels (the byte-store path), against the oracle's resize and numpy slicing."""
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, size=(1, 200, 200, 3), dtype=np.uint8)
    items = [(0, 100, 0, 0), (0, 150, -20, LR), (0, 333, 61, UD | RB), (0, 100, 3, THR)]
    got = engine.augment_u8(torch.from_numpy(src).cuda(), items, 17, out_hw=(98, 98)).cpu().numpy()
    for (s, n, shift, flags), g in zip(items, got):
        r = OIP.resize_linear_u8(src[0], (n, n)).astype(np.int64)
        if flags & THR:
            r = np.where(r > 125, 255, 0)
        if flags & RB:
            r = r[..., ::-1]
        canvas = np.full((98, 98, 3), 17, np.int64)
        idx = np.arange(98) + shift
        ok = (idx >= 0) & (idx < n)
        canvas[np.ix_(ok, ok)] = r[np.ix_(idx[ok], idx[ok])]
        assert np.array_equal(g, _flip(canvas, flags & UD, flags & LR).astype(np.uint8)), (n, shift, flags)


def test_device_augment_gen_equals_train_data_gen_over_the_written_folder(engine, tmp_path):
    seed = 4
    names = ["1.png", "10.png", "3.tif"]
    idir, ldir = _sources(tmp_path, names)
    tiles = R.enhance(R.read_sources(idir, ldir), random.Random(seed))
    R.write_folder(tiles, str(tmp_path / "aug_img"), str(tmp_path / "aug_lab"))
    assert sorted(os.listdir(tmp_path / "aug_img")) == [e.name for e in A.plan(names, seed)]
    cycle = len(tiles)
    imgs = [str(tmp_path / "aug_img" / n) for n in sorted(tiles)]
    labs = [str(tmp_path / "aug_lab" / n) for n in sorted(tiles)]
    bs = 4
    host = OIP.data_gen(imgs, labs, bs)
    dev = A.device_augment_gen([os.path.join(idir, n) for n in names], [os.path.join(ldir, n) for n in names], bs, engine,
                               seed=seed, depth=2, workers=3)
    for _ in range(cycle // bs + 2):                       # past the end of the first cycle
        xh, yh = next(host)
        xd, yd = next(dev)
        assert xd.is_cuda and xd.dtype == torch.float32 and yd.dtype == torch.float32
        assert tuple(xd.shape) == (bs, 512, 512, 3) and tuple(yd.shape) == (bs, 512, 512, 4)
        assert np.array_equal(xd.cpu().numpy(), xh)
        assert np.array_equal(yd.cpu().numpy().astype(np.float64), yh)
    dev.close()


def test_data_enhance_writes_the_restated_folder(engine, tmp_path):
    from PIL import Image
    seed = 11
    idir, ldir = _sources(tmp_path, ["1.png", "10.png", "2.png"], seed=3)
    out_i, out_l = str(tmp_path / "out_img"), str(tmp_path / "out_lab")
    A.Data_Enhance(idir, ldir, out_i, out_l, seed=seed, engine=engine).run()
    tiles = R.enhance(R.read_sources(idir, ldir), random.Random(seed))
    assert sorted(os.listdir(out_i)) == sorted(tiles) == sorted(os.listdir(out_l))
    for name, (img, lab, _) in tiles.items():
        with Image.open(os.path.join(out_i, name)) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), img), name
        with Image.open(os.path.join(out_l, name)) as im:
            assert im.mode == "L" and np.array_equal(np.asarray(im), lab), name


def test_redraw_continues_the_random_sequence(engine, tmp_path):
    seed = 6
    names = ["1.png", "10.png"]
    idir, ldir = _sources(tmp_path, names)
    srcs = R.read_sources(idir, ldir)
    rng = random.Random(seed)
    c1, c2 = R.enhance(srcs, rng), R.enhance(srcs, rng)
    assert [c1[k][2] for k in sorted(c1)] != [c2[k][2] for k in sorted(c2)]   # the second cycle is a fresh draw
    want = [c1[k] for k in sorted(c1)] + [c2[k] for k in sorted(c2)]
    bs = 3
    paths = ([os.path.join(idir, n) for n in names], [os.path.join(ldir, n) for n in names])
    runs = []
    for _ in range(2):
        dev = A.device_augment_gen(list(paths[0]), list(paths[1]), bs, engine, seed=seed, redraw=True, depth=1, workers=2)
        runs.append([tuple(t.cpu().numpy() for t in next(dev)) for _ in range(-(-len(want) // bs))])
        dev.close()
    for (x0, y0), (x1, y1) in zip(*runs):                   # deterministic per seed
        assert np.array_equal(x0, x1) and np.array_equal(y0, y1)
    xs = np.concatenate([b[0] for b in runs[0]])
    ys = np.concatenate([b[1] for b in runs[0]])
    for k, (img, lab, _) in enumerate(want):
        x, y = R.xy(img, lab)
        assert np.array_equal(xs[k], x), k
        assert np.array_equal(ys[k].astype(np.float64), y), k


def test_bad_items_and_sources_are_refused_before_a_launch(engine, tmp_path):
    lib = engine.lib
    src = torch.zeros((2, 512, 512, 3), dtype=torch.uint8, device=engine.device)
    dst = torch.full((_lib.SG_AUGMENT_MAX_ITEMS + 1, 512, 512, 3), 7, dtype=torch.uint8, device=engine.device)

    def call(items, c=3, n=None):
        table = (_lib.AugmentItem * len(items))(*[_lib.AugmentItem(*it) for it in items])
        return lib.sg_augment_u8(engine.h, engine.stream, 2, 512, 512, c, C.c_void_p(src.data_ptr()),
                                 len(items) if n is None else n, table, 512, 512, 128, C.c_void_p(dst.data_ptr()))

    good = (0, 512, 0, 0)
    assert call([good, (2, 512, 0, 0)]) == -1                   # source index at S
    assert "source 2" in lib.sg_last_error().decode()
    assert call([good, (-1, 512, 0, 0)]) == -1
    assert call([(0, 0, 0, 0)]) == -1                           # n < 1
    assert call([good, (0, 512, 0, 16)]) == -1                  # unknown flag
    assert call([good] * (_lib.SG_AUGMENT_MAX_ITEMS + 1)) == -1  # over the cap
    assert call([good], c=2) == -1                               # C neither 1 nor 3
    assert call([good], n=0) == -1
    torch.cuda.synchronize()
    assert bool((dst == 7).all()), "a refused call wrote its output"
    with pytest.raises(_lib.SgError, match="sg_augment_u8"):
        engine.augment_u8(src[..., 0].contiguous(), [(0, 512, 0, RB)], 0)   # the swap needs C = 3
    with pytest.raises(_lib.SgError, match="sg_augment_u8"):
        engine.augment_u8(src, [(0, -5, 0, 0)], 128)

    idir, ldir = _sources(tmp_path, ["a.png"])
    from PIL import Image
    Image.fromarray(np.zeros((384, 384, 3), np.uint8)).save(os.path.join(idir, "b.png"))
    Image.fromarray(np.zeros((384, 384), np.uint8)).save(os.path.join(ldir, "b.png"))
    dev = A.device_augment_gen([os.path.join(idir, n) for n in ("a.png", "b.png")],
                               [os.path.join(ldir, n) for n in ("a.png", "b.png")], 64, engine, seed=0)
    with pytest.raises(ValueError, match="b.png"):
        next(dev)
    dev.close()
    with pytest.raises(ValueError, match="b.png"):
        A.Data_Enhance(idir, ldir, str(tmp_path / "o_i"), str(tmp_path / "o_l"), engine=engine).run()


def test_fit_generator_consumes_the_augmented_feed(engine, tmp_path):
    from building_detection_amd import zoo
    from building_detection_amd.losses import edge_focal_loss, PA, IoU, MIoU, F1_score
    names = ["1.png", "2.png"]
    idir, ldir = _sources(tmp_path, names)
    dev = A.device_augment_gen([os.path.join(idir, n) for n in names], [os.path.join(ldir, n) for n in names], 2, engine,
                               seed=1, redraw=True)
    model = zoo.HRNet((512, 512, 3))
    model.compile(optimizer="adam", loss=edge_focal_loss, metrics=[PA, IoU, MIoU, F1_score])
    hist = model.fit_generator(dev, steps_per_epoch=2, epochs=1, verbose=0)
    assert np.isfinite(hist.history["loss"][-1])
    dev.close()
