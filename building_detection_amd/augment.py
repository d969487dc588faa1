"""The reference's offline augmentation, data_enhancement.py (`Data_Enhance.run`, :62-135), on the GPU.

The reference writes every training tile plus up to four variants into a second folder, which the training scripts then
read through train_data_gen.  The variants of one source, drawn in this order from one `random.random` sequence:

    _1   r() > 0.2    image and label flipped up-down
    _2   r() > 0.2    image and label flipped left-right
    _3   r() > 0.2    s = randint(6, 20) / 10, n = int(512 * s): image and label resized to n x n (cv.resize INTER_LINEAR),
                      the label thresholded (> 125 -> 255, else 0; `label_`); s < 1: centred on a 512 x 512 canvas of 128
                      (image) / 0 (label) at (512 - n) // 2; else the 512 x 512 crop at max((n - 512) // 2 - 1, 0); then
                      a = r(): 0.4 <= a < 0.7 flips up-down, otherwise b = r() >= 0.7 flips left-right
    _4   r() > 0.7    the image with channels 0 and 2 swapped (cvtColor(BGR2RGB) before imwrite); the label unchanged

and the source itself, always, with an empty suffix.  A variant is written as `stem + suffix + '.png'`, stem =
name.split('.')[0]; train_data_gen over that folder sorts the names as strings and cycles them.

Here the per-tile arithmetic is one kernel (sg_augment_u8, Engine.augment_u8) and the rest is this module:
  * `plan(names, seed)`            the virtual folder: (name, source index, variant) in the order train_data_gen reads it;
  * `device_augment_gen(...)`      that stream as an online stage of the device feed: each source decoded once per batch,
                                   uint8 over PCIe, variants + normalisation + label channels on the device;
  * `Data_Enhance(...).run()`      the reference's offline writer (same class, attribute and method names), lossless PNG.

Two departures from the reference, both deliberate: the draws walk the sources in sorted name order (the reference walks
os.listdir order, which no seed fixes), and two sources whose virtual names could collide (`a.tif` / `a.png`, or `a.png` /
`a_1.png`) raise ValueError (the reference silently overwrites one file with the other).  Sources are 512 x 512 (the WHU
tile size; anything else raises ValueError naming the file) and labels are grey: `_decode_u8` reduces a label file by
BGR2GRAY, which for grey label files is what the reference's three identical channels hold.
"""
from __future__ import annotations

import os
import random
from collections import namedtuple

import numpy as np

from . import _lib
from .input_pipeline import SIZE, Prefetcher, _decode_u8

IMAGE_FILL, LABEL_FILL = 128, 0   # the canvases of random_scale_resize (:116-117)

# suffix: "", "_1" ... "_4"; scale: the s of the rescale (_3) or None; flips / swap as applied to the tile
Variant = namedtuple("Variant", "suffix scale flip_ud flip_lr swap_rb")
Entry = namedtuple("Entry", "name source variant")

_SUFFIXES = ("", "_1", "_2", "_3", "_4")
_ORIGINAL = Variant("", None, False, False, False)


def _stem(name) -> str:
    return os.path.basename(str(name)).split(".")[0]


def scale_geometry(s, size: int = SIZE):
    """random_scale_resize's geometry (:111-126) for the factor s: (n, shift), n = int(size * s) the resized size and
    resized index = canvas index + shift, i.e. shift = -pad of the centred pad (s < 1) or +crop of the crop (s >= 1)."""
    n = int(size * s)
    if s < 1:
        return n, -((size - n) // 2)
    return n, max((n - size) // 2 - 1, 0)


def _check_names(names):
    """ValueError when two sources could write the same virtual file (the reference overwrites one of them)."""
    owner = {}
    for name in names:
        for suffix in _SUFFIXES:
            v = _stem(name) + suffix
            if v in owner:
                raise ValueError(f"sources {owner[v]!r} and {name!r} both map to the augmented file name {v + '.png'!r}")
        for suffix in _SUFFIXES:
            owner[_stem(name) + suffix] = name


def _draw(names, rng: random.Random):
    """One pass of Data_Enhance.run's draws over the sources in sorted name order, as the sorted virtual folder."""
    entries = []
    for i in sorted(range(len(names)), key=lambda k: os.path.basename(str(names[k]))):
        stem = _stem(names[i])
        entries.append(Entry(stem + ".png", i, _ORIGINAL))
        if rng.random() > 0.2:
            entries.append(Entry(stem + "_1.png", i, Variant("_1", None, True, False, False)))
        if rng.random() > 0.2:
            entries.append(Entry(stem + "_2.png", i, Variant("_2", None, False, True, False)))
        if rng.random() > 0.2:
            s = rng.randint(6, 20) / 10
            ud = 0.7 > rng.random() >= 0.4
            lr = (not ud) and rng.random() >= 0.7
            entries.append(Entry(stem + "_3.png", i, Variant("_3", s, ud, lr, False)))
        if rng.random() > 0.7:
            entries.append(Entry(stem + "_4.png", i, Variant("_4", None, False, False, True)))
    entries.sort(key=lambda e: e.name)
    return entries


def plan(image_names, seed=0):
    """The reference's augmented folder as train_data_gen reads it: [(virtual_name, source_index, variant)] sorted by
    name; source_index indexes `image_names` as given.  Pure Python (random.Random(seed)), no GPU."""
    _check_names(image_names)
    return _draw(list(image_names), random.Random(seed))


def item(variant: Variant, label: bool, src: int = 0, size: int = SIZE):
    """(src, n, shift, flags) of sg_augment_u8 for one variant of an image (label=False) or its label."""
    n, shift = (size, 0) if variant.scale is None else scale_geometry(variant.scale, size)
    flags = (_lib.SG_AUG_FLIP_UD if variant.flip_ud else 0) | (_lib.SG_AUG_FLIP_LR if variant.flip_lr else 0)
    if label:
        flags |= _lib.SG_AUG_THRESHOLD if variant.scale is not None else 0
    elif variant.swap_rb:
        flags |= _lib.SG_AUG_SWAP_RB
    return (src, n, shift, flags)


def _decode_512(img, seg):
    """uint8 RGB [512,512,3] and grey [512,512] of one (image, label) pair; ValueError naming a file of another size."""
    rgb, gray = _decode_u8(img, seg, resize=False)
    for path, a in ((img, rgb), (seg, gray)):
        if a.shape[:2] != (SIZE, SIZE):
            raise ValueError(f"{path}: {a.shape[1]} x {a.shape[0]} pixels; the augmentation takes {SIZE} x {SIZE} tiles")
    return rgb, gray


def _augment_sources(engine, rgb_u8, gray_u8, entries, slot):
    """Device uint8 variants (images [N,512,512,3], labels [N,512,512]) of `entries` from the uploaded sources; slot maps
    an entry's source index to its row in the uploaded batch."""
    xi = [item(e.variant, False, slot[e.source]) for e in entries]
    li = [item(e.variant, True, slot[e.source]) for e in entries]
    return engine.augment_u8(rgb_u8, xi, IMAGE_FILL), engine.augment_u8(gray_u8, li, LABEL_FILL)


def device_augment_gen(img_path, lab_path, BATCH_SIZE, engine, seed=0, redraw=False, depth: int = 2, workers: int = 4,
                       separation=None):
    """device_data_gen over the reference's augmented folder, without writing it: the (image, label) pairs sorted and zipped
    as train_data_gen pairs them, the virtual stream of `plan` cycled.  Per batch every distinct source is decoded once
    (`workers` threads, `depth` batches ahead), crosses PCIe as pinned uint8 and is expanded on the device (sg_augment_u8,
    once for the images, once for the labels), then normalised (sg_u8_to_f32) and given its label channels
    (sg_edge_labels).  Yields device tensors x float32 [N,512,512,3], y float32 [N,512,512,4], bit-identical to
    train_data_gen over the folder Data_Enhance would write with the same seed.
    redraw=False repeats that one folder (the reference); redraw=True draws a fresh plan for every cycle, continuing the
    same random.Random(seed) sequence (online augmentation).
    separation=(w0, sigma): Engine.edge_labels adds the separation weight of narrow gaps to f_edge, as in device_data_gen."""
    import torch
    if separation is not None:
        from .data import check_separation
        separation = check_separation(separation)
    from concurrent.futures import ThreadPoolExecutor
    images, label = img_path, lab_path
    images.sort()  # in place, as train_data_gen does
    label.sort()
    pairs = list(zip(images, label))
    names = [p[0] for p in pairs]
    _check_names(names)
    rng = random.Random(seed)

    def stream():
        entries = _draw(names, rng)
        while True:
            yield from entries
            if redraw:
                entries = _draw(names, rng)

    def host_batches():
        virtual = stream()
        with ThreadPoolExecutor(max_workers=max(1, int(workers))) as pool:
            while True:
                batch = [next(virtual) for _ in range(BATCH_SIZE)]
                srcs = list(dict.fromkeys(e.source for e in batch))
                dec = list(pool.map(lambda i: _decode_512(*pairs[i]), srcs))
                xb = torch.from_numpy(np.stack([d[0] for d in dec]))
                lb = torch.from_numpy(np.stack([d[1] for d in dec]))
                if torch.cuda.is_available():
                    xb, lb = xb.pin_memory(), lb.pin_memory()
                yield xb, lb, batch, {s: k for k, s in enumerate(srcs)}

    feed = Prefetcher(host_batches(), depth)
    try:
        for xb, lb, batch, slot in feed:
            xd = xb.to(engine.device, non_blocking=True)
            ld = lb.to(engine.device, non_blocking=True)
            xa, la = _augment_sources(engine, xd, ld, batch, slot)
            x = engine.u8_to_f32(xa, 127.5, 1.0)
            y = engine.edge_labels(engine.u8_to_f32(la, 255.0, 0.0), separation=separation)
            yield x, y
    finally:
        feed.close()


class Data_Enhance:
    """data_enhancement.py's Data_Enhance with the paths as arguments and the draws seeded: run() writes every source of
    read_img_path (its label: the same file name in read_lab_path) and its variants as lossless PNG - the images RGB, the
    labels grey - into save_img_path / save_lab_path, through the same plan and kernel as device_augment_gen."""

    def __init__(self, read_img_path, read_lab_path, save_img_path, save_lab_path, seed=0, engine=None):
        self.img_w = self.img_h = SIZE
        self.read_img_path = read_img_path
        self.read_lab_path = read_lab_path
        self.save_img_path = save_img_path
        self.save_lab_path = save_lab_path
        if not os.path.exists(self.read_img_path) or not os.path.exists(self.read_lab_path):
            raise FileNotFoundError(f"{self.read_img_path} or {self.read_lab_path} does not exist")
        self.mkdirs_path(self.save_img_path)
        self.mkdirs_path(self.save_lab_path)
        self.seed = seed
        self.engine = engine
        self.save_format = ".png"

    def run(self, use_process=True):
        """Writes the augmented folder; use_process=True encodes the PNG files on a pool of writer threads (the reference
        starts one process per pair)."""
        import torch
        from concurrent.futures import ThreadPoolExecutor
        if self.engine is None:
            from .ops import get_engine
            self.engine = get_engine(0)
        names = sorted(os.listdir(self.read_img_path))
        entries = plan(names, self.seed)
        by_source = {}
        for e in entries:
            by_source.setdefault(e.source, []).append(e)
        pool = ThreadPoolExecutor(max_workers=4) if use_process else None
        pending = []
        try:
            for i in sorted(by_source):
                rgb, gray = _decode_512(os.path.join(self.read_img_path, names[i]), os.path.join(self.read_lab_path, names[i]))
                xd = torch.from_numpy(rgb[None].copy()).to(self.engine.device)   # Pillow's arrays are read-only
                ld = torch.from_numpy(gray[None].copy()).to(self.engine.device)
                xa, la = _augment_sources(self.engine, xd, ld, by_source[i], {i: 0})
                xa, la = xa.cpu().numpy(), la.cpu().numpy()
                for k, e in enumerate(by_source[i]):
                    args = (xa[k], la[k], os.path.join(self.save_img_path, e.name), os.path.join(self.save_lab_path, e.name))
                    if pool is None:
                        self.start_process(*args)
                    else:
                        pending.append(pool.submit(self.start_process, *args))
            for f in pending:
                f.result()
        finally:
            if pool is not None:
                pool.shutdown(wait=True)

    def start_process(self, img, lab, img_path, lab_path):
        """Writes one (image, label) pair: RGB and grey PNG, lossless (compression levels 0 and 9, as the reference)."""
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(img)).save(img_path, compress_level=0)
        Image.fromarray(np.ascontiguousarray(lab)).save(lab_path, compress_level=9)

    def mkdirs_path(self, new_path):
        os.makedirs(new_path, exist_ok=True)
