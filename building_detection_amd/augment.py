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

Beyond the reference (second half of this module): online random augmentation.  `RandomPolicy` says what may
happen to a sample, `draw(policy, seed, k)` decides it for sample k from a counter-based generator, `warp_items` turns the
decision into the integer items of sg_warp_u8 (Engine.warp_u8: affine warp, colour matrix, tone table, noise), and
`device_random_gen` is the feed on top: sources of any size, reproducible per sample, sharded and resumable.
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


# ---- not in the reference: online random augmentation ----------------------------------------------------------
# One kernel (sg_warp_u8, Engine.warp_u8) warps and jitters; everything random is decided here, per sample, by a counter-based
# generator: draw(policy, seed, k) is a pure function, so sample k of the stream looks the same whatever the batch size, the
# worker count, the prefetch depth, the rank or the restart point.
_M0, _M1, _W0, _W1, _MASK32 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
DRAW_STREAM = 0x64726177          # "draw": counter word 3 of the parameter draws (the kernel's noise uses SG_WARP_NOISE_STREAM)
NOISE_T_STD = (4 * (256 ** 2 - 1) / 12) ** 0.5   # 147.80: the standard deviation of the kernel's t (include/segengine.h)
_LUMA = (0.299, 0.587, 0.114)


def philox4x32_10(counter, key):
    """Philox4x32-10 in plain Python integers (the round function of csrc/sg_philox.h): four counter words and two key words
    in, four 32-bit words out."""
    c0, c1, c2, c3 = (int(c) & _MASK32 for c in counter)
    k0, k1 = (int(k) & _MASK32 for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK32
        k0, k1 = (k0 + _W0) & _MASK32, (k1 + _W1) & _MASK32
    return c0, c1, c2, c3


_POLICY_FIELDS = ("rotate", "scale", "shear", "translate", "flip", "brightness", "contrast", "saturation", "gamma", "hue", "noise",
                  "swap_rb", "border", "p_geometric", "p_photometric")


class RandomPolicy(namedtuple("RandomPolicy", _POLICY_FIELDS)):
    """What device_random_gen may do to a sample; every option is off by default.
      rotate       degrees; the angle is uniform in [-rotate, rotate]                       0 <= rotate <= 180
      scale        (lo, hi); the zoom is log-uniform in [lo, hi] (> 1 enlarges the objects)   1/16 <= lo <= hi <= 16
      shear        degrees; the x-shear angle is uniform in [-shear, shear]                  0 <= shear <= 60
      translate    fraction of the crop; both shifts are uniform in [-translate, translate]  0 <= translate <= 4
      flip         True: one of the eight symmetries of the square, equiprobable
      brightness   b uniform in [-brightness, brightness], added on the 0 .. 1 scale          0 <= brightness <= 1
      contrast     factor uniform in [1 - contrast, 1 + contrast] about mid-grey             0 <= contrast < 1
      saturation   factor uniform in [1 - saturation, 1 + saturation] about the luma         0 <= saturation <= 1
      gamma        exponent log-uniform in [1 / (1 + gamma), 1 + gamma]                      0 <= gamma <= 3
      hue          degrees; rotation about the grey axis, uniform in [-hue, hue]             0 <= hue <= 180
      noise        sigma of the sensor noise in grey levels                                  0 <= noise <= 64
      swap_rb      probability of swapping channels 0 and 2
      border       "constant" (image 128, label 0, as the offline augmentation's canvas) or "reflect"
      p_geometric, p_photometric   probability that the geometric / the photometric group applies at all
    Bad values raise ValueError here."""
    __slots__ = ()

    def __new__(cls, rotate=0.0, scale=(1.0, 1.0), shear=0.0, translate=0.0, flip=False, brightness=0.0, contrast=0.0,
                saturation=0.0, gamma=0.0, hue=0.0, noise=0.0, swap_rb=0.0, border="constant", p_geometric=1.0, p_photometric=1.0):
        def num(name, v, lo, hi, open_hi=False):
            try:
                f = float(v)
            except (TypeError, ValueError):
                raise ValueError(f"RandomPolicy: {name} = {v!r} is not a number") from None
            if not (lo <= f <= hi) or (open_hi and f == hi):   # NaN fails the first test
                raise ValueError(f"RandomPolicy: {name} = {v!r} outside [{lo}, {hi}{')' if open_hi else ']'}")
            return f
        try:
            lo, hi = scale
        except (TypeError, ValueError):
            raise ValueError(f"RandomPolicy: scale = {scale!r} is not a (lo, hi) pair") from None
        lo, hi = num("scale[0]", lo, 1 / 16, 16), num("scale[1]", hi, 1 / 16, 16)
        if lo > hi:
            raise ValueError(f"RandomPolicy: scale = {scale!r}: lo > hi")
        if border not in ("constant", "reflect"):
            raise ValueError(f"RandomPolicy: border = {border!r} (\"constant\" or \"reflect\")")
        if not isinstance(flip, (bool, np.bool_)):
            raise ValueError(f"RandomPolicy: flip = {flip!r} is not a bool")
        return super().__new__(cls, num("rotate", rotate, 0, 180), (lo, hi), num("shear", shear, 0, 60),
                               num("translate", translate, 0, 4), bool(flip), num("brightness", brightness, 0, 1),
                               num("contrast", contrast, 0, 1, True), num("saturation", saturation, 0, 1), num("gamma", gamma, 0, 3),
                               num("hue", hue, 0, 180), num("noise", noise, 0, 64), num("swap_rb", swap_rb, 0, 1), border,
                               num("p_geometric", p_geometric, 0, 1), num("p_photometric", p_photometric, 0, 1))


# angle, shear, hue in degrees; tx, ty in crops; sym: SG_SYM_* bits (1 up-down, 2 left-right, 4 transpose); brightness on
# the 0 .. 1 scale; contrast, saturation factors; gamma the exponent; noise the sigma in grey levels
Params = namedtuple("Params", "sample angle scale shear tx ty sym brightness contrast saturation gamma hue swap_rb noise border")

# the uniform that decides each parameter: a fixed word of the sample's draws, so switching one option on moves no other
_U = {k: i for i, k in enumerate(("geometric", "angle", "scale", "shear", "tx", "ty", "sym", "photometric", "brightness", "contrast",
                                  "saturation", "gamma", "hue", "swap_rb"))}


def _uniforms(seed, sample, n):
    """n uniforms (word + 0.5) / 2^32 in (0, 1) of sample `sample`: blocks j = 0, 1, ... of Philox4x32-10 at counter
    (j, sample mod 2^32, sample >> 32, DRAW_STREAM), key (seed mod 2^32, seed >> 32)."""
    seed, sample = int(seed) & (2 ** 64 - 1), int(sample) & (2 ** 64 - 1)
    words = []
    for j in range(-(-n // 4)):
        words += philox4x32_10((j, sample & _MASK32, sample >> 32, DRAW_STREAM), (seed & _MASK32, seed >> 32))
    return [(w + 0.5) / 4294967296.0 for w in words[:n]]


def draw(policy: RandomPolicy, seed, sample) -> Params:
    """The parameters of sample `sample` (its 64-bit number in the endless stream) under `policy`: a pure function of
    (policy, seed, sample), with no state and no dependence on the order of calls."""
    import math
    u = _uniforms(seed, sample, len(_U))
    sym_pm = lambda name, r: (2.0 * u[_U[name]] - 1.0) * r   # uniform in (-r, r)
    geo = u[_U["geometric"]] < policy.p_geometric
    pho = u[_U["photometric"]] < policy.p_photometric
    lo, hi = policy.scale
    return Params(
        sample=int(sample) & (2 ** 64 - 1),
        angle=sym_pm("angle", policy.rotate) if geo else 0.0,
        scale=min(max(math.exp(math.log(lo) + u[_U["scale"]] * (math.log(hi) - math.log(lo))), lo), hi) if geo else 1.0,
        shear=sym_pm("shear", policy.shear) if geo else 0.0,
        tx=sym_pm("tx", policy.translate) if geo else 0.0,
        ty=sym_pm("ty", policy.translate) if geo else 0.0,
        sym=min(int(u[_U["sym"]] * 8), 7) if (geo and policy.flip) else 0,
        brightness=sym_pm("brightness", policy.brightness) if pho else 0.0,
        contrast=1.0 + sym_pm("contrast", policy.contrast) if pho else 1.0,
        saturation=1.0 + sym_pm("saturation", policy.saturation) if pho else 1.0,
        gamma=math.exp(sym_pm("gamma", math.log1p(policy.gamma))) if (pho and policy.gamma > 0) else 1.0,
        hue=sym_pm("hue", policy.hue) if pho else 0.0,
        swap_rb=bool(pho and u[_U["swap_rb"]] < policy.swap_rb),
        noise=policy.noise if pho else 0.0,
        border=policy.border)


def _geometry(p: Params, src_hw, out_hw):
    """(a00, a01, a10, a11) Q16 and (b0, b1) in 1/65536 pixel of the map output pixel -> source position:
        p_src = c_src + (tx OW, ty OH) + M (p_out - c_out),  M = (1 / scale) R(angle) Sh(shear) D(sym),
    R = [[cos, -sin], [sin, cos]] (x right, y down: a positive angle turns the picture counter-clockwise, 90 degrees = np.rot90),
    Sh = [[1, tan], [0, 1]], D the symmetry (transpose first, then the flips), c = ((w - 1) / 2, (h - 1) / 2) the centres.
    Composed in float64 and rounded once."""
    import math
    (sh, sw), (oh, ow) = src_hw, out_hw
    ca, sa = math.cos(math.radians(p.angle)), math.sin(math.radians(p.angle))
    R = np.array([[ca, -sa], [sa, ca]], np.float64)
    Sh = np.array([[1.0, math.tan(math.radians(p.shear))], [0.0, 1.0]], np.float64)
    P = np.array([[0.0, 1.0], [1.0, 0.0]]) if p.sym & _lib.SG_SYM_TRANSPOSE else np.eye(2)
    F = np.diag([-1.0 if p.sym & _lib.SG_SYM_FLIP_LR else 1.0, -1.0 if p.sym & _lib.SG_SYM_FLIP_UD else 1.0])
    M = (R @ Sh @ F @ P) / p.scale
    c_out = np.array([(ow - 1) / 2.0, (oh - 1) / 2.0])
    c_src = np.array([(sw - 1) / 2.0, (sh - 1) / 2.0])
    t = c_src + np.array([p.tx * ow, p.ty * oh]) - M @ c_out
    a = [int(round(float(v) * 65536.0)) for v in (M[0, 0], M[0, 1], M[1, 0], M[1, 1])]
    b = [int(round(float(v) * 65536.0)) for v in t]
    return a, b


def _colour(p: Params):
    """(m[9] Q12, lut uint8 [3,256] or None, noise_q12): m = Hue(hue) Sat(saturation) Swap in float64, rounded once - the
    saturation mixes with the luma (0.299, 0.587, 0.114), the hue turns about the grey axis, the swap exchanges channels 0 and
    2 first; lut[u] = clip(rint(255 ((u / 255)^gamma - 0.5) contrast + 0.5 + brightness)), the same for the three channels, or
    None when it would be the identity."""
    import math
    L = np.tile(np.array(_LUMA, np.float64), (3, 1))
    S = p.saturation * np.eye(3) + (1.0 - p.saturation) * L
    ch, shh = math.cos(math.radians(p.hue)), math.sin(math.radians(p.hue))
    K = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
    Hm = ch * np.eye(3) + (1.0 - ch) / 3.0 * np.ones((3, 3)) + shh / math.sqrt(3.0) * K
    M = Hm @ S
    if p.swap_rb:
        M = M[:, ::-1]
    m = [int(round(float(v) * 4096.0)) for v in M.reshape(-1)]
    lut = None
    if p.brightness != 0.0 or p.contrast != 1.0 or p.gamma != 1.0:
        x = np.arange(256, dtype=np.float64) / 255.0
        y = (np.power(x, p.gamma) - 0.5) * p.contrast + 0.5 + p.brightness
        lut = np.tile(np.clip(np.rint(255.0 * y), 0, 255).astype(np.uint8), (3, 1))
    return m, lut, int(round(p.noise / NOISE_T_STD * 4096.0))


_IDENTITY_M = (4096, 0, 0, 0, 4096, 0, 0, 0, 4096)


def warp_items(record: Params, src_hw, out_hw, label: bool):
    """(item, lut) of sg_warp_u8 for one sample: `item` a mapping with the fields of sg_warp_item (src = 0: the caller places
    it), `lut` uint8 [3,256] or None.  The label shares the image's geometry and takes the nearest tap, fill 0 and no colour;
    the image is bilinear with fill 128.  With every option off the item is the exact identity, without flags."""
    a, b = _geometry(record, src_hw, out_hw)
    reflect = _lib.SG_WARP_REFLECT if record.border == "reflect" else 0
    item = dict(src=0, sh=int(src_hw[0]), sw=int(src_hw[1]), a=tuple(a), b=tuple(b), sample=record.sample)
    if label:
        item.update(flags=_lib.SG_WARP_NEAREST | reflect, fill=LABEL_FILL)
        return item, None
    m, lut, noise_q12 = _colour(record)
    colour = tuple(m) != _IDENTITY_M or lut is not None or noise_q12 > 0
    item.update(flags=reflect | (_lib.SG_WARP_COLOR if colour else 0), fill=IMAGE_FILL)
    if colour:
        item.update(m=tuple(m), noise_q12=noise_q12)
    return item, lut


def device_random_gen(img_path, lab_path, BATCH_SIZE, engine, policy, seed=0, crop=SIZE, start=0, shard=(0, 1), depth: int = 2,
                      workers: int = 4, separation=None):
    """Online augmentation as a stage of the device feed: the sorted, cycled (image, label) pairs of device_data_gen, sample k
    of the endless stream = pair k mod len under draw(policy, seed, k).  Sources may be any size: per batch every distinct
    source is decoded once (`workers` threads, `depth` batches ahead), the batch's sources are padded into one pinned uint8
    array (their extents travel in the items) and cross PCIe as uint8; the device warps images and labels (sg_warp_u8, one call
    each), normalises (sg_u8_to_f32) and builds the label channels from the WARPED label (sg_edge_labels), so the rims keep
    their width.  Yields device tensors x float32 [N,crop,crop,3], y float32 [N,crop,crop,4].
    start: the first sample (resume);  shard=(r, w): this consumer takes batches r, r + w, ... of the stream that begins at
    `start` (rank r of w);  separation=(w0, sigma): as in device_data_gen.  With every option of `policy` off and 512 x 512
    files the stream is device_data_gen's, bit for bit."""
    import torch
    if not isinstance(policy, RandomPolicy):
        raise ValueError(f"policy = {policy!r} is not a RandomPolicy")
    r, w = (int(v) for v in shard)
    if not (w >= 1 and 0 <= r < w):
        raise ValueError(f"shard = {shard!r}: expected (rank, world) with 0 <= rank < world")
    crop, start, BATCH_SIZE = int(crop), int(start), int(BATCH_SIZE)
    if crop < 1 or crop > (1 << 14) or start < 0 or BATCH_SIZE < 1:
        raise ValueError(f"crop = {crop}, start = {start}, BATCH_SIZE = {BATCH_SIZE}: crop in [1, 16384], start >= 0, BATCH_SIZE >= 1")
    if separation is not None:
        from .data import check_separation
        separation = check_separation(separation)
    from concurrent.futures import ThreadPoolExecutor
    images, label = img_path, lab_path
    images.sort()  # in place, as train_data_gen does
    label.sort()
    pairs = list(zip(images, label))
    if not pairs:
        raise ValueError("device_random_gen: no (image, label) pairs")

    def decode(i):
        rgb, gray = _decode_u8(*pairs[i], resize=False)
        if rgb.shape[:2] != gray.shape[:2]:
            raise ValueError(f"{pairs[i][0]} is {rgb.shape[1]} x {rgb.shape[0]} but its label {pairs[i][1]} is "
                             f"{gray.shape[1]} x {gray.shape[0]}")
        return rgb, gray

    def host_batches():
        with ThreadPoolExecutor(max_workers=max(1, int(workers))) as pool:
            t = r
            while True:
                ks = [start + t * BATCH_SIZE + j for j in range(BATCH_SIZE)]
                t += w
                srcs = list(dict.fromkeys(k % len(pairs) for k in ks))
                dec = list(pool.map(decode, srcs))
                slot = {s: n for n, s in enumerate(srcs)}
                extents = [d[1].shape[:2] for d in dec]
                hm, wm = max(e[0] for e in extents), max(e[1] for e in extents)
                xa = np.zeros((len(srcs), hm, wm, 3), np.uint8)
                la = np.zeros((len(srcs), hm, wm), np.uint8)
                for n, (rgb, gray) in enumerate(dec):
                    xa[n, :rgb.shape[0], :rgb.shape[1]] = rgb
                    la[n, :gray.shape[0], :gray.shape[1]] = gray
                xb, lb = torch.from_numpy(xa), torch.from_numpy(la)
                xi, li, luts = [], [], []
                for k in ks:
                    rec, n = draw(policy, seed, k), slot[k % len(pairs)]
                    it, lut = warp_items(rec, extents[n], (crop, crop), False)
                    xi.append(dict(it, src=n))
                    li.append(dict(warp_items(rec, extents[n], (crop, crop), True)[0], src=n))
                    luts.append(lut)
                lt = None
                if any(l is not None for l in luts):   # an item without a table of its own reads the identity
                    ident = np.tile(np.arange(256, dtype=np.uint8), (3, 1))
                    lt = torch.from_numpy(np.stack([ident if l is None else l for l in luts]))
                if torch.cuda.is_available():
                    xb, lb = xb.pin_memory(), lb.pin_memory()
                    lt = lt.pin_memory() if lt is not None else None
                yield xb, lb, lt, xi, li

    feed = Prefetcher(host_batches(), depth)
    try:
        for xb, lb, lt, xi, li in feed:
            xd = xb.to(engine.device, non_blocking=True)
            ld = lb.to(engine.device, non_blocking=True)
            ltd = lt.to(engine.device, non_blocking=True) if lt is not None else None
            xa = engine.warp_u8(xd, xi, ltd, seed, out_hw=(crop, crop))
            la = engine.warp_u8(ld, li, None, seed, out_hw=(crop, crop))
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
