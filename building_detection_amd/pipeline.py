"""Inference pipeline of predict.py:17-116 and the ensemble vote of model_fuse.py:315-323, on the engine.

    load_model()                 -> (res_model, hr_model, v3_model, unet_model, bam_model)   predict.py:17-54
    detection(img, user_path, model, save_name)  sliding 512-px window, stride 360, argmax, OR-merge   :90-116
    vote(masks, k=3)             -> 255 where at least k of the 5 cleaned masks agree          model_fuse.py:315-323
    detection_soft(img, user_path, models, ...)  probability-domain counterpart (no reference: SoftScene below)
    evaluate_objects(pred, truth, iou=0.5)       per-building TP / FP / FN, precision, recall, F1 of a scene (objects.py)

What changes against the reference: tiles of one image are predicted in batches on the GPU instead of one
`model.predict` per tile (BatchNorm runs on moving statistics in inference, so per-tile results do not depend
on the batching), the argmax / int8 accumulation / vote run as HIP kernels (sg_argmax_accumulate_i8,
sg_vote_ge), and images may be passed as arrays (OpenCV is not available here; PNG I/O uses Pillow).  The
contour clean-up around the vote (model_fuse.py:9-218) runs on the GPU as label-map kernels (cleanup.py, csrc/morph.hip:
`model_confuse` below); polygonisation (edge_3.py) is CPU OpenCV geometry and out of scope.

`reference_jloop=True` keeps the reference's column loop `for j in range(0, new_h-152, 360)` (predict.py:106
iterates the HEIGHT for columns): for landscape images the right-hand columns beyond new_h are never
predicted, for portrait images whose extra rows would index tiles past the canvas the reference fails inside
TensorFlow — here that case raises ValueError.  `reference_jloop=False` iterates new_w (the evident intent).
"""
from __future__ import annotations

import math
import os
from typing import List, Sequence

import numpy as np

TILE, STRIDE, OVERLAP = 512, 360, 152


def tile_origins(h: int, w: int, reference_jloop: bool = True):
    """Canvas size and tile origins exactly as predict.py:98-106 computes them."""
    h_num = math.ceil((h - OVERLAP) / STRIDE)
    w_num = math.ceil((w - OVERLAP) / STRIDE)
    new_h, new_w = h_num * STRIDE + OVERLAP, w_num * STRIDE + OVERLAP
    ch, cw = max(new_h, TILE), max(new_w, TILE)
    rows = list(range(0, new_h - OVERLAP, STRIDE))
    cols = list(range(0, (new_h if reference_jloop else new_w) - OVERLAP, STRIDE))
    if reference_jloop:
        for j in cols:
            if j + TILE > cw:
                raise ValueError(
                    f"image {h}x{w}: the reference's column loop (predict.py:106 uses new_h) indexes a tile at column {j} "
                    f"past the {cw}-px canvas; tf.keras would reject the truncated tile. Use reference_jloop=False.")
    return (ch, cw), [(i, j) for i in rows for j in cols]


def read_rgb(path: str) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def detection(img, user_path=None, model=None, save_name="model", batch: int = 8, reference_jloop: bool = True):
    """predict.py:90-116 for one model.  `img`: path or uint8 RGB array [h,w,3].  Returns the uint8 mask
    (0/255) of shape [h,w]; writes `<user_path>/<save_name>.png` when user_path is given.

    A model of C > 2 classes: the canvas is a uint8 class map and a tile's argmax is merged into it by MAXIMUM
    (sg_argmax_max_u8: where tiles overlap the higher class index wins, whatever the order of the tiles; at two
    classes that is the reference's OR).  The returned array and the PNG then hold class indices 0 ... C-1."""
    import torch
    from .ops import get_engine
    if isinstance(img, (str, os.PathLike)):
        img = read_rgb(str(img))
    arr = np.asarray(img)
    h, w = arr.shape[:2]
    x = arr.astype(np.float64) / 127.5 - 1                      # predict.py:93 (float64, like the reference)
    (ch, cw), origins = tile_origins(h, w, reference_jloop)
    canvas_img = np.zeros((ch, cw, 3))                           # zeros = mid-grey padding (:102)
    canvas_img[:h, :w, :] = x
    rt = model._runtime()
    eng = rt.eng
    class_map = model.num_classes > 2
    pred = torch.zeros(ch, cw, dtype=torch.uint8 if class_map else torch.int8, device=eng.device)
    for s in range(0, len(origins), batch):
        chunk = origins[s:s + batch]
        tiles = np.stack([canvas_img[i:i + TILE, j:j + TILE, :] for i, j in chunk]).astype(np.float32)
        p = model.predict_device(torch.from_numpy(tiles).to(eng.device))
        for k, (i, j) in enumerate(chunk):
            if class_map:
                eng.argmax_max(p[k], pred, i, j)                # argmax (ties -> lowest index), merged by maximum
            else:
                eng.argmax_accumulate(p[k], pred, i, j)         # argmax (ties -> 0) and int8 `+=` (:110-113)
    if class_map:
        out = np.ascontiguousarray(pred.cpu().numpy()[:h, :w])
    else:
        out = np.where(pred.cpu().numpy() >= 1, 255, 0).astype(np.uint8)[:h, :w]   # :114
    if user_path is not None:
        from PIL import Image
        os.makedirs(user_path, exist_ok=True)
        Image.fromarray(out).save(os.path.join(user_path, f"{save_name}.png"), compress_level=0)
    return out


# ------------------------------------------------------------------------------------------------ soft scene inference
# Beside the reference's hard-decision loop above: tiles are cut from the uint8 scene on the device (sg_scene_tiles_u8),
# their probabilities are averaged where tiles overlap, optionally under a window and over the symmetries of the square
# (sg_prob_accumulate), and several models meet as a weighted mean of probabilities (sg_prob_finalize takes the argmax).
TTA_PRESETS = {1: [0], 2: [0, 2], 4: [0, 1, 2, 3], 8: list(range(8))}


def scene_origins(h: int, w: int, tile: int = TILE, stride: int = STRIDE):
    """((ch, cw), [(y0, x0), ...]) row-major: per axis num = max(1, ceil((dim - overlap) / stride)) tiles at multiples of
    `stride`, overlap = tile - stride.  At 512/360 these are tile_origins(h, w, reference_jloop=False) for axes longer than
    the overlap (a shorter axis gets no tile there and one tile here)."""
    tile, stride = int(tile), int(stride)
    if not 0 < stride <= tile:
        raise ValueError(f"stride {stride} outside (0, tile = {tile}]")
    overlap = tile - stride
    nums = [max(1, math.ceil((d - overlap) / stride)) for d in (h, w)]
    ch, cw = (max(n * stride + overlap, tile) for n in nums)
    rows, cols = (range(0, n * stride, stride) for n in nums)
    return (ch, cw), [(i, j) for i in rows for j in cols]


def make_window(window, tile: int) -> np.ndarray:
    """float32 [tile]: "flat" = ones, "pyramid" = min(i+1, tile-i) / ceil(tile/2), or a positive array of length `tile`."""
    if isinstance(window, str):
        if window == "flat":
            return np.ones(tile, np.float32)
        if window == "pyramid":
            i = np.arange(tile)
            return (np.minimum(i + 1, tile - i) / math.ceil(tile / 2)).astype(np.float32)
        raise ValueError(f"window={window!r}: 'flat', 'pyramid' or an array of {tile} positive weights")
    win = np.asarray(window, dtype=np.float32)
    if win.shape != (tile,):
        raise ValueError(f"window of shape {win.shape}, expected ({tile},)")
    if not (win > 0).all():       # also refuses NaN
        raise ValueError("window entries must be positive")
    return np.ascontiguousarray(win)


def tta_symmetries(tta) -> List[int]:
    """The symmetry codes of a `tta` argument: a preset (1, 2, 4, 8) or an iterable of codes 0 ... 7."""
    if isinstance(tta, (int, np.integer)):
        if int(tta) not in TTA_PRESETS:
            raise ValueError(f"tta={tta}: presets are {sorted(TTA_PRESETS)}; pass a list for other symmetry sets")
        return list(TTA_PRESETS[int(tta)])
    syms = [int(s) for s in tta]
    if not syms or any(not 0 <= s < 8 for s in syms):
        raise ValueError(f"tta={tta!r}: symmetry codes are 0 ... 7 (SG_SYM_FLIP_UD | _FLIP_LR | _TRANSPOSE)")
    return syms


SCALE_RANGE = (0.25, 4.0)      # of a multi-scale pass
SCENE_MAX_EXTENT = 16384       # ... and its limit on every scene and scaled-scene axis (sg_prob_resize_accumulate)


def check_scales(scales):
    """The scales of a multi-scale pass as floats: a non-empty sequence of finite values in SCALE_RANGE."""
    try:
        out = [float(s) for s in scales]
    except TypeError:
        raise ValueError(f"scales={scales!r}: a sequence of floats in {list(SCALE_RANGE)}") from None
    if not out or any(not (SCALE_RANGE[0] <= s <= SCALE_RANGE[1]) for s in out):   # also refuses NaN
        raise ValueError(f"scales={scales!r}: a non-empty sequence of floats in {list(SCALE_RANGE)}")
    return out


def scaled_size(h: int, w: int, s: float):
    """(hs, ws) of an h x w scene at scale s: max(1, floor(d * s + 1/2)) per axis.  ValueError beyond the limits of the resize
    (one image below 2^31 bytes) and of the fold (every extent at most SCENE_MAX_EXTENT)."""
    hs, ws = (max(1, int(math.floor(d * float(s) + 0.5))) for d in (h, w))
    if max(h, w, hs, ws) > SCENE_MAX_EXTENT:
        raise ValueError(f"scene {h} x {w} at scale {s} = {hs} x {ws}: an extent above the multi-scale limit {SCENE_MAX_EXTENT}")
    if max(h * w, hs * ws) * 3 >= 2 ** 31:
        raise ValueError(f"scene {h} x {w} at scale {s} = {hs} x {ws}: an image of 2^31 bytes or more (resize_linear_u8's limit)")
    return hs, ws


class SoftScene:
    """Probability canvases of one scene: `acc` [h,w,C] = sum of w * p and `wsum` [h,w] = sum of w on the device, filled by
    add() model by model and read by result().  The image is uploaded once as uint8; overhanging tiles are clipped by the
    kernels (no padded canvas)."""

    def __init__(self, img, num_classes: int, tile: int = TILE, stride: int = STRIDE, window="flat", engine=None):
        import torch
        from .ops import get_engine
        if isinstance(img, (str, os.PathLike)):
            img = read_rgb(str(img))
        arr = np.ascontiguousarray(img)
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError(f"img: expected a uint8 RGB array [h,w,3], got {arr.dtype} {arr.shape}")
        self.eng = engine if engine is not None else get_engine(0)
        self.num_classes, self.tile, self.stride = int(num_classes), int(tile), int(stride)
        self.h, self.w = arr.shape[:2]
        _, self.origins = scene_origins(self.h, self.w, self.tile, self.stride)
        dev = self.eng.device
        self.scene = torch.from_numpy(arr).to(dev)
        self.win = torch.from_numpy(make_window(window, self.tile)).to(dev)
        self.acc = torch.zeros(self.h, self.w, self.num_classes, dtype=torch.float32, device=dev)
        self.wsum = torch.zeros(self.h, self.w, dtype=torch.float32, device=dev)
        self._kind = None   # "plain" | "scaled": what add() has put on the canvases

    @classmethod
    def _on_device(cls, scene, like):
        """A scene of its own canvases around a uint8 [h,w,3] device tensor, with `like`'s classes, tile, stride and window."""
        import torch
        self = cls.__new__(cls)
        self.eng, self.num_classes, self.tile, self.stride, self.win = like.eng, like.num_classes, like.tile, like.stride, like.win
        self.h, self.w = int(scene.shape[0]), int(scene.shape[1])
        _, self.origins = scene_origins(self.h, self.w, self.tile, self.stride)
        self.scene = scene
        self.acc = torch.zeros(self.h, self.w, self.num_classes, dtype=torch.float32, device=scene.device)
        self.wsum = torch.zeros(self.h, self.w, dtype=torch.float32, device=scene.device)
        self._kind = None
        return self

    def work_list(self, tta=1):
        """[(y0, x0, sym), ...]: origins-major, then symmetries."""
        syms = tta_symmetries(tta)
        return [(i, j, s) for i, j in self.origins for s in syms]

    def add(self, model, tta=1, weight: float = 1.0, batch: int = 8, scale=None):
        """Adds one model's pass over the scene.  scale=None: its windowed tile probabilities go straight onto the canvases.
        scale=s (SCALE_RANGE, 1.0 included): the pass runs on the scene resized to scaled_size(h, w, s), is stitched on canvases
        of that size, and enters as a normalised probability map under `weight` (sg_prob_resize_accumulate); a scene takes
        passes of one kind only, since raw window sums and normalised maps must not meet on one canvas."""
        import torch
        shape = tuple(model.inputs[0].shape[1:])
        if shape != (self.tile, self.tile, 3):
            raise ValueError(f"model input {shape} is not the scene's tile {(self.tile, self.tile, 3)}")
        if model.num_classes != self.num_classes:
            raise ValueError(f"model has {model.num_classes} classes, the scene {self.num_classes}")
        kind = "plain" if scale is None else "scaled"
        if self._kind not in (None, kind):
            raise ValueError(f"SoftScene.add: a {kind} pass on a scene that holds {self._kind} passes (give every pass a scale, "
                             "1.0 included, or none)")
        if scale is not None:
            s = check_scales([scale])[0]
            weight = float(weight)
            if not (weight > 0 and math.isfinite(weight)):
                raise ValueError(f"SoftScene.add: weight {weight} is not positive and finite")
            hs, ws = scaled_size(self.h, self.w, s)
            sub = SoftScene._on_device(self.eng.resize_linear_u8(self.scene[None], hs, ws)[0], self)
            sub.add(model, tta=tta, weight=1.0, batch=batch)
            self.eng.prob_resize_accumulate(sub.acc, sub.wsum, self.acc, self.wsum, weight)
            self._kind = kind
            return self
        self._kind = kind
        eng = self.eng
        work = self.work_list(tta)
        for s in range(0, len(work), batch):
            chunk = work[s:s + batch]
            p = model.predict_device(eng.scene_tiles(self.scene, chunk, self.tile))
            if p.dtype != torch.float32:
                p = eng.cast(p, torch.float32)
            eng.prob_accumulate(p, chunk, self.win, self.acc, self.wsum, scale=weight)
        return self

    def result(self, return_probs: bool = False):
        """The uint8 array [h,w] (0/255 at two classes, class indices otherwise); with return_probs also acc / wsum as
        float32 [h,w,C]."""
        import torch
        probs = torch.empty_like(self.acc) if return_probs else None
        out = self.eng.prob_finalize(self.acc, self.wsum, 255 if self.num_classes == 2 else 1, probs).cpu().numpy()
        return (out, probs.cpu().numpy()) if return_probs else out


def detection_soft(img, user_path=None, models=None, save_name="model", batch: int = 8, tta=1, window="flat", weights=None,
                   tile=None, stride=None, return_probs: bool = False, scales=None, scale_weights=None):
    """Soft counterpart of detection(): `models` is one model or a sequence (the soft ensemble: the mean of the models'
    probabilities under `weights`, default all 1).  tile defaults to the model's input height; stride to 360 at tile 512.
    scales (a sequence of floats in SCALE_RANGE, e.g. (0.75, 1.0, 1.25)) adds the scale axis: every (model, scale) pass runs
    on the scene resized by cv.resize's INTER_LINEAR (Engine.resize_linear_u8), is stitched at its own size with the same
    tile, stride, window and tta, and enters as a normalised probability map under weight_model * weight_scale
    (scale_weights, default all 1), so the result is sum(w P) / sum(w); scales=None is the single-scale path.
    Returns the uint8 array (and the probabilities with return_probs); writes `<user_path>/<save_name>.png` when given."""
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    if not models or models[0] is None:
        raise ValueError("detection_soft: no model")
    weights = [1.0] * len(models) if weights is None else [float(v) for v in weights]
    if len(weights) != len(models):
        raise ValueError(f"{len(weights)} weights for {len(models)} models")
    if scales is None:
        if scale_weights is not None:
            raise ValueError("scale_weights without scales")
        passes = [(None, 1.0)]
    else:
        scales = check_scales(scales)
        scale_weights = [1.0] * len(scales) if scale_weights is None else [float(v) for v in scale_weights]
        if len(scale_weights) != len(scales):
            raise ValueError(f"{len(scale_weights)} scale_weights for {len(scales)} scales")
        if any(not (v > 0 and math.isfinite(v)) for v in scale_weights):
            raise ValueError(f"scale_weights={scale_weights!r}: positive and finite values")
        passes = list(zip(scales, scale_weights))
    tile = int(models[0].inputs[0].shape[1]) if tile is None else int(tile)
    if stride is None:
        if tile != TILE:
            raise ValueError(f"tile {tile}: give a stride (only {TILE} has the default {STRIDE})")
        stride = STRIDE
    scene = SoftScene(img, models[0].num_classes, tile, stride, window, engine=models[0]._runtime().eng)
    for m, wt in zip(models, weights):
        for sc, swt in passes:
            scene.add(m, tta=tta, weight=wt * swt, batch=batch, scale=sc)
    res = scene.result(return_probs)
    if user_path is not None:
        from PIL import Image
        os.makedirs(user_path, exist_ok=True)
        Image.fromarray(res[0] if return_probs else res).save(os.path.join(user_path, f"{save_name}.png"), compress_level=0)
    return res


def vote(masks: Sequence[np.ndarray], k: int = 3) -> np.ndarray:
    """model_fuse.py:315-323: `final = sum(l_i // 255)`; `np.where(final >= 3, 255, 0)` as one HIP kernel."""
    import torch
    from . import cleanup
    from .ops import get_engine
    for m in masks:
        cleanup.require_binary(np.asarray(m), "vote")
    eng = get_engine(0)
    dev = [torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8)).to(eng.device) for m in masks]
    return eng.vote_ge(dev, k).cpu().numpy()


def model_confuse(path, name: str = ""):
    """model_fuse.py:271-350: the five `*.png` masks in `path` (what run_model wrote) -> clean each, 3-of-5 vote, clean
    again -> `<path>/<name>_result.png`; returns the uint8 mask.  Also accepts a list of five arrays (then nothing is
    written).  Fewer / more than five images: prints 'no five images' and returns None, like the reference."""
    import glob
    from . import cleanup
    if isinstance(path, (str, os.PathLike)):
        files = sorted(glob.glob(os.path.join(str(path), "*.png")))
        files = [f for f in files if not f.endswith("_result.png")]
        if len(files) != 5:
            print("no five images")
            return None
        from PIL import Image
        masks = [np.asarray(Image.open(f).convert("L")) for f in files]
        out = cleanup.model_confuse(masks)
        Image.fromarray(out).save(os.path.join(str(path), f"{name}_result.png"), compress_level=0)
        return out
    if len(path) != 5:
        print("no five images")
        return None
    return cleanup.model_confuse(list(path))


def evaluate_objects(pred, truth, iou=0.5, clean: bool = False, **kw):
    """Scores a whole-scene result (what detection, detection_soft or model_confuse return: a 0/255 mask or a class map, array
    or device tensor) against the ground-truth scene building by building: objects.ObjectScores(iou, **kw) over this one
    scene -> its result() (tp / fp / fn, precision, recall, f1, mean IoU of the matches, recall per truth-area bin, per-class
    figures for a class map).  clean=True passes a binary prediction through cleanup.clean first; a class map is refused."""
    from . import cleanup, objects
    if clean:
        import torch
        if isinstance(pred, torch.Tensor):   # require_binary reads host arrays only: hand it the one value it judges by
            if pred.dtype == torch.uint8 and pred.numel():
                cleanup.require_binary(np.array([int(pred.max())], np.uint8), "evaluate_objects(clean=True)")
        else:
            cleanup.require_binary(np.asarray(pred), "evaluate_objects(clean=True)")
        pred = cleanup.clean(pred, kw.get("engine"))
    scores = objects.ObjectScores(iou, **kw)
    scores.update(pred, truth)
    return scores.result()


def load_model(weight_dir: str = ".", shape=(512, 512, 3)):
    """predict.py:17-54: builds the five models, loads `<weight_dir>/{resnet34,hrnet,deep,scse,bam}.h5`; a
    missing file is reported and the model keeps its random initialisation, exactly like the reference."""
    from . import zoo
    specs = [("res_model", lambda: zoo.ResNetFamily(shape).run_model("res34"), "resnet34.h5"),
             ("hr_model", lambda: zoo.HRNet(shape), "hrnet.h5"),
             ("v3_model", lambda: zoo.Xception_DeepLabV3_Plus(shape), "deep.h5"),
             ("unet_model", lambda: zoo.UNet(2, shape), "scse.h5"),
             ("bam_model", lambda: zoo.Xception_DeepLabV3_Plus_bam(shape), "bam.h5")]
    models = []
    for i, (name, build, fname) in enumerate(specs, 1):
        m = build()
        try:
            m.load_weights(os.path.join(weight_dir, fname))
            print(f"load weights {name} {i}/5")
        except OSError as e:
            print(f"error while loading {name}: {e}")
        models.append(m)
    return tuple(models)


def run_model(img, user_path, models, name="", batch: int = 8, reference_jloop: bool = True) -> List[np.ndarray]:
    """predict.py:75-87: the five detections in the reference's order and file names."""
    prefixes = ["res34_", "hrnet_", "v3plus_", "scse_", "bam_"]
    return [detection(img, user_path, m, p + name, batch, reference_jloop) for m, p in zip(models, prefixes)]
