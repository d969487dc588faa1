"""Test-side restatement of the reference's data_enhancement.py (Data_Enhance.run, random_scale_resize, label_: :62-135)
for 512 x 512 tiles with grey labels, from the oracle's materialised cv.resize (oracle.input_pipeline.resize_linear_u8),
numpy slicing, flips and np.where, with the draws of one random.Random in the reference's order.  Images are RGB (as the
training generator reads them back), so cvtColor(BGR2RGB) before imwrite is a swap of channels 0 and 2 either way.
The sources are walked in sorted name order (the product's deliberate departure from os.listdir order)."""
import os

import numpy as np

from oracle import input_pipeline as OIP


def scale_pad_crop(img, lab, s):
    """random_scale_resize (:102-126) up to, not including, its random flip: resize to int(512 * s), threshold the label,
    centred pad on a canvas of 128 / 0 (s < 1) or the 512 x 512 crop at max((n - 512) // 2 - 1, 0)."""
    img_h, img_w = img.shape[:2]
    n_h, n_w = int(img_h * s), int(img_w * s)
    x, y = (img_w - n_w) // 2, (img_h - n_h) // 2
    image = OIP.resize_linear_u8(img, (n_h, n_w))
    label = np.where(OIP.resize_linear_u8(lab, (n_h, n_w)) > 125, 255, 0).astype(np.uint8)   # label_
    if s < 1:
        new_image = np.full((img_h, img_w, 3), 128, np.uint8)
        new_label = np.zeros((img_h, img_w), np.uint8)
        new_image[y:y + n_h, x:x + n_w, :] = image
        new_label[y:y + n_h, x:x + n_w] = label
    else:
        x, y = max((n_w - img_w) // 2 - 1, 0), max((n_h - img_h) // 2 - 1, 0)
        new_image = image[y:y + 512, x:x + 512, :]
        new_label = label[y:y + 512, x:x + 512]
    return new_image, new_label


def enhance_one(stem, img, lab, rng):
    """[(file name, image, label, (s, flip_ud, flip_lr, swap))] that Data_Enhance.run writes for one source, in its order;
    img / lab may be None (the draws and names only)."""
    have = img is not None
    out = [(stem + ".png", img, lab, (None, False, False, False))]
    if rng.random() > 0.2:
        out.append((stem + "_1.png", img[::-1] if have else None, lab[::-1] if have else None, (None, True, False, False)))
    if rng.random() > 0.2:
        out.append((stem + "_2.png", img[:, ::-1] if have else None, lab[:, ::-1] if have else None, (None, False, True, False)))
    if rng.random() > 0.2:
        s = rng.randint(6, 20) / 10
        i3, l3 = scale_pad_crop(img, lab, s) if have else (None, None)
        ud = lr = False
        if 0.7 > rng.random() >= 0.4:
            ud = True
        elif rng.random() >= 0.7:
            lr = True
        if have and ud:
            i3, l3 = i3[::-1], l3[::-1]
        if have and lr:
            i3, l3 = i3[:, ::-1], l3[:, ::-1]
        out.append((stem + "_3.png", i3, l3, (s, ud, lr, False)))
    if rng.random() > 0.7:
        out.append((stem + "_4.png", img[..., ::-1] if have else None, lab, (None, False, False, True)))
    return out


def enhance(sources, rng):
    """One pass of Data_Enhance.run over sources [(file name, rgb or None, grey label or None)] in sorted name order:
    {virtual file name: (rgb, label, params)}."""
    out = {}
    for name, img, lab in sorted(sources, key=lambda t: t[0]):
        for vname, i, l, params in enhance_one(name.split(".")[0], img, lab, rng):
            assert vname not in out
            out[vname] = (None if i is None else np.ascontiguousarray(i), None if l is None else np.ascontiguousarray(l), params)
    return out


def read_sources(img_dir, lab_dir):
    """[(file name, rgb, grey label)] of a source folder pair (labels under the images' file names, as the reference reads)."""
    return [(n, OIP.imread_rgb(os.path.join(img_dir, n)), OIP.bgr2gray_u8(OIP.imread_rgb(os.path.join(lab_dir, n))))
            for n in sorted(os.listdir(img_dir))]


def write_folder(tiles, img_dir, lab_dir):
    """The augmented folder the reference writes: RGB and grey PNG files under the virtual names."""
    from PIL import Image
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(lab_dir, exist_ok=True)
    for vname, (img, lab, _) in tiles.items():
        Image.fromarray(img).save(os.path.join(img_dir, vname))
        Image.fromarray(lab).save(os.path.join(lab_dir, vname))


def xy(img, lab):
    """decode_img / decode_lbel + train_data_gen's label channels of one in-memory tile (oracle arithmetic)."""
    x = np.array(img, np.float32) / 127.5 - 1
    y = OIP.label_channels(np.array(lab, np.float32) / 255)
    return x, y
