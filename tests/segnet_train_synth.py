"""Synthetic zips for the SegNet training tests: a textured grey road trapezoid in the lower part of each image, the
rest random smooth colours.  Train labels are the road masks (cli.write_label_zip), validation labels labelIds PNGs
(7 road, 21 elsewhere, 0 = ignored in the top rows)."""
import io
import os
import zipfile

import numpy as np


def road_mask(H, W, rng):
    top = int(H * rng.uniform(0.45, 0.6))
    m = np.zeros((H, W), bool)
    for y in range(top, H):
        f = (y - top) / float(H - top)
        half = int(W * (0.15 + 0.35 * f))
        c = W // 2 + int(rng.integers(-2, 3))
        m[y, max(c - half, 0):min(c + half, W)] = True
    return m


def image(H, W, rng):
    m = road_mask(H, W, rng)
    yy, xx = np.mgrid[0:H, 0:W] / float(max(H, W))
    img = np.empty((H, W, 3), np.float64)
    for c in range(3):
        a, b, d = rng.uniform(40, 220), rng.uniform(-80, 80), rng.uniform(-80, 80)
        img[..., c] = a + b * yy + d * xx
    img += rng.normal(0, 6, img.shape)
    road = 110 + rng.normal(0, 3, (H, W, 1)) + np.array([0, 0, 6]) + 12 * ((np.arange(W) // 3) % 2)[None, :, None]
    img[m] = road[m]
    return np.clip(img, 0, 255).astype(np.uint8), m


def write(root, n_train, n_val, H, W, seed=0):
    """-> (train_img_zip, train_label_zip, val_img_zip, val_label_zip)"""
    from PIL import Image
    from importlib import import_module
    cli = import_module('superpixel-align_amd.cli')
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    lab_dir = os.path.join(root, 'est')
    os.makedirs(lab_dir, exist_ok=True)
    out = [os.path.join(root, f) for f in ('train_imgs.zip', 'train_labels.zip', 'val_imgs.zip', 'val_labels.zip')]

    def png(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format='PNG')
        return buf.getvalue()

    with zipfile.ZipFile(out[0], 'w') as zi:
        for i in range(n_train):
            key = 'synth_%06d_000019' % i
            im, m = image(H, W, rng)
            zi.writestr('leftImg8bit/train/synth/%s_leftImg8bit.png' % key, png(im))
            np.save(os.path.join(lab_dir, '%s_leftImg8bit.npy' % key), m)
    cli.write_label_zip(lab_dir, out[1])
    with zipfile.ZipFile(out[2], 'w') as zi, zipfile.ZipFile(out[3], 'w') as zl:
        for i in range(n_val):
            key = 'synthval_%06d_000019' % i
            im, m = image(H, W, rng)
            lab = np.where(m, 7, 21).astype(np.uint8)
            lab[:4] = 0
            zi.writestr('leftImg8bit/val/synth/%s_leftImg8bit.png' % key, png(im))
            zl.writestr('gtFine/val/synth/%s_gtFine_labelIds.png' % key, png(lab))
    return out
