"""Synthetic zips for the SegNet training tests: a textured grey road trapezoid in the lower part of each image, the
rest random smooth colours.  Train labels are the road masks (cli.write_label_zip), validation labels labelIds PNGs
(7 road, 21 elsewhere, 0 = ignored in the top rows).  Below them, the one copy of the process, archive and snapshot
helpers of the SegNet test files.  No torch at module level: the CPU loader tests import this module and check what
their worker processes import."""
import io
import json
import os
import re
import socket
import subprocess
import sys
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
    from importlib import import_module
    cli = import_module('superpixel-align_amd.cli')
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    lab_dir = os.path.join(root, 'est')
    os.makedirs(lab_dir, exist_ok=True)
    out = [os.path.join(root, f) for f in ('train_imgs.zip', 'train_labels.zip', 'val_imgs.zip', 'val_labels.zip')]

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


# ------------------------------------------------------------------------------- bytes, archives, processes
def png(a, mode=None):
    """the array as PNG bytes; mode 'P': through a 16-colour palette"""
    from PIL import Image
    buf = io.BytesIO()
    im = Image.fromarray(a)
    if mode == 'P':
        im = im.convert('P', palette=Image.ADAPTIVE, colors=16)
    im.save(buf, format='PNG')
    return buf.getvalue()


def npy(a):
    buf = io.BytesIO()
    np.save(buf, a)
    return buf.getvalue()


def decoded(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as f:
        return np.asarray(f)


def rewrite(src, dst, changes):
    """a copy of the zip with member k replaced by changes[k](its bytes)"""
    with zipfile.ZipFile(src) as zi, zipfile.ZipFile(dst, 'w') as zo:
        for k, name in enumerate(zi.namelist()):
            data = zi.read(name)
            zo.writestr(name, changes[k](data) if k in changes else data)
    return dst


def bits(a):
    """float32 values as their bit patterns (NaNs and signed zeros compare as bits); other dtypes as they are"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def shm_names(prefix=''):
    """the names under /dev/shm; prefix 'psm_': the blocks Python's SharedMemory creates (the loaders' slabs)"""
    return set(f for f in os.listdir('/dev/shm') if f.startswith(prefix)) if os.path.isdir('/dev/shm') else set()


def alive(pid):
    """the process exists and is no zombie"""
    try:
        os.kill(pid, 0)
    except OSError:
        return False
    try:
        with open('/proc/%d/stat' % pid) as f:
            return f.read().rsplit(')', 1)[1].split()[0] != 'Z'
    except OSError:
        return False


def declaration(header, name):
    """the argument list of `int name(...);` in the header text, whitespace collapsed"""
    m = re.search(r'\bint\s+%s\s*\(([^;]*)\)\s*;' % name, header)
    assert m, '%s is not declared' % name
    return re.sub(r'\s+', ' ', m.group(1)).strip()


def free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def env(**kw):
    """this process's environment without the launch variables of a rank group, then kw"""
    e = {k: v for k, v in os.environ.items()
         if k not in ('SPA_DIST_FORCE', 'SPA_DIST_BACKEND', 'SPA_BENCH_SAME_DEVICE', 'RANK', 'WORLD_SIZE',
                      'LOCAL_RANK', 'MASTER_PORT', 'MASTER_ADDR')}
    e.update(kw)
    return e


def run_python(args, cwd, timeout=900):
    """python <args> to the end; a non-zero exit fails the test with the tails of its output"""
    r = subprocess.run([sys.executable] + args, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def run(cmd, env, cwd, timeout, ok=True):
    """cmd in the given environment; ok: a non-zero exit fails the test with the tails of its output"""
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    if ok:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def train_args(z, iters, val_every, log_every, input_shape=(64, 128), eval_shape=(64, 128), extra=()):
    """train_segnet.py's arguments for the zips of write(): batches of 2, limits and intervals in iterations"""
    return ['--train_img_zip', z[0], '--train_label_zip', z[1], '--val_img_zip', z[2], '--val_label_zip', z[3],
            '--batchsize', '2', '--input_shape', str(input_shape[0]), str(input_shape[1]),
            '--eval_shape', str(eval_shape[0]), str(eval_shape[1]), '--train_limit', str(iters), 'iteration',
            '--val_interval', str(val_every), 'iteration', '--log_interval', str(log_every), 'iteration'] + list(extra)


def same_snapshot(fa, fb, keys=None, bitwise=False):
    """the two snapshots hold equal entries of equal dtype.  keys 'common': only the entries both have (otherwise the
    two sets of names must be equal); bitwise: equal shapes and bytes instead of np.array_equal.  -> the names"""
    with np.load(fa) as a, np.load(fb) as b:
        ks = set(a.files) & set(b.files) if keys == 'common' else set(a.files)
        if keys != 'common':
            assert set(a.files) == set(b.files)
        for k in ks:
            assert a[k].dtype == b[k].dtype, k
            if bitwise:
                assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
            else:
                assert np.array_equal(a[k], b[k]), k
        return ks


def losses(d):
    return [(e['iteration'], e['epoch'], e['main/loss'], e['val/main/iou/road']) for e in
            json.load(open(os.path.join(d, 'log')))]


class FakeTrainer(object):
    """what save_snapshot reads from a trainer, without a GPU: the parameters p, an optimizer at step t with one
    momentum entry, bn_n as every layer's BatchNorm count, and attrs (dtype, split_planes) as attributes"""

    def __init__(self, p, t, bn_n, **attrs):
        from importlib import import_module
        import torch
        st = import_module('superpixel-align_amd.segnet_train')
        self._p = p
        self._bn_n = bn_n
        self._layers = import_module('superpixel-align_amd.segnet').LAYERS
        self.opt = st.MomentumSGD(0.01)
        self.opt.t = t
        self.opt.state = {'conv1/W': {'v': torch.ones((64, 3, 7, 7))}}
        for k, v in attrs.items():
            setattr(self, k, v)

    def params_numpy(self):
        out = dict(self._p)
        for n in self._layers:
            out[n + '_bn/N'] = np.asarray(self._bn_n)
        return out
