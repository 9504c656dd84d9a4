"""SegNet-Basic host side (no GPU): snapshot loading with the reference's selection quirks, BatchNorm folding (on the
float64 restatement of tests/segnet_ref.py, which the GPU tests share), the labels_from_segnet.py CLI, the zipped
dataset and the host form of the Pillow BILINEAR score resize."""
import importlib
import json
import os
import sys
import zipfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402
segnet = importlib.import_module('superpixel-align_amd.segnet')
cli = importlib.import_module('superpixel-align_amd.cli')


def random_params(rng, classes=2):
    """Chainer-layout parameters, scaled so activations stay O(1)."""
    p = {}
    for i, name in enumerate(segnet.LAYERS):
        cin = 3 if i == 0 else 64
        p[name + '/W'] = (rng.standard_normal((64, cin, 7, 7)) / np.sqrt(cin * 49)).astype(np.float32)
        p[name + '_bn/gamma'] = rng.uniform(0.5, 1.5, 64).astype(np.float32)
        p[name + '_bn/beta'] = rng.uniform(-0.2, 0.2, 64).astype(np.float32)
        p[name + '_bn/avg_mean'] = rng.uniform(-0.2, 0.2, 64).astype(np.float32)
        p[name + '_bn/avg_var'] = rng.uniform(0.5, 2.0, 64).astype(np.float32)
    p['conv_classifier/W'] = (rng.standard_normal((classes, 64, 1, 1)) / 8).astype(np.float32)
    p['conv_classifier/b'] = rng.uniform(-0.1, 0.1, classes).astype(np.float32)
    return p


def write_snapshot(path, params, drop=()):
    """A Chainer trainer snapshot: an npz without extension (snapshot_iter_<n>) holding the whole updater."""
    with open(path, 'wb') as f:
        np.savez(f, **{segnet.PREFIX + k: v for k, v in params.items() if k not in drop},
                 **{'updater/optimizer:main/t': np.array(5)})


def write_args(param_dir, model='basic', input_shape=(32, 64)):
    with open(os.path.join(param_dir, 'args.txt'), 'w') as f:
        json.dump({'model': model, 'input_shape': list(input_shape), 'batchsize': 8}, f)


# ------------------------------------------------------------------------------- snapshot
def test_snapshot_keys_and_shapes(tmp_path):
    rng = np.random.default_rng(0)
    p = random_params(rng)
    write_args(str(tmp_path))
    write_snapshot(str(tmp_path / 'snapshot_iter_100'), p)
    args, snap, q = segnet.load_snapshot(str(tmp_path), 100)
    assert args['model'] == 'basic' and snap.endswith('snapshot_iter_100')
    assert set(q) == set(p)
    for k in p:
        assert q[k].dtype == np.float32 and q[k].shape == p[k].shape
        assert np.array_equal(q[k], p[k])


def test_snapshot_selection_quirks(tmp_path):
    rng = np.random.default_rng(1)
    p = random_params(rng)
    write_args(str(tmp_path))
    for it in (1000, 200):
        write_snapshot(str(tmp_path / ('snapshot_iter_%d' % it)), p)
    base = lambda it: os.path.basename(segnet.find_snapshot(str(tmp_path), it))
    assert base(1) == 'snapshot_iter_1000'        # substring: 'iter_1' is in 'snapshot_iter_1000', which sorts first
    assert base(20) == 'snapshot_iter_200'        # substring of iter_200
    assert base(200) == 'snapshot_iter_200'
    assert base(7) == 'snapshot_iter_200'         # no match: the last of the sorted list


def test_snapshot_refusals(tmp_path):
    rng = np.random.default_rng(2)
    p = random_params(rng)
    write_args(str(tmp_path), model='normal')
    write_snapshot(str(tmp_path / 'snapshot_iter_1'), p)
    with pytest.raises(ValueError, match="'normal'"):
        segnet.load_snapshot(str(tmp_path), 1)
    write_args(str(tmp_path))
    write_snapshot(str(tmp_path / 'snapshot_iter_1'), p, drop=('conv3_bn/avg_var',))
    with pytest.raises(KeyError, match='conv3_bn/avg_var'):
        segnet.load_snapshot(str(tmp_path), 1)


# ------------------------------------------------------------------------------- BN folding
def test_bn_folding_float64():
    rng = np.random.default_rng(3)
    p = random_params(rng)
    x = torch.from_numpy(rng.standard_normal((1, 3, 32, 48)))
    pu, hu = sref.forward64(p, x)                                 # BN unfolded (test mode), as the model states it
    pf, hf = sref.forward64(p, x, layer=sref.folded_conv)
    scale = float(hu.abs().max())
    assert float((hu - hf).abs().max()) <= 1e-12 * scale
    assert float((pu - pf).abs().max()) <= 1e-12


def test_pack_weight():
    rng = np.random.default_rng(4)
    w3 = rng.standard_normal((64, 3, 7, 7)).astype(np.float32)
    w64 = rng.standard_normal((64, 64, 7, 7)).astype(np.float32)
    p3, p64 = segnet.pack_weight(w3), segnet.pack_weight(w64)
    assert p3.shape == (49, 64, 4) and p64.shape == (49, 64, 64)
    assert np.all(p3[:, :, 3] == 0)
    for ky, kx, n, c in ((0, 0, 0, 0), (6, 2, 17, 2), (3, 6, 63, 1)):
        assert p3[ky * 7 + kx, n, c] == w3[n, c, ky, kx]
        assert p64[ky * 7 + kx, n, 40 + c] == w64[n, 40 + c, ky, kx]


def test_layer_flops_table():
    f = segnet.layer_flops()
    assert round(f['conv1'] / 1e9, 1) == 9.9 and round(f['conv2'] / 1e9, 1) == 52.6
    assert abs(f['conv_decode1'] / 1e9 - 210.4) < 0.1
    assert round(sum(f.values()) / 1e9) == 358


# ------------------------------------------------------------------------------- CLI
def test_cli_defaults_match_reference():
    lfs = importlib.import_module('labels_from_segnet')
    a = lfs.get_parser().parse_args([])
    assert (a.param_dir, a.iteration, a.gpu, a.img_zip_fn, a.label_zip_fn, a.out_dir, a.start_index,
            a.end_index, a.soft_label, a.eval_shape) == (None, None, -1, None, None, None, None, None, False, [1024, 2048])
    assert a.no_figure is False and a.batchsize == 4
    a = lfs.get_parser().parse_args(['--eval_shape', '64', '128', '--iteration', '3', '--soft_label'])
    assert a.eval_shape == [64, 128] and a.iteration == 3 and a.soft_label


# ------------------------------------------------------------------------------- dataset
def make_zips(tmp_path, keys, extra_label_keys=(), H=24, W=40, seed=5):
    rng = np.random.default_rng(seed)
    img_zip, label_zip = str(tmp_path / 'img.zip'), str(tmp_path / 'label.zip')
    imgs, labels = {}, {}
    with zipfile.ZipFile(img_zip, 'w') as zi, zipfile.ZipFile(label_zip, 'w') as zl:
        for k in keys:
            city = k.split('_')[0]
            imgs[k] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            zi.writestr('leftImg8bit/val/%s/%s_leftImg8bit.png' % (city, k), syn.png(imgs[k]))
        zi.writestr('leftImg8bit/val/README.txt', b'not an image')
        for k in list(keys) + list(extra_label_keys):
            city = k.split('_')[0]
            labels[k] = rng.integers(0, 12, (H, W), dtype=np.uint8)
            zl.writestr('gtFine/val/%s/%s_gtFine_labelIds.png' % (city, k), syn.png(labels[k]))
            zl.writestr('gtFine/val/%s/%s_gtFine_color.png' % (city, k), syn.png(labels[k]))
    return img_zip, label_zip, imgs, labels


def test_dataset_pairing_labels_standardisation(tmp_path):
    keys = ['munster_000002_000019', 'frankfurt_000000_000294', 'lindau_000001_000019']
    img_zip, label_zip, imgs, labels = make_zips(tmp_path, keys, extra_label_keys=['aachen_000000_000019'])
    d = segnet.ZippedCityscapesRoadDataset(img_zip, label_zip, (24, 40))
    assert len(d) == 3                                   # the image side has fewer members: its keys, archive order
    for i, k in enumerate(keys):
        assert os.path.basename(d.img_fns[i]) == k + '_leftImg8bit.png'
        assert os.path.basename(d.label_fns[i]) == k + '_gtFine_labelIds.png'
        img, label = d[i]
        want = imgs[k].transpose(2, 0, 1).astype(np.float32)
        want = (want - segnet.MEAN[:, None, None]) / segnet.STD[:, None, None]
        assert img.dtype == np.float32 and np.array_equal(img.view(np.uint32), want.view(np.uint32))
        lab = labels[k].astype(np.int64)
        assert label.dtype == np.int32
        assert np.array_equal(label, np.where(lab <= 6, -1, np.where(lab == 7, 1, 0)))
    # resized: OpenCV cubic of the uint8 image first, then the two float32 operations
    d2 = segnet.ZippedCityscapesRoadDataset(img_zip, label_zip, (16, 32))
    img, label = d2[1]
    want = cli.resize_cvcubic_chw(imgs[keys[1]].transpose(2, 0, 1), (16, 32)).astype(np.float32)
    want -= segnet.MEAN[:, None, None]
    want /= segnet.STD[:, None, None]
    assert img.shape == (3, 16, 32) and np.array_equal(img, want) and label.shape == (24, 40)


def test_dataset_missing_archive(tmp_path):
    with pytest.raises(ValueError, match='does not exist'):
        segnet.ZippedCityscapesRoadDataset(str(tmp_path / 'a.zip'), str(tmp_path / 'b.zip'), (16, 16))


# ------------------------------------------------------------------------------- score resize
@pytest.mark.parametrize('src,dst', [((7, 9), (14, 18)), ((7, 9), (17, 23)), ((16, 32), (32, 64)), ((5, 6), (5, 13))])
def test_resize_matches_pillow_bilinear(src, dst):
    from PIL import Image
    rng = np.random.default_rng(6)
    s = rng.random((2,) + src).astype(np.float32)
    got = segnet.resize_bilinear_pil(s, dst)
    want = np.stack([np.asarray(Image.fromarray(c, mode='F').resize(dst[::-1], Image.BILINEAR), np.float32) for c in s])
    assert got.shape == want.shape == (2,) + dst
    np.testing.assert_allclose(got, want, atol=1e-6, rtol=0)


def test_resize_refuses_downscale():
    with pytest.raises(ValueError, match='downscale'):
        segnet.resize_bilinear_pil(np.zeros((2, 8, 8), np.float32), (4, 16))
