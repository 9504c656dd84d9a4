"""CPU tests of SegNet-Basic training (segnet_train.py, train_segnet.py): Chainer's BatchNorm update, losses,
MomentumSGD / WeightDecay / ExponentialShift and Adam against hand-derived values, HeNormal, the float 'F' bicubic and
NEAREST resizes against Pillow, dataset pairing, snapshots that segnet.load_snapshot reads, the CLI and refusals."""
import importlib
import json
import os
import sys
import zipfile

import numpy as np
import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
cli = importlib.import_module('superpixel-align_amd.cli')
train_segnet = importlib.import_module('train_segnet')


def test_bn_running_update_matches_chainer():
    # y over (B, C, H, W) = (2, 1, 1, 2): values 1, 2, 3, 6 -> mean 3, biased var 3.5, unbiased 14/3
    y = torch.tensor([1.0, 2.0, 3.0, 6.0], dtype=torch.float64).view(2, 1, 1, 2)
    P = {}
    mean = torch.zeros(1, dtype=torch.float64)
    var = torch.ones(1, dtype=torch.float64)
    st.bn_update(mean, var, y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False), 4.0)
    assert mean.item() == pytest.approx(0.9 * 0 + 0.1 * 3.0, abs=1e-15)
    assert var.item() == pytest.approx(0.9 * 1 + 0.1 * 14.0 / 3.0, abs=1e-15)
    # and the normalisation uses the biased variance + 2e-5 (F.batch_norm training, eps 2e-5)
    F = torch.nn.functional
    out = F.batch_norm(y, None, None, torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64),
                       training=True, eps=st.BN_EPS)
    assert torch.allclose(out.flatten(), (y.flatten() - 3.0) / np.sqrt(3.5 + 2e-5), atol=1e-14)
    del P


def test_losses_hand_derived():
    score = torch.zeros((1, 2, 1, 3), dtype=torch.float64)
    score[0, 1, 0, 0] = np.log(3.0)                              # p(class 1) = 3/4 at pixel 0
    t = torch.tensor([[[1, 0, -1]]])
    # pixel 0: -log(3/4); pixel 1: -log(1/2); pixel 2 ignored -> divided by 2
    want = (-np.log(0.75) - np.log(0.5)) / 2
    assert st.softmax_cross_entropy(score, t).item() == pytest.approx(want, abs=1e-14)
    # all ignored: 0 / max(0, 1)
    assert st.softmax_cross_entropy(score, torch.full((1, 1, 3), -1)).item() == 0.0
    ts = torch.zeros((1, 2, 1, 3), dtype=torch.float64)
    ts[0, 1, 0, 0] = 1.0
    ts[0, 0, 0, 1] = 0.5
    # -mean over all 6 elements of t * log_softmax
    want = -(1.0 * np.log(0.75) + 0.5 * np.log(0.5)) / 6
    assert st.soft_label_loss(score, ts).item() == pytest.approx(want, abs=1e-14)
    assert st.mse_loss(score, ts).item() == pytest.approx(((np.log(3.0) - 1) ** 2 + 0.25) / 6, abs=1e-14)


def test_momentum_sgd_chainer_form_with_decay_and_shift():
    p = {'w': torch.tensor([1.0], dtype=torch.float64)}
    opt = st.MomentumSGD(lr=0.1, weight_decay=0.5)
    g = {'w': torch.tensor([2.0], dtype=torch.float64)}
    # step 1: g' = 2 + 0.5 * 1 = 2.5; v = -0.25; p = 0.75
    opt.update(p, g)
    assert p['w'].item() == pytest.approx(0.75, abs=1e-15)
    opt.lr *= 0.1                                                # ExponentialShift
    # step 2: g' = 2 + 0.375 = 2.375; v = 0.9 * -0.25 - 0.01 * 2.375 = -0.24875; p = 0.50125
    opt.update(p, g)
    assert p['w'].item() == pytest.approx(0.50125, abs=1e-15)
    # torch's SGD (v = 0.9 v + g; p -= lr v) gives another value once lr changed
    q = torch.tensor([1.0], dtype=torch.float64, requires_grad=True)
    tor = torch.optim.SGD([q], lr=0.1, momentum=0.9, weight_decay=0.5)
    for lr in (0.1, 0.01):
        tor.param_groups[0]['lr'] = lr
        q.grad = torch.tensor([2.0], dtype=torch.float64)
        tor.step()
    assert abs(q.item() - 0.50125) > 1e-3


def test_adam_chainer_form():
    p = {'w': torch.tensor([1.0], dtype=torch.float64)}
    opt = st.Adam()
    g = {'w': torch.tensor([0.5], dtype=torch.float64)}
    m = v = 0.0
    w = 1.0
    for t in (1, 2):
        opt.update(p, g)
        m += 0.1 * (0.5 - m)
        v += 0.001 * (0.25 - v)
        lr = 0.001 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        w -= lr * m / (np.sqrt(v) + 1e-8)
    assert p['w'].item() == pytest.approx(w, abs=1e-15)


def test_he_normal_init():
    p = st.init_params(0)
    for i, name in enumerate(segnet.LAYERS):
        w = p[name + '/W'].astype(np.float64)
        std = np.sqrt(2.0 / ((3 if i == 0 else 64) * 49))
        assert abs(w.mean()) < 4 * std / np.sqrt(w.size)
        assert abs(w.std() / std - 1) < 0.05
        assert np.all(p[name + '_bn/gamma'] == 1) and np.all(p[name + '_bn/beta'] == np.float32(0.001))
        assert np.all(p[name + '_bn/avg_mean'] == 0) and np.all(p[name + '_bn/avg_var'] == 1)
    assert abs(p['conv_classifier/W'].std() / np.sqrt(2.0 / 64) - 1) < 0.3
    assert np.all(p['conv_classifier/b'] == 0)


def test_float_bicubic_and_nearest_against_pillow():
    from PIL import Image
    rng = np.random.default_rng(0)
    img = (rng.random((3, 37, 53)) * 255).astype(np.float32)
    out = st.resize_bicubic_float(img, (64, 96))
    for c in range(3):
        want = np.asarray(Image.fromarray(img[c], mode='F').resize((96, 64), Image.BICUBIC))
        assert np.array_equal(out[c], want)
    # not the 8-bit path
    assert not np.array_equal(out, cli.resize_bicubic_chw(img.astype(np.uint8), (64, 96)).astype(np.float32))
    label = rng.integers(-1, 2, (1, 37, 53)).astype(np.int32)
    lo = st.resize_nearest_label(label, (64, 96))
    want = np.asarray(Image.fromarray(label[0].astype(np.float32), mode='F').resize((96, 64), Image.NEAREST))
    assert lo.dtype == np.int32 and np.array_equal(lo[0], want.astype(np.int32))


def _write_zips(tmp, n, shape=(32, 48), soft=False):
    from PIL import Image
    rng = np.random.default_rng(1)
    lab_dir = tmp / 'labels'
    lab_dir.mkdir()
    img_zip = str(tmp / 'imgs.zip')
    with zipfile.ZipFile(img_zip, 'w') as zf:
        for i in range(n):
            key = 'city_%06d_%06d' % (i, 19)
            im = (rng.random(shape + (3,)) * 255).astype(np.uint8)
            buf = __import__('io').BytesIO()
            Image.fromarray(im).save(buf, format='PNG')
            zf.writestr('leftImg8bit/train/city/%s_leftImg8bit.png' % key, buf.getvalue())
            if i < n - 1:                                           # one image without a label
                np.save(str(lab_dir / ('%s_leftImg8bit.npy' % key)), rng.random(shape) > 0.5)
    lab_zip = str(tmp / 'labels.zip')
    cli.write_label_zip(str(lab_dir), lab_zip)
    return img_zip, lab_zip


def test_dataset_pairing(tmp_path):
    img_zip, lab_zip = _write_zips(tmp_path, 4)
    d = st.ZippedEstimatedCityscapesDataset(img_zip, lab_zip, (64, 96))
    assert len(d) == 3                                           # the label side has fewer keys
    for i in range(3):
        k = os.path.basename(d.img_fns[i]).split('_leftImg8bit')[0]
        assert os.path.basename(d.label_fns[i]).startswith(k)
    img, lab = d.get_example(0)
    assert img.shape == (3, 64, 96) and img.dtype == np.float32 and lab.shape == (64, 96) and lab.dtype == np.int32
    with np.load(lab_zip) as z:
        raw = z[d.label_fns[0][:-4]]
    assert np.array_equal(lab, st.resize_nearest_label(raw.astype(np.int32)[None], (64, 96))[0])
    np.random.seed(3)
    dr = st.ZippedEstimatedCityscapesDataset(img_zip, lab_zip, (32, 48), random=True)
    a, la = dr.get_example(1)
    b, lb = d.get_example(1)[0], None
    assert a.shape == (3, 32, 48) and la.shape == (32, 48)


def _tiny_trainer_state():
    p = st.init_params(1)
    p['conv1_bn/avg_mean'] = np.linspace(-1, 1, 64).astype(np.float32)
    p['conv1_bn/avg_var'] = np.linspace(0.5, 2, 64).astype(np.float32)
    return p


def test_snapshot_loads_with_segnet(tmp_path):
    p = _tiny_trainer_state()
    d = tmp_path / 'run'
    d.mkdir()
    json.dump({'model': 'basic', 'input_shape': [32, 64]}, open(str(d / 'args.txt'), 'w'))
    it = st.ShuffledIterator(5, 2)
    st.save_snapshot(str(d / 'snapshot_iter_20'), syn.FakeTrainer(p, 7, 3), 20, 0.001, it.state())
    args, snap, params = segnet.load_snapshot(str(d), 20)
    for k in st.PARAM_KEYS + st.STAT_KEYS:
        assert np.array_equal(params[k], p[k]), k
    folded = segnet.fold_bn(params)
    g = p['conv1_bn/gamma'].astype(np.float64) / np.sqrt(p['conv1_bn/avg_var'].astype(np.float64) + 2e-5)
    assert np.allclose(folded['conv1'][1], (p['conv1_bn/beta'] - p['conv1_bn/avg_mean'] * g).astype(np.float32))
    params2, state, t, lr, iteration, its, rnd = st.load_snapshot_state(snap)
    assert (t, lr, iteration) == (7, 0.001, 20) and np.array_equal(state['conv1/W']['v'], np.ones((64, 3, 7, 7)))
    assert np.array_equal(its['order'], it.order) and params2['conv1_bn/N'] == 3


def test_cli_defaults_match_reference():
    a = train_segnet.get_args([])
    want = dict(train_img_zip='data/cityscapes_train_imgs.0.zip', train_label_zip='results/estimated_train_labels.0.zip',
                val_img_zip='data/cityscapes_val_imgs.0.zip', val_label_zip='data/cityscapes_gtFine_val_labels.0.zip',
                model='basic', batchsize=4, lr=0.01, decay_iteration=300, weight_decay=0.0005,
                train_limit=['1000', 'iteration'], optimizer='MomentumSGD', input_shape=[512, 1024], random=False,
                communicator='single_node', prefix='results/round_1', resume=None, log_interval=['50', 'iteration'],
                val_interval=['50', 'iteration'], eval_shape=[1024, 2048], result_dir=None, use_soft_label=False,
                use_mse=False, n_use_data=None)
    assert vars(a) == want


def test_create_result_dir(tmp_path):
    prefix = str(tmp_path / 'results' / 'round_1')
    d0 = train_segnet.create_result_dir(prefix)
    d1 = train_segnet.create_result_dir(prefix)
    assert os.path.isdir(d0) and os.path.isdir(d1) and d0 != d1
    assert os.path.exists(os.path.join(d0, 'train_segnet.py'))
    if d0[:-2] == d1[:-2]:                                       # same second: the counter goes up
        assert d0.endswith('_0') and d1.endswith('_1')


def test_refusals(monkeypatch):
    with pytest.raises(ValueError, match="only SegNet-Basic"):
        train_segnet.check_supported(train_segnet.get_args(['--model', 'normal']))
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(RuntimeError, match='one process'):
        train_segnet.check_supported(train_segnet.get_args([]))


def test_reference_step_index_override():
    """the float64 restatement takes given index maps: with the maps its own argmax chose, the same loss"""
    p = st.init_params(2)
    P = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in st.PARAM_KEYS}
    S1 = {k: torch.tensor(p[k], dtype=torch.float64) for k in st.STAT_KEYS}
    S2 = {k: v.clone() for k, v in S1.items()}
    img = torch.rand((1, 3, 16, 32), dtype=torch.float64) * 255
    t = torch.randint(-1, 2, (1, 16, 32))
    l1, maps = st.reference_loss(P, S1, img, t, st.softmax_cross_entropy)
    l2, _ = st.reference_loss(P, S2, img, t, st.softmax_cross_entropy, idx_maps=maps)
    assert l1.item() == l2.item()
    assert all(torch.equal(S1[k], S2[k]) for k in S1)
