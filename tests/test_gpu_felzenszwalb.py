"""GPU parity of the felzenszwalb branch (spa_felzenszwalb through the C ABI): bit-exact label
maps against the oracle — which itself is pinned bit for bit against scikit-image's compiled core
(tests/golden/fz_*.npz) — on fixtures, batches and edge shapes."""
import glob
import importlib
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


FZ_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, 'fz_s*.npz')))


@pytest.mark.parametrize('name', FZ_CASES)
def test_felzenszwalb_golden(eng, synth, name):
    g = golden(name)
    seed, H, W, min_size, integer = (int(v) for v in g['meta'])
    scale, sigma = (float(v) for v in g['params'])
    img = synth.synth_scene(seed, H, W, integer_valued=bool(integer))
    labels, n_labels = eng.felzenszwalb(torch.from_numpy(img[None]).cuda(), scale, sigma, min_size)
    eng.raise_on_status()
    assert np.array_equal(labels[0].cpu().numpy(), g['pinned'])        # skimage core, bit exact
    assert int(n_labels[0]) == int(g['pinned'].max()) + 1


def test_felzenszwalb_batch_vs_oracle(eng, orc, synth):
    """Reference operating point: 224x224, scale 300, sigma 0.8, min_size 20, a batch at once."""
    imgs = np.stack([synth.synth_scene(20 + i, 224, 224, integer_valued=(i % 2 == 0)) for i in range(6)])
    imgs[5] = synth.synth_image(5, 224, 224)                  # smooth image: very few segments
    labels, n_labels = eng.felzenszwalb(torch.from_numpy(imgs).cuda(), 300.0, 0.8, 20)
    eng.raise_on_status()
    for b in range(6):
        ref = orc.felzenszwalb(imgs[b], 300.0, 0.8, 20)
        assert np.array_equal(labels[b].cpu().numpy().astype(np.int64), ref), b
        assert int(n_labels[b]) == ref.max() + 1


@pytest.mark.parametrize('H,W,scale,sigma,min_size', [(31, 47, 50.0, 0.8, 5), (2, 64, 10.0, 0.5, 2),
                                                     (64, 2, 10.0, 0.5, 2), (128, 160, 1.0, 2.0, 1),
                                                     (200, 300, 1000.0, 0.8, 200)])
def test_felzenszwalb_edge_shapes(eng, orc, synth, H, W, scale, sigma, min_size):
    img = synth.synth_scene(H + W, H, W, n_rect=12)
    labels, n_labels = eng.felzenszwalb(torch.from_numpy(img[None]).cuda(), scale, sigma, min_size)
    eng.raise_on_status()
    ref = orc.felzenszwalb(img, scale, sigma, min_size)
    assert np.array_equal(labels[0].cpu().numpy().astype(np.int64), ref)


@pytest.mark.parametrize('H,W', [(255, 257), (256, 256), (257, 256)])
def test_felzenszwalb_lds_parent_boundary(eng, orc, synth, H, W):
    """65 535 pixels is the last size whose pixel indices fit the 16-bit parent entries (0xFFFF = root) that k_fz_pass_tab<true>
    keeps in LDS.  fz_run switches to the global-array form, k_fz_pass_tab<false>, earlier — above 57 344 pixels, where the array
    and the root table no longer fit in LDS together — so all three sizes here run that form;
    test_gpu_felzenszwalb_hostile.py brackets the switch itself.  Batches of three, so the sorts also take the three-stream path."""
    imgs = np.stack([synth.synth_scene(300 + i, H, W, n_rect=40) for i in range(3)])
    labels, n_labels = eng.felzenszwalb(torch.from_numpy(imgs).cuda(), 120.0, 0.8, 20)
    eng.raise_on_status()
    for b in range(3):
        ref = orc.felzenszwalb(imgs[b], 120.0, 0.8, 20)
        assert np.array_equal(labels[b].cpu().numpy().astype(np.int64), ref), (H, W, b)
        assert int(n_labels[b]) == ref.max() + 1


def test_felzenszwalb_full_size(eng, orc, synth):
    """1024x2048 (8.4 M edges): the reservation scheme at scale."""
    img = synth.synth_scene(77, 1024, 2048, n_rect=120)
    labels, n_labels = eng.felzenszwalb(torch.from_numpy(img[None]).cuda(), 300.0, 0.8, 20)
    eng.raise_on_status()
    ref = orc.felzenszwalb(img, 300.0, 0.8, 20)
    assert np.array_equal(labels[0].cpu().numpy().astype(np.int64), ref)


def test_felzenszwalb_full_size_smooth_image(eng, orc, synth):
    """The bench generator's smooth 1024x2048 image: it ends in ~15 segments, i.e. nearly every live edge of a late window joins a
    small component to one giant one — the case the hub chains of k_fz_pass_tab walk (round 5); labels against the oracle."""
    img = synth.synth_image(3, 1024, 2048)
    labels, n_labels = eng.felzenszwalb(torch.from_numpy(img[None]).cuda(), 300.0, 0.8, 20)
    eng.raise_on_status()
    ref = orc.felzenszwalb(img, 300.0, 0.8, 20)
    assert int(n_labels[0]) == ref.max() + 1 and int(n_labels[0]) < 100
    assert np.array_equal(labels[0].cpu().numpy().astype(np.int64), ref)
