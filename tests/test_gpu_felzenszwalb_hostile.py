"""The felzenszwalb kernels on the inputs of fz_cases.py (noise, few-valued and two-valued images, degenerate ends, radius 0
and 31, the sizes either side of the switch between k_fz_pass_tab<true> and <false> at 57 344 pixels), in mixed batches, in
batches larger than one launch holds and in alternating shapes.  Every comparison is of the int32 label map with the oracle's,
bit for bit (test_fz_cases_cpu.py holds the oracle against a plain sequential reference on these families).  Every call
writes into poisoned buffers with a guard behind them and is repeated for equal bits."""
import hashlib
import importlib

import numpy as np
import pytest

import fz_cases as fz

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

POISON = 0x7f7f7f7f
GUARD = 1024


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


@pytest.fixture(scope='module')
def reference(orc):
    """The oracle's label map of one image, computed once per (image, arguments, form)."""
    memo = {}

    def get(img, scale, sigma, min_size, uint8_image=False):
        key = (hashlib.sha1(np.ascontiguousarray(img).tobytes()).hexdigest(), img.shape, scale, sigma, min_size, uint8_image)
        if key not in memo:
            memo[key] = orc.felzenszwalb_u8(img.astype(np.uint8), scale, sigma, min_size) if uint8_image else \
                orc.felzenszwalb(img, scale, sigma, min_size)
            memo[key].setflags(write=False)
        return memo[key]
    return get


def poisoned(n):
    buf = torch.full((n + GUARD,), POISON, dtype=torch.int32, device='cuda')
    return buf[:n], buf


def run(eng, imgs, scale, sigma, min_size, uint8_image=False):
    """One call into poisoned, guarded buffers, and a second one for equal bits -> labels (B, H, W), n_labels (B) as numpy."""
    B, _, H, W = imgs.shape
    x = torch.from_numpy(np.ascontiguousarray(imgs, dtype=np.float32)).cuda()
    got = []
    for _ in range(2):
        labels, lbuf = poisoned(B * H * W)
        n_labels, nbuf = poisoned(B)
        eng.felzenszwalb(x, scale, sigma, min_size, uint8_image=uint8_image, out=(labels.view(B, H, W), n_labels))
        eng.raise_on_status()
        assert bool((lbuf[B * H * W:] == POISON).all()) and bool((nbuf[B:] == POISON).all()), 'guard overwritten'
        assert not bool((labels == POISON).any()) and not bool((n_labels == POISON).any()), 'output not written'
        got.append((labels.view(B, H, W).cpu().numpy(), n_labels.cpu().numpy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1]), 'second call differs'
    return got[0]


def check(eng, reference, imgs, scale, sigma, min_size, uint8_image=False):
    labels, n_labels = run(eng, imgs, scale, sigma, min_size, uint8_image)
    assert labels.dtype == np.int32
    for b in range(len(imgs)):
        ref = reference(imgs[b], scale, sigma, min_size, uint8_image)
        assert np.array_equal(labels[b], ref), (b, int((labels[b] != ref).sum()))
        assert int(n_labels[b]) == ref.max() + 1, b
    print('label maps compared: %d' % len(imgs))
    return labels


FORMS = [(c, u8) for c in fz.CASES for u8 in ((False, True) if c.forms == 'both' else (False,))]


@pytest.mark.parametrize('case,uint8_image', FORMS, ids=['%s-%s' % (c.name, 'u8' if u8 else 'f32') for c, u8 in FORMS])
def test_case(eng, reference, synth, case, uint8_image):
    imgs = fz.batch(case, synth, uint8_image).astype(np.float32)
    check(eng, reference, imgs, case.scale, case.sigma, case.min_size, uint8_image)


@pytest.mark.parametrize('scale,sigma,min_size', [(300.0, 0.8, 20), (30.0, 0.1, 20)])
@pytest.mark.parametrize('H,W', [(224, 256), (239, 240)])
def test_mixed_batch(eng, reference, synth, H, W, scale, sigma, min_size):
    """Images of one launch that finish at very different times; the constant one runs no window at all."""
    imgs = np.stack([fz.noise(31, H, W), fz.constant(H, W, 90.0), fz.checker(H, W, 1),
                     synth.synth_scene(32, H, W, n_rect=40), fz.noise(33, H, W, 0, 4)])
    labels = check(eng, reference, imgs, scale, sigma, min_size)
    assert labels[1].max() == 0


def test_batch_larger_than_the_chip(eng, reference):
    """More images than one launch takes (one resident workgroup per image): fz_run splits the batch."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    B = min(n_cu, 256) + 3
    imgs = np.stack([fz.noise(5000 + i, 16, 24) for i in range(B)])
    check(eng, reference, imgs, 30.0, 0.8, 4)


@pytest.mark.parametrize('H,W,B', [(64, 96, 7), (239, 240, 4)])
def test_batch_split_tails(eng, reference, monkeypatch, H, W, B):
    """Sub-batches of 3, 3 and 1 (3 and 1): the three-stream sort, then the single-stream sort with re-entered, smaller
    workspace reservations, into one label tensor."""
    monkeypatch.setenv('SPA_FZ_MAXB', '3')
    imgs = np.stack([fz.noise(6000 + i, H, W) for i in range(B)])
    check(eng, reference, imgs, 30.0, 0.8, 20)


def test_alternating_shapes(eng, reference):
    """The workspace shrinks and grows between calls of one context, across both pass kernels."""
    first = last = None
    for i, (H, W) in enumerate([(239, 240), (16, 24), (224, 256), (239, 240)]):
        imgs = np.stack([fz.noise(7000 + H, H, W), fz.noise(7001 + H, H, W, 0, 4)])
        labels = check(eng, reference, imgs, 300.0, 0.8, 20)
        first, last = (labels if i == 0 else first), labels
    assert np.array_equal(first, last)
