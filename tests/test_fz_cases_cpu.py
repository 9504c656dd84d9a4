"""The felzenszwalb cases of fz_cases.py, checked on the CPU: (a) a plain sequential restatement of the published
algorithm equals the oracle on every small case — the oracle is pinned against scikit-image's compiled core on
synth_scene / synth_image fixtures only, so this is what gives it authority on noise and tie-heavy inputs —,
(b) every case has the property it claims, (c) the sizes bracket the kernel switch of fz_run."""
import os
import re

import numpy as np
import pytest

import fz_cases as fz
from conftest import ROOT


# ------------------------------------------------------------------------------------------ (a) the plain reference
def plain_costs(orc, img_chw, sigma, uint8_image=False):
    """The oracle's own smoothing and edge costs: x / 255 in float32 (float64 for a uint8 image), fz_blur, fz_edges."""
    x = np.asarray(img_chw).transpose(1, 2, 0)
    x = x.astype(np.float64) / 255. if uint8_image else (x.astype(np.float32) / np.float32(255.)).astype(np.float64)
    return orc.fz_edges(orc.fz_blur(x, sigma=sigma))


def plain_felzenszwalb(costs, edges, npix, scale, min_size):
    """Felzenszwalb & Huttenlocher, as the header of oracle/fz_oracle.c restates it: edges in stable cost order, one
    union-find loop (root = smaller pixel index; merge if cost < min over both sides of float32(int + k / size)),
    a second loop over the same order merging components below min_size.  -> labels, unions of pass 1, of pass 2."""
    order = np.argsort(costs, kind='stable')
    k = float(scale) / 255.
    parent = list(range(npix))
    size = [1] * npix
    inner = [0.0] * npix
    ea, eb, cs = edges[:, 0].tolist(), edges[:, 1].tolist(), costs.tolist()

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:
            parent[i], i = r, parent[i]
        return r

    unions = [0, 0]
    for second in (0, 1):
        for e in order.tolist():
            a, b = find(ea[e]), find(eb[e])
            if a == b:
                continue
            if second:
                merge = size[a] < min_size or size[b] < min_size
            else:
                merge = cs[e] < float(min(np.float32(inner[a] + k / size[a]), np.float32(inner[b] + k / size[b])))
            if merge:
                r, o = (a, b) if a < b else (b, a)
                parent[o] = r
                size[r] = size[a] + size[b]
                inner[r] = cs[e]
                unions[second] += 1
    roots = np.array([find(i) for i in range(npix)])
    return np.unique(roots, return_inverse=True)[1].reshape(-1), unions[0], unions[1]


@pytest.fixture(scope='module')
def oracle_labels(orc, synth):
    """name, form -> the oracle's labels of image 0 of the case (computed once)."""
    memo = {}

    def get(case, uint8_image=False):
        key = (case.name, uint8_image)
        if key not in memo:
            f = orc.felzenszwalb_u8 if uint8_image else orc.felzenszwalb
            memo[key] = f(fz.image(case, synth, 0, uint8_image), case.scale, case.sigma, case.min_size)
        return memo[key]
    return get


def test_small_version_of_every_family():
    kinds = {c.gen[0] + ('_few' if c.gen[0] == 'noise' and len(c.gen) > 2 else '') for c in fz.CASES}
    assert {c.gen[0] + ('_few' if c.gen[0] == 'noise' and len(c.gen) > 2 else '') for c in fz.SMALL} == kinds
    assert kinds >= {'noise', 'noise_few', 'checker', 'stripes', 'constant', 'synth_image', 'synth_scene'}
    assert len({c.name for c in fz.CASES}) == len(fz.CASES)


@pytest.mark.parametrize('case', fz.SMALL, ids=lambda c: c.name)
@pytest.mark.parametrize('uint8_image', [False, True], ids=['f32', 'u8'])
def test_plain_reference_equals_oracle(orc, synth, oracle_labels, case, uint8_image):
    costs, edges = plain_costs(orc, fz.image(case, synth, 0, uint8_image), case.sigma, uint8_image)
    labels, u0, u1 = plain_felzenszwalb(costs, edges, case.H * case.W, case.scale, case.min_size)
    ref = oracle_labels(case, uint8_image)
    assert np.array_equal(labels.reshape(case.H, case.W), ref)
    assert case.H * case.W - u0 - u1 == ref.max() + 1
    if case.prop.get('cleanup_majority'):
        assert u1 > u0, (u0, u1)


# ------------------------------------------------------------------------------------------ (b) the claimed properties
@pytest.mark.parametrize('case', fz.CASES, ids=lambda c: c.name)
def test_claimed_property(orc, synth, oracle_labels, case):
    ref = oracle_labels(case)
    assert ref.shape == (case.H, case.W) and ref.min() == 0
    sizes = np.bincount(ref.ravel())
    n = len(sizes)
    assert sizes.min() > 0
    p = dict(case.prop)
    if 'n' in p:
        assert n == p.pop('n')
    if 'n_min' in p:
        assert n >= p.pop('n_min'), n
    if 'smallest' in p:
        assert sizes.min() == p.pop('smallest')
    if 'largest_min' in p:
        assert sizes.max() >= p.pop('largest_min'), sizes.max()
    if 'sizes' in p:
        assert tuple(sorted(sizes.tolist())) == p.pop('sizes')
    if 'zero_cost' in p or 'max_costs' in p:
        if p.pop('zero_cost', False):
            assert not plain_costs(orc, fz.image(case, synth), case.sigma)[0].any()
        if 'max_costs' in p:
            costs, _ = plain_costs(orc, fz.image(case, synth, 0, True), case.sigma, True)
            distinct = np.unique(costs[costs > 0])
            assert len(distinct) <= p.pop('max_costs'), len(distinct)
            assert (costs > 0).sum() / len(distinct) > p.pop('tie_group_min', 0)
    if p.pop('cleanup_majority', False):
        assert case in fz.SMALL                 # counted by the plain reference, in test_plain_reference_equals_oracle
    assert not p, p
    if n > 1:
        assert sizes.min() >= min(case.min_size, case.H * case.W)
    # the 8-bit form (x / 255 in float64) is run on the GPU exactly where it gives other labels
    differs = not np.array_equal(oracle_labels(case, True), ref)
    assert differs == (case.forms == 'both'), int((oracle_labels(case, True) != ref).sum())


def test_radius():
    r = {c.name: orc_radius(c.sigma) for c in fz.CASES}
    assert r['noise_239x240_r0'] == 0 and r['few_224x256'] == 0 and r['nomerge_96x128'] == 0
    assert r['r31_40x56'] == 31 and r['r31_5x9'] == 31 and 2 * 31 + 1 <= 64         # the oracle's cap is 64 weights
    assert r['r31_5x9'] > 2 * max(5, 9) and r['r12_3x5'] > 2 * 5                    # the reflection wraps more than one period
    assert orc_radius(7.9) == 32                                                   # ... and 7.8 is the last sigma below it


def orc_radius(sigma):
    return int(4.0 * sigma + 0.5)


# ------------------------------------------------------------------------------------------ (c) the boundary arithmetic
def test_kernel_switch_brackets():
    """If this fails, fz_run's constants moved: move the boundary shapes of fz_cases.CASES (and LPAR_MAX_NPIX) with them."""
    assert fz.lpar(224 * 256) and 224 * 256 == 57344 == fz.LPAR_MAX_NPIX
    assert fz.lpar(143 * 401) and 143 * 401 == 57343 and fz.par_bytes(57343) == fz.par_bytes(57344)
    assert not fz.lpar(15 * 3823) and 15 * 3823 == 57345
    assert not fz.lpar(239 * 240) and 239 * 240 == 57360
    assert not fz.lpar(240 * 241)
    assert fz.cells(57344) == 2560 == fz.MIN_CELLS and fz.cells(57343) == 2560
    assert fz.cells(224 * 224) == 3456 and fz.cells(96 * 128) == 4096 and fz.cells(57345) == 4096
    shapes = {(c.H, c.W) for c in fz.CASES}
    assert {(224, 256), (143, 401), (15, 3823), (239, 240)} <= shapes
    assert max(c.H * c.W for c in fz.CASES) <= 240 * 241


def test_kernel_switch_restates_fz_run():
    """The restatement in fz_cases.py, held against the source lines of fz_run it restates."""
    src = open(os.path.join(ROOT, 'superpixel-align_amd', 'csrc', 'spa_felz.hip')).read()
    flat = re.sub(r'\s+', ' ', src)
    assert 'const size_t lds_limit = 156 * 1024;' in flat
    assert 'const size_t par_bytes = ((size_t)npix * 2 + 15) & ~(size_t)15;' in flat
    assert 'npix <= 65535 && par_bytes + 2560 * 16 + FZ_THREADS * 4 <= lds_limit' in flat
    assert 'long long cells = lpar ? (long long)((lds_limit - par_bytes - FZ_THREADS * 4) / 16) : 4096;' in flat
    assert 'if (cells > 4096) cells = 4096;' in flat
    assert re.search(r'#define FZ_THREADS 1024\b', src)
