"""GPU tests of the device-resident cache of decoded examples (train_segnet.py --device_cache_gb): the input kernels
that read their sources through a table of addresses (Engine.segnet_train_input_ptrs / segnet_train_label_ptrs)
against their contiguous twins, bit for bit; segnet_loader.TrainLoader with a DeviceStage and a DeviceFrameCache against
the same loader without one; train_segnet.py with the flag against the run without it (losses, snapshots, --resume),
also as two gloo ranks on one GPU; and what a cached run whose step raises leaves behind.  Every child runs under a
time limit; a failing child ends the test."""
import ctypes
import importlib
import os
import re
import sys
import uuid
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

st = importlib.import_module('superpixel-align_amd.segnet_train')
sl = importlib.import_module('superpixel-align_amd.segnet_loader')
fc = importlib.import_module('superpixel-align_amd.frame_cache')
cli = importlib.import_module('superpixel-align_amd.cli')
_lib = importlib.import_module('superpixel-align_amd._lib')

TIMEOUT = 900
SCRIPT = os.path.join(ROOT, 'train_segnet.py')

# (source, target): both passes down, both passes up, equal sizes (widen only), one axis
SHAPES = [((37, 53), (16, 24)), ((16, 24), (37, 53)), ((24, 40), (24, 40)), ((24, 40), (24, 20))]
B = 3


@pytest.fixture(scope='module')
def eng():
    return importlib.import_module('superpixel-align_amd.engine').default_engine()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _draws(rng, augment):
    if not augment:
        return None, None
    shifts = np.stack([st.pca_lighting_shift(rng.normal(0, 25.5, 3)) for _ in range(B)])
    return _dev(shifts), _dev(np.array([1, 0, 1], np.uint8))


def _tables(items):
    """items: B host arrays of one shape and dtype -> [(name, what to keep alive, table (B,) int64 on the device, the
    contiguous batch the table stands for)]: addresses into one contiguous batch; separately allocated items in
    permuted order with one of them twice; every item one byte into its allocation"""
    nbytes = items[0].nbytes
    batch = _dev(np.stack(items))
    out = [('contiguous', batch, [batch.data_ptr() + j * nbytes for j in range(B)], batch)]
    apart = [_dev(a) for a in items]
    order = [2, 0, 2]
    out.append(('apart', apart, [apart[j].data_ptr() for j in order], _dev(np.stack([items[j] for j in order]))))
    odd = []
    for a in items:
        buf = torch.empty(nbytes + 1, dtype=torch.uint8, device='cuda')
        buf[1:] = _dev(a.reshape(-1).view(np.uint8))
        odd.append(buf)
    out.append(('odd', odd, [b.data_ptr() + 1 for b in odd], batch))
    assert all(p % 2 == 1 for p in out[-1][2])
    return [(name, keep, torch.tensor(addr, dtype=torch.int64, device='cuda'), twin) for name, keep, addr, twin in out]


def _twice_into_poison(run, want):
    """run(out) writes `want`, bit for bit, into a poisoned buffer, twice"""
    out = torch.empty_like(want)
    for _ in range(2):
        out.view(torch.uint8).fill_(0xCD)
        assert run(out) is out
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize('augment', [False, True])
@pytest.mark.parametrize('src,dst', SHAPES)
@pytest.mark.parametrize('backend', ['pil', 'cv2'])
def test_input_ptrs_equals_the_contiguous_entry_point(eng, monkeypatch, backend, src, dst, augment):
    monkeypatch.setattr(cli, 'RESIZE_BACKEND', [backend])
    rng = np.random.default_rng(src[0] * 7 + dst[1])
    frames = [rng.integers(0, 256, src + (3,), dtype=np.uint8) for _ in range(B)]
    frames[0][:5] = 255
    shifts, flips = _draws(rng, augment)
    for name, keep, table, twin in _tables(frames):
        want = eng.segnet_train_input(twin, dst, shifts, flips)
        assert want.shape == (B, 3) + dst
        _twice_into_poison(lambda out: eng.segnet_train_input_ptrs(table, B, src, dst, shifts, flips, out=out), want)
    torch.cuda.synchronize()


@pytest.mark.parametrize('augment', [False, True])
@pytest.mark.parametrize('src,dst', SHAPES)
@pytest.mark.parametrize('backend', ['pil', 'cv2'])
def test_label_ptrs_equals_the_contiguous_entry_point(eng, monkeypatch, backend, src, dst, augment):
    monkeypatch.setattr(cli, 'RESIZE_BACKEND', [backend])
    rng = np.random.default_rng(src[1] * 5 + dst[0])
    masks = [rng.integers(0, 256, src, dtype=np.uint8) for _ in range(B)]
    scores = [rng.normal(0, 1, (2,) + src).astype(np.float32) for _ in range(B)]
    _, flips = _draws(rng, augment)
    for items, shape, dtype in ((masks, src, np.uint8), (scores, (2,) + src, np.float32)):
        for name, keep, table, twin in _tables(items):
            want = eng.segnet_train_label(twin, dst, flips)
            assert want.shape == (B,) + shape[:-2] + dst
            _twice_into_poison(lambda out: eng.segnet_train_label_ptrs(table, B, shape, dtype, dst, flips, out=out),
                               want)
    torch.cuda.synchronize()


def test_refusals_launch_nothing(eng):
    """a null table, B = 0 and the twins' refusals: an error code, and the poisoned output as it was"""
    src, dst = (37, 53), (16, 24)
    frames = torch.zeros((B,) + src + (3,), dtype=torch.uint8, device='cuda')
    table = torch.tensor([frames[j].data_ptr() for j in range(B)], dtype=torch.int64, device='cuda')
    out = torch.empty((B, 3) + dst, dtype=torch.float32, device='cuda')
    lab = torch.empty((B,) + dst, dtype=torch.int32, device='cuda')
    out.view(torch.uint8).fill_(0xCD)
    lab.view(torch.uint8).fill_(0xCD)
    with pytest.raises(_lib.SpalignError):
        eng.segnet_train_input_ptrs(None, B, src, dst, out=out)
    with pytest.raises(_lib.SpalignError):
        eng.segnet_train_label_ptrs(None, B, src, np.uint8, dst, out=lab)
    with pytest.raises(_lib.SpalignError):
        eng.segnet_train_input_ptrs(table, B, src, dst, backend='nearest', out=out)
    with pytest.raises(_lib.SpalignError):
        eng.segnet_train_label_ptrs(table, B, (2,) + src, np.uint8, dst, out=lab)
    L, p = eng._lib, lambda t: ctypes.c_void_p(t.data_ptr())
    xb, xk, ksx = eng._input_tables('cubic', src[1], dst[1], 'pil')
    yb, yk, ksy = eng._input_tables('cubic', src[0], dst[0], 'pil')
    yi, xi = eng._input_tables('nearest', src[0], dst[0], 'pil'), eng._input_tables('nearest', src[1], dst[1], 'pil')
    tmp = torch.empty((B, 3, src[0], dst[1]), dtype=torch.float32, device='cuda')
    for n, tab in ((0, p(table)), (B, None), (65536, p(table))):
        assert L.spa_segnet_train_input_ptrs(eng._ctx, tab, n, src[0], src[1], dst[0], dst[1], 0, p(xb), p(xk), ksx,
                                             p(yb), p(yk), ksy, None, None, p(tmp), p(out), eng._s()) != 0
        assert L.spa_segnet_train_label_ptrs(eng._ctx, tab, 0, n, 1, src[0], src[1], dst[0], dst[1], p(yi), p(xi),
                                             None, p(lab), eng._s()) != 0
    # the resize tables a pass needs, and the scratch of two passes, are asked for as by the twin
    assert L.spa_segnet_train_input_ptrs(eng._ctx, p(table), B, src[0], src[1], dst[0], dst[1], 0, None, p(xk), ksx,
                                         p(yb), p(yk), ksy, None, None, p(tmp), p(out), eng._s()) != 0
    assert L.spa_segnet_train_input_ptrs(eng._ctx, p(table), B, src[0], src[1], dst[0], dst[1], 0, p(xb), p(xk), ksx,
                                         p(yb), p(yk), ksy, None, None, None, p(out), eng._s()) != 0
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == 0xCD).all()) and bool((lab.view(torch.uint8) == 0xCD).all())


# ------------------------------------------------------------------------------- TrainLoader with a DeviceStage
H, W = 32, 48
FRAME, LABEL = H * W * 3, H * W


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    return syn.write(str(tmp_path_factory.mktemp('cache')), 8, 4, H, W)


def _epochs(eng, ds, iters, seed, cache=None):
    np.random.seed(seed)
    it = st.ShuffledIterator(8, 2)
    loader = sl.TrainLoader(ds, np.arange(8), it, 2, sl.DeviceStage(ds, eng), cache=cache)
    count = [0]
    submit = loader.slabs.submit

    def counted(fn, task):
        count[0] += 1
        return submit(fn, task)
    loader.slabs.submit = counted
    out, tasks = [], []
    try:
        for _ in range(iters):
            img, lab, state = loader.next()
            out.append((img.clone(), lab.clone(), state))
            tasks.append(count[0])
        torch.cuda.synchronize()
        return out, tasks, (loader.cache_hits, loader.cache_misses, loader.n_host_batches)
    finally:
        loader.close()


@pytest.fixture(scope='module')
def uncached(eng, data):
    """the loader without a cache, per --random: computed once and left as it is"""
    out = {}
    for random in (False, True):
        ds = st.ZippedEstimatedCityscapesDataset(data[0], data[1], (16, 24), random, False)
        out[random] = _epochs(eng, ds, 12, seed=5)[0]
    return out


def _compare(plain, got):
    assert len(plain) == len(got)
    for (pi, pl, ps), (gi, gl, gs) in zip(plain, got):
        assert gi.dtype == pi.dtype and gl.dtype == pl.dtype
        assert torch.equal(gi.view(torch.int32), pi.view(torch.int32)) and torch.equal(gl, pl)
        (ia, ra), (ib, rb) = ps, gs
        assert set(ia) == set(ib) and all(np.array_equal(ia[k], ib[k]) for k in ia)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and ra[2:] == rb[2:]


@pytest.mark.parametrize('random', [False, True])
def test_device_loader_three_epochs_equal_the_uncached_loader(eng, data, uncached, random):
    ds = st.ZippedEstimatedCityscapesDataset(data[0], data[1], (16, 24), random, False)
    before = syn.shm_names()
    cache = fc.DeviceFrameCache(1 << 20, eng.device)
    try:
        got, tasks, (hits, misses, n_host) = _epochs(eng, ds, 12, seed=5, cache=cache)
        _compare(uncached[random], got)
        assert tasks[3] == tasks[-1] == 16 and n_host == 0 and misses == 8 and hits >= 16
        assert cache.counters()['entries'] == 16 and cache.counters()['bytes'] == 8 * (FRAME + LABEL)
        assert len(cache.chunks) == 1 and cache.chunks[0].is_cuda and sum(cache.sizes) <= cache.budget
    finally:
        cache.close()
    assert cache.chunks == [] and syn.shm_names() == before


def test_device_loader_partial_budget(eng, data, uncached):
    ds = st.ZippedEstimatedCityscapesDataset(data[0], data[1], (16, 24), True, False)
    cache = fc.DeviceFrameCache(3 * (FRAME + LABEL), eng.device)
    try:
        got, tasks, (hits, misses, n_host) = _epochs(eng, ds, 12, seed=5, cache=cache)
        _compare(uncached[True], got)
        frames = [k for k in cache.table if k[0] == data[0]]
        assert len(frames) == 3 and cache.counters()['entries'] == 6 and sum(cache.sizes) <= cache.budget
        assert tasks[-1] == 2 * misses and 18 <= misses <= 24 and hits >= 6 and n_host == 0
    finally:
        cache.close()


# ------------------------------------------------------------------------------- train_segnet.py
def _run(cmd, env, ok=True):
    return syn.run(cmd, env, ROOT, TIMEOUT, ok)


def _same_snapshot(fa, fb):
    ks = syn.same_snapshot(fa, fb, bitwise=True)
    assert 'extensions/np_random/keys' in ks and 'updater/iterator:main/order' in ks
    return len(ks)


def _summary(stderr):
    """-> (train hits, validation misses after the first pass) of the run's line about its cache"""
    lines = [ln for ln in stderr.splitlines() if 'device cache: hits' in ln]
    assert len(lines) == 1, stderr[-3000:]
    m = re.search(r'train hits (\d+) misses (\d+); validation hits (\d+) misses (\d+) \((\d+) after the first pass\)',
                  lines[0])
    assert m, lines[0]
    return [int(v) for v in m.groups()]


def test_cached_run_equals_the_loader_run_and_resumes_without_the_cache(tmp_path):
    """--random, MomentumSGD, 64 x 128, 6 training and 4 validation frames in batches of 2, 8 iterations, validation
    and a snapshot every 2"""
    z = syn.write(str(tmp_path / 'data'), 6, 4, 64, 128)
    common = syn.train_args(z, 8, 2, 2, extra=['--random', '--optimizer', 'MomentumSGD'])
    d = {k: str(tmp_path / k) for k in ('loader', 'cached', 'resumed')}
    base = [sys.executable, SCRIPT, '--loader_procs', '2']
    _run(base + common + ['--result_dir', d['loader']], syn.env())
    r = _run(base + ['--device_cache_gb', '1'] + common + ['--result_dir', d['cached']], syn.env())
    import json
    assert json.load(open(os.path.join(d['cached'], 'args.txt')))['device_cache_gb'] == 1.0
    assert 'device_cache_gb' not in json.load(open(os.path.join(d['loader'], 'args.txt')))
    assert syn.losses(d['loader']) == syn.losses(d['cached']) and len(syn.losses(d['loader'])) == 4
    for it in (2, 4, 6, 8):
        assert _same_snapshot(os.path.join(d['loader'], 'snapshot_iter_%d' % it),
                              os.path.join(d['cached'], 'snapshot_iter_%d' % it)) > 60
    hits, misses, val_hits, val_misses, val_late = _summary(r.stderr)
    assert hits > 0 and misses == 6                       # every training example is decoded once
    assert val_hits == 3 * 2 and val_misses == 2 and val_late == 0
    # resume from the cached run's snapshot, without the cache
    _run(base + common + ['--result_dir', d['resumed'], '--resume', os.path.join(d['cached'], 'snapshot_iter_4')],
         syn.env())
    _same_snapshot(os.path.join(d['loader'], 'snapshot_iter_8'), os.path.join(d['resumed'], 'snapshot_iter_8'))
    assert syn.losses(d['resumed'])[-1][:3] == syn.losses(d['loader'])[-1][:3]


def test_two_gloo_ranks_with_the_cache_equal_the_launch_without(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 9, 4, 48, 96)
    env = syn.env(SPA_DIST_BACKEND='gloo', SPA_BENCH_SAME_DEVICE='1')
    common = syn.train_args(z, 8, 4, 4, (32, 64), (48, 96), ['--random', '--optimizer', 'MomentumSGD'])

    def torchrun(argv):
        return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                '--master-addr', '127.0.0.1', '--master-port', str(syn.free_port()), SCRIPT] + argv
    da, db = str(tmp_path / 'loader'), str(tmp_path / 'cached')
    _run(torchrun(['--data_parallel', '--loader_procs', '2'] + common + ['--result_dir', da]), env)
    r = _run(torchrun(['--data_parallel', '--loader_procs', '2', '--device_cache_gb', '0.5'] + common +
                      ['--result_dir', db]), env)
    assert syn.losses(da) == syn.losses(db)
    for it in (4, 8):
        _same_snapshot(os.path.join(da, 'snapshot_iter_%d' % it), os.path.join(db, 'snapshot_iter_%d' % it))
    # every rank has its own cache of its own shard
    lines = [ln for ln in r.stderr.splitlines() if 'device cache: hits' in ln]
    assert sorted(re.search(r'rank (\d+) device cache', ln).group(1) for ln in lines) == ['0', '1']


def _marked_processes(mark):
    """pids of the live processes that carry the marker in their environment (a run's workers inherit it)"""
    out = []
    for pid in os.listdir('/proc'):
        if not pid.isdigit() or int(pid) == os.getpid():
            continue
        try:
            with open('/proc/%s/environ' % pid, 'rb') as f:
                if mark.encode() in f.read():
                    out.append(int(pid))
        except OSError:
            pass
    return out


def test_nothing_is_left_after_a_cached_run_whose_step_raises(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 5, 2, 48, 96)
    # scores with three channels: the soft-label loss of the first step refuses them against the two-channel output
    bad = str(tmp_path / 'bad_scores.zip')
    rng = np.random.default_rng(1)
    with zipfile.ZipFile(z[1]) as zl, zipfile.ZipFile(bad, 'w', zipfile.ZIP_STORED) as zo:
        for name in zl.namelist():
            zo.writestr(name[:-len('.npy')] + '_scores.npy', syn.npy(rng.random((3, 48, 96)).astype(np.float32)))
    before = set(os.listdir('/dev/shm'))
    mark = 'SPA_TEST_MARK_%s' % uuid.uuid4().hex
    zb = [z[0], bad, z[2], z[3]]
    common = syn.train_args(zb, 4, 2, 2, (32, 64), (48, 96), ['--random', '--optimizer', 'MomentumSGD',
                                                              '--use_soft_label'])
    r = _run([sys.executable, SCRIPT, '--loader_procs', '2', '--device_cache_gb', '1'] + common +
             ['--result_dir', str(tmp_path / 'bad')], syn.env(**{mark: '1'}), ok=False)
    assert r.returncode != 0 and 'Traceback' in r.stderr
    assert not os.path.exists(str(tmp_path / 'bad' / 'snapshot_iter_2'))
    assert 'device cache: hits' in r.stderr               # the cache was closed on the way out
    assert _marked_processes(mark) == [] and set(os.listdir('/dev/shm')) == before
