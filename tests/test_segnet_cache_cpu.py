"""CPU tests of the cache of decoded examples (train_segnet.py --device_cache_gb, superpixel-align_amd/frame_cache.py):
the bookkeeping with numpy storage, and the two loaders of segnet_loader.py with the host stages and real spawned
workers against the same loaders without a cache: every batch and every yielded state as arrays, the number of decode
tasks (counted at slabs.submit), a partial budget, an example twice in one batch, a member of another shape, two and
abandoned passes of the label loader, and the flags."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
sl = importlib.import_module('superpixel-align_amd.segnet_loader')
fc = importlib.import_module('superpixel-align_amd.frame_cache')
train_segnet = importlib.import_module('train_segnet')
rtr = importlib.import_module('utils.run_train_rounds')

H, W = 32, 48
FRAME, LABEL = H * W * 3, H * W                       # bytes of one decoded frame and of one mask


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('cache'))
    return dict(root=root, z=syn.write(root, 8, 4, H, W))


# ------------------------------------------------------------------------------- the bookkeeping
def test_budget_order_and_counters():
    c = fc.HostFrameCache(3 * (FRAME + LABEL))
    owner = object()
    kept = []
    for i in range(5):
        got = c.reserve([(('f.zip', 'frame%d' % i), FRAME), (('l.zip', 'label%d' % i), LABEL)], owner)
        assert (got is not None) == (i < 3)            # first come, first kept; a frame is never kept without its label
        if got is not None:
            assert c.lookup(('f.zip', 'frame%d' % i)) is None and c.pending(('f.zip', 'frame%d' % i), owner) is got[0]
            assert c.pending(('f.zip', 'frame%d' % i), object()) is None
            for e, n in zip(got, (FRAME, LABEL)):
                c.write(e, np.full(n, i + 1, np.uint8))
                c.commit(e)
            kept.append(got)
        c.note(got is not None)
    assert c.counters() == {'hits': 3, 'misses': 2, 'entries': 6, 'bytes': 3 * (FRAME + LABEL)}
    assert sum(c.sizes) <= c.budget and c.bytes <= c.budget
    assert c.reserve([(('f.zip', 'small'), 16)], owner) is None                # full stays full
    assert c.reserve([(('f.zip', 'frame0'), FRAME)], owner) is None            # a key is kept once
    spans = sorted((e.chunk, e.offset, e.offset + e.nbytes) for got in kept for e in got)
    assert all(a[2] <= b[1] for a, b in zip(spans, spans[1:]) if a[0] == b[0])  # no two entries overlap
    for i, (ef, el) in enumerate(kept):
        assert c.lookup(ef.key) is ef and (c.view(ef, (H, W, 3), np.uint8) == i + 1).all()
        assert (c.view(el, (H, W), np.uint8) == i + 1).all() and not c.view(el, (H, W), np.uint8).flags.writeable
    c.close()
    c.close()
    assert c.chunks == [] and c.reserve([(('f.zip', 'late'), 16)], owner) is None
    assert c.counters()['entries'] == 6                                          # the counters outlive close()


def test_small_budget_chunks_and_returned_reservations():
    c = fc.HostFrameCache(FRAME - 1)
    assert c.reserve([(('f', 'a'), FRAME)], None) is None and c.chunks == [] and c.counters()['entries'] == 0
    c = fc.HostFrameCache(10 * FRAME, chunk_bytes=2 * FRAME + 100)              # several chunks, none above the budget
    got = [c.reserve([(('f', i), FRAME)], None) for i in range(10)]
    assert sum(g is not None for g in got) == 9 and len(c.chunks) == 5 and sum(c.sizes) <= c.budget
    e = got[3][0]
    c.release(e)                                                                 # not filled: the range is free again
    assert c.lookup(('f', 3)) is None and c.pending(('f', 3), None) is None
    again = c.reserve([(('f', 'other'), FRAME)], None)[0]
    assert (again.chunk, again.offset) == (e.chunk, e.offset)
    c.commit(again)
    c.release(again)                                                             # a committed entry stays
    assert c.lookup(('f', 'other')) is again
    odd = fc.HostFrameCache(1000)                                                # entries start on 16-byte boundaries
    a, b = odd.reserve([(('f', 'a'), 33), (('f', 'b'), 7)], None)
    assert (a.offset, b.offset) == (0, 48)
    odd.write(b, np.arange(7, dtype=np.uint8))
    assert odd.view(b, (7,), np.uint8).tolist() == list(range(7))


# ------------------------------------------------------------------------------- TrainLoader
def _epochs(ds, n, batchsize, iters, seed, cache=None, depth=None, ids=None):
    """-> (batches, tasks submitted before each batch was handed out, the loader's counters)"""
    np.random.seed(seed)
    it = st.ShuffledIterator(n, batchsize)
    loader = sl.TrainLoader(ds, np.arange(n) if ids is None else ids, it, 2, sl.HostStage(ds), depth=depth,
                            cache=cache)
    count = [0]
    submit = loader.slabs.submit

    def counted(fn, task):
        count[0] += 1
        return submit(fn, task)
    loader.slabs.submit = counted
    out, tasks = [], []
    try:
        for _ in range(iters):
            out.append(loader.next())
            tasks.append(count[0])
        return out, tasks, (loader.cache_hits, loader.cache_misses, loader.n_host_batches)
    finally:
        loader.close()


def _same_state(a, b):
    (ia, ra), (ib, rb) = a, b
    assert set(ia) == set(ib)
    for k in ia:
        assert np.array_equal(ia[k], ib[k]), k
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and ra[2:] == rb[2:]


def _compare(plain, got):
    assert len(plain) == len(got)
    for (pi, pl, ps), (gi, gl, gs) in zip(plain, got):
        assert gi.dtype == np.float32 and gi.shape == pi.shape and gl.dtype == pl.dtype and gl.shape == pl.shape
        assert np.array_equal(syn.bits(gi), syn.bits(pi))
        assert np.array_equal(gl, pl)
        _same_state(ps, gs)


@pytest.mark.parametrize('random', [False, True])
def test_three_epochs_equal_the_uncached_loader(data, random):
    """8 examples in batches of 2 for 12 iterations: three epochs.  Epoch 1 decodes every example once (16 tasks, also
    for the batches produced ahead of the staging), later epochs nothing."""
    z = data['z']
    ds = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (16, 24), random, False)
    before = syn.shm_names()
    plain, plain_tasks, _ = _epochs(ds, 8, 2, 12, seed=5)
    assert plain_tasks[-1] >= 12 * 4                   # the uncached loader decodes everything every time
    cache = fc.HostFrameCache(1 << 20)
    got, tasks, (hits, misses, n_host) = _epochs(ds, 8, 2, 12, seed=5, cache=cache)
    _compare(plain, got)
    assert tasks[3] == tasks[-1] == 16 and n_host == 0
    assert misses == 8 and hits >= 16 and hits + misses >= 24
    assert cache.counters()['entries'] == 16 and cache.counters()['bytes'] == 8 * (FRAME + LABEL)
    assert cache.counters()['hits'] == hits and cache.counters()['misses'] == misses
    # a second loader over the same zips finds everything: the keys are (zip path, member name)
    got2, tasks2, (hits2, misses2, _) = _epochs(ds, 8, 2, 4, seed=5, cache=cache)
    _compare(plain[:4], got2)
    assert tasks2[-1] == 0 and misses2 == 0 and hits2 >= 8
    cache.close()
    assert syn.shm_names() == before


def test_soft_labels_are_cached_as_float32(data, tmp_path):
    import io
    import zipfile
    z = data['z']
    soft = str(tmp_path / 'soft.zip')
    rng = np.random.default_rng(5)
    with zipfile.ZipFile(z[1]) as zl, zipfile.ZipFile(soft, 'w', zipfile.ZIP_STORED) as zo:
        for name in zl.namelist():
            m = np.load(io.BytesIO(zl.read(name)))
            zo.writestr(name, zl.read(name))
            zo.writestr(name[:-len('.npy')] + '_scores.npy', syn.npy(rng.random((2,) + m.shape).astype(np.float32)))
    ds = st.ZippedEstimatedCityscapesDataset(z[0], soft, (16, 24), True, True)
    plain, _, _ = _epochs(ds, 8, 2, 9, seed=2)
    cache = fc.HostFrameCache(1 << 20)
    got, tasks, _ = _epochs(ds, 8, 2, 9, seed=2, cache=cache)
    _compare(plain, got)
    assert tasks[-1] == 16 and cache.counters()['bytes'] == 8 * (FRAME + 2 * LABEL * 4)
    cache.close()


@pytest.mark.parametrize('budget,frames', [(3 * (FRAME + LABEL), 3), (FRAME - 1, 0), (FRAME + LABEL - 1, 0)])
def test_partial_budget_mixes_cached_and_new_members(data, budget, frames):
    z = data['z']
    ds = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (16, 24), True, False)
    plain, _, _ = _epochs(ds, 8, 2, 12, seed=7)
    cache = fc.HostFrameCache(budget)
    got, tasks, (hits, misses, n_host) = _epochs(ds, 8, 2, 12, seed=7, cache=cache)
    _compare(plain, got)
    c = cache.counters()
    frame_entries = [e for k, e in cache.table.items() if k[0] == z[0]]
    assert len(frame_entries) == frames and c['entries'] == 2 * frames and c['bytes'] == frames * (FRAME + LABEL)
    assert sum(cache.sizes) <= budget and n_host == 0
    # epoch 1 decodes all 8 examples, epochs 2 and 3 the 8 - frames that were not kept; up to 3 batches of epoch 4 have
    # been produced ahead.  Two tasks per example that is not served from the cache.
    assert tasks[-1] == 2 * misses
    assert 8 + 2 * (8 - frames) <= misses <= 8 + 2 * (8 - frames) + 6
    assert hits + misses >= 24 and (hits >= 2 * frames if frames else hits == 0)
    cache.close()


def test_an_example_twice_in_one_batch(data):
    """3 examples in batches of 2: the second batch holds the last example of epoch 1 and the first of epoch 2, and
    with this seed they are the same example, which no earlier batch has held"""
    z = data['z']
    ds = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (16, 24), False, False)    # no draws between the batches
    seed = None
    for s in range(200):
        np.random.seed(s)
        it = st.ShuffledIterator(3, 2)
        a, b = it.next_indices(), it.next_indices()
        if b[0] == b[1] and b[0] not in a:
            seed = s
            break
    assert seed is not None
    plain, _, _ = _epochs(ds, 3, 2, 6, seed=seed)
    for depth in (1, 3):
        cache = fc.HostFrameCache(1 << 20)
        got, tasks, (hits, misses, _) = _epochs(ds, 3, 2, 6, seed=seed, cache=cache, depth=depth)
        _compare(plain, got)
        assert misses == 3 and tasks[-1] == 6 and cache.counters()['entries'] == 6
        cache.close()


def test_a_member_of_another_shape_is_never_cached(data, tmp_path):
    z = data['z']
    rng = np.random.default_rng(9)
    odd_img, odd_mask = syn.image(40, 72, rng)
    imgs = syn.rewrite(z[0], str(tmp_path / 'imgs.zip'), {3: lambda d: syn.png(odd_img)})
    labs = syn.rewrite(z[1], str(tmp_path / 'labs.zip'), {3: lambda d: syn.npy(odd_mask)})
    ds = st.ZippedEstimatedCityscapesDataset(imgs, labs, (16, 24), True, False)
    plain, _, (_, _, plain_host) = _epochs(ds, 8, 2, 12, seed=4)
    cache = fc.HostFrameCache(1 << 20)
    got, tasks, (hits, misses, n_host) = _epochs(ds, 8, 2, 12, seed=4, cache=cache)
    _compare(plain, got)
    assert 0 < plain_host < 12 and plain_host <= n_host < 12
    assert (imgs, ds.img_fns[3]) not in cache.table and (labs, ds.label_fns[3]) not in cache.table
    assert all(e.committed for e in cache.table.values())      # nothing is left reserved
    kept = set(k[1] for k in cache.table if k[0] == imgs)
    assert len(kept) >= 6 and kept <= set(ds.img_fns) - {ds.img_fns[3]}
    for k, e in cache.table.items():                           # and what is kept is the decoded member
        if k[0] == imgs:
            i = ds.img_fns.index(k[1])
            assert np.array_equal(cache.view(e, (H, W, 3), np.uint8).transpose(2, 0, 1), ds.decoded(i)[0])
    cache.close()


# ------------------------------------------------------------------------------- LabelLoader
def _passes(ds, indices, cache, keep_ids=False, abandon=False, batch=2):
    loader = sl.LabelLoader(ds, indices, batch, 2, sl.HostLabelStage(), depth=2, keep_ids=keep_ids, cache=cache)
    count = [0]
    submit = loader.slabs.submit

    def counted(fn, task):
        count[0] += 1
        return submit(fn, task)
    loader.slabs.submit = counted
    try:
        if abandon:
            it = loader.batches()
            next(it)
            del it
        first = [(b.indices, b.host, np.array(b.frames), np.array(b.label_ids),
                  None if b.ids_host is None else np.array(b.ids_host)) for b in loader.batches()]
        n_first = count[0]
        again = [(b.indices, b.host, np.array(b.frames), np.array(b.label_ids),
                  None if b.ids_host is None else np.array(b.ids_host)) for b in loader.batches()]
        return first, again, n_first, count[0], loader
    finally:
        loader.close()


def _same_batches(a, b):
    assert len(a) == len(b)
    for (ia, ha, fa, la, ka), (ib, hb, fb, lb, kb) in zip(a, b):
        assert ia == ib and ha == hb and np.array_equal(fa, fb) and np.array_equal(la, lb)
        assert (ka is None) == (kb is None) and (ka is None or np.array_equal(ka, kb))


@pytest.mark.parametrize('keep_ids', [False, True])
@pytest.mark.parametrize('abandon', [False, True])
def test_label_loader_second_pass_comes_from_the_cache(data, keep_ids, abandon):
    z = data['z']
    ds = segnet.ZippedCityscapesRoadDataset(z[2], z[3], (16, 24))
    want, want_again, n, n2, _ = _passes(ds, range(4), None, keep_ids)
    assert n > 0 and n2 == 2 * n
    cache = fc.HostFrameCache(1 << 20)
    first, again, n_first, n_all, loader = _passes(ds, range(4), cache, keep_ids, abandon)
    _same_batches(want, first)
    _same_batches(want, again)
    assert n_all == n_first                                    # the second pass submits nothing
    assert n_first == n if not abandon else n <= n_first <= 2 * n
    for j, i in enumerate(first[1][0]):
        img, label = ds.get_raw(i)
        assert np.array_equal(again[1][2][j].transpose(2, 0, 1), img)
        assert np.array_equal(segnet.label_mask(again[1][3][j]), label)
        assert not keep_ids or np.array_equal(again[1][4][j], again[1][3][j])
    assert cache.counters()['entries'] == 2 and cache.counters()['bytes'] == 2 * loader.layout.prefix(2)
    if not abandon:
        assert (loader.cache_hits, loader.cache_misses, loader.first_pass_misses) == (2, 2, 2)
    cache.close()


def test_label_loader_small_budget_and_shared_budget(data):
    z = data['z']
    ds = segnet.ZippedCityscapesRoadDataset(z[2], z[3], (16, 24))
    train = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (16, 24), False, False)
    want, _, n, _, _ = _passes(ds, range(4), None)
    one = sl.Layout(2, [('frames', (H, W, 3), np.uint8), ('label_ids', (H, W), np.uint8)]).prefix(2)
    cache = fc.HostFrameCache(one)                             # one validation batch: the first is kept
    first, again, n_first, n_all, loader = _passes(ds, range(4), cache)
    _same_batches(want, first)
    _same_batches(want, again)
    assert n_first == n and n_all == n + n // 2 and cache.counters()['entries'] == 1
    assert (loader.cache_hits, loader.cache_misses, loader.first_pass_misses) == (1, 3, 2)
    cache.close()
    cache = fc.HostFrameCache(one + FRAME + LABEL)             # one validation batch and one training example
    first, again, n_first, n_all, _ = _passes(ds, range(2), cache)
    _same_batches(want[:1], first)
    _same_batches(want[:1], again)
    assert n_all == n_first == n // 2
    plain, _, _ = _epochs(train, 8, 2, 8, seed=1)
    got, tasks, (hits, misses, _) = _epochs(train, 8, 2, 8, seed=1, cache=cache)
    _compare(plain, got)
    assert cache.counters()['entries'] == 3 and sum(cache.sizes) <= cache.budget and hits >= 1
    assert cache.counters()['bytes'] == one + FRAME + LABEL and tasks[-1] == 2 * misses
    cache.close()


# ------------------------------------------------------------------------------- flags
def test_flag_needs_the_loader_and_is_recorded_only_when_given():
    reference = vars(train_segnet.get_parser().parse_args([]))
    pre, args = train_segnet.run_args([])
    assert pre.device_cache_gb == 0 and 'device_cache_gb' not in vars(args)
    assert vars(args) == dict(reference, dtype='fp32')
    pre, args = train_segnet.run_args(['--loader_procs', '2'])
    assert 'device_cache_gb' not in vars(args)
    pre, args = train_segnet.run_args(['--loader_procs', '2', '--device_cache_gb', '1.5'])
    assert pre.device_cache_gb == 1.5
    assert vars(args) == dict(reference, dtype='fp32', loader_procs=2, device_cache_gb=1.5)
    assert json.loads(json.dumps(vars(args), sort_keys=True))['device_cache_gb'] == 1.5
    with pytest.raises(ValueError, match='--loader_procs'):
        train_segnet.run_args(['--device_cache_gb', '1'])
    with pytest.raises(ValueError):
        train_segnet.run_args(['--loader_procs', '2', '--device_cache_gb', '-1'])
    with pytest.raises(SystemExit):                            # the reference parser does not take it
        train_segnet.get_args(['--device_cache_gb', '1'])


def test_main_refuses_before_anything_is_written(tmp_path, data):
    z = data['z']
    d = str(tmp_path / 'result')
    with pytest.raises(ValueError, match='--loader_procs'):
        train_segnet.main(syn.train_args(z, 2, 2, 2) + ['--device_cache_gb', '1', '--result_dir', d])
    assert not os.path.exists(d)


def test_rounds_driver_forwards_the_flag_to_training_only():
    def argvs(argv):
        a = rtr.get_args(argv)
        steps = [s for s in rtr.plan(a, 'R/train_round1_x_0') if s['kind'] == 'train']
        dirs = {i + 1: 'D%d' % (i + 1) for i in range(len(steps))}
        return a, [rtr.train_argv(a, s, 'D%d' % (i + 1), dirs) for i, s in enumerate(steps)]
    base = ['--n_round', '3', '--iteration', '100', '--val_iteration', '50', '--n_use_data', '40', '--random',
            '--loader_procs', '4']
    _, plain = argvs(base)
    a, cached = argvs(base + ['--device_cache_gb', '12'])
    for p, c in zip(plain, cached):
        assert '--device_cache_gb' not in p and c == p + ['--device_cache_gb', '12.0']
    pre, rest = train_segnet.get_pre_args(cached[1])
    assert pre.device_cache_gb == 12.0 and pre.loader_procs == 4 and '--device_cache_gb' not in rest
    train_segnet.get_args(rest)
    for spec in rtr.label_specs(a, 'P', 100, 'out'):
        assert 'device_cache_gb' not in spec


def test_entry_points_declared_as_bound():
    import ctypes
    lib = importlib.import_module('superpixel-align_amd._lib')
    header = open(os.path.join(ROOT, 'include', 'spalign.h')).read()
    ctype = {'int32_t': ctypes.c_int32}
    for name in ('spa_segnet_train_input_ptrs', 'spa_segnet_train_label_ptrs'):
        params = [p.strip() for p in syn.declaration(header, name).split(',')]
        want = [ctypes.c_void_p if '*' in p else ctype[p.split()[0]] for p in params]
        assert lib.PROTOTYPES[name] == (ctypes.c_int, want), name
        twin = name[:-len('_ptrs')]
        assert lib.PROTOTYPES[name][1] == lib.PROTOTYPES[twin][1]         # a table of addresses where the batch was
        assert [p.split()[-1].lstrip('*') for p in params][2:] == \
            [p.split()[-1].lstrip('*') for p in syn.declaration(header, twin).split(',')][2:]
    engine = importlib.import_module('superpixel-align_amd.engine')
    assert hasattr(engine.Engine, 'segnet_train_input_ptrs') and hasattr(engine.Engine, 'segnet_train_label_ptrs')
