"""CPU tests of the labelling and validation input stage (labels_from_segnet.py --loader_procs,
superpixel-align_amd/segnet_loader.py LabelLoader): the loader with the host stage and real spawned workers against
get_raw, the members that send a batch down the host path, the worker task, the slab helper shared with TrainLoader,
cleanup, the flags of the three drivers, and the small /dev/shm fall-back of save_labels."""
import importlib
import json
import os
import subprocess
import sys
import types
import zipfile
from multiprocessing import shared_memory

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
slabs = importlib.import_module('superpixel-align_amd.slabs')
dw = importlib.import_module('superpixel-align_amd.decode_worker')
cli = importlib.import_module('superpixel-align_amd.cli')
lfs = importlib.import_module('labels_from_segnet')
train_segnet = importlib.import_module('train_segnet')
rtr = importlib.import_module('utils.run_train_rounds')

H, W = 32, 64


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('label_loader'))
    z = syn.write(root, 4, 6, H, W)
    return dict(root=root, z=z, ds=segnet.ZippedCityscapesRoadDataset(z[2], z[3], (H // 2, W // 2)))


def _run(ds, indices, batch=2, depth=2, **kw):
    loader = sl.LabelLoader(ds, indices, batch, 2, sl.HostLabelStage(), depth=depth, **kw)
    try:
        first = list(loader.batches())
        again = list(loader.batches())                      # a second pass over the same indices
        return first, again, loader.n_host_batches, loader.worker_pids
    finally:
        loader.close()


# ------------------------------------------------------------------------------- the loader
def test_loader_yields_get_raw_in_order(data):
    ds = data['ds']
    before = syn.shm_names()
    first, again, n_host, pids = _run(ds, range(1, 5), keep_ids=True)
    assert [b.indices for b in first] == [[1, 2], [3, 4]] == [b.indices for b in again]
    assert n_host == 0 and 1 <= len(pids) <= 2
    for batches in (first, again):
        for b in batches:
            assert not b.host and b.frames.dtype == np.uint8 and b.frames.shape == (2, H, W, 3)
            assert b.label_ids.dtype == np.uint8 and b.label_ids.shape == (2, H, W)
            for j, i in enumerate(b.indices):
                img, label = ds.get_raw(i)
                assert np.array_equal(b.frames[j].transpose(2, 0, 1), img)
                assert np.array_equal(segnet.label_mask(b.label_ids[j]), label)
                assert np.array_equal(b.ids_host[j], b.label_ids[j])
    assert (first[0].label_ids[:, :4] == 0).all()           # the synthetic labels' ignored rows are ids, not classes
    assert syn.shm_names() == before and not any(syn.alive(p) for p in pids)


def test_short_last_batch_and_depth_rule(data):
    first, _, n_host, _ = _run(data['ds'], range(0, 5), depth=None)
    assert [b.indices for b in first] == [[0, 1], [2, 3], [4]] and n_host == 0
    assert first[2].frames.shape == (1, H, W, 3) and first[2].ids_host is None
    loader = sl.LabelLoader(data['ds'], [], 2, 2, sl.HostLabelStage())
    try:
        assert loader.depth == sl.default_depth(2, 2) and list(loader.batches()) == []
    finally:
        loader.close()


@pytest.mark.parametrize('what', ['palette_frame', 'rgba_frame', 'other_size_frame', 'rgb_label'])
def test_other_modes_and_shapes_mark_their_batch_only(data, tmp_path, what):
    z = data['z']
    imgs, labs = z[2], z[3]
    k = 3                                                   # index 3: the second batch of range(1, 5)
    if what == 'palette_frame':
        imgs = syn.rewrite(z[2], str(tmp_path / 'i.zip'), {k: lambda d: syn.png(syn.decoded(d), 'P')})
    elif what == 'rgba_frame':
        imgs = syn.rewrite(z[2], str(tmp_path / 'i.zip'),
                           {k: lambda d: syn.png(np.dstack([syn.decoded(d), np.full((H, W), 200, np.uint8)]))})
    elif what == 'other_size_frame':
        imgs = syn.rewrite(z[2], str(tmp_path / 'i.zip'),
                           {k: lambda d: syn.png(np.zeros((H + 8, W + 16, 3), np.uint8))})
    else:
        labs = syn.rewrite(z[3], str(tmp_path / 'l.zip'), {k: lambda d: syn.png(np.dstack([syn.decoded(d)] * 3))})
    ds = segnet.ZippedCityscapesRoadDataset(imgs, labs, (H // 2, W // 2))
    first, again, n_host, _ = _run(ds, range(1, 5))
    assert [b.host for b in first] == [False, True] == [b.host for b in again] and n_host == 2
    assert first[1].frames is None and first[1].label_ids is None and first[1].indices == [3, 4]
    for j, i in enumerate(first[0].indices):
        img, label = ds.get_raw(i)
        assert np.array_equal(first[0].frames[j].transpose(2, 0, 1), img)
        assert np.array_equal(segnet.label_mask(first[0].label_ids[j]), label)


def test_close_twice_and_after_a_failed_constructor(data, monkeypatch):
    before = syn.shm_names()
    loader = sl.LabelLoader(data['ds'], range(6), 2, 2, sl.HostLabelStage())
    pids = loader.worker_pids
    it = loader.batches()
    next(it)                                                # batches in flight when it is closed
    loader.close()
    loader.close()
    assert syn.shm_names() == before and not any(syn.alive(p) for p in pids)

    class Failing(sl.HostLabelStage):
        n = 0

        def register(self, shm):
            Failing.n += 1
            if Failing.n == 2:
                raise RuntimeError('no second slab')
            return sl.HostLabelStage.register(self, shm)
    with pytest.raises(RuntimeError, match='no second slab'):
        sl.LabelLoader(data['ds'], range(6), 2, 2, Failing())
    assert syn.shm_names() == before
    monkeypatch.setattr(slabs, '_shm_free', lambda: 1 << 20)
    with pytest.raises(cli.ShmTooSmall, match='label loader'):
        sl.LabelLoader(data['ds'], range(6), 2, 2, sl.HostLabelStage())
    assert syn.shm_names() == before


# ------------------------------------------------------------------------------- the worker task
def test_png_task_checks_shape_and_mode(data):
    z = data['z']
    with zipfile.ZipFile(z[2]) as zi, zipfile.ZipFile(z[3]) as zl:
        frame, label = zi.namelist()[0], zl.namelist()[0]
        want_f, want_l = syn.decoded(zi.read(frame)), syn.decoded(zl.read(label))
    shm = shared_memory.SharedMemory(create=True, size=H * W * 4 + 64)
    try:
        buf = np.frombuffer(shm.buf, dtype=np.uint8)
        buf[:] = 0xAB
        assert dw.png_into((shm.name, 64, (H, W, 3), 'RGB', (z[2], frame))) == ((H, W, 3), 'RGB')
        assert np.array_equal(buf[64:64 + H * W * 3].reshape(H, W, 3), want_f) and (buf[:64] == 0xAB).all()
        assert (buf[64 + H * W * 3:] == 0xAB).all()
        buf[:] = 0xAB
        assert dw.png_into((shm.name, 0, (H, W), 'L', (z[3], label))) == ((H, W), 'L')
        assert np.array_equal(buf[:H * W].reshape(H, W), want_l) and (buf[H * W:] == 0xAB).all()
        buf[:] = 0xAB
        # a mismatch of the mode, and of the shape: reported, nothing written
        assert dw.png_into((shm.name, 0, (H, W), 'L', (z[2], frame))) == ((H, W, 3), 'RGB')
        assert dw.png_into((shm.name, 0, (H, W, 3), 'RGB', (z[3], label))) == ((H, W), 'L')
        assert dw.png_into((shm.name, 0, (H + 1, W, 3), 'RGB', (z[2], frame))) == ((H, W, 3), 'RGB')
        assert (buf == 0xAB).all()
        # the existing task keeps its return value
        assert dw.decode_into((shm.name, 0, (H, W, 3), (z[2], frame))) == (H, W, 3)
        del buf
    finally:
        dw._SHM.pop(shm.name).close() if shm.name in dw._SHM else None
        shm.close()
        shm.unlink()


def test_worker_module_imports_nothing_heavy():
    r = subprocess.run([sys.executable, '-c', "import importlib, sys; sys.path.insert(0, %r); "
                        "m = importlib.import_module('superpixel-align_amd.decode_worker'); assert m.png_into; "
                        "print(int('torch' in sys.modules))" % ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == '0', r.stderr[-2000:]


# ------------------------------------------------------------------------------- the shared helper
def test_two_loaders_share_one_pool(data):
    z = data['z']
    before = syn.shm_names()
    train = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (H // 2, W // 2), False, False)
    np.random.seed(0)
    tl = sl.TrainLoader(train, np.arange(4), st.ShuffledIterator(4, 2), 2, sl.HostStage(train))
    ll = None
    try:
        ll = sl.LabelLoader(data['ds'], range(6), 2, 2, sl.HostLabelStage(), pool=tl.workers)
        assert ll.worker_pids == tl.worker_pids and 1 <= len(tl.worker_pids) <= 2 and ll.workers is tl.workers
        assert len(list(ll.batches())) == 3
        img, lab, _ = tl.next()
        assert img.shape == (2, 3, H // 2, W // 2)
        ll.close()                                          # the other loader goes on, on the same workers
        assert all(syn.alive(p) for p in tl.worker_pids)
        tl.next()
        ll = sl.LabelLoader(data['ds'], range(6), 2, 2, sl.HostLabelStage(), pool=tl.workers)
        tl.close()                                          # and the other way round
        assert [b.indices for b in ll.batches()] == [[0, 1], [2, 3], [4, 5]]
        assert all(syn.alive(p) for p in ll.worker_pids)
    finally:
        if ll is not None:
            ll.close()
        tl.close()
    assert syn.shm_names() == before and not any(syn.alive(p) for p in tl.worker_pids)


# ------------------------------------------------------------------------------- flags
def test_labels_from_segnet_flag():
    p = lfs.get_parser()
    assert p.parse_args([]).loader_procs == 0 and p.parse_args(['--loader_procs', '3']).loader_procs == 3
    with pytest.raises(SystemExit):
        p.parse_args(['--loader_procs', '-1'])


def test_rounds_driver_label_flag(monkeypatch, tmp_path):
    base = ['--n_round', '3', '--iteration', '100', '--val_iteration', '50', '--n_use_data', '40', '--random',
            '--n_gpus', '2', '--n_labels', '10']
    a0 = rtr.get_args(base)
    a1 = rtr.get_args(base + ['--label_loader_procs', '4'])
    a2 = rtr.get_args(base + ['--loader_procs', '3'])
    assert (a0.label_loader_procs, a0.loader_procs) == (0, 0)
    assert (a1.label_loader_procs, a1.loader_procs) == (4, 0)
    assert (a2.label_loader_procs, a2.loader_procs) == (0, 3)
    assert 'CPUs for the decode workers' in ' '.join(rtr.get_parser().format_help().split())
    specs = rtr.label_specs(a1, 'P', 100, str(tmp_path / 'out'))
    assert len(specs) == 2 and all(s['loader_procs'] == 4 for s in specs)
    assert all(s['loader_procs'] == 0 for s in rtr.label_specs(a2, 'P', 100, str(tmp_path / 'out')))

    def argvs(a):
        steps = [s for s in rtr.plan(a, 'R/train_round1_x_0') if s['kind'] == 'train']
        dirs = {i + 1: 'D%d' % (i + 1) for i in range(len(steps))}
        return [rtr.train_argv(a, s, 'D%d' % (i + 1), dirs) for i, s in enumerate(steps)]
    assert argvs(a0) == argvs(a1)                          # the training argv does not change
    # label_worker hands the spec's value to save_labels; a spec without the key gives 0
    seen = []
    fake = types.ModuleType('labels_from_segnet')
    fake.save_labels = lambda *a, **kw: seen.append(kw['loader_procs'])
    monkeypatch.setitem(sys.modules, 'labels_from_segnet', fake)
    spec = dict(specs[0], spool=str(tmp_path / 'spool'))
    rtr.label_worker(spec)
    del spec['loader_procs']
    rtr.label_worker(spec)
    assert seen == [4, 0]


def test_entry_point_declared_and_bound():
    lib = importlib.import_module('superpixel-align_amd._lib')
    header = open(os.path.join(ROOT, 'include', 'spalign.h')).read()
    assert 'spa_segnet_label_eval' in lib.PROTOTYPES and 'int spa_segnet_label_eval(' in header
    engine = importlib.import_module('superpixel-align_amd.engine')
    assert hasattr(engine.Engine, 'segnet_label_eval')
    sh = open(os.path.join(ROOT, 'utils', 'create_from_segnet.sh')).read()
    assert 'LOADER_PROCS=${9:-0}' in sh and '--loader_procs $LOADER_PROCS' in sh


# ------------------------------------------------------------------------------- too small a /dev/shm
class _StubEngine(object):
    """what the plain loop calls, on the CPU: an all-zero mask, and a count of the per-image confusion launches"""
    device = 'cpu'

    def __init__(self):
        self.confusions = 0
        self.label_evals = 0

    def resize_cvcubic_u8(self, u8, shape):
        return u8

    def segnet_score(self, prob, shape, want_scores=False):
        import torch
        return torch.zeros((prob.shape[0],) + tuple(shape), dtype=torch.uint8), None

    def segnet_label_eval(self, *a, **kw):
        self.label_evals += 1
        raise AssertionError('the loader path was taken')

    def confusion(self, road, gt):
        import torch
        self.confusions += 1
        return torch.tensor([[int(((gt == 0) & (road == 0)).sum()), 0, int((gt == 1).sum()), 0]])


def test_small_shm_takes_the_plain_loop(data, tmp_path, monkeypatch, capsys):
    torch = pytest.importorskip('torch')
    eng = _StubEngine()
    model = types.SimpleNamespace(engine=eng, forward=lambda x: x)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    monkeypatch.setattr(segnet.SegNetBasic, 'from_snapshot', classmethod(lambda cls, *a, **kw: model))
    monkeypatch.setattr(sl, 'DeviceLabelStage', lambda engine: sl.HostLabelStage())
    monkeypatch.setattr(slabs, '_shm_free', lambda: 1 << 20)
    param_dir = tmp_path / 'run'
    param_dir.mkdir()
    with open(str(param_dir / 'args.txt'), 'w') as f:
        json.dump({'model': 'basic', 'input_shape': [H // 2, W // 2], 'batchsize': 2}, f)
    z = data['z']
    before = syn.shm_names()
    stats = {}
    out = str(tmp_path / 'out')
    lfs.save_labels(str(param_dir), 1, 0, z[2], z[3], out, 0, 5, False, [H, W], save_each=True, figure=False,
                    batchsize=2, loader_procs=2, loader_stats=stats)
    printed = capsys.readouterr().out
    assert printed.count('\n') == 1 and printed.startswith('--loader_procs: /dev/shm has 1 MB free')
    assert printed.rstrip().endswith('; the images are decoded on the host')
    assert eng.confusions == 5 and eng.label_evals == 0 and list(stats) == ['loop_s']
    assert len(open(os.path.join(out, 'result.json')).readlines()) == 5
    assert len([f for f in os.listdir(out) if f.endswith('.npy')]) == 10 and syn.shm_names() == before


# ------------------------------------------------------------------------------- the loader run's order, no GPU
class _MapEngine(_StubEngine):
    """a stand-in network on the CPU: the 'probabilities' are the red channel of a crop of the frame, so every image
    has its own mask, scores and counts, and both loops compute them with the same function"""

    def resize_cvcubic_u8(self, u8, shape):
        import torch
        return torch.as_tensor(np.asarray(u8))[:, :H // 2, :W // 2, :].contiguous()

    def _maps(self, x):
        import torch
        base = x[..., 0].float().repeat_interleave(2, 1).repeat_interleave(2, 2)
        sc = torch.stack([base / 255.0, 1 - base / 255.0], 1).contiguous()
        return (sc[:, 1] > sc[:, 0]).to(torch.uint8), sc

    def segnet_score(self, prob, shape, want_scores=False):
        m, sc = self._maps(prob)
        return m, (sc if want_scores else None)

    def confusion(self, road, gt):
        import torch
        self.confusions += 1
        out = torch.zeros((road.shape[0], 4), dtype=torch.int64)
        for b in range(road.shape[0]):
            k = gt[b] >= 0
            out[b] = torch.bincount((2 * gt[b][k].long() + road[b][k].long()).flatten(), minlength=4)
        return out

    def segnet_label_eval(self, prob, shape, label_ids=None, want_scores=False):
        import torch
        self.label_evals += 1
        m, sc = self._maps(prob)
        gt = torch.from_numpy(segnet.label_mask(np.asarray(label_ids)))
        n = self.confusions
        counts = self.confusion(m, gt)
        self.confusions = n
        return m, (sc if want_scores else None), counts


def test_loader_run_keeps_the_plain_loops_outputs_and_order(data, tmp_path, monkeypatch):
    """save_labels' two loops around a stand-in network (host stage, real workers; events and pinning are no-ops):
    the ring, the deferred output of batch k-1, the fall-back batches and the refused label, without a GPU"""
    torch = pytest.importorskip('torch')
    eng = _MapEngine()
    model = types.SimpleNamespace(engine=eng, forward=lambda x: x)
    monkeypatch.setattr(torch.cuda, 'set_device', lambda d: None)
    monkeypatch.setattr(torch.cuda, 'Event', lambda: types.SimpleNamespace(record=lambda: None, synchronize=lambda: None))
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    copy_ = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, 'copy_',
                        lambda self, src, non_blocking=False: copy_(self, torch.as_tensor(np.asarray(src))))
    monkeypatch.setattr(segnet.SegNetBasic, 'from_snapshot', classmethod(lambda cls, *a, **kw: model))
    monkeypatch.setattr(sl, 'DeviceLabelStage', lambda engine: sl.HostLabelStage())
    param_dir = tmp_path / 'run'
    param_dir.mkdir()
    with open(str(param_dir / 'args.txt'), 'w') as f:
        json.dump({'model': 'basic', 'input_shape': [H // 2, W // 2], 'batchsize': 2}, f)
    z = data['z']
    rng = np.random.default_rng(2)
    fb = syn.rewrite(z[2], str(tmp_path / 'fb.zip'),
                     {2: lambda b: syn.png(rng.integers(0, 256, (H + 16, W + 16, 3), dtype=np.uint8)),
                      4: lambda b: syn.png(syn.decoded(b)[:, :, 1].copy())})
    bad = syn.rewrite(z[3], str(tmp_path / 'bad.zip'), {3: lambda b: syn.png(syn.decoded(b)[:H - 8].copy())})

    def save(out, procs, imgs=z[2], labs=z[3], **kw):
        return lfs.save_labels(str(param_dir), 7, 0, imgs, labs, out, 0, 5, False, [H, W], figure=False, batchsize=2,
                               loader_procs=procs, **kw)

    def files(out):
        return {f: open(os.path.join(out, f), 'rb').read() for f in sorted(os.listdir(out)) if f.endswith('.npy')}

    def lines(out):
        got = [json.loads(l) for l in open(os.path.join(out, 'result.json'))]
        assert all(l.pop('out_dir') == out for l in got)
        return got
    before = syn.shm_names()
    for name, imgs, n_host in (('same', z[2], 0), ('fallback', fb, 2)):
        a, b = str(tmp_path / (name + '_plain')), str(tmp_path / (name + '_loader'))
        stats = {}
        save(a, 0, imgs, save_each=True)
        assert eng.label_evals == 0
        save(b, 2, imgs, save_each=True, loader_stats=stats)
        assert files(a) == files(b) and len(files(a)) == 10 and lines(a) == lines(b) and len(lines(a)) == 5
        assert any(l['TP'] + l['FP'] + l['FN'] for l in lines(a)) and len({v for v in files(a).values()}) >= 3
        assert stats['n_host_batches'] == n_host and eng.label_evals == 3 - n_host
        eng.label_evals = 0
        ra, rb = save(a, 0, imgs), save(b, 2, imgs)
        sa, sb = [], []
        assert save(a, 0, imgs, on_labels=lambda k, v: sa.append((k, v))) == {}
        assert save(b, 2, imgs, on_labels=lambda k, v: sb.append((k, v))) == {}
        eng.label_evals = 0
        for x, y in ((list(ra.items()), list(rb.items())), (sa, sb), (sb, list(rb.items()))):
            assert [os.path.basename(k) for k, _ in x] == [os.path.basename(k) for k, _ in y] and len(x) == 10
            assert all(u.dtype == v.dtype and v.flags.owndata and np.array_equal(u, v) for (_, u), (_, v) in zip(x, y))
    errs = []
    for out, procs in ((str(tmp_path / 'bad_plain'), 0), (str(tmp_path / 'bad_loader'), 2)):
        with pytest.raises(ValueError, match='has shape') as e:
            save(out, procs, labs=bad, save_each=True)
        errs.append(str(e.value))
    assert errs[0] == errs[1]
    assert files(str(tmp_path / 'bad_plain')) == files(str(tmp_path / 'bad_loader'))
    assert len(files(str(tmp_path / 'bad_plain'))) == 6
    assert lines(str(tmp_path / 'bad_plain')) == lines(str(tmp_path / 'bad_loader'))
    assert syn.shm_names() == before
