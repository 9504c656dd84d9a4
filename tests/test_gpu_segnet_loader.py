"""GPU tests of the training input stage (train_segnet.py --loader_procs): Engine.segnet_train_input and
segnet_train_label against the dataset's own host functions, bit for bit, for both resize backends; train_segnet.py
with the loader against the same run without it (losses, every snapshot entry, --resume in both directions); two gloo
ranks on one GPU with and without it; and what a loader run leaves behind, also one that fails in a step.  Every
child runs under a time limit; a failing child ends the test."""
import importlib
import json
import os
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
cli = importlib.import_module('superpixel-align_amd.cli')

TIMEOUT = 900
SCRIPT = os.path.join(ROOT, 'train_segnet.py')
DS = st.ZippedEstimatedCityscapesDataset

# (source, target): the training size, a non-integer downscale, an upscale, equal sizes, one axis only
SHAPES = [((1024, 2048), (512, 1024)), ((97, 131), (40, 56)), ((40, 56), (97, 131)), ((64, 96), (64, 96)),
          ((64, 96), (64, 48))]


@pytest.fixture(scope='module')
def eng():
    return importlib.import_module('superpixel-align_amd.engine').default_engine()


def _draws(B, rng, augment):
    if not augment:
        return None, None
    shifts = np.stack([st.pca_lighting_shift(rng.normal(0, 25.5, 3)) for _ in range(B)])
    flips = np.array([1, 0, 1, 1][:B], np.uint8)
    return shifts, flips


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize('augment', [False, True])
@pytest.mark.parametrize('src,dst', SHAPES)
@pytest.mark.parametrize('backend', ['pil', 'cv2'])
def test_train_input_equals_the_dataset_functions(eng, monkeypatch, backend, src, dst, augment):
    monkeypatch.setattr(cli, 'RESIZE_BACKEND', [backend])
    rng = np.random.default_rng(src[0] + dst[1])
    B = 2 if src[0] >= 1024 else 3
    u8 = rng.integers(0, 256, (B,) + src + (3,), dtype=np.uint8)
    u8[0, :5] = 255                                               # saturated rows: overshoot above 255 stays float
    u8[0, 5:9] = 0
    shifts, flips = _draws(B, rng, augment)
    got = eng.segnet_train_input(_dev(u8), dst, _dev(shifts), _dev(flips)).cpu().numpy()
    assert got.shape == (B, 3) + dst and got.dtype == np.float32
    for j in range(B):
        img = u8[j].astype(np.float32).transpose(2, 0, 1)
        if img.shape[1:] != dst:
            img = st.resize_bicubic_float(img, dst)
        if augment:
            img, _ = DS.augmented(img, np.zeros(dst, np.int32), shifts[j], bool(flips[j]))
        n = int((syn.bits(got[j]) != syn.bits(img)).sum())
        print('%s %s -> %s augment %d image %d: %d differing values' % (backend, src, dst, augment, j, n))
        assert n == 0


@pytest.mark.parametrize('augment', [False, True])
@pytest.mark.parametrize('src,dst', SHAPES)
@pytest.mark.parametrize('backend', ['pil', 'cv2'])
def test_train_label_equals_the_dataset_functions(eng, monkeypatch, backend, src, dst, augment):
    monkeypatch.setattr(cli, 'RESIZE_BACKEND', [backend])
    rng = np.random.default_rng(src[1] + dst[0])
    B = 3
    masks = (rng.random((B,) + src) > 0.6).astype(np.uint8)
    masks[1, ::7] = 200                                           # any byte value, not only 0 / 1
    scores = rng.random((B, 2) + src).astype(np.float32)
    _, flips = _draws(B, rng, augment)
    got_m = eng.segnet_train_label(_dev(masks), dst, _dev(flips)).cpu().numpy()
    got_s = eng.segnet_train_label(_dev(scores), dst, _dev(flips)).cpu().numpy()
    assert got_m.dtype == np.int32 and got_m.shape == (B,) + dst
    assert got_s.dtype == np.float32 and got_s.shape == (B, 2) + dst
    for j in range(B):
        m = masks[j].astype(np.int32)
        s = scores[j]
        if src != dst:
            m = st.resize_nearest_label(m[None], dst)[0]
            s = st.resize_nearest_label(s, dst)
        if augment and flips[j]:
            m, s = m[..., ::-1], s[..., ::-1]
        assert np.array_equal(got_m[j], m)
        assert np.array_equal(syn.bits(got_s[j]), syn.bits(s))


# ------------------------------------------------------------------------------- train_segnet.py
def _run(cmd, env, ok=True):
    return syn.run(cmd, env, ROOT, TIMEOUT, ok)


def _common(z, iters, every, extra=()):
    return syn.train_args(z, iters, every, every, (32, 64), (48, 96),
                          ['--random', '--optimizer', 'MomentumSGD'] + list(extra))


def _same_snapshot(fa, fb):
    ks = syn.same_snapshot(fa, fb, bitwise=True)
    assert 'extensions/np_random/keys' in ks and 'updater/iterator:main/order' in ks
    assert any(k.startswith('updater/optimizer:main/predictor/') for k in ks)
    return len(ks)


def test_loader_run_equals_plain_run_and_resumes_both_ways(tmp_path):
    """float32, --random, MomentumSGD, 12 iterations over 5 examples in batches of 2 (the epochs' boundaries fall
    inside batches), snapshots at 6 and 12"""
    z = syn.write(str(tmp_path / 'data'), 5, 2, 48, 96)
    d = {k: str(tmp_path / k) for k in ('plain', 'loader', 'from_loader', 'from_plain')}
    _run([sys.executable, SCRIPT] + _common(z, 12, 6) + ['--result_dir', d['plain']], syn.env())
    r = _run([sys.executable, SCRIPT, '--loader_procs', '2'] + _common(z, 12, 6) + ['--result_dir', d['loader']],
             syn.env())
    assert 'prepared on the host' not in r.stdout
    assert json.load(open(os.path.join(d['loader'], 'args.txt')))['loader_procs'] == 2
    assert 'loader_procs' not in json.load(open(os.path.join(d['plain'], 'args.txt')))
    assert syn.losses(d['plain']) == syn.losses(d['loader']) and len(syn.losses(d['plain'])) == 2
    for it in (6, 12):
        n = _same_snapshot(os.path.join(d['plain'], 'snapshot_iter_%d' % it),
                           os.path.join(d['loader'], 'snapshot_iter_%d' % it))
        assert n > 60
    # resume: the loader run's snapshot without the flag, the plain run's snapshot with it
    _run([sys.executable, SCRIPT] + _common(z, 12, 6) +
         ['--result_dir', d['from_loader'], '--resume', os.path.join(d['loader'], 'snapshot_iter_6')], syn.env())
    _run([sys.executable, SCRIPT, '--loader_procs', '2'] + _common(z, 12, 6) +
         ['--result_dir', d['from_plain'], '--resume', os.path.join(d['plain'], 'snapshot_iter_6')], syn.env())
    for k in ('from_loader', 'from_plain'):
        _same_snapshot(os.path.join(d['plain'], 'snapshot_iter_12'), os.path.join(d[k], 'snapshot_iter_12'))
        assert syn.losses(d[k])[-1][:3] == syn.losses(d['plain'])[-1][:3]


def test_two_gloo_ranks_with_the_loader_equal_the_launch_without(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 9, 2, 48, 96)
    env = syn.env(SPA_DIST_BACKEND='gloo', SPA_BENCH_SAME_DEVICE='1')

    def torchrun(argv):
        return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                '--master-addr', '127.0.0.1', '--master-port', str(syn.free_port()), SCRIPT] + argv
    da, db = str(tmp_path / 'plain'), str(tmp_path / 'loader')
    _run(torchrun(['--data_parallel'] + _common(z, 8, 4) + ['--result_dir', da]), env)
    _run(torchrun(['--data_parallel', '--loader_procs', '2'] + _common(z, 8, 4) + ['--result_dir', db]), env)
    assert syn.losses(da) == syn.losses(db)
    for it in (4, 8):
        _same_snapshot(os.path.join(da, 'snapshot_iter_%d' % it), os.path.join(db, 'snapshot_iter_%d' % it))
    assert st.snapshot_world_size(os.path.join(db, 'snapshot_iter_8')) == 2
    args = json.load(open(os.path.join(db, 'args.txt')))
    assert args['loader_procs'] == 2 and args['world_size'] == 2


# ------------------------------------------------------------------------------- what a run leaves behind
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


def test_nothing_is_left_after_a_run_or_a_failing_step(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 5, 2, 48, 96)
    # scores with three channels: the soft-label loss of the first step refuses them against the two-channel output
    bad = str(tmp_path / 'bad_scores.zip')
    rng = np.random.default_rng(1)
    with zipfile.ZipFile(z[1]) as zl, zipfile.ZipFile(bad, 'w', zipfile.ZIP_STORED) as zo:
        for name in zl.namelist():
            zo.writestr(name[:-len('.npy')] + '_scores.npy', syn.npy(rng.random((3, 48, 96)).astype(np.float32)))
    before = set(os.listdir('/dev/shm'))
    mark = 'SPA_TEST_MARK_%s' % uuid.uuid4().hex
    r = _run([sys.executable, SCRIPT, '--loader_procs', '2'] + _common(z, 4, 2) +
             ['--result_dir', str(tmp_path / 'good')], syn.env(**{mark: '1'}))
    assert os.path.exists(str(tmp_path / 'good' / 'snapshot_iter_4'))
    assert _marked_processes(mark) == [] and set(os.listdir('/dev/shm')) == before
    assert 'leaked' not in r.stderr
    zb = [z[0], bad, z[2], z[3]]
    r = _run([sys.executable, SCRIPT, '--loader_procs', '2'] + _common(zb, 4, 2, ['--use_soft_label']) +
             ['--result_dir', str(tmp_path / 'bad')], syn.env(**{mark: '1'}), ok=False)
    assert r.returncode != 0 and 'Traceback' in r.stderr
    assert not os.path.exists(str(tmp_path / 'bad' / 'snapshot_iter_2'))
    assert _marked_processes(mark) == [] and set(os.listdir('/dev/shm')) == before
