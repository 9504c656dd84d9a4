"""CPU tests of the training input stage (train_segnet.py --loader_procs, superpixel-align_amd/segnet_loader.py): the
float64 coefficient tables and the two-pass arithmetic the kernels run against Pillow's mode 'F' BICUBIC, the nearest
index tables against Pillow's NEAREST, the label task of decode_worker.py, the loader's draw order and yielded states
against the plain get_example loop (host stage, real spawned workers), the host path of an off-size frame, the small
/dev/shm refusal, cleanup, the workers' parent-death signal, and the flags."""
import importlib
import io
import json
import os
import signal
import subprocess
import sys
import time
import zipfile
from multiprocessing import shared_memory

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

st = importlib.import_module('superpixel-align_amd.segnet_train')
sl = importlib.import_module('superpixel-align_amd.segnet_loader')
slabs = importlib.import_module('superpixel-align_amd.slabs')
dw = importlib.import_module('superpixel-align_amd.decode_worker')
cli = importlib.import_module('superpixel-align_amd.cli')
train_segnet = importlib.import_module('train_segnet')
rtr = importlib.import_module('utils.run_train_rounds')

SHAPES = [((256, 512), (128, 256)), ((97, 131), (40, 56)), ((40, 56), (97, 131)), ((64, 96), (64, 48)),
          ((203, 77), (64, 48))]


@pytest.mark.parametrize('src,dst', SHAPES)
def test_float_bicubic_restatement_equals_pillow(src, dst):
    """pil_bicubic_coeffs + the two-pass float64 accumulation (what spa_segnet_train_input runs) against Pillow's mode
    'F' BICUBIC, through the dataset's own resize_bicubic_float: no float32 value differs."""
    rng = np.random.default_rng(src[0] * 1000 + dst[1])
    for img in (rng.integers(0, 256, (3,) + src).astype(np.float32),              # widened bytes: the loader's input
                rng.normal(100, 80, (2,) + src).astype(np.float32)):
        ref = st.resize_bicubic_float(img, dst)
        got = st.pil_resize_float(img, dst)
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert int((syn.bits(got) != syn.bits(ref)).sum()) == 0


def test_coefficient_tables_are_bounded_and_normalised():
    for n_in, n_out in [(2048, 1024), (1024, 512), (131, 56), (56, 131), (77, 48)]:
        b, k = st.pil_bicubic_coeffs(n_in, n_out)
        assert b.dtype == np.int32 and k.dtype == np.float64 and b.shape == (n_out, 2) and k.shape[0] == n_out
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= k.shape[1]).all()
        assert np.allclose(k.sum(1), 1.0, atol=1e-12)
        for o in range(n_out):
            assert not k[o, b[o, 1]:].any()


@pytest.mark.parametrize('n_src,n_dst', [(1024, 512), (2048, 1024), (97, 40), (40, 97), (131, 56), (77, 48), (64, 64),
                                         (1000, 333), (333, 1000)])
def test_nearest_index_table(n_src, n_dst):
    lab = np.arange(n_src, dtype=np.int32)[None, None, :].repeat(2, 1)
    assert np.array_equal(st.resize_nearest_label(lab, (2, n_dst))[0, 0], st.nearest_index_table(n_src, n_dst))
    assert np.array_equal(cli.resize_nearest(lab[0], (2, n_dst))[0], st.nearest_index_table(n_src, n_dst, 'cv2'))


# ------------------------------------------------------------------------------- the label task
def test_label_task_reads_masks_and_scores(tmp_path):
    rng = np.random.default_rng(3)
    mask = rng.random((20, 36)) > 0.5
    mask8 = (rng.random((20, 36)) > 0.5).astype(np.uint8)
    scores = rng.random((2, 20, 36)).astype(np.float32)
    wide = rng.integers(0, 5, (20, 36)).astype(np.int64)
    zfn = str(tmp_path / 'labels.zip')
    with zipfile.ZipFile(zfn, 'w', zipfile.ZIP_STORED) as zf:
        zf.writestr('d/a_leftImg8bit.npy', syn.npy(mask))
        zf.writestr('d/a_leftImg8bit_scores.npy', syn.npy(scores))
    with zipfile.ZipFile(zfn, 'a', zipfile.ZIP_DEFLATED) as zf:
        zf.writestr('d/b_leftImg8bit.npy', syn.npy(mask8))
        zf.writestr('d/c_leftImg8bit.npy', syn.npy(wide))
        zf.writestr('d/f_leftImg8bit_scores.npy', syn.npy(np.asfortranarray(scores)))
    shm = shared_memory.SharedMemory(create=True, size=1 << 16)
    try:
        buf = np.frombuffer(shm.buf, dtype=np.uint8)
        buf[:] = 255
        assert dw.label_into((shm.name, 64, (20, 36), (zfn, 'd/a_leftImg8bit.npy'))) == ((20, 36), '|b1')
        assert np.array_equal(buf[64:64 + 720].reshape(20, 36), mask.astype(np.uint8))
        assert (buf[:64] == 255).all() and (buf[64 + 720:] == 255).all()
        assert dw.label_into((shm.name, 1024, (20, 36), (zfn, 'd/b_leftImg8bit.npy'))) == ((20, 36), '|u1')
        assert np.array_equal(buf[1024:1024 + 720].reshape(20, 36), mask8)
        assert dw.label_into((shm.name, 4096, (2, 20, 36), (zfn, 'd/a_leftImg8bit_scores.npy'))) == ((2, 20, 36), '<f4')
        assert np.array_equal(buf[4096:4096 + 5760].view(np.float32).reshape(2, 20, 36), scores)
        # what the slab cannot take as it is is reported and not written: another shape, dtype or order
        buf[:] = 255
        assert dw.label_into((shm.name, 0, (21, 36), (zfn, 'd/a_leftImg8bit.npy'))) == ((20, 36), '|b1')
        assert dw.label_into((shm.name, 0, (20, 36), (zfn, 'd/c_leftImg8bit.npy'))) == ((20, 36), '<i8')
        assert dw.label_into((shm.name, 0, (2, 20, 36), (zfn, 'd/f_leftImg8bit_scores.npy')))[0] == (2, 20, 36)
        assert (buf == 255).all()
        del buf
    finally:
        dw._SHM.pop(shm.name).close()
        shm.close()
        shm.unlink()


# ------------------------------------------------------------------------------- the loader against the plain loop
def _soft_zip(z, path, C=2, seed=5):
    """the scores members run_train_rounds.py writes, for the synthetic masks of z[1]"""
    rng = np.random.default_rng(seed)
    with zipfile.ZipFile(z[1]) as zl, zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED) as zo:
        for name in zl.namelist():
            m = np.load(io.BytesIO(zl.read(name)))
            zo.writestr(name, zl.read(name))
            zo.writestr(name[:-len('.npy')] + '_scores.npy', syn.npy(rng.random((C,) + m.shape).astype(np.float32)))
    return path


def _plain(ds, n, batchsize, iters, seed):
    np.random.seed(seed)
    it = st.ShuffledIterator(n, batchsize)
    out = []
    for _ in range(iters):
        batch = [ds.get_example(i) for i in np.arange(n)[it.next_indices()]]
        out.append((np.stack([b[0] for b in batch]), np.stack([b[1] for b in batch]),
                    ({k: np.array(v) for k, v in it.state().items()}, np.random.get_state())))
    return out


def _loaded(ds, n, batchsize, iters, seed, procs=2, depth=None):
    np.random.seed(seed)
    it = st.ShuffledIterator(n, batchsize)
    loader = sl.TrainLoader(ds, np.arange(n), it, procs, sl.HostStage(ds), depth=depth)
    try:
        return [loader.next() for _ in range(iters)], loader.n_host_batches, loader.worker_pids
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


@pytest.mark.parametrize('soft,random', [(False, True), (True, True), (False, False)])
def test_loader_yields_the_plain_loop(tmp_path, soft, random):
    """7 examples in batches of 3 for 9 iterations: more than three epochs, batches that cross epoch boundaries.  The
    arrays and every yielded (iterator state, numpy state) are the plain loop's; afterwards no worker and no shared
    memory segment is left."""
    z = syn.write(str(tmp_path / 'data'), 7, 1, 48, 96)
    label_zip = _soft_zip(z, str(tmp_path / 'soft.zip')) if soft else z[1]
    ds = st.ZippedEstimatedCityscapesDataset(z[0], label_zip, (32, 64), random, soft)
    before = syn.shm_names()
    plain = _plain(ds, 7, 3, 9, seed=11)
    assert plain[-1][2][0]['epoch'] >= 3
    got, n_host, pids = _loaded(ds, 7, 3, 9, seed=11)
    _compare(plain, got)
    assert n_host == 0 and len(pids) >= 1
    assert not any(syn.alive(p) for p in pids)
    assert syn.shm_names() == before


def test_equal_size_frames_pass_through(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 4, 1, 32, 64)
    ds = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (32, 64), True, False)
    got, n_host, _ = _loaded(ds, 4, 2, 5, seed=2, depth=2)
    _compare(_plain(ds, 4, 2, 5, seed=2), got)
    assert n_host == 0


def test_off_size_frame_takes_the_host_path(tmp_path):
    """one frame (and its label) of another size than the first example's: its batches go through the dataset's host
    functions with the draws already made, and every batch still has the plain loop's bits"""
    from PIL import Image
    z = syn.write(str(tmp_path / 'data'), 5, 1, 48, 96)
    rng = np.random.default_rng(9)
    odd_img, odd_mask = syn.image(40, 72, rng)
    imgs, labs = str(tmp_path / 'imgs.zip'), str(tmp_path / 'labs.zip')
    with zipfile.ZipFile(z[0]) as zi, zipfile.ZipFile(imgs, 'w') as zo:
        for k, name in enumerate(zi.namelist()):
            data = zi.read(name)
            if k == 3:
                buf = io.BytesIO()
                Image.fromarray(odd_img).save(buf, format='PNG')
                data = buf.getvalue()
            zo.writestr(name, data)
    with zipfile.ZipFile(z[1]) as zl, zipfile.ZipFile(labs, 'w') as zo:
        for k, name in enumerate(zl.namelist()):
            zo.writestr(name, syn.npy(odd_mask) if k == 3 else zl.read(name))
    ds = st.ZippedEstimatedCityscapesDataset(imgs, labs, (32, 64), True, False)
    got, n_host, _ = _loaded(ds, 5, 2, 8, seed=4)
    _compare(_plain(ds, 5, 2, 8, seed=4), got)
    assert 0 < n_host < 8


def test_small_shm_is_refused_before_any_draw(tmp_path, monkeypatch):
    z = syn.write(str(tmp_path / 'data'), 4, 1, 32, 64)
    ds = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (32, 64), True, False)
    monkeypatch.setattr(slabs, '_shm_free', lambda: 1 << 20)
    np.random.seed(0)
    it = st.ShuffledIterator(4, 2)
    state = np.random.get_state()
    before = syn.shm_names()
    with pytest.raises(cli.ShmTooSmall):
        sl.TrainLoader(ds, np.arange(4), it, 2, sl.HostStage(ds))
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
    assert it.current_position == 0 and syn.shm_names() == before


def test_driver_says_so_once_and_goes_on_without_the_loader(tmp_path, monkeypatch, capsys):
    """train_segnet.open_loader, what main() calls: a /dev/shm too small for the slabs gives one line and no loader
    (the loop then prepares its batches itself), with nothing drawn; enough room gives the loader"""
    z = syn.write(str(tmp_path / 'data'), 4, 1, 32, 64)
    ds = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (32, 64), True, False)
    np.random.seed(0)
    it = st.ShuffledIterator(4, 2)
    state = np.random.get_state()
    with monkeypatch.context() as m:
        m.setattr(slabs, '_shm_free', lambda: 1 << 20)
        assert train_segnet.open_loader(2, ds, np.arange(4), it, sl.HostStage(ds)) is None
    out = capsys.readouterr().out
    assert out.count('\n') == 1 and '--loader_procs: /dev/shm has 1 MB free' in out
    assert 'the batches are prepared on the host' in out
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
    loader = train_segnet.open_loader(2, ds, np.arange(4), it, sl.HostStage(ds))
    try:
        assert isinstance(loader, sl.TrainLoader) and loader.pinned is False
        assert capsys.readouterr().out == ''
    finally:
        loader.close()


_KILLED_PARENT = r'''
import importlib, os, sys, time
import numpy as np
sys.path.insert(0, sys.argv[1])
st = importlib.import_module('superpixel-align_amd.segnet_train')
sl = importlib.import_module('superpixel-align_amd.segnet_loader')
if __name__ == '__main__':
    ds = st.ZippedEstimatedCityscapesDataset(sys.argv[2], sys.argv[3], (32, 64), True, False)
    loader = sl.TrainLoader(ds, np.arange(len(ds)), st.ShuffledIterator(len(ds), 2), 2, sl.HostStage(ds))
    loader.next()
    print(' '.join(str(p) for p in loader.worker_pids), flush=True)
    time.sleep(120)
'''


def test_workers_do_not_outlive_a_killed_trainer(tmp_path):
    """the workers carry the parent-death signal: SIGKILL to the process that owns the loader ends them"""
    z = syn.write(str(tmp_path / 'data'), 4, 1, 32, 64)
    script = str(tmp_path / 'owner.py')
    with open(script, 'w') as f:
        f.write(_KILLED_PARENT)
    p = subprocess.Popen([sys.executable, script, ROOT, z[0], z[1]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True)
    try:
        line = p.stdout.readline()
        pids = [int(v) for v in line.split()]
        assert pids, p.stderr.read()[-2000:]
        assert all(syn.alive(q) for q in pids)
        p.send_signal(signal.SIGKILL)
        p.wait(timeout=30)
        deadline = time.time() + 30
        while time.time() < deadline and any(syn.alive(q) for q in pids):
            time.sleep(0.1)
        assert not any(syn.alive(q) for q in pids)
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()


def test_workers_import_nothing_heavy():
    r = subprocess.run([sys.executable, '-c', "import importlib, sys; sys.path.insert(0, %r); "
                        "importlib.import_module('superpixel-align_amd.decode_worker'); "
                        "print(int('torch' in sys.modules))" % ROOT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == '0', r.stderr[-2000:]


# ------------------------------------------------------------------------------- flags
def test_flag_is_recorded_only_when_given():
    reference = vars(train_segnet.get_parser().parse_args([]))
    pre, args = train_segnet.run_args([])
    assert pre.loader_procs == 0 and vars(args) == dict(reference, dtype='fp32')     # a default run's args.txt entries
    pre, args = train_segnet.run_args(['--batchsize', '2', '--loader_procs', '3', '--random'])
    assert pre.loader_procs == 3
    assert vars(args) == dict(reference, dtype='fp32', loader_procs=3, batchsize=2, random=True)
    assert json.loads(json.dumps(vars(args), sort_keys=True))['loader_procs'] == 3
    with pytest.raises(SystemExit):                       # the reference parser does not take it
        train_segnet.get_args(['--loader_procs', '3'])
    with pytest.raises(ValueError):
        train_segnet.run_args(['--loader_procs', '-1'])


def test_rounds_driver_forwards_the_flag():
    def argvs(argv):
        a = rtr.get_args(argv)
        steps = [s for s in rtr.plan(a, 'R/train_round1_x_0') if s['kind'] == 'train']
        dirs = {i + 1: 'D%d' % (i + 1) for i in range(len(steps))}
        return [rtr.train_argv(a, s, 'D%d' % (i + 1), dirs) for i, s in enumerate(steps)]
    base = ['--n_round', '3', '--iteration', '100', '--val_iteration', '50', '--n_use_data', '40', '--random']
    for a, b in zip(argvs(base), argvs(base + ['--loader_procs', '4'])):
        assert '--loader_procs' not in a
        assert b == a + ['--loader_procs', '4']
    pre, rest = train_segnet.get_pre_args(argvs(base + ['--loader_procs', '4'])[1])
    assert pre.loader_procs == 4 and pre.data_parallel and '--loader_procs' not in rest
    train_segnet.get_args(rest)


def test_entry_points_declared_and_bound():
    lib = importlib.import_module('superpixel-align_amd._lib')
    header = open(os.path.join(ROOT, 'include', 'spalign.h')).read()
    for name in ('spa_segnet_train_input', 'spa_segnet_train_label'):
        assert name in lib.PROTOTYPES and ('int %s(' % name) in header
    engine = importlib.import_module('superpixel-align_amd.engine')
    assert hasattr(engine.Engine, 'segnet_train_input') and hasattr(engine.Engine, 'segnet_train_label')
