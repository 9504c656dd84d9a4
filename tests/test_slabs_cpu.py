"""CPU tests of superpixel-align_amd/slabs.py, the slab ring under the three decode loaders: a ring of PNG frames with a
host stage and two real workers.  Order and number of batches in flight, the wait before a slab is decoded into again,
the stage-ahead rule, an abandoned pass, cleanup, and the /dev/shm refusal of each of the three users."""
import concurrent.futures
import importlib
import os
import sys
import zipfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

slabs = importlib.import_module('superpixel-align_amd.slabs')
sl = importlib.import_module('superpixel-align_amd.segnet_loader')
st = importlib.import_module('superpixel-align_amd.segnet_train')
segnet = importlib.import_module('superpixel-align_amd.segnet')
dw = importlib.import_module('superpixel-align_amd.decode_worker')
cli = importlib.import_module('superpixel-align_amd.cli')

H, W, N, B, DEPTH = 16, 24, 7, 2, 2


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    z = syn.write(str(tmp_path_factory.mktemp('slabs')), 2, N, H, W)
    with zipfile.ZipFile(z[2]) as zf:
        names = zf.namelist()
        frames = [syn.decoded(zf.read(n)) for n in names]
    return dict(z=z, names=names, frames=frames)


class Recorder(slabs.HostSlabStage):
    """a host stage that numbers its slabs and writes down what the ring asks of it"""

    def __init__(self):
        self.log, self.ring = [], None

    def register(self, shm):
        self.log.append(('register', shm.name))
        return {'pinned': False, 'name': shm.name}

    def wait(self, handle):
        self.log.append(('wait', handle['name']))

    def run(self, handle, layout, views, n):
        assert len(self.ring.pending) <= self.ring.depth
        self.log.append(('run', handle['name']))
        return slabs.HostSlabStage.run(self, handle, layout, views, n)

    def on_slab(self, fields):
        return fields[0].copy()


class FrameRing(slabs.Ring):
    """the frames of a zip in batches of B, in order; restart() begins another pass"""

    def __init__(self, data, stage, depth=DEPTH, n_items=N):
        self.zip_fn, self.names, self.n_items, self.pos = data['z'][2], data['names'], n_items, 0
        slabs.Ring.__init__(self, 'the test', slabs.Layout(B, [('frames', (H, W, 3), np.uint8)]), depth, 2, stage)
        stage.ring = self
        submit = self.slabs.submit

        def recorded(fn, task):
            stage.log.append(('submit', task[0]))
            return submit(fn, task)
        self.slabs.submit = recorded

    def produce(self, name):
        ids = list(range(self.n_items))[self.pos:self.pos + self.B]
        if not ids:
            return None
        self.pos += len(ids)
        return {'n': len(ids), 'ids': ids}, [
            (dw.png_into, (name, self.layout.offset('frames', j), (H, W, 3), 'RGB', (self.zip_fn, self.names[i])))
            for j, i in enumerate(ids)]

    def fits(self, rec, got):
        return all((tuple(g[0]), g[1]) == ((H, W, 3), 'RGB') for g in got)

    def run(self, rec, handle, views):
        return self.stage.run(handle, self.layout, views, rec['n'])

    def host(self, rec):
        return None

    def restart(self):
        self.drain()
        self.pos = 0

    def rest(self):
        out = []
        while True:
            rec = self.take()
            if rec is None:
                return out
            assert len(self.pending) <= self.depth
            out.append((rec['ids'], rec['out']))


def _check(data, batches):
    assert [ids for ids, _ in batches] == [[0, 1], [2, 3], [4, 5], [6]]
    for ids, out in batches:
        assert out.shape == (len(ids), H, W, 3)
        for j, i in enumerate(ids):
            assert np.array_equal(out[j], data['frames'][i])


def test_order_depth_and_the_wait_before_a_slab_is_reused(data):
    before, blocks = syn.shm_names(), syn.shm_names('psm_')
    stage = Recorder()
    ring = FrameRing(data, stage)
    try:
        assert len(ring.slabs.slots) == DEPTH + 1 == len(syn.shm_names('psm_') - blocks) and len(ring.worker_pids) <= 2
        pids = ring.worker_pids
        _check(data, ring.rest())
        ring.restart()
        _check(data, ring.rest())                           # a second pass: every slab has been used more than once
        assert ring.n_host_batches == 0
    finally:
        ring.close()
    assert syn.shm_names() == before and not any(syn.alive(p) for p in pids)
    runs = [name for what, name in stage.log if what == 'run']
    assert len(runs) == 8 and all(runs.count(name) >= 2 for name in set(runs)) and len(set(runs)) == DEPTH + 1
    # a staged slab (its upload may be in flight) is decoded into again only after wait() for it
    staged = set()
    for what, name in stage.log:
        if what == 'run':
            staged.add(name)
        elif what == 'wait':
            staged.discard(name)
        elif what == 'submit':
            assert name not in staged
    for name in set(runs):                                  # and wait() comes right before each batch's tasks
        mine = [what for what, n in stage.log if n == name]
        assert all(mine[k - 1] in ('wait', 'submit') for k, what in enumerate(mine) if what == 'submit')


def test_stage_ahead_only_when_the_next_decodes_are_done(data):
    stage = Recorder()
    ring = FrameRing(data, stage)
    runs = lambda: sum(what == 'run' for what, _ in stage.log)
    try:
        ring._fill()
        concurrent.futures.wait([f for rec in ring.pending for f in rec['futures']])
        assert ring.take()['ids'] == [0, 1] and runs() == 2     # [2, 3] was staged inside the same take()
        ring._fill()
        held = concurrent.futures.Future()                  # one task of [4, 5] that has not ended
        ring.pending[1]['futures'].append(held)
        concurrent.futures.wait(ring.pending[1]['futures'][:-1])
        assert ring.take()['ids'] == [2, 3] and runs() == 2     # [4, 5] waits for its last task
        held.set_result(((H, W, 3), 'RGB'))
        concurrent.futures.wait(ring.pending[1]['futures'])
        assert ring.take()['ids'] == [4, 5] and runs() == 4
    finally:
        ring.close()


def test_abandoned_pass(data):
    ring = FrameRing(data, Recorder())
    try:
        assert ring.take()['ids'] == [0, 1]
        left = [f for rec in ring.pending for f in (rec['futures'] or ())]
        assert left
        ring.restart()
        assert all(f.done() for f in left) and not ring.pending and len(ring.free) == DEPTH + 1
        _check(data, ring.rest())
    finally:
        ring.close()


def test_close_twice_and_after_a_failed_register(data):
    before = syn.shm_names()
    ring = FrameRing(data, Recorder())
    pids = ring.worker_pids
    ring.take()                                             # batches in flight when it is closed
    ring.close()
    ring.close()
    assert syn.shm_names() == before and not any(syn.alive(p) for p in pids)

    class Failing(Recorder):
        def register(self, shm):
            if len(self.log) == 1:
                raise RuntimeError('no second slab')
            return Recorder.register(self, shm)
    with pytest.raises(RuntimeError, match='no second slab'):
        FrameRing(data, Failing())
    assert syn.shm_names() == before


def test_small_shm_refuses_each_user_before_any_worker(data, tmp_path, monkeypatch):
    from PIL import Image
    z = data['z']

    def no_pool(n_procs):
        raise AssertionError('a worker pool was made')
    monkeypatch.setattr(slabs, 'WorkerPool', no_pool)
    monkeypatch.setattr(slabs, '_shm_free', lambda: 1 << 20)
    before = syn.shm_names()
    train = st.ZippedEstimatedCityscapesDataset(z[0], z[1], (H, W), True, False)
    with pytest.raises(slabs.ShmTooSmall, match="training loader's slabs need"):
        sl.TrainLoader(train, np.arange(2), st.ShuffledIterator(2, 2), 2, sl.HostStage(train))
    valid = segnet.ZippedCityscapesRoadDataset(z[2], z[3], (H, W))
    with pytest.raises(slabs.ShmTooSmall, match="label loader's slabs need"):
        sl.LabelLoader(valid, range(N), 2, 2, sl.HostLabelStage())
    # cli.ProcessDecoder: refused before a worker starts and before CUDA is touched, so this needs no GPU
    fns = [str(tmp_path / 'f.png'), str(tmp_path / 'l.png')]
    Image.fromarray(data['frames'][0]).save(fns[0])
    Image.fromarray(data['frames'][0][:, :, 0].copy()).save(fns[1])
    assert cli.ShmTooSmall is slabs.ShmTooSmall
    with pytest.raises(cli.ShmTooSmall, match=r'^/dev/shm has 1 MB free, the decode slabs need 0 MB$'):
        cli.ProcessDecoder(cli.ImageList(fns[:1], None, np.uint8), cli.ImageList(fns[1:], None, np.uint8), 2, 2, 'cuda:0')
    assert syn.shm_names() == before
