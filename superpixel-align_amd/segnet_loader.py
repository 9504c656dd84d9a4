"""The input stage of SegNet-Basic training (train_segnet.py --loader_procs N): decode in worker processes, resize and
augment on the GPU, a few batches ahead of the step, with the bits of the plain loop

    ids = train_ids[it.next_indices()];  batch = [train.get_example(i) for i in ids]

Workers (decode_worker.py: numpy and Pillow only, spawned, never on the GPU, SIGTERM when the trainer dies) decode the
PNGs and read the label members into shared-memory slabs that the device stage registers as pinned host memory.  A
slab holds one batch: the frames (B,H,W,3) uint8, the labels (uint8 masks (B,H,W) or float32 scores (B,C,H,W)), and the
batch's draws (lighting shifts (B,3) float64, flips (B,) uint8).  The device stage uploads it with one copy on a side
stream and runs Engine.segnet_train_input / segnet_train_label there; the training stream waits for that batch's event
only.

What keeps the bits:
  * every random draw is made by the trainer's process in the plain loop's order: per batch it.next_indices() (which
    may draw the next epoch's permutation), then with --random per example np.random.normal(0, 25.5, 3) and
    np.random.rand().  Workers draw nothing.
  * after a batch's draws the loader captures (it.state(), np.random.get_state()) and yields the pair with the batch:
    it is the state the plain loop has after that iteration, so a snapshot that stores it (not the live state, which
    has run ahead) is the plain run's snapshot, and --resume continues from it with or without the loader.
  * a batch with a frame or label whose shape or dtype is not the first example's goes through the dataset's host
    functions with the draws already made.
HostStage runs the device stage's arithmetic with the dataset's numpy and Pillow functions (no GPU): the tests of
the draw order use it, with real workers.

LabelLoader feeds the two loops that read a ZippedCityscapesRoadDataset with get_raw (labels_from_segnet.save_labels
and train_segnet.evaluate, --loader_procs) the same way: frames and raw labelIds bytes, in index order, nothing drawn.
Both loaders keep their slabs and workers in one helper, Slabs, and may share one WorkerPool.
"""
import collections
import os

import numpy as np

from . import decode_worker
from . import segnet_train as st


def default_depth(n_procs, batchsize):
    """batches in flight: enough image tasks to occupy every worker, plus the batch being uploaded; 3..6"""
    return max(3, min(6, -(-int(n_procs) // max(int(batchsize), 1)) + 1))


def _shm_free():
    try:
        s = os.statvfs('/dev/shm')
        return s.f_bavail * s.f_frsize
    except OSError:
        return None


def _first_shapes(ds):
    """((H, W, 3), label shape) of the dataset's first example, from the file headers"""
    import zipfile
    from numpy.lib import format as npf
    from PIL import Image
    with zipfile.ZipFile(ds.img_zip_fn) as zf, Image.open(zf.open(ds.img_fns[0])) as f:
        W, H = f.size
    with zipfile.ZipFile(ds.label_zip_fn) as zf, zf.open(ds.label_fns[0]) as fp:
        version = npf.read_magic(fp)
        shape = (npf.read_array_header_1_0 if version == (1, 0) else npf.read_array_header_2_0)(fp)[0]
    return (H, W, 3), tuple(shape)


class HostStage(object):
    """The device stage's work with get_example's own functions: numpy batches in, numpy batches out."""

    def __init__(self, dataset):
        self.ds = dataset

    def register(self, shm):
        return {'pinned': False}

    def unregister(self, handle):
        pass

    def wait(self, handle):
        pass

    def run(self, handle, views, n, random):
        imgs, labs, shifts, flips = views
        out = []
        for j in range(n):
            img = imgs[j].astype(np.float32).transpose(2, 0, 1)
            lab = labs[j].astype(np.float32 if self.ds.use_soft_label else np.int32)
            img, lab = self.ds.resized(img, lab)
            if random:
                out.append(self.ds.augmented(img, lab, shifts[j], bool(flips[j])))
            else:
                out.append((np.ascontiguousarray(img, np.float32), np.ascontiguousarray(lab)))
        return self.from_host(out)

    def from_host(self, batch):
        return np.stack([b[0] for b in batch]), np.stack([b[1] for b in batch])

    def finish(self, out):
        return out

    def close(self):
        pass


class DeviceStage(object):
    """One upload of the slab and the two input kernels on a side stream; finish() makes the current stream wait for
    the batch's event."""

    def __init__(self, dataset, engine):
        import torch
        self.torch, self.ds, self.eng = torch, dataset, engine
        self.side = torch.cuda.Stream(engine.device)
        self.warned = False

    def register(self, shm):
        torch = self.torch
        t = torch.frombuffer(shm.buf, dtype=torch.uint8)
        pinned = False
        try:
            rc = torch.cuda.cudart().cudaHostRegister(t.data_ptr(), t.numel(), 0)
            pinned = rc is None or int(rc) == 0
        except Exception:
            pinned = False
        if not pinned and not self.warned:
            self.warned = True                              # pageable slabs: same bits, but the upload is a staged copy
            print('segnet_loader: the slabs could not be registered as pinned host memory; uploads will not overlap '
                  'the step', flush=True)
        return {'t': t, 'pinned': pinned, 'ev': None}

    def unregister(self, handle):
        if handle['pinned']:
            try:
                self.torch.cuda.cudart().cudaHostUnregister(handle['t'].data_ptr())
            except Exception:
                pass
        handle['t'] = None

    def wait(self, handle):
        if handle['ev'] is not None:
            handle['ev'].synchronize()                      # the slab's last upload has finished

    def run(self, handle, views, n, random):
        torch = self.torch
        imgs, labs, shifts, flips = views
        base = imgs.__array_interface__['data'][0]

        def dev_view(d, a, dtype):
            off = a.__array_interface__['data'][0] - base
            return d[off:off + a.nbytes].view(dtype).view(tuple(a.shape))

        end = flips.__array_interface__['data'][0] + flips.nbytes - base
        with torch.cuda.stream(self.side):
            d = handle['t'][:end].to(self.eng.device, non_blocking=True)
            handle['ev'] = torch.cuda.Event()
            handle['ev'].record(self.side)
            sh = dev_view(d, shifts[:n], torch.float64) if random else None
            fl = dev_view(d, flips[:n], torch.uint8) if random else None
            img = self.eng.segnet_train_input(dev_view(d, imgs[:n], torch.uint8), self.ds.resize_shape, sh, fl)
            lab = self.eng.segnet_train_label(dev_view(d, labs[:n], getattr(torch, str(labs.dtype))),
                                              self.ds.resize_shape, fl)
            ready = torch.cuda.Event()
            ready.record(self.side)
        return img, lab, ready

    def from_host(self, batch):
        torch = self.torch
        return (torch.from_numpy(np.stack([b[0] for b in batch])).to(self.eng.device),
                torch.from_numpy(np.stack([b[1] for b in batch])).to(self.eng.device), None)

    def finish(self, out):
        img, lab, ready = out
        if ready is not None:
            cur = self.torch.cuda.current_stream(self.eng.device)
            cur.wait_event(ready)
            img.record_stream(cur)
            lab.record_stream(cur)
        return img, lab

    def close(self):
        self.side.synchronize()


class WorkerPool(object):
    """The spawned decode workers of one process (decode_worker.py), shared by its loaders: every user acquire()s it
    and release()s it in its close(); the last release shuts it down.  spawn, not fork: the process may have
    initialised the GPU.  The workers end with the process that made them (die_with_parent)."""

    def __init__(self, n_procs):
        import multiprocessing as mp
        from concurrent.futures import ProcessPoolExecutor
        self.n_procs = int(n_procs)
        self.executor = ProcessPoolExecutor(max_workers=self.n_procs, mp_context=mp.get_context('spawn'),
                                            initializer=decode_worker.die_with_parent, initargs=(os.getpid(),))
        self.users = 0
        self.pids = None

    def acquire(self):
        self.users += 1
        return self

    def warm(self):
        """-> the workers' pids; the first call starts every worker and imports Pillow's PNG plugin in it"""
        if self.pids is None:
            self.pids = sorted(set(self.executor.map(decode_worker.warm, range(4 * self.n_procs))))
        return self.pids

    def release(self):
        self.users -= 1
        if self.users <= 0 and self.executor is not None:
            self.executor.shutdown(wait=True, cancel_futures=True)
            self.executor = None


class Slabs(object):
    """What a loader holds besides its batches: n_slabs shared-memory slabs of slab_bytes each (the caller counts one
    spare, so a batch is never decoded into the slab whose upload was just enqueued), each registered with the stage
    (DeviceStage: as pinned host memory, with one notice when that fails), and the worker pool, its own or the one
    given.  Raises cli.ShmTooSmall where /dev/shm cannot hold the slabs, before anything else happens.  A
    constructor that fails has closed what it had opened.  close() may be called any number of times."""

    def __init__(self, what, slab_bytes, n_slabs, n_procs, stage, pool=None):
        from multiprocessing import shared_memory
        self.stage, self.slots, self.workers = stage, [], None
        free = _shm_free()
        if free is not None and free < n_slabs * slab_bytes + (16 << 20):
            from .cli import ShmTooSmall
            raise ShmTooSmall('/dev/shm has %d MB free, %s slabs need %d MB'
                              % (free >> 20, what, (n_slabs * slab_bytes) >> 20))
        try:
            for _ in range(n_slabs):
                shm = shared_memory.SharedMemory(create=True, size=slab_bytes)
                slot = {'shm': shm, 'handle': None}
                self.slots.append(slot)
                slot['handle'] = stage.register(shm)
            self.workers = (pool if pool is not None else WorkerPool(n_procs)).acquire()
            self.pinned = all(s['handle']['pinned'] for s in self.slots)    # every slab is pinned host memory
            self.worker_pids = self.workers.warm()
        except BaseException:
            self.close()
            raise

    def submit(self, fn, task):
        return self.workers.executor.submit(fn, task)

    def close(self, futures=()):
        """futures: the owner's tasks still in flight; none of them writes into a slab after this returns"""
        for f in futures:
            f.cancel()
        for f in futures:
            if not f.cancelled():
                try:
                    f.exception()
                except BaseException:
                    pass
        workers, self.workers = self.workers, None
        if workers is not None:
            workers.release()
        slots, self.slots = self.slots, []
        try:
            self.stage.close()
        finally:                                            # the slabs go whatever state the device is in
            for s in slots:
                if s['handle'] is not None:
                    self.stage.unregister(s['handle'])
                    s['handle'] = None
                for release in (s['shm'].close, s['shm'].unlink):
                    try:
                        release()
                    except Exception:
                        pass


class TrainLoader(object):
    """next() -> (images (B,3,h,w) float32, labels, (iterator state, numpy state) after that batch's draws): the plain
    loop's batches in its order.  dataset: a ZippedEstimatedCityscapesDataset; ids: the rank's example indices
    (train_ids); iterator: the ShuffledIterator the plain loop would call.  stage: a DeviceStage or a HostStage.
    pool: a WorkerPool to share (another loader's .workers); None: n_procs workers of its own.
    Raises cli.ShmTooSmall where /dev/shm cannot hold the slabs, before anything is drawn.  close() stops the workers
    and unregisters and unlinks the slabs; call it in a finally."""

    def __init__(self, dataset, ids, iterator, n_procs, stage, depth=None, pool=None):
        self.ds, self.ids, self.it, self.stage = dataset, np.asarray(ids), iterator, stage
        self.B = int(iterator.batchsize)
        self.depth = depth = int(depth or default_depth(n_procs, self.B))
        self.ishape, self.lshape = _first_shapes(dataset)
        self.ldtype = np.dtype(np.float32 if dataset.use_soft_label else np.uint8)
        align = lambda n: (n + 63) // 64 * 64
        self.ibytes = int(np.prod(self.ishape))
        self.lbytes = int(np.prod(self.lshape)) * self.ldtype.itemsize
        self.lab_off = align(self.B * self.ibytes)
        self.shift_off = align(self.lab_off + self.B * self.lbytes)
        self.flip_off = self.shift_off + self.B * 24
        slab = align(self.flip_off + self.B)
        self.slots, self.free, self.pending = [], [], collections.deque()
        self.pool = self.slabs = None
        self.n_host_batches = 0            # batches that took the host path (another shape than the first example's)
        self.slabs = Slabs('the training loader\'s', slab, depth + 1, n_procs, stage, pool)
        self.slots, self.free = self.slabs.slots, list(self.slabs.slots)
        self.workers, self.pool = self.slabs.workers, self.slabs.workers.executor
        self.pinned, self.worker_pids = self.slabs.pinned, self.slabs.worker_pids

    def _views(self, slot):
        buf = np.frombuffer(slot['shm'].buf, dtype=np.uint8)
        B = self.B
        return (buf[:B * self.ibytes].reshape((B,) + self.ishape),
                buf[self.lab_off:self.lab_off + B * self.lbytes].view(self.ldtype).reshape((B,) + self.lshape),
                buf[self.shift_off:self.shift_off + B * 24].view(np.float64).reshape(B, 3),
                buf[self.flip_off:self.flip_off + B])

    def _submit(self):
        """the draws of the next batch, in the plain loop's order, and its decode tasks"""
        ids = self.ids[self.it.next_indices()]
        shifts = flips = None
        if self.ds.random:
            shifts, flips = np.empty((len(ids), 3), np.float64), np.empty(len(ids), np.uint8)
            for j in range(len(ids)):
                shifts[j] = st.pca_lighting_shift(np.random.normal(0, 25.5, size=3))
                flips[j] = np.random.rand() > 0.5
        state = ({k: np.array(v) for k, v in self.it.state().items()}, np.random.get_state())
        slot = self.free.pop(0)
        self.stage.wait(slot['handle'])
        name = slot['shm'].name
        tasks = [(decode_worker.decode_into, (name, j * self.ibytes, self.ishape,
                                              (self.ds.img_zip_fn, self.ds.img_fns[i]))) for j, i in enumerate(ids)]
        tasks += [(decode_worker.label_into, (name, self.lab_off + j * self.lbytes, self.lshape,
                                              (self.ds.label_zip_fn, self.ds.label_fns[i]))) for j, i in enumerate(ids)]
        self.pending.append({'ids': ids, 'shifts': shifts, 'flips': flips, 'state': state, 'slot': slot, 'out': None,
                             'futures': [self.slabs.submit(fn, t) for fn, t in tasks]})

    def _fill(self):
        while self.free and len(self.pending) < self.depth:
            self._submit()

    def _stage(self, rec):
        """wait for the batch's tasks, then the stage on its slab, or the host path for a batch with another shape"""
        n = len(rec['ids'])
        got = [f.result() for f in rec['futures']]
        rec['futures'] = None
        slot, rec['slot'] = rec['slot'], None
        ok = all(tuple(g) == self.ishape for g in got[:n]) and all(
            tuple(g[0]) == self.lshape and (np.dtype(g[1]) == self.ldtype or
                                            (self.ldtype == np.uint8 and np.dtype(g[1]) == np.bool_)) for g in got[n:])
        if ok:
            views = self._views(slot)
            if self.ds.random:
                views[2][:n] = rec['shifts']
                views[3][:n] = rec['flips']
            rec['out'] = self.stage.run(slot['handle'], views, n, self.ds.random)
            del views
        else:
            batch = []
            for j, i in enumerate(rec['ids']):
                img, lab = self.ds.resized(*self.ds.decoded(i))
                if self.ds.random:
                    batch.append(self.ds.augmented(img, lab, rec['shifts'][j], bool(rec['flips'][j])))
                else:
                    batch.append((np.ascontiguousarray(img, np.float32), np.ascontiguousarray(lab)))
            rec['out'] = self.stage.from_host(batch)
            self.n_host_batches += 1
        self.free.append(slot)

    def next(self):
        self._fill()
        rec = self.pending.popleft()
        if rec['out'] is None:
            self._stage(rec)
        self._fill()
        # the batch after this one, when its decodes are done already: its upload and kernels overlap the step
        if self.pending and self.pending[0]['out'] is None and all(f.done() for f in self.pending[0]['futures']):
            self._stage(self.pending[0])
            self._fill()
        img, lab = self.stage.finish(rec['out'])
        return img, lab, rec['state']

    def close(self):
        futures = [f for rec in self.pending for f in (rec['futures'] or ())]
        self.pending.clear()
        self.free, self.slots, self.pool = [], [], None
        slabs, self.slabs = self.slabs, None
        if slabs is not None:
            slabs.close(futures)


# ------------------------------------------------------------------------------- labelling and validation
def _first_png_shapes(ds):
    """((H, W, 3), (Hl, Wl)) of a ZippedCityscapesRoadDataset's first frame and labelIds image, from the headers"""
    import zipfile
    from PIL import Image
    with zipfile.ZipFile(ds.img_zip_fn) as zf, Image.open(zf.open(ds.img_fns[0])) as f:
        W, H = f.size
    with zipfile.ZipFile(ds.label_zip_fn) as zf, Image.open(zf.open(ds.label_fns[0])) as f:
        Wl, Hl = f.size
    return (H, W, 3), (Hl, Wl)


class LabelBatch(object):
    """One batch of a LabelLoader.  indices: the dataset indices, in order.  host False: frames (n,H,W,3) uint8 and
    label_ids (n,Hl,Wl) uint8, the stage's arrays (device tensors the current stream may use, or numpy copies), and
    ids_host, a numpy copy of the label ids where the loader keeps one (else None).  host True: the batch holds a
    member of another shape or mode and must go through the dataset's get_raw; the arrays are None."""

    def __init__(self, indices):
        self.indices, self.host = indices, False
        self.frames = self.label_ids = self.ids_host = None


class HostLabelStage(HostStage):
    """numpy in, numpy out, no GPU: copies of the slab's frames and label ids."""

    def __init__(self, dataset=None):
        HostStage.__init__(self, dataset)

    def run(self, handle, views, n):
        return views[0][:n].copy(), views[1][:n].copy()


class DeviceLabelStage(DeviceStage):
    """One upload of the slab's frames and label ids on a side stream; finish() makes the current stream wait for it."""

    def __init__(self, engine):
        DeviceStage.__init__(self, None, engine)

    def run(self, handle, views, n):
        torch = self.torch
        imgs, ids = views[0][:n], views[1][:n]
        base = views[0].__array_interface__['data'][0]
        off = ids.__array_interface__['data'][0] - base
        with torch.cuda.stream(self.side):
            d = handle['t'][:off + ids.nbytes].to(self.eng.device, non_blocking=True)
            handle['ev'] = torch.cuda.Event()
            handle['ev'].record(self.side)
        return (d[:imgs.nbytes].view(tuple(imgs.shape)), d[off:off + ids.nbytes].view(tuple(ids.shape)), handle['ev'])

    def finish(self, out):
        frames, ids, ready = out
        cur = self.torch.cuda.current_stream(self.eng.device)
        cur.wait_event(ready)
        frames.record_stream(cur)
        return frames, ids


class LabelLoader(object):
    """The frames and labelIds images of a ZippedCityscapesRoadDataset's examples `indices`, in order, in batches of
    `batchsize` (the last may be short), decoded by workers a few batches ahead (default_depth) into slabs: what
    labels_from_segnet.save_labels and train_segnet.evaluate read with get_raw, one image after the other.
    batches() yields LabelBatch objects; it may be called again for another pass over the same indices.  A batch with
    a frame or label of another shape than the first example's, or of another mode than RGB / L (for which np.asarray
    of the decoded image is not what get_raw's convert() gives), is marked host.  stage: a DeviceLabelStage or a
    HostLabelStage.  pool: a WorkerPool to share (a TrainLoader's .workers).  keep_ids: every batch also carries a
    numpy copy of its label ids.  Raises cli.ShmTooSmall like TrainLoader; close() in a finally."""

    def __init__(self, dataset, indices, batchsize, n_procs, stage, depth=None, pool=None, keep_ids=False):
        self.ds, self.indices, self.stage = dataset, [int(i) for i in indices], stage
        self.B = max(int(batchsize), 1)
        self.depth = depth = int(depth or default_depth(n_procs, self.B))
        self.keep_ids = bool(keep_ids)
        self.free, self.pending, self.pos = [], collections.deque(), 0
        self.slabs = None
        self.n_host_batches = 0
        self.ishape, self.lshape = _first_png_shapes(dataset) if self.indices else ((1, 1, 3), (1, 1))
        align = lambda n: (n + 63) // 64 * 64
        self.ibytes, self.lbytes = int(np.prod(self.ishape)), int(np.prod(self.lshape))
        self.lab_off = align(self.B * self.ibytes)
        slab = align(self.lab_off + self.B * self.lbytes)
        self.slabs = Slabs('the label loader\'s', slab, depth + 1, n_procs, stage, pool)
        self.free = list(self.slabs.slots)
        self.workers = self.slabs.workers
        self.pinned, self.worker_pids = self.slabs.pinned, self.slabs.worker_pids

    def _views(self, slot):
        buf = np.frombuffer(slot['shm'].buf, dtype=np.uint8)
        B = self.B
        return (buf[:B * self.ibytes].reshape((B,) + self.ishape),
                buf[self.lab_off:self.lab_off + B * self.lbytes].reshape((B,) + self.lshape))

    def _submit(self):
        ids = self.indices[self.pos:self.pos + self.B]
        self.pos += len(ids)
        slot = self.free.pop(0)
        self.stage.wait(slot['handle'])
        name = slot['shm'].name
        tasks = [(name, j * self.ibytes, self.ishape, 'RGB', (self.ds.img_zip_fn, self.ds.img_fns[i]))
                 for j, i in enumerate(ids)]
        tasks += [(name, self.lab_off + j * self.lbytes, self.lshape, 'L', (self.ds.label_zip_fn, self.ds.label_fns[i]))
                  for j, i in enumerate(ids)]
        self.pending.append({'batch': LabelBatch(ids), 'slot': slot, 'out': None,
                             'futures': [self.slabs.submit(decode_worker.png_into, t) for t in tasks]})

    def _fill(self):
        while self.free and len(self.pending) < self.depth and self.pos < len(self.indices):
            self._submit()

    def _stage(self, rec):
        batch = rec['batch']
        n = len(batch.indices)
        got = [f.result() for f in rec['futures']]
        rec['futures'] = None
        slot, rec['slot'] = rec['slot'], None
        want = [(self.ishape, 'RGB')] * n + [(self.lshape, 'L')] * n
        if all((tuple(g[0]), g[1]) == w for g, w in zip(got, want)):
            views = self._views(slot)
            if self.keep_ids:
                batch.ids_host = views[1][:n].copy()
            rec['out'] = self.stage.run(slot['handle'], views, n)
            del views
        else:
            batch.host = True
            rec['out'] = ()
            self.n_host_batches += 1
        self.free.append(slot)

    def _drain(self):
        """an abandoned pass: its tasks end before their slabs are used again"""
        for rec in self.pending:
            for f in rec['futures'] or ():
                f.cancel()
            for f in rec['futures'] or ():
                if not f.cancelled():
                    try:
                        f.exception()
                    except BaseException:
                        pass
            if rec['slot'] is not None:
                self.free.append(rec['slot'])
        self.pending.clear()

    def batches(self):
        self._drain()
        self.pos = 0
        while True:
            self._fill()
            if not self.pending:
                return
            rec = self.pending.popleft()
            if rec['out'] is None:
                self._stage(rec)
            self._fill()
            # the batch after this one, when its decodes are done already: its upload overlaps this batch's work
            if self.pending and self.pending[0]['out'] is None and all(f.done() for f in self.pending[0]['futures']):
                self._stage(self.pending[0])
                self._fill()
            batch = rec['batch']
            if not batch.host:
                batch.frames, batch.label_ids = self.stage.finish(rec['out'])
            yield batch

    __iter__ = batches

    def close(self):
        futures = [f for rec in self.pending for f in (rec['futures'] or ())]
        self.pending.clear()
        self.free = []
        slabs, self.slabs = self.slabs, None
        if slabs is not None:
            slabs.close(futures)
