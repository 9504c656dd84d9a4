"""Shared-memory slabs, spawned decode workers (decode_worker.py) and the prefetch ring over them: what
segnet_loader.TrainLoader, segnet_loader.LabelLoader and cli.ProcessDecoder stand on.  Nothing here knows what a batch
holds: a Layout says where its fields lie in a slab, a stage (HostSlabStage, DeviceSlabStage) what becomes of a decoded
slab, and a Ring's subclass which batches there are.  torch is imported where a GPU is used, not on import: the CPU
tests and the tools load this module without one, and decode_worker.py never imports it.
"""
import collections
import os

import numpy as np

from . import decode_worker


class ShmTooSmall(RuntimeError):
    """/dev/shm cannot hold the slabs: the caller goes on without its decode workers."""


def open_or_none(factory, line, file=None):
    """factory(), or None where it raises ShmTooSmall: then `line % the reason` is printed, once"""
    try:
        return factory()
    except ShmTooSmall as e:
        print(line % e, file=file, flush=True)
        return None


def _shm_free():
    try:
        s = os.statvfs('/dev/shm')
        return s.f_bavail * s.f_frsize
    except OSError:
        return None


def _settle(futures):
    """cancel what has not started and wait for the rest: none of the tasks writes into a slab afterwards"""
    for f in futures:
        f.cancel()
    for f in futures:
        if not f.cancelled():
            try:
                f.exception()
            except BaseException:
                pass


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
    """n_slabs shared-memory slabs of slab_bytes each, every one registered with the stage (stage.register(shm) -> a
    handle with 'pinned'; stage.unregister(handle); stage.close()), and the worker pool, its own or the one given.
    Raises ShmTooSmall where /dev/shm cannot hold the slabs, before anything else happens: on a tmpfs smaller than
    they are (a container's default is 64 MB) creating a slab still succeeds and the workers die with
    SIGBUS on their first write.  A constructor that fails has closed what it had opened.  close() may be called any
    number of times."""

    def __init__(self, what, slab_bytes, n_slabs, n_procs, stage, pool=None):
        from multiprocessing import shared_memory
        self.stage, self.slots, self.workers = stage, [], None
        free = _shm_free()
        if free is not None and free < n_slabs * slab_bytes + (16 << 20):
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
        _settle(futures)
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


class Layout(object):
    """Where one batch lies in a slab.  fields: (name, per-item shape, dtype) in slab order; every field holds `batch`
    items and starts on a 64-byte boundary.  nbytes: the slab's size."""

    def __init__(self, batch, fields):
        self.B, self.fields, off = int(batch), {}, 0
        for name, shape, dtype in fields:
            dtype = np.dtype(dtype)
            item = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
            self.fields[name] = (off, item, tuple(shape), dtype)
            off = (off + self.B * item + 63) // 64 * 64
        self.nbytes = off

    def offset(self, name, j):
        """the byte at which item j of a field starts"""
        return self.fields[name][0] + j * self.fields[name][1]

    def prefix(self, n):
        """the bytes of a slab that a batch of n items uses"""
        off, item = list(self.fields.values())[-1][:2]
        return off + n * item

    def views(self, buf):
        """the fields of a slab (its buffer) as numpy arrays of `batch` items"""
        a = np.frombuffer(buf, dtype=np.uint8)
        return tuple(a[off:off + self.B * item].view(dtype).reshape((self.B,) + shape)
                     for off, item, shape, dtype in self.fields.values())

    def tensor_views(self, t, n):
        """the first n items of every field in t: a uint8 tensor over a slab, or a copy of at least its prefix(n)"""
        import torch
        return tuple(t[off:off + n * item].view(getattr(torch, dtype.name)).view((n,) + shape)
                     for off, item, shape, dtype in self.fields.values())


class PinnedSlabs(object):
    """Slabs that are uploaded: register() makes a slab pinned host memory (one notice from `who` when that fails:
    same bits, but the upload is a staged copy) and gives a handle {'t': the slab as a uint8 tensor, 'pinned', 'ev':
    the event of its last upload}; wait() returns when that upload has finished."""

    def __init__(self, who):
        import torch
        self.torch, self.who, self.warned = torch, who, False

    def register(self, shm):
        torch = self.torch
        t = torch.frombuffer(shm.buf, dtype=torch.uint8)
        try:
            rc = torch.cuda.cudart().cudaHostRegister(t.data_ptr(), t.numel(), 0)
            pinned = rc is None or int(rc) == 0
        except Exception:
            pinned = False
        if not pinned and not self.warned:
            self.warned = True
            print('%s: the slabs could not be registered as pinned host memory; uploads will not overlap the step'
                  % self.who, flush=True)
        return {'t': t, 'pinned': pinned, 'ev': None}

    def unregister(self, handle):
        if handle['pinned']:
            try:
                self.torch.cuda.cudart().cudaHostUnregister(handle['t'].data_ptr())
            except Exception:
                pass
        handle['t'] = None

    def uploaded(self, handle, stream):
        """the slab's upload has just been enqueued on the stream"""
        handle['ev'] = self.torch.cuda.Event()
        handle['ev'].record(stream)

    def wait(self, handle):
        if handle['ev'] is not None:
            handle['ev'].synchronize()

    def close(self):
        pass


class HostSlabStage(object):
    """A ring's stage without a GPU: on_slab() gets the slab's numpy views and must not keep them."""

    def register(self, shm):
        return {'pinned': False}

    def unregister(self, handle):
        pass

    def wait(self, handle):
        pass

    def run(self, handle, layout, views, n):
        return self.on_slab(tuple(v[:n] for v in views))

    def finish(self, out):
        return out

    def close(self):
        pass


class DeviceSlabStage(PinnedSlabs):
    """A ring's stage on the GPU: one upload of the slab's prefix on a side stream, then on_slab() there with the
    fields as device tensors -> a tuple of tensors.  finish() makes the current stream wait for that batch only."""

    def __init__(self, device, who):
        PinnedSlabs.__init__(self, who)
        self.device = device
        self.side = self.torch.cuda.Stream(device)

    def run(self, handle, layout, views, n):
        torch = self.torch
        with torch.cuda.stream(self.side):
            d = handle['t'][:layout.prefix(n)].to(self.device, non_blocking=True)
            self.uploaded(handle, self.side)
            out = self.on_slab(layout.tensor_views(d, n))
            ready = torch.cuda.Event()
            ready.record(self.side)
        return out, ready

    def finish(self, out):
        tensors, ready = out
        if ready is not None:
            cur = self.torch.cuda.current_stream(self.device)
            cur.wait_event(ready)
            for t in tensors:
                t.record_stream(cur)
        return tensors

    def close(self):
        self.side.synchronize()


class Ring(object):
    """`depth` batches in flight over `depth + 1` slabs (one spare, so a batch is never decoded into the slab whose
    upload was just enqueued), handed out by take() in the order they were submitted.  The loader is a subclass with

      produce(name)            -> (record, tasks) of the next batch, or None when there is none: a dict with 'n', the
                                  number of items, and [(decode_worker function, task)] that write into the slab `name`
      fits(rec, got)           -> whether the tasks' return values say that the batch lies in its slab
      run(rec, handle, views)  -> the staged batch: stage.run on the slab, after whatever the loader adds to it
      host(rec)                -> the staged batch where it does not fit

    stage: a HostSlabStage or a DeviceSlabStage; stage.wait(handle) is called before a slab is decoded into again.
    pool: a WorkerPool to share (another ring's .workers); None: n_procs workers of its own.  Raises ShmTooSmall
    before produce() is ever called.  close() stops the workers and unregisters and unlinks the slabs; call it in a
    finally."""

    def __init__(self, what, layout, depth, n_procs, stage, pool=None):
        self.layout, self.stage, self.B, self.depth = layout, stage, layout.B, int(depth)
        self.pending = collections.deque()
        self.n_host_batches = 0            # batches that did not fit their slab
        self.slabs = Slabs(what, layout.nbytes, self.depth + 1, n_procs, stage, pool)
        self.free = list(self.slabs.slots)
        self.workers = self.slabs.workers
        self.pinned, self.worker_pids = self.slabs.pinned, self.slabs.worker_pids

    def _fill(self):
        while self.free and len(self.pending) < self.depth:
            made = self.produce(self.free[0]['shm'].name)
            if made is None:
                return
            rec, tasks = made
            slot = self.free.pop(0)
            self.stage.wait(slot['handle'])
            rec.update(slot=slot, out=None, futures=[self.slabs.submit(fn, t) for fn, t in tasks])
            self.pending.append(rec)

    def _stage(self, rec):
        """wait for the batch's tasks, stage it, give the slab back"""
        got = [f.result() for f in rec['futures']]
        rec['futures'] = None
        slot, rec['slot'] = rec['slot'], None
        if self.fits(rec, got):
            rec['out'] = self.run(rec, slot['handle'], self.layout.views(slot['shm'].buf))
        else:
            rec['out'] = self.host(rec)
            self.n_host_batches += 1
        self.free.append(slot)

    def take(self):
        """-> the next batch's record with its staged 'out', or None when produce() has no more"""
        self._fill()
        if not self.pending:
            return None
        rec = self.pending.popleft()
        if rec['out'] is None:
            self._stage(rec)
        self._fill()
        # the batch after this one, when its decodes are done already: its upload overlaps this batch's work
        if self.pending and self.pending[0]['out'] is None and all(f.done() for f in self.pending[0]['futures']):
            self._stage(self.pending[0])
            self._fill()
        return rec

    def drain(self):
        """an abandoned pass: its tasks end before their slabs are used again"""
        _settle([f for rec in self.pending for f in (rec['futures'] or ())])
        self.free += [rec['slot'] for rec in self.pending if rec['slot'] is not None]
        self.pending.clear()

    def close(self):
        futures = [f for rec in self.pending for f in (rec['futures'] or ())]
        self.pending.clear()
        self.free = []
        slabs, self.slabs = self.slabs, None
        if slabs is not None:
            slabs.close(futures)
