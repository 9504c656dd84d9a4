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

With a frame_cache.FrameCache (train_segnet.py --device_cache_gb) a decoded example is kept where the stage works and
never decoded again: TrainLoader keeps every frame and label array it has staged, by (zip path, member name), and
assembles a batch from a table of addresses that point into the cache or into the uploaded slab (Engine.
segnet_train_input_ptrs / segnet_train_label_ptrs); LabelLoader, whose order is fixed, keeps whole staged batches.  The
draws, the yielded states and the bits are the same; without a cache nothing here runs differently.

Both loaders are a slabs.Ring: the slabs, the workers (one WorkerPool may serve both), the batches in flight and the
close sequence live there, and the stages' registration, upload, wait and finish in slabs.HostSlabStage and
slabs.DeviceSlabStage.  What is here is what differs: the draws or the index order, the slab's fields, the test of the
workers' return values, the host path, and what a stage does with the fields (on_slab).
"""
import numpy as np

from . import decode_worker
from . import segnet_train as st
from .slabs import DeviceSlabStage, HostSlabStage, Layout, Ring, Slabs, WorkerPool, open_or_none  # noqa: F401


def default_depth(n_procs, batchsize):
    """batches in flight: enough image tasks to occupy every worker, plus the batch being uploaded; 3..6"""
    return max(3, min(6, -(-int(n_procs) // max(int(batchsize), 1)) + 1))


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


def _host_batch(batch):
    return np.stack([b[0] for b in batch]), np.stack([b[1] for b in batch])


class HostStage(HostSlabStage):
    """The device stage's work with get_example's own functions: numpy batches in, numpy batches out."""

    def __init__(self, dataset):
        self.ds = dataset

    def on_slab(self, fields):
        imgs, labs, shifts, flips = fields
        out = []
        for j in range(len(imgs)):
            img = imgs[j].astype(np.float32).transpose(2, 0, 1)
            lab = labs[j].astype(np.float32 if self.ds.use_soft_label else np.int32)
            img, lab = self.ds.resized(img, lab)
            if self.ds.random:
                out.append(self.ds.augmented(img, lab, shifts[j], bool(flips[j])))
            else:
                out.append((np.ascontiguousarray(img, np.float32), np.ascontiguousarray(lab)))
        return _host_batch(out)

    from_host = staticmethod(_host_batch)

    def run_cached(self, cache, handle, layout, views, n, src, made, shifts, flips, shapes):
        """a batch whose member j lies in the slab (src[j] = ('slab', slot)) or in the cache (('cache', frame entry,
        label entry)); afterwards the members `made` [(slot, frame entry, label entry)] are copied into the cache"""
        ishape, lshape, ldtype = shapes
        imgs = [views[0][s[1]] if s[0] == 'slab' else cache.view(s[1], ishape, np.uint8) for s in src]
        labs = [views[1][s[1]] if s[0] == 'slab' else cache.view(s[2], lshape, ldtype) for s in src]
        out = self.on_slab((imgs, labs, shifts, flips))
        for j, ef, el in made:
            cache.write(ef, views[0][j])
            cache.write(el, views[1][j])
            cache.commit(ef)
            cache.commit(el)
        return out


class DeviceStage(DeviceSlabStage):
    """The two input kernels on the uploaded slab, on the side stream."""

    def __init__(self, dataset, engine):
        DeviceSlabStage.__init__(self, engine.device, 'segnet_loader')
        self.ds, self.eng = dataset, engine

    def on_slab(self, fields):
        imgs, labs, shifts, flips = fields
        if not self.ds.random:
            shifts = flips = None
        return (self.eng.segnet_train_input(imgs, self.ds.resize_shape, shifts, flips),
                self.eng.segnet_train_label(labs, self.ds.resize_shape, flips))

    def from_host(self, batch):
        return tuple(self.torch.from_numpy(a).to(self.device) for a in _host_batch(batch)), None

    N_ROWS = 8                                       # the pinned ring of batch tables

    def _row(self, n):
        """the next row of the pinned ring, (41 n) bytes: n frame addresses, n label addresses (int64), n x 3 shifts
        (float64), n flips; its last copy to the device has finished"""
        torch = self.torch
        if getattr(self, 'rows', None) is None or self.rows.shape[1] < 41 * n:
            self.rows = torch.empty((self.N_ROWS, (41 * n + 63) // 64 * 64), dtype=torch.uint8).pin_memory()
            self.row_events, self.row_at = [None] * self.N_ROWS, 0
        k, self.row_at = self.row_at, (self.row_at + 1) % self.N_ROWS
        if self.row_events[k] is not None:
            self.row_events[k].synchronize()
        return k, self.rows[k]

    def run_cached(self, cache, handle, layout, views, n, src, made, shifts, flips, shapes):
        """HostStage.run_cached on the device: the slab is uploaded only when a member lies in it; the kernels read
        every member through the batch's table of addresses, which goes up with one non-blocking copy of a pinned
        row together with the draws; the new members are copied into the cache behind the kernels.  All of it on the
        side stream."""
        torch = self.torch
        ishape, lshape, ldtype = shapes
        with torch.cuda.stream(self.side):
            d = None
            if any(s[0] == 'slab' for s in src):
                d = handle['t'][:layout.prefix(n)].to(self.device, non_blocking=True)
                self.uploaded(handle, self.side)
            k, row = self._row(n)
            host = row.numpy()
            addr = host[:16 * n].view(np.int64)
            for j, s in enumerate(src):
                if s[0] == 'slab':
                    addr[j] = d.data_ptr() + layout.offset('frames', s[1])
                    addr[n + j] = d.data_ptr() + layout.offset('labels', s[1])
                else:
                    for e in s[1:]:
                        if e.ready is not None and e.meta['writer'] is not self:
                            self.side.wait_event(e.ready)    # filled on another stage's stream
                    addr[j], addr[n + j] = cache.address(s[1]), cache.address(s[2])
            if self.ds.random:
                host[16 * n:40 * n].view(np.float64)[:] = np.asarray(shifts, np.float64).reshape(-1)
                host[40 * n:41 * n] = flips
            tab = row[:41 * n].to(self.device, non_blocking=True)
            self.row_events[k] = torch.cuda.Event()
            self.row_events[k].record(self.side)
            dshift = dflip = None
            if self.ds.random:
                dshift, dflip = tab[16 * n:40 * n].view(torch.float64).view(n, 3), tab[40 * n:41 * n]
            out = (self.eng.segnet_train_input_ptrs(tab[:8 * n].view(torch.int64), n, ishape[:2], self.ds.resize_shape,
                                                    dshift, dflip),
                   self.eng.segnet_train_label_ptrs(tab[8 * n:16 * n].view(torch.int64), n, lshape, ldtype,
                                                    self.ds.resize_shape, dflip))
            if made:
                fields = layout.tensor_views(d, n)
                for j, ef, el in made:
                    cache.bytes_of(ef).copy_(fields[0][j].reshape(-1), non_blocking=True)
                    cache.bytes_of(el).copy_(fields[1][j].reshape(-1).view(torch.uint8), non_blocking=True)
                filled = torch.cuda.Event()
                filled.record(self.side)
                for j, ef, el in made:
                    cache.commit(ef, filled, {'writer': self})
                    cache.commit(el, filled, {'writer': self})
            ready = torch.cuda.Event()
            ready.record(self.side)
        return out, ready


class TrainLoader(Ring):
    """next() -> (images (B,3,h,w) float32, labels, (iterator state, numpy state) after that batch's draws): the plain
    loop's batches in its order.  dataset: a ZippedEstimatedCityscapesDataset; ids: the rank's example indices
    (train_ids); iterator: the ShuffledIterator the plain loop would call.  stage: a DeviceStage or a HostStage.
    pool: a WorkerPool to share (another loader's .workers); None: n_procs workers of its own.
    cache: a frame_cache.FrameCache of the stage's kind (HostFrameCache with a HostStage, DeviceFrameCache with a
    DeviceStage), which whoever made it closes after the loaders; None: every example is decoded every time.
    Raises slabs.ShmTooSmall where /dev/shm cannot hold the slabs, before anything is drawn.  close() stops the
    workers and unregisters and unlinks the slabs; call it in a finally."""

    def __init__(self, dataset, ids, iterator, n_procs, stage, depth=None, pool=None, cache=None):
        self.ds, self.ids, self.it = dataset, np.asarray(ids), iterator
        self.cache, self.cache_hits, self.cache_misses = cache, 0, 0
        B = int(iterator.batchsize)
        self.ishape, self.lshape = _first_shapes(dataset)
        self.ldtype = np.dtype(np.float32 if dataset.use_soft_label else np.uint8)
        layout = Layout(B, [('frames', self.ishape, np.uint8), ('labels', self.lshape, self.ldtype),
                            ('shifts', (3,), np.float64), ('flips', (), np.uint8)])
        Ring.__init__(self, 'the training loader\'s', layout, depth or default_depth(n_procs, B), n_procs, stage, pool)
        if cache is not None:
            cache.attach(stage)

    def _plan(self, ids):
        """where every member of the batch will be read from, in the order the cache first sees the examples ->
        (src, new, made, deps): src[j] = ('cache', frame entry, label entry) or ('slab', slot); new: the slots to
        decode; made: [(slot, frame entry, label entry)] to fill after staging; deps: entries that an earlier batch in
        flight fills (this loader's own, so they are filled on this stage's stream before this batch reads them)"""
        cache, fields = self.cache, self.layout.fields
        src, new, made, deps, first = [], [], [], [], {}
        for j, i in enumerate(ids):
            i = int(i)
            kf, kl = (self.ds.img_zip_fn, self.ds.img_fns[i]), (self.ds.label_zip_fn, self.ds.label_fns[i])
            ef, el = cache.lookup(kf), cache.lookup(kl)
            if (ef is None or el is None) and i not in first:
                ef, el = cache.pending(kf, self), cache.pending(kl, self)
                if ef is not None and el is not None:
                    deps += [ef, el]
            if i in first:
                src.append(('slab', first[i]))
            elif ef is not None and el is not None:
                src.append(('cache', ef, el))
            else:
                first[i] = j
                new.append(j)
                src.append(('slab', j))
                got = cache.reserve([(kf, fields['frames'][1]), (kl, fields['labels'][1])], self)
                if got is not None:
                    made.append((j, got[0], got[1]))
                cache.note(False)
                self.cache_misses += 1
                continue
            cache.note(True)
            self.cache_hits += 1
        return src, new, made, deps

    def produce(self, name):
        """the draws of the next batch, in the plain loop's order, and its decode tasks"""
        ids = self.ids[self.it.next_indices()]
        shifts = flips = None
        if self.ds.random:
            shifts, flips = np.empty((len(ids), 3), np.float64), np.empty(len(ids), np.uint8)
            for j in range(len(ids)):
                shifts[j] = st.pca_lighting_shift(np.random.normal(0, 25.5, size=3))
                flips[j] = np.random.rand() > 0.5
        state = ({k: np.array(v) for k, v in self.it.state().items()}, np.random.get_state())
        at = self.layout.offset
        rec = {'n': len(ids), 'ids': ids, 'shifts': shifts, 'flips': flips, 'state': state}
        new = range(len(ids))
        if self.cache is not None:
            rec['src'], new, rec['made'], rec['deps'] = self._plan(ids)
            rec['new'] = new
        tasks = [(decode_worker.decode_into, (name, at('frames', j), self.ishape,
                                              (self.ds.img_zip_fn, self.ds.img_fns[ids[j]]))) for j in new]
        tasks += [(decode_worker.label_into, (name, at('labels', j), self.lshape,
                                              (self.ds.label_zip_fn, self.ds.label_fns[ids[j]]))) for j in new]
        return rec, tasks

    def fits(self, rec, got):
        n = rec['n']
        if self.cache is not None:
            n = len(rec['new'])
            if not all(e.committed for e in rec['deps']):       # the batch that was to fill them took the host path
                return False
        return all(tuple(g) == self.ishape for g in got[:n]) and all(
            tuple(g[0]) == self.lshape and (np.dtype(g[1]) == self.ldtype or
                                            (self.ldtype == np.uint8 and np.dtype(g[1]) == np.bool_)) for g in got[n:])

    def run(self, rec, handle, views):
        if self.cache is not None:
            made, rec['made'] = rec['made'], []
            return self.stage.run_cached(self.cache, handle, self.layout, views, rec['n'], rec['src'], made,
                                         rec['shifts'], rec['flips'], (self.ishape, self.lshape, self.ldtype))
        if self.ds.random:
            views[2][:rec['n']] = rec['shifts']
            views[3][:rec['n']] = rec['flips']
        return self.stage.run(handle, self.layout, views, rec['n'])

    def _give_up(self, rec):
        """the batch's reservations will not be filled"""
        for _, ef, el in rec.get('made') or ():
            self.cache.release(ef)
            self.cache.release(el)
        rec['made'] = []

    def host(self, rec):
        """a batch with another shape: the dataset's host functions with the draws already made"""
        self._give_up(rec)
        batch = []
        for j, i in enumerate(rec['ids']):
            img, lab = self.ds.resized(*self.ds.decoded(i))
            if self.ds.random:
                batch.append(self.ds.augmented(img, lab, rec['shifts'][j], bool(rec['flips'][j])))
            else:
                batch.append((np.ascontiguousarray(img, np.float32), np.ascontiguousarray(lab)))
        return self.stage.from_host(batch)

    def next(self):
        rec = self.take()
        img, lab = self.stage.finish(rec['out'])
        return img, lab, rec['state']

    def close(self):
        for rec in self.pending:
            self._give_up(rec)
        Ring.close(self)


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


class HostLabelStage(HostSlabStage):
    """numpy in, numpy out, no GPU: copies of the slab's frames and label ids."""

    def on_slab(self, fields):
        return tuple(f.copy() for f in fields)

    def cached(self, cache, e, layout, n):
        """the fields of a cached batch: read-only arrays over the cache"""
        return tuple(cache.view(e, (n,) + shape, dtype, off) for off, _, shape, dtype in layout.fields.values())

    def run_into(self, cache, e, handle, layout, views, n, meta):
        """the slab's batch straight into its cache entry"""
        for v, (off, _, _, _) in zip(views, layout.fields.values()):
            cache.write(e, v[:n], off)
        cache.commit(e, None, meta)
        return self.cached(cache, e, layout, n)


class DeviceLabelStage(DeviceSlabStage):
    """The uploaded frames and label ids as they are."""

    def __init__(self, engine):
        DeviceSlabStage.__init__(self, engine.device, 'segnet_loader')

    def on_slab(self, fields):
        return fields

    def cached(self, cache, e, layout, n):
        """the fields of a cached batch: tensors over the cache, and the event after which they are filled"""
        return layout.tensor_views(cache.bytes_of(e), n), e.ready

    def run_into(self, cache, e, handle, layout, views, n, meta):
        """the slab's upload straight into its cache entry, on the side stream"""
        torch = self.torch
        with torch.cuda.stream(self.side):
            cache.bytes_of(e, 0, layout.prefix(n)).copy_(handle['t'][:layout.prefix(n)], non_blocking=True)
            self.uploaded(handle, self.side)
            ready = torch.cuda.Event()
            ready.record(self.side)
        cache.commit(e, ready, meta)
        return self.cached(cache, e, layout, n)


class LabelLoader(Ring):
    """The frames and labelIds images of a ZippedCityscapesRoadDataset's examples `indices`, in order, in batches of
    `batchsize` (the last may be short), decoded by workers a few batches ahead (default_depth) into slabs: what
    labels_from_segnet.save_labels and train_segnet.evaluate read with get_raw, one image after the other.
    batches() yields LabelBatch objects; it may be called again for another pass over the same indices.  A batch with
    a frame or label of another shape than the first example's, or of another mode than RGB / L (for which np.asarray
    of the decoded image is not what get_raw's convert() gives), is marked host.  stage: a DeviceLabelStage or a
    HostLabelStage.  pool: a WorkerPool to share (a TrainLoader's .workers).  keep_ids: every batch also carries a
    numpy copy of its label ids.  cache: a frame_cache.FrameCache of the stage's kind; a staged batch that the budget
    admits whole is kept in it under its members' names, and every later pass yields it from there, read-only for the
    consumer, without a task or an upload.  Raises slabs.ShmTooSmall like TrainLoader; close() in a finally."""

    def __init__(self, dataset, indices, batchsize, n_procs, stage, depth=None, pool=None, keep_ids=False, cache=None):
        self.ds, self.indices, self.pos = dataset, [int(i) for i in indices], 0
        self.cache, self.cache_hits, self.cache_misses, self.first_pass_misses, self.passes = cache, 0, 0, 0, 0
        self.keep_ids = bool(keep_ids)
        B = max(int(batchsize), 1)
        self.ishape, self.lshape = _first_png_shapes(dataset) if self.indices else ((1, 1, 3), (1, 1))
        layout = Layout(B, [('frames', self.ishape, np.uint8), ('label_ids', self.lshape, np.uint8)])
        Ring.__init__(self, 'the label loader\'s', layout, depth or default_depth(n_procs, B), n_procs, stage, pool)
        if cache is not None:
            cache.attach(stage)

    def _cached(self, ids):
        """-> (the batch's key, its committed entry or None)"""
        key = ((self.ds.img_zip_fn, self.ds.label_zip_fn),
               tuple(self.ds.img_fns[i] for i in ids) + tuple(self.ds.label_fns[i] for i in ids))
        e = self.cache.lookup(key)
        if e is not None and self.keep_ids and e.meta.get('ids_host') is None:
            e = None                                            # kept by a loader that needed no host copy
        self.cache.note(e is not None)
        if e is not None:
            self.cache_hits += 1
        else:
            self.cache_misses += 1
            self.first_pass_misses += self.passes <= 1
        return key, e

    def produce(self, name):
        ids = self.indices[self.pos:self.pos + self.B]
        if not ids:
            return None
        self.pos += len(ids)
        if self.cache is not None:
            key, e = self._cached(ids)
            if e is not None:
                return {'n': len(ids), 'batch': LabelBatch(ids), 'entry': e}, []
        at = self.layout.offset
        tasks = [(name, at('frames', j), self.ishape, 'RGB', (self.ds.img_zip_fn, self.ds.img_fns[i]))
                 for j, i in enumerate(ids)]
        tasks += [(name, at('label_ids', j), self.lshape, 'L', (self.ds.label_zip_fn, self.ds.label_fns[i]))
                  for j, i in enumerate(ids)]
        rec = {'n': len(ids), 'batch': LabelBatch(ids)}
        if self.cache is not None:
            rec['key'] = key
        return rec, [(decode_worker.png_into, t) for t in tasks]

    def fits(self, rec, got):
        if rec.get('entry') is not None:
            return True
        want = [(self.ishape, 'RGB')] * rec['n'] + [(self.lshape, 'L')] * rec['n']
        return all((tuple(g[0]), g[1]) == w for g, w in zip(got, want))

    def run(self, rec, handle, views):
        n = rec['n']
        if rec.get('entry') is not None:
            rec['batch'].ids_host = rec['entry'].meta.get('ids_host') if self.keep_ids else None
            return self.stage.cached(self.cache, rec['entry'], self.layout, n)
        if self.keep_ids:
            rec['batch'].ids_host = views[1][:n].copy()
        if self.cache is not None:
            got = self.cache.reserve([(rec['key'], self.layout.prefix(n))], self)
            if got is not None:
                meta = {'writer': self.stage, 'ids_host': rec['batch'].ids_host}
                return self.stage.run_into(self.cache, got[0], handle, self.layout, views, n, meta)
        return self.stage.run(handle, self.layout, views, n)

    def host(self, rec):
        rec['batch'].host = True
        return ()

    def batches(self):
        self.drain()
        self.pos = 0
        self.passes += 1
        while True:
            rec = self.take()
            if rec is None:
                return
            batch = rec['batch']
            if not batch.host:
                batch.frames, batch.label_ids = self.stage.finish(rec['out'])
            yield batch

    __iter__ = batches
