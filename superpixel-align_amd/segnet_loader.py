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


class TrainLoader(Ring):
    """next() -> (images (B,3,h,w) float32, labels, (iterator state, numpy state) after that batch's draws): the plain
    loop's batches in its order.  dataset: a ZippedEstimatedCityscapesDataset; ids: the rank's example indices
    (train_ids); iterator: the ShuffledIterator the plain loop would call.  stage: a DeviceStage or a HostStage.
    pool: a WorkerPool to share (another loader's .workers); None: n_procs workers of its own.
    Raises slabs.ShmTooSmall where /dev/shm cannot hold the slabs, before anything is drawn.  close() stops the
    workers and unregisters and unlinks the slabs; call it in a finally."""

    def __init__(self, dataset, ids, iterator, n_procs, stage, depth=None, pool=None):
        self.ds, self.ids, self.it = dataset, np.asarray(ids), iterator
        B = int(iterator.batchsize)
        self.ishape, self.lshape = _first_shapes(dataset)
        self.ldtype = np.dtype(np.float32 if dataset.use_soft_label else np.uint8)
        layout = Layout(B, [('frames', self.ishape, np.uint8), ('labels', self.lshape, self.ldtype),
                            ('shifts', (3,), np.float64), ('flips', (), np.uint8)])
        Ring.__init__(self, 'the training loader\'s', layout, depth or default_depth(n_procs, B), n_procs, stage, pool)

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
        tasks = [(decode_worker.decode_into, (name, at('frames', j), self.ishape,
                                              (self.ds.img_zip_fn, self.ds.img_fns[i]))) for j, i in enumerate(ids)]
        tasks += [(decode_worker.label_into, (name, at('labels', j), self.lshape,
                                              (self.ds.label_zip_fn, self.ds.label_fns[i]))) for j, i in enumerate(ids)]
        return {'n': len(ids), 'ids': ids, 'shifts': shifts, 'flips': flips, 'state': state}, tasks

    def fits(self, rec, got):
        n = rec['n']
        return all(tuple(g) == self.ishape for g in got[:n]) and all(
            tuple(g[0]) == self.lshape and (np.dtype(g[1]) == self.ldtype or
                                            (self.ldtype == np.uint8 and np.dtype(g[1]) == np.bool_)) for g in got[n:])

    def run(self, rec, handle, views):
        if self.ds.random:
            views[2][:rec['n']] = rec['shifts']
            views[3][:rec['n']] = rec['flips']
        return self.stage.run(handle, self.layout, views, rec['n'])

    def host(self, rec):
        """a batch with another shape: the dataset's host functions with the draws already made"""
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


class DeviceLabelStage(DeviceSlabStage):
    """The uploaded frames and label ids as they are."""

    def __init__(self, engine):
        DeviceSlabStage.__init__(self, engine.device, 'segnet_loader')

    def on_slab(self, fields):
        return fields


class LabelLoader(Ring):
    """The frames and labelIds images of a ZippedCityscapesRoadDataset's examples `indices`, in order, in batches of
    `batchsize` (the last may be short), decoded by workers a few batches ahead (default_depth) into slabs: what
    labels_from_segnet.save_labels and train_segnet.evaluate read with get_raw, one image after the other.
    batches() yields LabelBatch objects; it may be called again for another pass over the same indices.  A batch with
    a frame or label of another shape than the first example's, or of another mode than RGB / L (for which np.asarray
    of the decoded image is not what get_raw's convert() gives), is marked host.  stage: a DeviceLabelStage or a
    HostLabelStage.  pool: a WorkerPool to share (a TrainLoader's .workers).  keep_ids: every batch also carries a
    numpy copy of its label ids.  Raises slabs.ShmTooSmall like TrainLoader; close() in a finally."""

    def __init__(self, dataset, indices, batchsize, n_procs, stage, depth=None, pool=None, keep_ids=False):
        self.ds, self.indices, self.pos = dataset, [int(i) for i in indices], 0
        self.keep_ids = bool(keep_ids)
        B = max(int(batchsize), 1)
        self.ishape, self.lshape = _first_png_shapes(dataset) if self.indices else ((1, 1, 3), (1, 1))
        layout = Layout(B, [('frames', self.ishape, np.uint8), ('label_ids', self.lshape, np.uint8)])
        Ring.__init__(self, 'the label loader\'s', layout, depth or default_depth(n_procs, B), n_procs, stage, pool)

    def produce(self, name):
        ids = self.indices[self.pos:self.pos + self.B]
        if not ids:
            return None
        self.pos += len(ids)
        at = self.layout.offset
        tasks = [(name, at('frames', j), self.ishape, 'RGB', (self.ds.img_zip_fn, self.ds.img_fns[i]))
                 for j, i in enumerate(ids)]
        tasks += [(name, at('label_ids', j), self.lshape, 'L', (self.ds.label_zip_fn, self.ds.label_fns[i]))
                  for j, i in enumerate(ids)]
        return {'n': len(ids), 'batch': LabelBatch(ids)}, [(decode_worker.png_into, t) for t in tasks]

    def fits(self, rec, got):
        want = [(self.ishape, 'RGB')] * rec['n'] + [(self.lshape, 'L')] * rec['n']
        return all((tuple(g[0]), g[1]) == w for g, w in zip(got, want))

    def run(self, rec, handle, views):
        if self.keep_ids:
            rec['batch'].ids_host = views[1][:rec['n']].copy()
        return self.stage.run(handle, self.layout, views, rec['n'])

    def host(self, rec):
        rec['batch'].host = True
        return ()

    def batches(self):
        self.drain()
        self.pos = 0
        while True:
            rec = self.take()
            if rec is None:
                return
            batch = rec['batch']
            if not batch.host:
                batch.frames, batch.label_ids = self.stage.finish(rec['out'])
            yield batch

    __iter__ = batches
