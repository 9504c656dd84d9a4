"""The tasks of the decode worker PROCESSES: for the labelled driver (input stage of batch_spalign_kmeans.py:486-548:
ResizeImageDataset / ZippedCityscapesRoadDataset decode one PNG per image on the main thread) and for the SegNet
loaders.  The parent's side (slabs, the pool that starts these workers, the ring) is slabs.py.

Threads scale the decode itself (zlib releases the GIL) but every thread still runs PIL's Python-level chunk loop,
and with 32 of them the main thread — which issues ~400 kernel launches per batch from Python — waits 40-100 ms per
batch for the interpreter lock (measured, HISTORY.md section 5).  Worker processes have their own interpreters: they
decode straight into shared-memory slabs the parent has registered as pinned host memory, so a batch goes from PNG
to the GPU with one asynchronous DMA and no copy in the parent.

Imports nothing heavier than numpy and Pillow (a worker must not pull in torch)."""
import os
import zipfile
from multiprocessing import shared_memory

import numpy as np

_SHM = {}            # name -> SharedMemory (attached once per worker)
_ZIP = {}            # path -> ZipFile (opened once per worker)


def _attach(name):
    shm = _SHM.get(name)
    if shm is None:
        shm = shared_memory.SharedMemory(name=name)
        _SHM[name] = shm
    return shm


def _open(src):
    """src: a path, or (zip path, member name)."""
    if isinstance(src, tuple):
        zf = _ZIP.get(src[0])
        if zf is None:
            zf = zipfile.ZipFile(src[0])
            _ZIP[src[0]] = zf
        return zf.open(src[1])
    return src


def decode_into(task):
    """(shm name, byte offset, (H, W, C) expected or None for a 2-D label image, source) -> the decoded shape.
    The frame is written at the offset when its shape is the expected one; the caller falls back otherwise."""
    from PIL import Image
    name, offset, shape, src = task
    with Image.open(_open(src)) as f:
        a = np.asarray(f, dtype=np.uint8)
    if len(shape) == 2:
        a = a if a.ndim == 2 else a[:, :, 0]
    else:
        if a.ndim == 2:
            a = a[:, :, None]
        a = a[:, :, :3]
    if tuple(a.shape) != tuple(shape):
        return tuple(a.shape)
    dst = np.ndarray(shape, dtype=np.uint8, buffer=_attach(name).buf, offset=offset)
    dst[...] = a
    return tuple(a.shape)


def png_into(task):
    """(shm name, byte offset, expected array shape, expected Pillow mode, source) -> (array shape, mode) of the image.
    For a PNG whose mode matters (segnet_loader.LabelLoader): 'RGB' for a frame, (H, W, 3), 'L' for a labelIds image,
    (H, W).  For these two modes np.asarray(f) is what convert('RGB') / convert('L') give, so the image is written at
    the offset only when both its shape and its mode are the expected ones; the caller falls back otherwise."""
    from PIL import Image
    name, offset, shape, mode, src = task
    with Image.open(_open(src)) as f:
        got_mode = f.mode
        got_shape = (f.size[1], f.size[0]) + ((len(f.getbands()),) if len(f.getbands()) > 1 else ())
        if got_mode != mode or got_shape != tuple(shape):
            return got_shape, got_mode
        a = np.asarray(f, dtype=np.uint8)
    dst = np.ndarray(shape, dtype=np.uint8, buffer=_attach(name).buf, offset=offset)
    dst[...] = a
    return tuple(a.shape), got_mode


def label_into(task):
    """(shm name, byte offset, expected shape, (zip path, member name)) -> (shape, dtype string) of the .npy member
    of an npz-style label zip (cli.write_label_zip, run_train_rounds.py): a 2-D road mask of bool or uint8, or a
    float32 (C,H,W) score map.  Its bytes are read straight into the slab at the offset when it is C-ordered, of
    one of those dtypes and of the expected shape; the caller falls back otherwise."""
    from numpy.lib import format as npf
    name, offset, shape, src = task
    with _open(src) as fp:
        version = npf.read_magic(fp)
        head = npf.read_array_header_1_0 if version == (1, 0) else npf.read_array_header_2_0
        a_shape, fortran, dtype = head(fp)
        ok = not fortran and tuple(a_shape) == tuple(shape) and (
            (len(a_shape) == 2 and dtype in (np.dtype(np.bool_), np.dtype(np.uint8)))
            or (len(a_shape) == 3 and dtype == np.dtype('<f4')))
        if ok:
            n = int(np.prod(a_shape)) * dtype.itemsize
            dst = memoryview(_attach(name).buf)[offset:offset + n]
            got = 0
            while got < n:
                k = fp.readinto(dst[got:])
                if not k:
                    raise EOFError('%s: %d of %d bytes' % (src[1], got, n))
                got += k
            dst.release()
    return tuple(a_shape), dtype.str


def die_with_parent(parent_pid):
    """initializer of a pool whose workers must not outlive the process that made it: SIGTERM once the parent is gone
    (Linux PR_SET_PDEATHSIG), and at once if it already is (utils/run_train_rounds.py gives its children the same)"""
    import ctypes
    import signal
    try:
        ctypes.CDLL(None, use_errno=True).prctl(1, int(signal.SIGTERM), 0, 0, 0)      # PR_SET_PDEATHSIG = 1
    except (OSError, AttributeError):
        return
    if os.getppid() != parent_pid:
        os.kill(os.getpid(), signal.SIGTERM)


def warm(_):
    """first task of every worker: import Pillow's PNG plugin now, not inside the first batch"""
    from PIL import Image, PngImagePlugin  # noqa: F401
    return os.getpid()
