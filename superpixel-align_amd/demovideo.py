"""The demo-video stage: utils/create_demovideo.py (a trained SegNet-Basic over the Cityscapes demoVideo frames, one
label PNG per frame) and utils/create_movie.py (the road colour blended into every frame, an MJPG .avi), without
Chainer and OpenCV.

label_frames is the reference's loop, batched.  Per batch the decoded uint8 frames are uploaded once; on the device
Engine.segnet_train_input makes the network's input (the reference reads the frame as float32 and resizes it with order
3: the float-image cubic resize the training dataset pins, host form segnet_train.resize_bicubic_float), the network
runs with logits=True (the reference's predict() without return_score resizes the classifier's raw scores and takes
their argmax: SegNetBasic.predict_labels), and one launch makes the mask -- Engine.segnet_score, or with a video
Engine.segnet_overlay, which blends the road colour into the frames that are on the device already.  Masks and blended
frames come back into one of two pinned buffer sets, and the host writes batch k-1's files while batch k is on the
device.  With loader_procs > 0 the frames are decoded by worker processes into pinned shared-memory slabs (slabs.Ring,
decode_worker.png_into), a few batches ahead.  With png_encoder='device' (--png_encoder device) the mask is not
downloaded: png.DeviceEncoder makes the PNG's compressed payload from it on the device and only those bytes come back.
With jpeg_encoder='device' (--jpeg_encoder device) and a video the blended frames are not downloaded either:
jpeg.DeviceEncoder makes each frame's entropy-coded scan on the device (this project's baseline JPEG at quality 75, not
Pillow's bytes), and the writer threads frame the scans that come back.

blend_host is create_movie.py's numpy statement, MjpegAviWriter a plain RIFF AVI of Pillow-encoded JPEG frames, and
write_movie the reference's second script on them.  What is pinned: the labels (the argmax of Pillow's BILINEAR resize
of the raw scores), the blend (numpy's arithmetic, every byte value), the container's structure, 30 fps and the frame
size.  What is not: OpenCV's own PNG and JPEG bytes (no cv2 here), and quality 75 is what OpenCV's MJPEG writer is
believed to use.
"""
import collections
import glob
import io
import os
import struct
import time

import numpy as np

from . import decode_worker
from . import jpeg
from . import png
from .slabs import DeviceSlabStage, Layout, Ring, open_or_none

ROAD_COLOR = (128, 64, 128)          # create_movie.py:23 (symmetric: the same in OpenCV's BGR and in RGB)
ALPHA = 0.5                          # create_movie.py:22
RIFF_LIMIT = (1 << 32) - 1           # what a 32-bit RIFF size field holds


def demo_frames(demoVideo_dir):
    """create_demovideo.py:58: the frames in the reference's order"""
    return sorted(glob.glob(os.path.join(demoVideo_dir, '*', '*.png')))


def read_frame(fn):
    """chainercv.utils.read_image's values as bytes: the file converted to RGB, (H,W,3) uint8"""
    from PIL import Image
    with Image.open(fn) as f:
        return np.asarray(f.convert('RGB'), dtype=np.uint8)


def blend_host(frame, mask, color=ROAD_COLOR, alpha=ALPHA):
    """create_movie.py:33-37 on a copy of frame (H,W,3) uint8: where mask (H,W) == 1 the road colour is blended in,
    img[pred == 1] = alpha * pred_color[pred == 1] + (1 - alpha) * img[pred == 1] in float64, truncated to uint8 by
    the assignment.  The host form of Engine.segnet_overlay."""
    img = np.array(frame, dtype=np.uint8)
    pred = np.asarray(mask)
    pred_color = np.zeros((img.shape[0], img.shape[1], 3))
    pred_color[pred == 1] = color
    img[pred == 1] = alpha * pred_color[pred == 1] + (1 - alpha) * img[pred == 1]
    return img


def encode_jpeg(frame, quality=75):
    """(H,W,3) uint8 RGB -> the bytes of Pillow's baseline JPEG at that quality (the same bytes for the same frame)"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, format='JPEG', quality=int(quality))
    return buf.getvalue()


def write_label_png(fn, mask):
    """the label as cv.imwrite stores the int32 0/1 array: an 8-bit single-channel PNG, at zlib level 1 (OpenCV's
    default for PNG; the pixels are the contract, the compressed bytes are not)"""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(mask, dtype=np.uint8)).save(fn, format='PNG', compress_level=1)


class MjpegAviWriter(object):
    """cv.VideoWriter(fn, fourcc('MJPG'), fps, size) as a plain RIFF AVI: LIST hdrl (avih; LIST strl: strh 'vids' /
    'MJPG', strf a 24-bit BITMAPINFOHEADER with compression 'MJPG'), LIST movi of '00dc' chunks padded to even length,
    then idx1 (offsets from the 'movi' tag).  size = (width, height) as OpenCV takes it; write() takes (height, width,
    3) uint8 RGB frames and raises on another shape (OpenCV drops such a frame silently).  Frames are JPEG-encoded with
    Pillow in encode_threads threads and stored in the order of the write() calls; write() copies nothing, so the frame
    must stay as it is until flush() or close() returns.  write_encoded() stores the bytes of a ready JPEG file as the
    next frame, after every frame given to write() before it.  The counts and sizes are patched in by close().  Raises
    ValueError before a chunk would take the file past what 32-bit RIFF sizes hold (riff_limit)."""
    HEADER_BYTES = 224               # everything before the first chunk

    def __init__(self, fn, size, fps=30.0, quality=75, encode_threads=4, riff_limit=RIFF_LIMIT):
        from concurrent.futures import ThreadPoolExecutor
        self.width, self.height = int(size[0]), int(size[1])
        if self.width <= 0 or self.height <= 0 or not float(fps) > 0:
            raise ValueError('MjpegAviWriter: size %r, fps %r' % (size, fps))
        self.fps, self.quality, self.riff_limit = float(fps), int(quality), int(riff_limit)
        # the rate as a fraction: 30.0 -> 30 / 1, 29.97 -> 29970 / 1000
        self.scale = 1 if self.fps == int(self.fps) else 1000
        self.rate = int(round(self.fps * self.scale))
        self.index = []              # (offset from the 'movi' tag, chunk bytes) per frame
        self.max_chunk = 0
        self.pending = collections.deque()
        self.pool = ThreadPoolExecutor(max_workers=max(int(encode_threads), 1))
        self.depth = 2 * max(int(encode_threads), 1)
        self.fp = open(fn, 'wb')
        self.fp.write(self._header())
        self.pos = self.HEADER_BYTES

    def _header(self):
        n, movi = len(self.index), 4 + self._movi_bytes()
        total = self.HEADER_BYTES + self._movi_bytes() + 8 + 16 * n
        avih = struct.pack('<14I', int(round(1e6 / self.fps)), int(self.max_chunk * self.fps), 0, 0x10, n, 0, 1,
                           self.max_chunk, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack('<4s4sIHHIIIIIIII4H', b'vids', b'MJPG', 0, 0, 0, 0, self.scale, self.rate, 0, n,
                           self.max_chunk, 0xffffffff, 0, 0, 0, self.width, self.height)
        strf = struct.pack('<IiiHH4sIiiII', 40, self.width, self.height, 1, 24, b'MJPG',
                           self.width * self.height * 3, 0, 0, 0, 0)
        strl = b'strl' + b'strh' + struct.pack('<I', len(strh)) + strh + b'strf' + struct.pack('<I', len(strf)) + strf
        hdrl = b'hdrl' + b'avih' + struct.pack('<I', len(avih)) + avih + b'LIST' + struct.pack('<I', len(strl)) + strl
        head = (b'RIFF' + struct.pack('<I', total - 8) + b'AVI ' + b'LIST' + struct.pack('<I', len(hdrl)) + hdrl +
                b'LIST' + struct.pack('<I', movi) + b'movi')
        assert len(head) == self.HEADER_BYTES
        return head

    def _movi_bytes(self):
        return self.pos - self.HEADER_BYTES if self.index else 0

    def write(self, frame):
        if self.fp is None:
            raise ValueError('MjpegAviWriter: the file is closed')
        if not (isinstance(frame, np.ndarray) and frame.dtype == np.uint8
                and frame.shape == (self.height, self.width, 3)):
            raise ValueError('MjpegAviWriter: a frame must be (%d, %d, 3) uint8, got %s %s'
                             % (self.height, self.width, getattr(frame, 'shape', None), getattr(frame, 'dtype', None)))
        self.pending.append(self.pool.submit(encode_jpeg, frame, self.quality))
        while len(self.pending) > self.depth:
            self._store(self.pending.popleft().result())

    def write_encoded(self, data):
        """the next frame is `data`, a whole JPEG file (SOI ... EOI) of the writer's frame size; the caller answers for
        the size.  Frames still being encoded for write() are stored first."""
        if self.fp is None:
            raise ValueError('MjpegAviWriter: the file is closed')
        if not (isinstance(data, (bytes, bytearray)) and len(data) >= 4 and bytes(data[:2]) == b'\xff\xd8'
                and bytes(data[-2:]) == b'\xff\xd9'):
            raise ValueError('MjpegAviWriter: write_encoded takes the bytes of a JPEG file, SOI to EOI')
        self.flush()
        self._store(bytes(data))

    def _store(self, data):
        padded = len(data) + (len(data) & 1)
        if self.pos + 8 + padded + 8 + 16 * (len(self.index) + 1) > self.riff_limit:
            raise ValueError('MjpegAviWriter: frame %d would take the file past %d bytes, the limit of 32-bit RIFF sizes'
                             % (len(self.index), self.riff_limit))
        self.fp.write(b'00dc' + struct.pack('<I', len(data)) + data + b'\0' * (padded - len(data)))
        self.index.append((self.pos - (self.HEADER_BYTES - 4), len(data)))
        self.max_chunk = max(self.max_chunk, len(data))
        self.pos += 8 + padded

    def flush(self):
        """every frame given to write() so far is encoded and in the file"""
        while self.pending:
            self._store(self.pending.popleft().result())

    def close(self):
        if self.fp is None:
            return
        try:
            self.flush()
            self.fp.write(b'idx1' + struct.pack('<I', 16 * len(self.index)))
            for off, n in self.index:
                self.fp.write(b'00dc' + struct.pack('<III', 0x10, off, n))       # AVIIF_KEYFRAME
            self.fp.seek(0)
            self.fp.write(self._header())
        finally:
            for f in self.pending:
                f.cancel()
            self.pending.clear()
            self.pool.shutdown(wait=True)
            fp, self.fp = self.fp, None
            fp.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def write_movie(pred_label_dir, img_dir, out_video_fn, alpha=ALPHA, color=ROAD_COLOR, size=(2048, 1024), fps=30.0,
                quality=75, encode_threads=4):
    """create_movie.py: sorted(img_dir/*/*.png) zipped with sorted(pred_label_dir/*.png) (the shorter list ends the
    movie), each frame blended on the host where its label is 1 and appended to out_video_fn.  -> the frame count."""
    from PIL import Image
    img_fns = demo_frames(img_dir)
    pred_fns = sorted(glob.glob(os.path.join(pred_label_dir, '*.png')))
    n = 0
    with MjpegAviWriter(out_video_fn, size, fps, quality, encode_threads) as out:
        for img_fn, pred_fn in zip(img_fns, pred_fns):
            with Image.open(pred_fn) as f:
                pred = np.asarray(f.convert('L'), dtype=np.uint8)
            out.write(blend_host(read_frame(img_fn), pred, color, alpha))
            n += 1
    return n


# ------------------------------------------------------------------------------- the frames, decoded ahead
def _frame_info(fn):
    """((H, W), Pillow mode) from the file's header"""
    from PIL import Image
    with Image.open(fn) as f:
        return (f.size[1], f.size[0]), f.mode


class FrameLoader(Ring):
    """The frames frame_fns in order, in batches of `batchsize` (the last may be short), decoded by n_procs worker
    processes a few batches ahead into pinned slabs and uploaded on a side stream.  batches() yields (file names,
    frames (n,H,W,3) uint8 on the device), or (file names, None) for a batch that holds a frame of another size than
    `shape` or of another mode than RGB: the caller decodes that one itself.  Raises slabs.ShmTooSmall where /dev/shm
    cannot hold the slabs; close() in a finally."""

    def __init__(self, frame_fns, shape, batchsize, n_procs, engine, depth=None):
        from .segnet_loader import default_depth
        self.fns, self.pos = list(frame_fns), 0
        self.ishape = (int(shape[0]), int(shape[1]), 3)
        B = max(int(batchsize), 1)
        stage = DeviceSlabStage(engine.device, 'demovideo')
        stage.on_slab = lambda fields: fields
        Ring.__init__(self, 'the frame loader\'s', Layout(B, [('frames', self.ishape, np.uint8)]),
                      depth or default_depth(n_procs, B), n_procs, stage)

    def produce(self, name):
        fns = self.fns[self.pos:self.pos + self.B]
        if not fns:
            return None
        self.pos += len(fns)
        tasks = [(decode_worker.png_into, (name, self.layout.offset('frames', j), self.ishape, 'RGB', fn))
                 for j, fn in enumerate(fns)]
        return {'n': len(fns), 'fns': fns}, tasks

    def fits(self, rec, got):
        return all((tuple(g[0]), g[1]) == (self.ishape, 'RGB') for g in got)

    def run(self, rec, handle, views):
        return self.stage.run(handle, self.layout, views, rec['n'])

    def host(self, rec):
        rec['host'] = True
        return ()

    def batches(self):
        while True:
            rec = self.take()
            if rec is None:
                return
            yield rec['fns'], (None if rec.get('host') else self.stage.finish(rec['out'])[0])


def label_frames(model, frame_fns, out_dir, input_shape=(512, 1024), pred_shape=(1024, 2048), batchsize=4,
                 loader_procs=0, video=None, encode_threads=4, color=ROAD_COLOR, alpha=ALPHA, stats=None,
                 png_encoder='pillow', jpeg_encoder='pillow', jpeg_restart=None):
    """create_demovideo.py:57-64 over frame_fns with model (a segnet.SegNetBasic): <out_dir>/<basename(frame)> = the
    label of SegNetBasic.predict_labels for the frame resized to input_shape (an 8-bit single-channel PNG of 0 / 1 at
    pred_shape), and with video (an MjpegAviWriter of size (pred W, pred H)) create_movie.py's frame appended to it, the
    blend made on the device in the launch that makes the mask.  loader_procs N > 0: N worker processes decode the
    frames ahead; the outputs are the same, byte for byte.  encode_threads: threads that write the PNGs.  With video a
    frame whose size is not pred_shape is refused (ValueError) before any file is written.  stats: a dict that
    receives loop_s, n_batches, n_host_batches and the seconds spent waiting for the loader (loader_wait_s), waiting for
    the device (device_wait_s) and writing (output_s).  png_encoder 'device': the PNG's compressed payload is made
    on the device from the mask where it is (png.DeviceEncoder; the same pixels in another stream), the mask itself is
    not downloaded, and with a stats dict png_payload_bytes counts what was.  jpeg_encoder 'device' (with video only;
    pred_shape a multiple of 16): the blended frames stay on the device, jpeg.DeviceEncoder makes their scans there in
    restart intervals of jpeg_restart MCUs (jpeg.DEFAULT_RI), only the scans come back, the writer threads make them
    files (jpeg.assemble) and the video takes them in order (write_encoded); the pinned blended ring is not
    allocated, and with a stats dict jpeg_payload_bytes counts what was downloaded.  -> the number of frames."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    clock = time.perf_counter
    eng = model.engine
    frame_fns = list(frame_fns)
    input_shape = tuple(int(v) for v in input_shape)
    pred_shape = tuple(int(v) for v in pred_shape)
    B = max(int(batchsize), 1)
    if png_encoder not in ('pillow', 'device'):
        raise ValueError('label_frames: png_encoder must be pillow or device, got %r' % (png_encoder,))
    if jpeg_encoder not in ('pillow', 'device'):
        raise ValueError('label_frames: jpeg_encoder must be pillow or device, got %r' % (jpeg_encoder,))
    enc = png.DeviceEncoder(eng, pred_shape, B) if png_encoder == 'device' else None
    jenc = None
    if jpeg_encoder == 'device' and video is not None:
        jenc = jpeg.DeviceEncoder(eng, pred_shape, B, jpeg.DEFAULT_RI if jpeg_restart is None else jpeg_restart)
    first = None
    if video is not None:
        if (video.height, video.width) != pred_shape:
            raise ValueError('label_frames: the video is %d x %d, pred_shape %s' % (video.width, video.height, pred_shape))
        for fn in frame_fns:
            if _frame_info(fn)[0] != pred_shape:
                raise ValueError('label_frames: %s is %s, not pred_shape %s: it cannot go into the video'
                                 % (fn, _frame_info(fn)[0], pred_shape))
        first = pred_shape
    elif frame_fns:
        first = _frame_info(frame_fns[0])[0]
    if not os.path.exists(out_dir):
        os.makedirs(out_dir, exist_ok=True)

    ring = [{'mask': torch.empty((B,) + pred_shape, dtype=torch.uint8).pin_memory() if enc is None else None,
             'blended': torch.empty((B,) + pred_shape + (3,), dtype=torch.uint8).pin_memory()
             if video is not None and jenc is None else None} for _ in range(2)]
    times = {'loader_wait_s': 0.0, 'device_wait_s': 0.0, 'output_s': 0.0}
    pending, count = [None], [0, 0]
    png_pool = ThreadPoolExecutor(max_workers=max(int(encode_threads), 1))

    def flush():
        rec, pending[0] = pending[0], None
        if rec is None:
            return
        t0 = clock()
        rec['event'].synchronize()
        t1 = clock()
        if enc is None:
            mask_h = rec['buf']['mask'].numpy()
            jobs = [png_pool.submit(write_label_png, os.path.join(out_dir, os.path.basename(fn)), mask_h[j])
                    for j, fn in enumerate(rec['fns'])]
        else:
            # the lengths are here: only the used bytes come down, on the encoder's stream; the writers wait for them
            enc.fetch(rec['slot'])
            jobs = [png_pool.submit(lambda j=j, fn=fn: png.write_file(os.path.join(out_dir, os.path.basename(fn)),
                                                                      enc.file_bytes(rec['slot'], j)))
                    for j, fn in enumerate(rec['fns'])]
        if jenc is not None:
            # as for the PNGs: the scans' used bytes come down on the encoder's stream, the writers frame them
            jenc.fetch(rec['jslot'])
            files = [png_pool.submit(jenc.file_bytes, rec['jslot'], j) for j in range(len(rec['fns']))]
            for job in files:
                video.write_encoded(job.result())
        elif video is not None:
            blended_h = rec['buf']['blended'].numpy()
            for j in range(len(rec['fns'])):
                video.write(blended_h[j])
            video.flush()
        for job in jobs:
            job.result()
        times['device_wait_s'] += t1 - t0
        times['output_s'] += clock() - t1

    def submit(frames, fns):
        """frames (n,H,W,3) uint8 on the device: the chain of one batch, then the files of the batch before it"""
        n = len(fns)
        x = eng.segnet_train_input(frames, input_shape)
        z = model.forward(x, logits=True)
        buf = ring[count[0] % 2]
        count[0] += 1
        slot = jslot = None
        if video is not None:
            mask, blended = eng.segnet_overlay(z, frames, color, alpha)
            if jenc is None:
                buf['blended'][:n].copy_(blended, non_blocking=True)
            else:
                jslot = jenc.encode(blended)
        else:
            mask, _ = eng.segnet_score(z, pred_shape)
        if enc is None:
            buf['mask'][:n].copy_(mask, non_blocking=True)
        else:
            slot = enc.encode(mask)
        event = torch.cuda.Event()
        event.record()
        flush()
        pending[0] = {'fns': fns, 'buf': buf, 'event': event, 'slot': slot, 'jslot': jslot}

    def host_batch(fns):
        """decoded here; frames of one size that follow each other share a chain"""
        frames = [read_frame(fn) for fn in fns]
        lo = 0
        for hi in range(1, len(fns) + 1):
            if hi == len(fns) or frames[hi].shape != frames[lo].shape:
                submit(torch.from_numpy(np.stack(frames[lo:hi])).to(eng.device), fns[lo:hi])
                lo = hi

    loader = None
    if int(loader_procs) > 0 and frame_fns:
        loader = open_or_none(lambda: FrameLoader(frame_fns, first, B, int(loader_procs), eng),
                              '--loader_procs: %s; the frames are decoded on the host')
    t_loop = clock()
    try:
        if loader is None:
            for lo in range(0, len(frame_fns), B):
                host_batch(frame_fns[lo:lo + B])
        else:
            batches = loader.batches()
            while True:
                t0 = clock()
                got = next(batches, None)
                times['loader_wait_s'] += clock() - t0
                if got is None:
                    break
                fns, frames = got
                if frames is None:
                    count[1] += 1
                    host_batch(fns)
                else:
                    submit(frames, fns)
        flush()
    finally:
        if loader is not None:
            loader.close()
        png_pool.shutdown(wait=True)
    if stats is not None:
        stats.update(times, loop_s=clock() - t_loop, n_batches=count[0], n_host_batches=count[1])
        if enc is not None:
            stats['png_payload_bytes'] = enc.downloaded
        if jenc is not None:
            stats['jpeg_payload_bytes'] = jenc.downloaded
    return len(frame_fns)


# ------------------------------------------------------------------------------- the two drivers
def _non_negative(v):
    import argparse
    n = int(v)
    if n < 0:
        raise argparse.ArgumentTypeError('must be >= 0, got %d' % n)
    return n


def demovideo_parser():
    """create_demovideo.py's flags and defaults, then the additions"""
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument('--snapshot', type=str)
    parser.add_argument('--out_dir', type=str)
    parser.add_argument('--gpu', type=int, default=-1)
    parser.add_argument('--demoVideo_dir', type=str, default='data/cityscapes/leftImg8bit/demoVideo')
    parser.add_argument('--batchsize', type=int, default=4)
    parser.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    parser.add_argument('--split_planes', action='store_true', default=False)
    parser.add_argument('--loader_procs', type=_non_negative, default=0,
                        help='decode worker processes that feed the network; 0: the loop decodes every frame itself')
    parser.add_argument('--input_shape', type=int, nargs=2, default=[512, 1024])
    parser.add_argument('--eval_shape', type=int, nargs=2, default=[1024, 2048])
    parser.add_argument('--out_video_fn', type=str, default=None,
                        help='also write create_movie.py\'s video, in the same pass')
    parser.add_argument('--encode_threads', type=int, default=4)
    parser.add_argument('--png_encoder', type=str, default='pillow', choices=['pillow', 'device'],
                        help='device: the label PNGs\' compressed payload is made on the device (the same pixels)')
    parser.add_argument('--jpeg_encoder', type=str, default='pillow', choices=['pillow', 'device'],
                        help='device: with --out_video_fn the video\'s JPEG frames are encoded on the device (baseline '
                             'JPEG at quality 75 with restart markers; not Pillow\'s bytes); --eval_shape must be '
                             'multiples of 16')
    return parser


def demovideo_main(argv=None):
    import torch
    from . import segnet
    parser = demovideo_parser()
    args = parser.parse_args(argv)
    if args.split_planes and args.dtype != 'fp32':
        parser.error('--split_planes is the float32-accurate mode: it cannot be combined with --dtype %s' % args.dtype)
    if args.jpeg_encoder == 'device' and args.out_video_fn and (args.eval_shape[0] % 16 or args.eval_shape[1] % 16):
        parser.error('--jpeg_encoder device encodes frames whose sides are multiples of 16, not --eval_shape %d %d'
                     % tuple(args.eval_shape))
    device = max(int(args.gpu), 0)                       # -1, the reference's CPU mode: device 0 (there is no CPU path)
    torch.cuda.set_device(device)
    model = segnet.SegNetBasic.from_snapshot_file(args.snapshot, pred_shape=args.eval_shape, device=device,
                                                  dtype=args.dtype, split_planes=args.split_planes)
    video = None
    if args.out_video_fn:
        video = MjpegAviWriter(args.out_video_fn, (args.eval_shape[1], args.eval_shape[0]),
                               encode_threads=args.encode_threads)
    try:
        return label_frames(model, demo_frames(args.demoVideo_dir), args.out_dir, args.input_shape, args.eval_shape,
                            args.batchsize, args.loader_procs, video, args.encode_threads,
                            png_encoder=args.png_encoder, jpeg_encoder=args.jpeg_encoder)
    finally:
        if video is not None:
            video.close()


def movie_parser():
    """create_movie.py's flags and defaults"""
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument('--pred_label_dir', type=str)
    parser.add_argument('--img_dir', type=str, default='data/cityscapes/leftImg8bit/demoVideo')
    parser.add_argument('--out_video_fn', type=str, default='results/preds_labels.avi')
    parser.add_argument('--size', type=int, nargs=2, default=[2048, 1024], metavar=('WIDTH', 'HEIGHT'),
                        help='the frame size (the reference hard-codes 2048 1024)')
    parser.add_argument('--encode_threads', type=int, default=4)
    return parser


def movie_main(argv=None):
    args = movie_parser().parse_args(argv)
    return write_movie(args.pred_label_dir, args.img_dir, args.out_video_fn, size=tuple(args.size),
                       encode_threads=args.encode_threads)
