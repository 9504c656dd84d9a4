"""The buffer ring under the device encoders (devenc.Ring) on the GPU, driven the way the batch loops drive it: rings
of three images take batches of 3, 3, 1 and 2 different images, every batch is encoded before the files of the one
before it are read (from a worker thread), and every file must be the framed host restatement of its image.  PNG plain
(the wedge masks at 64 x 700, two of them noise so that the lengths differ widely) and through the nearest tables
((37, 53) -> (64, 100)), JPEG at Ri = 1 and 3 on the noise (48 x 80) and MCU (64 x 96) frames; the same again from a
pinned buffer of 16 bytes, which the first fetch() of each set has to replace; and figure.DeviceFigures on a case with
blended panels, whose canvases live in the ring's sets."""
import importlib
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import figure_cases as fc  # noqa: E402
import jpeg_cases as jc  # noqa: E402
import png_cases as pc  # noqa: E402

png = importlib.import_module('superpixel-align_amd.png')
jpeg = importlib.import_module('superpixel-align_amd.jpeg')
figure = importlib.import_module('superpixel-align_amd.figure')
RING = 3
SIZES = (3, 3, 1, 2)                         # the batches; 9 images in all
N = sum(SIZES)
NEAREST_SRC, NEAREST_DST = pc.NEAREST[1]


def wedges():
    rng = np.random.RandomState(7)
    out = [np.roll(pc.wedge(), 41 * k, axis=1) ^ (k & 1) for k in range(N)]
    out[0], out[3] = (rng.randint(0, 256, (2, 64, 700))).astype(np.uint8)     # the first image of batches 0 and 1
    return np.stack(out).astype(np.uint8)


def speckles():
    return (np.random.RandomState(8).rand(N, *NEAREST_SRC) < 0.4).astype(np.uint8) * 7


def mcu_frames():
    base = jc.mcus()
    return np.stack([np.roll(np.roll(base, 16 * (k % 6), axis=1), 16 * (k // 6), axis=0) ^ (255 * (k & 1))
                     for k in range(N)]).astype(np.uint8)


def noise_frames():
    return np.stack([jc.noise(seed=20 + k) for k in range(N)])


class Kind(object):
    """one encoder under test: its images, how to build it, and the file each image must become"""

    def __init__(self, name, images, make, want):
        self.name, self.images, self.make, self.want = name, images, make, want


def png_kind(name, images, shape, tables):
    def want(img):
        stream, adler = png.deflate_rle_host(img, *tables)
        return len(stream), png.assemble(stream, adler, shape[0], shape[1])
    return Kind(name, images, lambda eng, **kw: png.DeviceEncoder(eng, shape, RING, **kw), want)


def jpeg_kind(name, images, Ri):
    H, W = images.shape[1:3]

    def want(frame):
        scan = jpeg.encode_host(frame, Ri)
        return len(scan), jpeg.assemble(scan, H, W, Ri)
    return Kind('%s-Ri%d' % (name, Ri), images, lambda eng, **kw: jpeg.DeviceEncoder(eng, (H, W), RING, Ri, **kw), want)


KINDS = [png_kind('png', wedges(), (64, 700), (None, None)),
         png_kind('png_nearest', speckles(), NEAREST_DST, png.nearest_tables(NEAREST_SRC, NEAREST_DST))] + \
        [jpeg_kind(name, images, Ri) for name, images in (('jpeg_noise', noise_frames()), ('jpeg_mcus', mcu_frames()))
         for Ri in (1, 3)]
kinds = pytest.mark.parametrize('kind', KINDS, ids=[k.name for k in KINDS])


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


@pytest.fixture(scope='module')
def reference():
    """{kind's name: [(payload bytes, file)] of its nine images}, computed once"""
    return {k.name: [k.want(img) for img in k.images] for k in KINDS}


def split(items):
    cuts = np.cumsum((0,) + SIZES)
    return [items[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])]


def padded(lengths):
    return sum((nb + 15) // 16 * 16 for nb in lengths)


def drive(enc, batches, encode=None):
    """The batch loops' protocol -> (the files in order, per batch (the set, its device buffers' addresses), per batch
    whether fetch() replaced the set's pinned buffer)"""
    encode = encode or enc.encode
    files, sets, grew, prev = [], [], [], None

    def read(slot, n):
        return [enc.file_bytes(slot, j) for j in range(n)]

    with ThreadPoolExecutor(1) as pool:
        for src in batches:
            slot = encode(src)                           # the next batch is enqueued ...
            sets.append((slot, {k: v.data_ptr() for k, v in slot.items() if isinstance(v, torch.Tensor) and v.is_cuda}))
            if prev is not None:
                files += pool.submit(read, *prev).result()       # ... before the files of this one are read
            done = torch.cuda.Event()
            done.record()
            done.synchronize()
            before = slot['out_h']
            enc.fetch(slot)
            grew.append(slot['out_h'] is not before)
            prev = (slot, slot['n'])
        files += pool.submit(read, *prev).result()
    return files, sets, grew


def check_sets(sets):
    for k in range(2, len(sets)):
        assert sets[k][0] is sets[k - 2][0] and sets[k][1] == sets[k - 2][1], 'batch %d: not batch %d\'s set' % (k, k - 2)
    for k in range(1, len(sets)):
        assert sets[k][0] is not sets[k - 1][0] and not set(sets[k][1].values()) & set(sets[k - 1][1].values()), k


@kinds
def test_sets_are_reused_while_files_are_read(eng, reference, kind):
    enc = kind.make(eng)
    files, sets, grew = drive(enc, split(torch.from_numpy(kind.images).cuda()))
    want = reference[kind.name]
    assert len(files) == N
    for i in range(N):
        assert files[i] == want[i][1], 'image %d (a ring of %d, batches of %s)' % (i, RING, SIZES)
    check_sets(sets)
    assert enc.downloaded == sum(nb for nb, _ in want) and enc.count == len(SIZES)
    if kind.name.startswith('png'):
        assert not any(grew), 'the PNG ring starts with every row\'s bound pinned: nothing to replace'


@kinds
def test_a_small_pinned_buffer_grows_once_per_set(eng, reference, kind):
    want = reference[kind.name]
    need = [padded(nb for nb, _ in part) for part in split(want)]
    assert 16 < need[2] <= need[0] and 16 < need[3] <= need[1], 'the images no longer fit this test: %s' % need
    enc = kind.make(eng, pinned_bytes=16)
    files, sets, grew = drive(enc, split(torch.from_numpy(kind.images).cuda()))
    assert grew == [True, True, False, False]
    assert [s[0]['out_h'].numel() for s in sets[2:]] == need[:2]
    assert files == [f for _, f in want]
    assert enc.downloaded == sum(nb for nb, _ in want)


def test_figures_compose_into_the_set_they_encode_from(eng):
    c = [c for c in fc.cases() if c.name == 'd3_pitch_batch'][0]
    assert 1 in c.modes and c.B == 3
    canvases = figure.compose_host(*c.args())
    Hc, Wc = canvases.shape[1:3]
    want = [jpeg.assemble(jpeg.encode_host(canvas), Hc, Wc, jpeg.DEFAULT_RI) for canvas in canvases]
    picks = [[0, 1, 2], [1], [2, 0]]                     # three batches of different content, one of a single image
    figs = figure.DeviceFigures(eng, (c.H, c.W), c.B, c.layout, c.d, c.gap)
    frames, planes = torch.from_numpy(c.frames).cuda(), [torch.from_numpy(p).cuda() for p in c.planes]
    batches = [(frames[idx].contiguous(), [p[idx].contiguous() for p in planes], c.luts, c.modes) for idx in picks]
    files, sets, _ = drive(figs, batches, encode=lambda args: figs.encode(*args))
    assert files == [want[i] for idx in picks for i in idx]
    check_sets(sets)
    for slot, ptrs in sets:
        assert ptrs['canvas'] == slot['canvas'].data_ptr() and tuple(slot['canvas'].shape) == (c.B, Hc, Wc, 3)
    assert sets[0][1]['canvas'] != sets[1][1]['canvas'] != sets[2][1]['canvas'] == sets[0][1]['canvas']
    # the canvas the scans were made from is the one composed for that batch: still in its set
    torch.cuda.synchronize()
    assert np.array_equal(sets[2][0]['canvas'][:2].cpu().numpy(), canvases[picks[2]])
    assert np.array_equal(sets[1][0]['canvas'][:1].cpu().numpy(), canvases[picks[1]])
    assert figs.downloaded == sum(len(f) - len(jpeg.header(Hc, Wc, jpeg.DEFAULT_RI)) - 2 for f in files)
