"""--jpeg_encoder device on the GPU.  Engine.jpeg_encode (spa_jpeg_encode_rgb8) against jpeg.encode_host on the frames
of jpeg_cases.py at every restart interval, alone and in batches of three different frames: the scan and its length,
byte for byte, twice into a buffer filled with 0xFF, of which every byte at or past nbytes must stay 0xFF; one pair of
256x512 frames at Ri = 1 (512 intervals a frame: more than the scan workgroup has threads, and 1024 MCUs for the
transform's workgroups of four); the refusals, which launch nothing; and label_frames with the video encoded on the
device: every AVI chunk is the framed restatement of the host blend, the PNGs are the pillow run's.  The host
restatement itself is held to Pillow in test_jpeg_device_cpu.py."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as jc  # noqa: E402
import segnet_train_synth as syn  # noqa: E402
from segnet_ref import random_params  # noqa: E402

jpeg = importlib.import_module('superpixel-align_amd.jpeg')
dv = importlib.import_module('superpixel-align_amd.demovideo')
segnet = importlib.import_module('superpixel-align_amd.segnet')
SpalignError = importlib.import_module('superpixel-align_amd._lib').SpalignError
CASES = jc.cases()
SLACK = 64                                   # bytes of stride past the bound
PARAMS = [(name, frame, Ri) for name, frame in CASES for Ri in jc.intervals_for(frame)]


def batch_of(frame):
    """three different frames of one shape: the case, its negative, and it turned by 180 degrees"""
    return np.stack([frame, 255 - frame, np.ascontiguousarray(frame[::-1, ::-1])])


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


@pytest.fixture(scope='module')
def reference():
    """{(name, Ri): the scans of batch_of(frame)}, computed once"""
    return {(name, Ri): [jpeg.encode_host(f, Ri) for f in batch_of(frame)] for name, frame, Ri in PARAMS}


def encode_twice_and_compare(eng, frames, Ri, want):
    B, H, W = frames.shape[:3]
    bound = jpeg.scan_bound(H, W, Ri)
    assert int(eng._lib.spa_jpeg_scan_bound(H, W, Ri)) == bound
    stride = bound + SLACK
    src = torch.from_numpy(frames).cuda()
    out = torch.empty((B, stride), dtype=torch.uint8, device='cuda')
    nbytes = torch.empty((B,), dtype=torch.int32, device='cuda')
    coef = torch.empty((B * H * W * 3 // 2,), dtype=torch.int16, device='cuda')
    for _ in range(2):
        out.fill_(0xFF)
        nbytes.fill_(-1)
        coef.fill_(0x5555)
        got = eng.jpeg_encode(src, Ri, out=out, nbytes=nbytes, coef=coef)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out.data_ptr()
        out_h, n_h = out.cpu().numpy(), nbytes.cpu().numpy()
        for b, scan in enumerate(want):
            n = int(n_h[b])
            assert n == len(scan) and n <= bound, (b, n, len(scan))
            assert out_h[b, :n].tobytes() == scan, b
            assert (out_h[b, n:] == 0xFF).all(), 'frame %d: a byte at or past nbytes was written' % b
    return coef


@pytest.mark.parametrize('name,frame,Ri', PARAMS, ids=['%s-%d' % (p[0], p[2]) for p in PARAMS])
def test_scan_and_length_are_the_restatement(eng, reference, name, frame, Ri):
    want = reference[name, Ri]
    coef = encode_twice_and_compare(eng, batch_of(frame), Ri, want)
    # what the transform left: the restatement's coefficients
    for b, f in enumerate(batch_of(frame)):
        n = f.shape[0] * f.shape[1] * 3 // 2
        assert np.array_equal(coef[b * n:(b + 1) * n].cpu().numpy().reshape(-1, 6, 64), jpeg.mcu_coefficients(f)), b
    encode_twice_and_compare(eng, frame[None], Ri, want[:1])


def test_more_intervals_than_scan_threads(eng):
    frames = np.stack([jc.noise(5, (256, 512)), jc.smooth((256, 512))])
    encode_twice_and_compare(eng, frames, 1, [jpeg.encode_host(f, 1) for f in frames])


def test_a_frame_at_an_odd_address(eng):
    """the transform's byte loads: frames that start 1 byte into an allocation"""
    frame = jc.noise(9, (32, 48))
    flat = torch.zeros((frame.size + 16,), dtype=torch.uint8, device='cuda')
    view = flat[1:1 + frame.size].view(1, 32, 48, 3)
    view.copy_(torch.from_numpy(frame))
    assert view.data_ptr() % 4 == 1
    out, nbytes = eng.jpeg_encode(view, 2)
    n = int(nbytes[0])
    assert out[0, :n].cpu().numpy().tobytes() == jpeg.encode_host(frame, 2)


def test_engine_owned_buffers_are_reused_and_make_files(eng):
    frames = batch_of(jc.smooth())
    src = torch.from_numpy(frames).cuda()
    ptrs = set()
    for _ in range(2):
        out, nbytes = eng.jpeg_encode(src)
        ptrs.add(out.data_ptr())
        n_h, out_h = nbytes.cpu().numpy(), out.cpu().numpy()
        for b in range(3):
            data = jpeg.assemble(out_h[b, :int(n_h[b])].tobytes(), 64, 96, jpeg.DEFAULT_RI)
            assert jc.psnr(frames[b], jc.decode(data)) > 35
    assert len(ptrs) == 1, 'the encode buffer was allocated again'


def test_refusals_launch_nothing(eng):
    lib, ctx = eng._lib, eng._ctx
    fn = lib.spa_jpeg_encode_rgb8
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    src = torch.zeros((2, 32, 48, 3), dtype=torch.uint8, device='cuda')
    bound = jpeg.scan_bound(32, 48, 2)
    out = torch.full((2, bound), 0xFF, dtype=torch.uint8, device='cuda')
    nb = torch.full((2,), -1, dtype=torch.int32, device='cuda')
    coef = torch.full((2 * 6 * 384,), 0x5555, dtype=torch.int16, device='cuda')
    assert fn(ctx, P(src), 2, 32, 48, 2, P(coef), P(out), bound, P(nb), s) == 0
    torch.cuda.synchronize()
    assert int(nb[0]) > 0
    out.fill_(0xFF)
    nb.fill_(-1)
    coef.fill_(0x5555)
    got = [
        fn(ctx, None, 2, 32, 48, 2, P(coef), P(out), bound, P(nb), s),                 # a NULL pointer
        fn(ctx, P(src), 2, 32, 48, 2, None, P(out), bound, P(nb), s),
        fn(ctx, P(src), 2, 32, 48, 2, P(coef), None, bound, P(nb), s),
        fn(ctx, P(src), 2, 32, 48, 2, P(coef), P(out), bound, None, s),
        fn(ctx, P(src), 2, 24, 48, 2, P(coef), P(out), bound, P(nb), s),               # not multiples of 16
        fn(ctx, P(src), 2, 32, 40, 2, P(coef), P(out), bound, P(nb), s),
        fn(ctx, P(src), 2, 0, 48, 2, P(coef), P(out), bound, P(nb), s),
        fn(ctx, P(src), 0, 32, 48, 2, P(coef), P(out), bound, P(nb), s),
        fn(ctx, P(src), 2, 32, 48, 0, P(coef), P(out), bound, P(nb), s),               # Ri < 1
        fn(ctx, P(src), 2, 32, 48, 2, P(coef), P(out), bound - 1, P(nb), s),           # a stride below the bound
        fn(ctx, P(src), 2, 32, 48, 1, P(coef), P(out), bound, P(nb), s),               # Ri = 1 needs 2 bytes more
        # 2^16 x 2^15 pixels may need 2^23 * 2490 bytes: more than nbytes holds
        fn(ctx, P(src), 1, 1 << 16, 1 << 15, 8, P(coef), P(out), 1 << 40, P(nb), s),
    ]
    torch.cuda.synchronize()
    assert got == [-1] * len(got)
    assert bool((out == 0xFF).all()) and bool((nb == -1).all()) and bool((coef == 0x5555).all())
    with pytest.raises(SpalignError):
        eng.jpeg_encode(src, 2, out=out[:, :bound - 1])
    with pytest.raises(SpalignError):
        eng.jpeg_encode(src[:, :24], 2)
    with pytest.raises(SpalignError):
        eng.jpeg_encode(src.float())
    with pytest.raises(SpalignError):
        eng.jpeg_encode(src, 0)


# ------------------------------------------------------------------------------- the demo-video stage
IN_SHAPE, PRED_SHAPE = (32, 64), (64, 128)


def read_png(fn):
    from PIL import Image
    with Image.open(fn) as f:
        assert f.mode == 'L'
        return np.asarray(f)


def test_label_frames_with_the_video_encoded_on_the_device(eng, tmp_path):
    from test_demovideo_cpu import parse_avi
    root = str(tmp_path)
    rng = np.random.default_rng(92)
    for i in range(6):
        city = 'ulm_%02d' % (i // 3)
        os.makedirs(os.path.join(root, 'demoVideo', city), exist_ok=True)
        img, _ = syn.image(PRED_SHAPE[0], PRED_SHAPE[1], rng)
        with open(os.path.join(root, 'demoVideo', city, '%s_000000_%06d_leftImg8bit.png' % (city, i)), 'wb') as f:
            f.write(syn.png(img, None))
    fns = dv.demo_frames(os.path.join(root, 'demoVideo'))
    assert len(fns) == 6
    model = segnet.SegNetBasic(random_params(91), pred_shape=PRED_SHAPE, engine=eng)
    size = (PRED_SHAPE[1], PRED_SHAPE[0])
    runs = {'pillow': {}, 'device': dict(jpeg_encoder='device'),
            'device_procs': dict(jpeg_encoder='device', loader_procs=2),
            'device_both': dict(jpeg_encoder='device', png_encoder='device'),
            'device_ri3': dict(jpeg_encoder='device', jpeg_restart=3)}
    for name, kw in runs.items():
        stats = {}
        with dv.MjpegAviWriter(os.path.join(root, name + '.avi'), size) as w:
            assert dv.label_frames(model, fns, os.path.join(root, name), IN_SHAPE, PRED_SHAPE, batchsize=4, video=w,
                                   stats=stats, **kw) == 6
        assert ('jpeg_payload_bytes' in stats) == (name != 'pillow')
        runs[name] = stats
    # without a video the flag changes nothing
    stats = {}
    dv.label_frames(model, fns, os.path.join(root, 'no_video'), IN_SHAPE, PRED_SHAPE, batchsize=4, stats=stats,
                    jpeg_encoder='device')
    assert 'jpeg_payload_bytes' not in stats
    with pytest.raises(ValueError, match='jpeg_encoder'):
        dv.label_frames(model, fns, os.path.join(root, 'x'), IN_SHAPE, PRED_SHAPE, jpeg_encoder='turbo')
    with dv.MjpegAviWriter(os.path.join(root, 'odd.avi'), (72, 64)) as w:
        with pytest.raises(ValueError, match='multiple of 16'):
            dv.label_frames(model, [], os.path.join(root, 'y'), IN_SHAPE, (64, 72), video=w, jpeg_encoder='device')

    masks, some_road = [], False
    for fn in fns:
        name = os.path.basename(fn)
        a = read_png(os.path.join(root, 'pillow', name))
        masks.append(a)
        some_road = some_road or 0 < a.mean() < 1
        for d in ('device', 'device_procs', 'no_video', 'device_ri3'):
            assert open(os.path.join(root, d, name), 'rb').read() == open(os.path.join(root, 'pillow', name), 'rb').read()
        assert np.array_equal(read_png(os.path.join(root, 'device_both', name)), a)
    assert some_road
    blends = [dv.blend_host(dv.read_frame(fn), m) for fn, m in zip(fns, masks)]
    pillow = parse_avi(open(os.path.join(root, 'pillow.avi'), 'rb').read())
    assert pillow['frames'] == [dv.encode_jpeg(b) for b in blends]
    for name, Ri in (('device', jpeg.DEFAULT_RI), ('device_procs', jpeg.DEFAULT_RI), ('device_both', jpeg.DEFAULT_RI),
                     ('device_ri3', 3)):
        a = parse_avi(open(os.path.join(root, name + '.avi'), 'rb').read())
        assert a['avih'][4] == 6 and a['avih'][8:10] == size and len(a['index']) == 6
        want = [jpeg.assemble(jpeg.encode_host(b, Ri), PRED_SHAPE[0], PRED_SHAPE[1], Ri) for b in blends]
        assert a['frames'] == want, name
        for k in range(6):
            assert a['index'][k][3] == len(want[k]) and a['movi'] + a['index'][k][2] == a['chunk_at'][k]
        # the scans and nothing else came down
        assert runs[name]['jpeg_payload_bytes'] == sum(len(jpeg.encode_host(b, Ri)) for b in blends)
    assert open(os.path.join(root, 'device.avi'), 'rb').read() == open(os.path.join(root, 'device_procs.avi'), 'rb').read()
    assert jc.decode(a['frames'][0]).shape == PRED_SHAPE + (3,)
