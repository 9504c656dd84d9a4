"""CPU tests of the demo-video stage (superpixel-align_amd/demovideo.py, utils/create_demovideo.py,
utils/create_movie.py): the host blend against create_movie.py's numpy statement, the RIFF structure of the MJPG AVI
(parsed here), write_movie's pairing, the label without a softmax against the label of the probabilities, and the two
drivers' flags."""
import importlib
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

dv = importlib.import_module('superpixel-align_amd.demovideo')
segnet = importlib.import_module('superpixel-align_amd.segnet')


# ------------------------------------------------------------------------------- the blend
def every_byte_frame():
    """(16, 48, 3): every byte value in every channel, each channel in another order"""
    v = np.arange(256, dtype=np.uint8)
    frame = np.stack([v, v[::-1], np.roll(v, 37)], -1).reshape(16, 16, 3)
    return np.ascontiguousarray(np.concatenate([frame, frame[::-1], frame[:, ::-1]], 1))


@pytest.mark.parametrize('alpha', [0.5, 0.3, 0.7])
def test_blend_host_is_the_numpy_statement(alpha):
    img = every_byte_frame()
    rng = np.random.default_rng(3)
    pred = (rng.random(img.shape[:2]) < 0.6).astype(np.uint8)
    pred[:, :16] = 1                                                  # every byte value under the road
    pred[0, 16:20] = 2                                                # neither 0 nor 1: left alone
    road_color = [128, 64, 128]
    got = dv.blend_host(img, pred, road_color, alpha)
    # create_movie.py:33-37, verbatim
    want = img.copy()
    pred_color = np.zeros((want.shape[0], want.shape[1], 3))
    pred_color[pred == 1] = road_color
    want[pred == 1] = alpha * pred_color[pred == 1] \
        + (1 - alpha) * want[pred == 1]
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(got[pred != 1], img[pred != 1])
    assert not np.shares_memory(got, img)
    if alpha == 0.5:                                                  # the reference's constants: color / 2 + (v >> 1)
        road = np.array(road_color, np.uint8) // 2 + (img >> 1)
        assert np.array_equal(got[pred == 1], road[pred == 1])


# ------------------------------------------------------------------------------- the AVI
def chunks(data, lo, hi):
    """[(fourcc, payload offset, payload size)] of the RIFF chunks in data[lo:hi]"""
    out = []
    while lo < hi:
        cc, n = data[lo:lo + 4], struct.unpack('<I', data[lo + 4:lo + 8])[0]
        out.append((cc, lo + 8, n))
        lo += 8 + n + (n & 1)
    assert lo == hi
    return out


def parse_avi(data):
    """-> dict(avih, strh, strf: the fields, frames: [JPEG bytes], index: [(fourcc, flags, offset, size)], movi: the
    position of the 'movi' tag); asserts the nesting and every size on the way"""
    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    assert struct.unpack('<I', data[4:8])[0] == len(data) - 8
    top = chunks(data, 12, len(data))
    assert [c[0] for c in top] == [b'LIST', b'LIST', b'idx1']
    (_, h0, hn), (_, m0, mn), (_, i0, inn) = top
    assert data[h0:h0 + 4] == b'hdrl' and data[m0:m0 + 4] == b'movi'
    hdrl = chunks(data, h0 + 4, h0 + hn)
    assert [c[0] for c in hdrl] == [b'avih', b'LIST']
    assert hdrl[0][2] == 56
    avih = struct.unpack('<14I', data[hdrl[0][1]:hdrl[0][1] + 56])
    s0, sn = hdrl[1][1], hdrl[1][2]
    assert data[s0:s0 + 4] == b'strl'
    strl = chunks(data, s0 + 4, s0 + sn)
    assert [(c[0], c[2]) for c in strl] == [(b'strh', 56), (b'strf', 40)]
    strh = struct.unpack('<4s4sIHHIIIIIIII4H', data[strl[0][1]:strl[0][1] + 56])
    strf = struct.unpack('<IiiHH4sIiiII', data[strl[1][1]:strl[1][1] + 40])
    movi = chunks(data, m0 + 4, m0 + mn)
    assert all(c[0] == b'00dc' for c in movi)
    index = [struct.unpack('<4sIII', data[i0 + 16 * k:i0 + 16 * k + 16]) for k in range(inn // 16)]
    assert inn == 16 * len(index)
    return dict(avih=avih, strh=strh, strf=strf, frames=[data[o:o + n] for _, o, n in movi], index=index, movi=m0,
                chunk_at=[o - 8 for _, o, n in movi])


def test_avi_structure(tmp_path):
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (48, 64, 3), dtype=np.uint8) for _ in range(2)]
    frames.append(np.full((48, 64, 3), 200, np.uint8))               # compresses to another (odd or even) length
    fn = str(tmp_path / 'a.avi')
    w = dv.MjpegAviWriter(fn, (64, 48), quality=60, encode_threads=2)
    for f in frames:
        w.write(f)
    with pytest.raises(ValueError, match='must be'):
        w.write(np.zeros((64, 48, 3), np.uint8))                      # (width, height) swapped
    with pytest.raises(ValueError, match='must be'):
        w.write(np.zeros((48, 64, 3), np.float32))
    w.close()
    w.close()                                                         # a second close is nothing
    data = open(fn, 'rb').read()
    a = parse_avi(data)
    # avih: microseconds per frame, flags HASINDEX, frame count, one stream, width, height
    assert a['avih'][0] == 33333 and a['avih'][3] & 0x10 and a['avih'][4] == 3 and a['avih'][6] == 1
    assert a['avih'][8:10] == (64, 48)
    # strh: vids / MJPG, rate / scale = 30, length; strf: 24-bit MJPG of the frame size
    assert a['strh'][0] == b'vids' and a['strh'][1] == b'MJPG'
    assert a['strh'][7] == 30 * a['strh'][6] and a['strh'][9] == 3
    assert a['strf'][:6] == (40, 64, 48, 1, 24, b'MJPG')
    # the frames: Pillow's bytes at that quality, in order; the index points at each chunk
    assert len(a['frames']) == 3 == len(a['index'])
    for k, f in enumerate(frames):
        assert a['frames'][k] == dv.encode_jpeg(f, 60)
        cc, flags, off, n = a['index'][k]
        assert cc == b'00dc' and flags & 0x10 and n == len(a['frames'][k])
        assert a['movi'] + off == a['chunk_at'][k]
        assert a['chunk_at'][k] % 2 == 0                              # padded to even length
    # default quality 75, and the same bytes whatever the number of threads
    for threads in (1, 3):
        fn2 = str(tmp_path / ('b%d.avi' % threads))
        with dv.MjpegAviWriter(fn2, (64, 48), encode_threads=threads) as w2:
            for f in frames:
                w2.write(f)
        b = parse_avi(open(fn2, 'rb').read())
        assert b['frames'] == [dv.encode_jpeg(f, 75) for f in frames]


def test_avi_refuses_a_file_past_the_riff_limit(tmp_path):
    frame = np.random.default_rng(6).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    one = len(dv.encode_jpeg(frame))
    one += one & 1
    # room for exactly two frames and their index, not for a third
    limit = dv.MjpegAviWriter.HEADER_BYTES + 2 * (8 + one) + 8 + 2 * 16
    w = dv.MjpegAviWriter(str(tmp_path / 'c.avi'), (64, 48), riff_limit=limit)
    w.write(frame)
    w.write(frame)
    w.flush()
    w.write(frame)
    with pytest.raises(ValueError, match='32-bit RIFF'):
        w.flush()
    w.close()
    a = parse_avi(open(str(tmp_path / 'c.avi'), 'rb').read())         # what was stored is a whole file
    assert len(a['frames']) == 2 and a['avih'][4] == 2
    assert dv.RIFF_LIMIT == 2 ** 32 - 1


def test_empty_avi_is_well_formed(tmp_path):
    fn = str(tmp_path / 'e.avi')
    dv.MjpegAviWriter(fn, (64, 48)).close()
    a = parse_avi(open(fn, 'rb').read())
    assert a['frames'] == [] and a['avih'][4] == 0


# ------------------------------------------------------------------------------- write_movie
def movie_tree(root, n_frames, n_labels, H=48, W=64):
    rng = np.random.default_rng(7)
    frames, labels = [], []
    for i in range(n_frames):
        city = 'stuttgart_%02d' % (i % 2)
        os.makedirs(os.path.join(root, 'demoVideo', city), exist_ok=True)
        img, m = syn.image(H, W, rng)
        name = '%s_000000_%06d_leftImg8bit.png' % (city, i)
        with open(os.path.join(root, 'demoVideo', city, name), 'wb') as f:
            f.write(syn.png(img))
        frames.append((os.path.join(city, name), img))
    frames.sort()
    os.makedirs(os.path.join(root, 'labels'), exist_ok=True)
    for k in range(n_labels):
        lab = (rng.random((H, W)) < 0.5).astype(np.uint8)
        dv.write_label_png(os.path.join(root, 'labels', os.path.basename(frames[k][0])), lab)
        labels.append(lab)
    return [f[1] for f in frames], labels


@pytest.mark.parametrize('n_frames,n_labels', [(4, 4), (5, 3), (2, 0)])
def test_write_movie_pairs_sorted_lists(tmp_path, n_frames, n_labels):
    root = str(tmp_path)
    frames, labels = movie_tree(root, n_frames, n_labels)
    fn = os.path.join(root, 'm.avi')
    n = dv.write_movie(os.path.join(root, 'labels'), os.path.join(root, 'demoVideo'), fn, size=(64, 48))
    a = parse_avi(open(fn, 'rb').read())
    assert n == min(n_frames, n_labels) == len(a['frames'])           # zip: the shorter list ends the movie
    for k in range(n):
        assert a['frames'][k] == dv.encode_jpeg(dv.blend_host(frames[k], labels[k]))
    if n_labels == 4:                                                 # a label PNG is 8-bit, single-channel, 0 / 1
        from PIL import Image
        with Image.open(os.path.join(root, 'labels', sorted(os.listdir(os.path.join(root, 'labels')))[0])) as f:
            assert f.mode == 'L' and set(np.unique(np.asarray(f))) <= {0, 1}
        # the driver as a child process: the same file
        fn2 = os.path.join(root, 'm2.avi')
        syn.run_python([os.path.join(ROOT, 'utils', 'create_movie.py'), '--pred_label_dir', os.path.join(root, 'labels'),
                        '--img_dir', os.path.join(root, 'demoVideo'), '--out_video_fn', fn2, '--size', '64', '48'],
                       cwd=root, timeout=120)
        assert open(fn2, 'rb').read() == open(fn, 'rb').read()


def test_write_movie_refuses_a_frame_of_another_size(tmp_path):
    root = str(tmp_path)
    movie_tree(root, 2, 2)
    with pytest.raises(ValueError, match='must be'):
        dv.write_movie(os.path.join(root, 'labels'), os.path.join(root, 'demoVideo'), os.path.join(root, 'm.avi'))


# ------------------------------------------------------------------------------- the label without a softmax
def test_logits_label_differs_from_probability_label():
    """columns alternate a very confident road pixel (scores 0, 20) and a mildly confident other pixel (3, 0).  At a
    2x upscale Pillow mixes them 1 : 3.  Raw scores: 0.25 * 20 > 0.75 * 3, road.  Probabilities saturate: 0.25 * 1 +
    0.75 * 0.047 < 0.75 * 0.953, not road."""
    z = np.zeros((2, 4, 8), np.float32)
    z[1, :, 0::2] = 20.0
    z[0, :, 1::2] = 3.0
    e = np.exp(z - z.max(0, keepdims=True))
    prob = (e / e.sum(0, keepdims=True)).astype(np.float32)
    label = lambda s: (lambda r: (r[1] > r[0]).astype(np.int32))(segnet.resize_bilinear_pil(s, (8, 16)))
    from_logits, from_prob = label(z), label(prob)
    assert (from_logits != from_prob).any()
    assert from_logits.sum() > from_prob.sum()                        # the confident pixels reach further
    # at the scores' own size there is nothing to mix: the two agree
    same = lambda s: (s[1] > s[0]).astype(np.int32)
    assert np.array_equal(same(z), same(prob))


# ------------------------------------------------------------------------------- the snapshot file and the flags
def test_read_snapshot_shares_load_snapshot_checks(tmp_path):
    rng = np.random.default_rng(8)
    p = {}
    for i, name in enumerate(segnet.LAYERS):
        p[name + '/W'] = rng.standard_normal((64, 3 if i == 0 else 64, 7, 7)).astype(np.float32)
        for k in segnet.BN_PARAMS:
            p['%s_bn/%s' % (name, k)] = rng.uniform(0.5, 1.5, 64).astype(np.float32)
    p['conv_classifier/W'] = rng.standard_normal((2, 64, 1, 1)).astype(np.float32)
    p['conv_classifier/b'] = rng.standard_normal(2).astype(np.float32)
    d = str(tmp_path)
    fn = os.path.join(d, 'snapshot_iter_7')
    with open(fn, 'wb') as f:
        np.savez(f, **{segnet.PREFIX + k: v for k, v in p.items()})
    got = segnet.read_snapshot(fn)
    assert set(got) == set(p) and all(np.array_equal(got[k], p[k]) for k in p)
    with open(os.path.join(d, 'args.txt'), 'w') as f:
        f.write('{"model": "basic", "input_shape": [32, 64]}')
    _, path, via_dir = segnet.load_snapshot(d, 7)
    assert path == fn and all(np.array_equal(via_dir[k], p[k]) for k in p)
    bad = os.path.join(d, 'short')
    with open(bad, 'wb') as f:
        np.savez(f, **{segnet.PREFIX + k: v for k, v in p.items() if k != 'conv_classifier/b'})
    with pytest.raises(KeyError, match='conv_classifier/b'):
        segnet.read_snapshot(bad)
    with open(bad, 'wb') as f:
        np.savez(f, **{segnet.PREFIX + k: (v[:1] if k == 'conv3/W' else v) for k, v in p.items()})
    with pytest.raises(ValueError, match='conv3/W'):
        segnet.read_snapshot(bad)


def test_driver_flags_keep_the_reference_defaults():
    a = dv.demovideo_parser().parse_args(['--snapshot', 's', '--out_dir', 'o'])
    assert (a.snapshot, a.out_dir, a.gpu, a.demoVideo_dir) == ('s', 'o', -1, 'data/cityscapes/leftImg8bit/demoVideo')
    assert (a.batchsize, a.dtype, a.split_planes, a.loader_procs) == (4, 'fp32', False, 0)
    assert (a.input_shape, a.eval_shape, a.out_video_fn, a.encode_threads) == ([512, 1024], [1024, 2048], None, 4)
    a = dv.demovideo_parser().parse_args(['--dtype', 'bf16', '--loader_procs', '8', '--out_video_fn', 'v.avi',
                                          '--input_shape', '32', '64', '--eval_shape', '64', '128', '--gpu', '0'])
    assert (a.dtype, a.loader_procs, a.out_video_fn, a.input_shape, a.eval_shape, a.gpu) == \
        ('bf16', 8, 'v.avi', [32, 64], [64, 128], 0)
    with pytest.raises(SystemExit):
        dv.demovideo_parser().parse_args(['--loader_procs', '-1'])
    m = dv.movie_parser().parse_args([])
    assert (m.pred_label_dir, m.img_dir, m.out_video_fn, m.size) == \
        (None, 'data/cityscapes/leftImg8bit/demoVideo', 'results/preds_labels.avi', [2048, 1024])
    assert dv.ALPHA == 0.5 and tuple(dv.ROAD_COLOR) == (128, 64, 128)
    for name in ('create_demovideo.py', 'create_movie.py'):
        assert os.path.exists(os.path.join(ROOT, 'utils', name))
