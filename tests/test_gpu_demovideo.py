"""GPU tests of the demo-video stage: decode1 with raw scores (spa_segnet_decode_logits / _bf16 / _f16x3) against the
float64 classifier sums of tests/segnet_ref.py on each family's own operands, the fused mask-and-blend kernel
(spa_segnet_overlay) against Engine.segnet_score and demovideo.blend_host bit for bit, and label_frames, write_movie and
the two drivers end to end on a synthetic demoVideo tree."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
F = torch.nn.functional
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402
from segnet_ref import channels_last, conv_bias, d64, r16, random_params, t64, unpool  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
dv = importlib.import_module('superpixel-align_amd.demovideo')
SpalignError = importlib.import_module('superpixel-align_amd._lib').SpalignError

# The raw scores are held to each family's layer bound, as a fraction of max|ref| (LAYER_TOL of test_gpu_segnet.py,
# test_gpu_segnet_bf16.py and test_gpu_segnet_f16x3.py): the classifier adds one 64-term float32 sum to a layer that
# is already held to it.  The reference multiplies the family's own operands in float64 (r16: the bf16 kernels round
# every product operand; the float32 and split-plane kernels multiply the float32 values).  Measured worst on an
# MI355X: 5.8e-7 (float32), 2.9e-7 (bf16), 3.9e-7 (split planes).
LOGIT_TOL = {'': 1e-5, '_bf16': 1e-5, '_f16x3': 1e-5}
OPERAND = {'': d64, '_bf16': r16, '_f16x3': d64}          # the maps, device tensors
W_OPERAND = {'': t64, '_bf16': r16, '_f16x3': t64}        # the folded weights, numpy arrays
FAMILIES = ['', '_bf16', '_f16x3']


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


def pooled_input(B, Hh, Wh, seed):
    """a pooled map and its index map as an encoder leaves them (non-negative values, every index 0..3)"""
    g = torch.Generator().manual_seed(seed)
    h = channels_last(torch.rand((B, 64, Hh, Wh), generator=g) * 2.0)
    idx = channels_last(torch.randint(0, 4, (B, 64, Hh, Wh), generator=g, dtype=torch.uint8))
    return h, idx


# ------------------------------------------------------------------------------- decode1 with raw scores
# decode1 outputs 32 x 64 (whole 8 x 32 tiles) and 20 x 36 (partial tiles both ways), B = 2
@pytest.mark.parametrize('out_hw', [(32, 64), (20, 36)])
@pytest.mark.parametrize('family', FAMILIES)
def test_logits_against_float64(eng, family, out_hw):
    B, (H, W) = 2, out_hw
    p = random_params(60)
    h, idx = pooled_input(B, H // 2, W // 2, 61)
    operand = OPERAND[family]
    w, b, w64, b64 = sref.folded(p, 'conv_decode1', operand=W_OPERAND[family])
    wc, bc, wc64, bc64 = sref.classifier(p)
    decode = getattr(eng, 'segnet_decode' + family)
    outs = []
    for _ in range(2):
        out, buf = sref.poisoned((B, 2, H, W))
        z = decode(h, idx, w, b, wc, bc, logits=True, out=out)
        torch.cuda.synchronize()
        assert z.data_ptr() == out.data_ptr() and not torch.isnan(out).any().item(), 'a score was not stored'
        sref.check_guard(buf, out.numel())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    y = conv_bias(unpool(operand(h.cpu()), idx.cpu()), w64, b64)
    ref = F.conv2d(y, wc64[:, :, None, None], bc64)
    e = sref.rel_err(outs[0], ref)
    print('logits%s %s: error %.3g of max|ref| (bound %.3g)' % (family, out_hw, e, LOGIT_TOL[family]))
    assert e <= LOGIT_TOL[family]
    if H % 16 == 0 and W % 16 == 0:
        # the softmax entry point consumes these sums: its probabilities are their softmax to float32 rounding
        prob = decode(h, idx, w, b, wc, bc)
        assert float((torch.softmax(outs[0].double(), 1) - prob.double()).abs().max()) <= 1e-6


@pytest.mark.parametrize('family', FAMILIES)
def test_logits_refusals_launch_nothing(eng, family):
    lib, ctx = eng._lib, eng._ctx
    fn = getattr(lib, 'spa_segnet_decode_logits' + family)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    x64 = torch.zeros((1, 64, 16, 16), device='cuda')
    idx = torch.zeros((1 << 16,), dtype=torch.uint8, device='cuda')
    w64 = torch.zeros((49, 64, 64), device='cuda')
    b = torch.zeros(128, device='cuda')
    out = torch.full((1 << 16,), float('nan'), device='cuda')
    NHWC, NCHW = 0, 1
    got = [
        fn(ctx, P(x64), P(idx), NHWC, 1, 16, 16, P(w64), P(b), None, None, P(out), s),          # no classifier
        fn(ctx, P(x64), P(idx), NHWC, 1, 16, 16, P(w64), P(b), P(b), None, P(out), s),          # half a classifier
        fn(ctx, P(x64), P(idx), NCHW, 1, 16, 16, P(w64), P(b), P(b), P(b), P(out), s),          # planar input
        fn(ctx, P(x64), P(idx), NHWC, 0, 16, 16, P(w64), P(b), P(b), P(b), P(out), s),          # B = 0
        fn(ctx, P(x64), ctypes.c_void_p(idx.data_ptr() + 1), NHWC, 1, 16, 16, P(w64), P(b), P(b), P(b), P(out), s),
        fn(ctx, P(x64), P(idx), NHWC, 1, 16, 16, ctypes.c_void_p(w64.data_ptr() + 4), P(b), P(b), P(b), P(out), s),
        fn(ctx, P(x64), P(idx), NHWC, 1, 16, 16, P(w64), P(b), P(b), P(b), None, s),            # no output
    ]
    torch.cuda.synchronize()
    assert got == [-1, -1, -4, -1, -1, -1, -1]
    assert torch.isnan(out).all().item()
    with pytest.raises(SpalignError, match='logits'):
        getattr(eng, 'segnet_decode' + family)(channels_last(x64), channels_last(idx[:64 * 256].view(1, 64, 16, 16)),
                                               w64, b[:64], logits=True)


@pytest.mark.parametrize('dtype,split', [('fp32', False), ('bf16', False), ('fp32', True)])
def test_forward_logits_feed_the_softmax(eng, dtype, split):
    model = segnet.SegNetBasic(random_params(62), pred_shape=(64, 128), engine=eng, dtype=dtype, split_planes=split)
    x = (torch.rand((2, 3, 32, 64), generator=torch.Generator().manual_seed(63)) * 255.0).cuda()
    z = model.forward(x, logits=True)
    prob = model.forward(x)
    assert z.shape == prob.shape == (2, 2, 32, 64)
    assert float((torch.softmax(z.double(), 1) - prob.double()).abs().max()) <= 1e-6
    labels = model.predict_labels(x)
    mask, _ = eng.segnet_score(z, (64, 128))
    assert len(labels) == 2 and labels[0].dtype == np.int32 and labels[0].shape == (64, 128)
    assert np.array_equal(np.stack(labels), mask.cpu().numpy().astype(np.int32))
    # the host restatement of predict_labels on the device's scores: resize, then argmax, no softmax
    for j in range(2):
        r = segnet.resize_bilinear_pil(z[j].cpu().numpy(), (64, 128))
        assert np.array_equal(labels[j], (r[1] > r[0]).astype(np.int32))


# ------------------------------------------------------------------------------- the overlay
POISON = 165


def guarded(shape, lead=1024, tail=1024, offset=0):
    """(view, whole buffer, first byte): a uint8 view of `shape` inside a buffer filled with POISON"""
    n = int(np.prod(shape))
    buf = torch.full((lead + offset + n + tail,), POISON, dtype=torch.uint8, device='cuda')
    return buf[lead + offset:lead + offset + n].view(shape), buf, lead + offset


def check_guards(buf, lo, n):
    assert bool((buf[:lo] == POISON).all()) and bool((buf[lo + n:] == POISON).all()), 'a kernel wrote outside its output'


def all_bytes_frame(H, W):
    v = np.arange(H * W, dtype=np.int64)
    return np.stack([v % 256, (v * 7 + 3) % 256, 255 - v % 256], -1).astype(np.uint8).reshape(1, H, W, 3)


def run_overlay(eng, score, frames_np, color, alpha, offset=0):
    B, H, W = frames_np.shape[:3]
    frames, fbuf, flo = guarded((B, H, W, 3), offset=offset)
    frames.copy_(torch.from_numpy(frames_np))
    mask, mbuf, mlo = guarded((B, H, W))
    blended, bbuf, blo = guarded((B, H, W, 3))
    m, bl = eng.segnet_overlay(score, frames, color, alpha, out_mask=mask, out_blended=blended)
    torch.cuda.synchronize()
    assert m.data_ptr() == mask.data_ptr() and bl.data_ptr() == blended.data_ptr()
    check_guards(mbuf, mlo, mask.numel())
    check_guards(bbuf, blo, blended.numel())
    check_guards(fbuf, flo, frames.numel())
    assert torch.equal(frames.cpu(), torch.from_numpy(frames_np)), 'the frames were changed'
    want_mask, _ = eng.segnet_score(score, (H, W))
    assert torch.equal(mask, want_mask)
    mask_h, blended_h = mask.cpu().numpy(), blended.cpu().numpy()
    for j in range(B):
        assert np.array_equal(blended_h[j], dv.blend_host(frames_np[j], mask_h[j], color, alpha)), 'image %d' % j
    return mask_h


# (h, w) -> (H, W), byte offset of the frames: the vector path; the byte path; several blocks in x, more than 16 rows
# and a tail; a frames view offset by one byte (the byte path at a width that is a multiple of 4)
OVERLAY_CASES = [((16, 24), (32, 48), 0), ((5, 7), (19, 30), 0), ((3, 70), (40, 1030), 0), ((16, 24), (32, 48), 1)]


@pytest.mark.parametrize('src,dst,offset', OVERLAY_CASES)
@pytest.mark.parametrize('color,alpha', [((128, 64, 128), 0.5), ((10, 250, 77), 0.3)])
def test_overlay_matches_score_and_host_blend(eng, src, dst, offset, color, alpha):
    B, (h, w), (H, W) = 3, src, dst
    g = torch.Generator().manual_seed(70)
    score = torch.randn((B, 2, h, w), generator=g)
    score[:, :, :2, :3] = 0.25                                        # exact ties: class 0
    rng = np.random.default_rng(71)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mask = run_overlay(eng, score.cuda(), frames, color, alpha, offset)
    assert 0 < mask.mean() < 1
    # logits, not only probabilities: large scores of both signs
    run_overlay(eng, (score * 50.0).cuda(), frames, color, alpha, offset)
    # every byte value in every channel under an all-road score
    road = torch.zeros((1, 2, h, w))
    road[:, 1] = 1.0
    mask = run_overlay(eng, road.cuda(), all_bytes_frame(H, W), color, alpha, offset)
    assert mask.all()


def test_overlay_refusals_launch_nothing(eng):
    score = torch.randn((3, 2, 16, 24), generator=torch.Generator().manual_seed(72)).cuda()
    frames, _, _ = guarded((3, 32, 48, 3))
    mask, mbuf, _ = guarded((3, 32, 48))
    blended, bbuf, _ = guarded((3, 32, 48, 3))
    untouched = lambda: bool((mbuf == POISON).all()) and bool((bbuf == POISON).all())
    for alpha in (1.5, -0.01, float('nan')):
        with pytest.raises(SpalignError, match='alpha'):
            eng.segnet_overlay(score, frames, alpha=alpha, out_mask=mask, out_blended=blended)
    with pytest.raises(SpalignError, match='overlaps'):
        eng.segnet_overlay(score, frames, out_mask=mask, out_blended=frames)
    both = torch.full((3 * 32 * 48 * 3 + 48,), POISON, dtype=torch.uint8, device='cuda')
    n = 3 * 32 * 48 * 3
    with pytest.raises(SpalignError, match='overlaps'):               # the last 48 bytes of one are the other's first
        eng.segnet_overlay(score, both[:n].view(3, 32, 48, 3), out_mask=mask, out_blended=both[48:].view(3, 32, 48, 3))
    big = torch.randn((3, 2, 33, 24), generator=torch.Generator().manual_seed(73)).cuda()
    with pytest.raises(SpalignError, match='downscale'):
        eng.segnet_overlay(big, frames, out_mask=mask, out_blended=blended)
    with pytest.raises(SpalignError, match='downscale'):
        eng.segnet_score(big, (32, 48))                               # as spa_segnet_score refuses it
    lib = eng._lib
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    col = (ctypes.c_uint8 * 3)(128, 64, 128)
    assert lib.spa_segnet_overlay(eng._ctx, P(score), 3, 16, 24, 32, 48, P(frames), None, 0.5, P(mask), P(blended),
                                  s) == -1
    assert lib.spa_segnet_overlay(eng._ctx, P(score), 3, 16, 24, 32, 48, None, col, 0.5, P(mask), P(blended), s) == -1
    assert lib.spa_segnet_overlay(eng._ctx, P(score), 3, 16, 24, 32, 48, P(frames), col, 0.5, None, P(blended),
                                  s) == -1
    torch.cuda.synchronize()
    assert untouched() and bool((both == POISON).all())


# ------------------------------------------------------------------------------- end to end
IN_SHAPE, PRED_SHAPE = (32, 64), (64, 128)


@pytest.fixture(scope='module')
def demo(tmp_path_factory, eng):
    """5 frames of 64 x 128 in two city folders, the third palette-mode (the host path), a random-weight snapshot
    file, the model and the labels of predict_labels on the host-resized frames"""
    root = str(tmp_path_factory.mktemp('demovideo'))
    rng = np.random.default_rng(80)
    names = []
    for i in range(5):
        city = 'stuttgart_%02d' % (i // 3)
        os.makedirs(os.path.join(root, 'demoVideo', city), exist_ok=True)
        img, _ = syn.image(PRED_SHAPE[0], PRED_SHAPE[1], rng)
        fn = os.path.join(root, 'demoVideo', city, '%s_000000_%06d_leftImg8bit.png' % (city, i))
        with open(fn, 'wb') as f:
            f.write(syn.png(img, 'P' if i == 2 else None))
        names.append(fn)
    snap = os.path.join(root, 'snapshot_iter_3')
    with open(snap, 'wb') as f:
        np.savez(f, **{segnet.PREFIX + k: v for k, v in random_params(81).items()})
    model = segnet.SegNetBasic.from_snapshot_file(snap, pred_shape=PRED_SHAPE, device=eng.device.index)
    fns = dv.demo_frames(os.path.join(root, 'demoVideo'))
    assert fns == sorted(names)
    frames = [dv.read_frame(fn) for fn in fns]
    x = np.stack([st.resize_bicubic_float(f.transpose(2, 0, 1).astype(np.float32), IN_SHAPE) for f in frames])
    labels = model.predict_labels(x)
    assert 0 < np.mean(labels) < 1
    yield dict(root=root, snap=snap, model=model, fns=fns, frames=frames, labels=labels)
    model.engine.close()


def read_pngs(d, fns):
    from PIL import Image
    out = []
    for fn in fns:
        with Image.open(os.path.join(d, os.path.basename(fn))) as f:
            assert f.mode == 'L'
            out.append(np.asarray(f))
    return out


def avi_frames(fn):
    import test_demovideo_cpu as cpu
    return cpu.parse_avi(open(fn, 'rb').read())


def test_label_frames_end_to_end(demo):
    root, model, fns = demo['root'], demo['model'], demo['fns']
    plain = os.path.join(root, 'plain')
    stats = {}
    assert dv.label_frames(model, fns, plain, IN_SHAPE, PRED_SHAPE, batchsize=2, stats=stats) == 5
    assert sorted(os.listdir(plain)) == sorted(os.path.basename(fn) for fn in fns)
    for got, want in zip(read_pngs(plain, fns), demo['labels']):
        assert got.dtype == np.uint8 and np.array_equal(got.astype(np.int32), want)
    assert stats['n_batches'] == 3 and stats['n_host_batches'] == 0
    # decode workers: the same files, byte for byte; the batch with the palette frame takes the host path
    procs = os.path.join(root, 'procs')
    before = syn.shm_names('psm_')
    stats = {}
    dv.label_frames(model, fns, procs, IN_SHAPE, PRED_SHAPE, batchsize=2, loader_procs=2, stats=stats)
    assert stats['n_host_batches'] == 1
    assert syn.shm_names('psm_') == before
    for fn in fns:
        name = os.path.basename(fn)
        assert open(os.path.join(procs, name), 'rb').read() == open(os.path.join(plain, name), 'rb').read()
    # with a video: the same labels, and the frames are Pillow's encoding of the host blend
    for k, n_procs in enumerate((0, 2)):
        out = os.path.join(root, 'video%d' % k)
        avi = os.path.join(root, 'v%d.avi' % k)
        with dv.MjpegAviWriter(avi, (PRED_SHAPE[1], PRED_SHAPE[0])) as w:
            dv.label_frames(model, fns, out, IN_SHAPE, PRED_SHAPE, batchsize=2, loader_procs=n_procs, video=w)
        for fn in fns:
            name = os.path.basename(fn)
            assert open(os.path.join(out, name), 'rb').read() == open(os.path.join(plain, name), 'rb').read()
        a = avi_frames(avi)
        assert a['avih'][4] == 5 and a['avih'][8:10] == (PRED_SHAPE[1], PRED_SHAPE[0])
        for j in range(5):
            assert a['frames'][j] == dv.encode_jpeg(dv.blend_host(demo['frames'][j], demo['labels'][j]))
    assert open(os.path.join(root, 'v0.avi'), 'rb').read() == open(os.path.join(root, 'v1.avi'), 'rb').read()
    # create_movie.py's pass over the written PNGs: the identical file
    movie = os.path.join(root, 'movie.avi')
    assert dv.write_movie(plain, os.path.join(root, 'demoVideo'), movie, size=(PRED_SHAPE[1], PRED_SHAPE[0])) == 5
    assert open(movie, 'rb').read() == open(os.path.join(root, 'v0.avi'), 'rb').read()


def test_video_refuses_a_frame_of_another_size_before_writing(demo, tmp_path):
    from PIL import Image
    root = str(tmp_path)
    os.makedirs(os.path.join(root, 'demoVideo', 'a'))
    fns = []
    for i, shape in enumerate([PRED_SHAPE, (PRED_SHAPE[0], PRED_SHAPE[1] + 4)]):
        fns.append(os.path.join(root, 'demoVideo', 'a', 'a_%d.png' % i))
        Image.fromarray(np.zeros(shape + (3,), np.uint8)).save(fns[-1])
    out = os.path.join(root, 'out')
    with dv.MjpegAviWriter(os.path.join(root, 'v.avi'), (PRED_SHAPE[1], PRED_SHAPE[0])) as w:
        with pytest.raises(ValueError, match='pred_shape'):
            dv.label_frames(demo['model'], fns, out, IN_SHAPE, PRED_SHAPE, batchsize=2, video=w)
        assert not os.path.exists(out) and w.index == []
    # without a video the frames may differ in size: each is resized to the input shape
    assert dv.label_frames(demo['model'], fns, out, IN_SHAPE, PRED_SHAPE, batchsize=2) == 2
    assert all(a.shape == PRED_SHAPE for a in read_pngs(out, fns))


def test_drivers_as_child_processes(demo):
    root = demo['root']
    out, avi = os.path.join(root, 'cli'), os.path.join(root, 'cli.avi')
    shapes = ['--input_shape', str(IN_SHAPE[0]), str(IN_SHAPE[1]), '--eval_shape', str(PRED_SHAPE[0]),
              str(PRED_SHAPE[1])]
    syn.run_python([os.path.join(ROOT, 'utils', 'create_demovideo.py'), '--snapshot', demo['snap'], '--out_dir', out,
                    '--gpu', '-1', '--demoVideo_dir', os.path.join(root, 'demoVideo'), '--batchsize', '2',
                    '--loader_procs', '2', '--out_video_fn', avi] + shapes, cwd=root, timeout=300)
    for got, want in zip(read_pngs(out, demo['fns']), demo['labels']):
        assert np.array_equal(got.astype(np.int32), want)
    movie = os.path.join(root, 'cli_movie.avi')
    syn.run_python([os.path.join(ROOT, 'utils', 'create_movie.py'), '--pred_label_dir', out, '--img_dir',
                    os.path.join(root, 'demoVideo'), '--out_video_fn', movie, '--size', str(PRED_SHAPE[1]),
                    str(PRED_SHAPE[0])], cwd=root, timeout=120)
    assert open(movie, 'rb').read() == open(avi, 'rb').read()
    a = avi_frames(avi)
    for j in range(5):
        assert a['frames'][j] == dv.encode_jpeg(dv.blend_host(demo['frames'][j], demo['labels'][j]))
