"""--png_encoder device on the GPU.  Engine.png_deflate (spa_png_deflate_u8) against png.deflate_rle_host on the images
of png_cases.py: the stream, its length and the Adler-32, byte for byte, twice into a buffer filled with 0xFF, of which
every byte from nbytes + 4 to the end of the stride must stay 0xFF (the kernel in fact writes nothing at or past
nbytes; the test states what the interface promises); the refusals, which launch nothing; and the two drivers, run
once per encoder: the same names in the same order, the same pixels, and for the demo video the same .avi from
create_movie.py over either directory.  The host restatement itself is held to Pillow and zlib in
test_png_device_cpu.py."""
import ctypes
import importlib
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases  # noqa: E402
import segnet_train_synth as syn  # noqa: E402
from segnet_ref import random_params  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
png = importlib.import_module('superpixel-align_amd.png')
dv = importlib.import_module('superpixel-align_amd.demovideo')
segnet = importlib.import_module('superpixel-align_amd.segnet')
SpalignError = importlib.import_module('superpixel-align_amd._lib').SpalignError
CASES = png_cases.cases()
SLACK = 64                                   # bytes of stride past the bound


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


@pytest.fixture(scope='module')
def reference():
    """(stream, adler) of every image of every case, computed once"""
    memo = {}
    for name, src, out_shape in CASES:
        rows = cols = None
        if out_shape is not None:
            rows, cols = png.nearest_tables(src.shape[1:], out_shape)
            # the tables against the host-resized image
            cli = importlib.import_module('superpixel-align_amd.cli')
            memo[name] = [png.deflate_rle_host(cli.resize_nearest(im, out_shape)) for im in src]
            assert memo[name] == [png.deflate_rle_host(im, rows, cols) for im in src]
        else:
            memo[name] = [png.deflate_rle_host(im) for im in src]
    return memo


@pytest.mark.parametrize('name,src,out_shape', CASES, ids=[c[0] for c in CASES])
def test_stream_length_and_adler_are_the_restatement(eng, reference, name, src, out_shape):
    B = src.shape[0]
    Ho, Wo = out_shape if out_shape is not None else src.shape[1:]
    bound = png.deflate_bound(Ho, Wo)
    assert int(eng._lib.spa_png_deflate_bound(Ho, Wo)) == bound
    stride = bound + SLACK
    src_d = torch.from_numpy(src).cuda()
    out = torch.empty((B, stride), dtype=torch.uint8, device='cuda')
    nbytes = torch.empty((B,), dtype=torch.int32, device='cuda')
    adler = torch.empty((B,), dtype=torch.int32, device='cuda')
    for _ in range(2):
        out.fill_(0xFF)
        nbytes.fill_(-1)
        adler.fill_(-1)
        got = eng.png_deflate(src_d, out_shape, out=out, nbytes=nbytes, adler=adler)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out.data_ptr()
        out_h, n_h, a_h = out.cpu().numpy(), nbytes.cpu().numpy(), adler.cpu().numpy()
        for b, (stream, ad) in enumerate(reference[name]):
            n = int(n_h[b])
            assert n == len(stream) and n <= bound, (b, n, len(stream))
            assert int(a_h[b]) & 0xffffffff == ad, b
            assert out_h[b, :n].tobytes() == stream, b
            assert (out_h[b, n + 4:] == 0xFF).all(), 'image %d: a byte past nbytes + 4 was written' % b


def test_engine_owned_buffers_are_reused_and_make_files(eng):
    src = np.stack([png_cases.wedge(), 1 - png_cases.wedge()])
    src_d = torch.from_numpy(src).cuda()
    ptrs = set()
    for _ in range(2):
        out, nbytes, adler = eng.png_deflate(src_d)
        ptrs.add(out.data_ptr())
        n_h, a_h, out_h = nbytes.cpu().numpy(), adler.cpu().numpy(), out.cpu().numpy()
        for b in range(2):
            data = png.assemble(out_h[b, :int(n_h[b])].tobytes(), int(a_h[b]) & 0xffffffff, 64, 700)
            png_cases.check_file(png, data, src[b])
    assert len(ptrs) == 1, 'the encode buffer was allocated again'


def test_refusals_launch_nothing(eng):
    lib, ctx = eng._lib, eng._ctx
    fn = lib.spa_png_deflate_u8
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    src = torch.zeros((2, 8, 16), dtype=torch.uint8, device='cuda')
    bound = png.deflate_bound(8, 16)
    out = torch.full((2, bound), 0xFF, dtype=torch.uint8, device='cuda')
    meta = torch.full((2, 2), -1, dtype=torch.int32, device='cuda')
    nb, ad = P(meta[0]), P(meta[1])
    rows = torch.zeros((1 << 20,), dtype=torch.int32, device='cuda')
    assert fn(ctx, P(src), 2, 8, 16, None, None, 8, 16, P(out), bound, nb, ad, s) == 0
    torch.cuda.synchronize()
    assert int(meta[0, 0]) > 0
    out.fill_(0xFF)
    meta.fill_(-1)
    got = [
        fn(ctx, P(src), 2, 8, 16, None, None, 8, 16, P(out), bound - 1, nb, ad, s),        # out_stride below the bound
        fn(ctx, P(src), 0, 8, 16, None, None, 8, 16, P(out), bound, nb, ad, s),            # a dimension of 0
        fn(ctx, P(src), 2, 0, 16, None, None, 0, 16, P(out), bound, nb, ad, s),
        fn(ctx, P(src), 2, 8, 16, P(rows), P(rows), 8, 0, P(out), bound, nb, ad, s),
        fn(ctx, P(src), 2, 8, 16, None, None, 4, 16, P(out), bound, nb, ad, s),            # identity, other shapes
        fn(ctx, P(src), 2, 8, 16, P(rows), None, 8, 32, P(out), bound, nb, ad, s),
        # 2^20 rows of 2049 bytes may need 2.4e9 bytes: more than an IDAT chunk's length field holds
        fn(ctx, P(src), 2, 8, 16, P(rows), P(rows), 1 << 20, 2048, P(out), 1 << 40, nb, ad, s),
    ]
    torch.cuda.synchronize()
    assert got == [-5, -1, -1, -1, -1, -1, -1]
    assert b'IDAT' in lib.spa_last_error()
    assert int(lib.spa_png_deflate_bound(1 << 20, 2048)) > (1 << 31) - 1
    assert bool((out == 0xFF).all()) and bool((meta == -1).all())
    with pytest.raises(SpalignError):
        eng.png_deflate(src, out=out[:, :bound - 1])
    with pytest.raises(SpalignError):
        eng.png_deflate(src.float())


# ------------------------------------------------------------------------------- the label-free driver
def read_png(fn):
    from PIL import Image
    with Image.open(fn) as f:
        assert f.mode == 'L'
        return np.asarray(f)


def test_labelfree_driver_writes_the_same_labels_with_either_encoder(tmp_path, capsys):
    from PIL import Image
    cli = importlib.import_module('superpixel-align_amd.cli')
    synth = importlib.import_module('superpixel-align_amd.synth')
    H, W, n = 96, 192, 5
    img_fns = []
    for i in range(n):
        img = synth.synth_image(40 + i, H, W, integer_valued=True).astype(np.uint8)
        img_fns.append(str(tmp_path / ('city_%06d_000019_leftImg8bit.png' % i)))
        Image.fromarray(img.transpose(1, 2, 0)).save(img_fns[-1])
    (tmp_path / 'imgs.txt').write_text('\n'.join(img_fns) + '\n')
    printed = {}
    for encoder in ('pillow', 'device'):
        out = tmp_path / encoder
        # bf16: the DRN forward has the same bits in every run, so the two runs label the same masks
        argv = ['--img_list_fn', str(tmp_path / 'imgs.txt'), '--label_shape', str(2 * H), str(2 * W), '--gpu', '0',
                '--out_dir', str(out), '--superpixel_method', 'slic', '--n_slic_segments', '30', '--n_clusters', '2',
                '--resize_shape', str(H), str(W), '--batchsize', '2', '--start_index', '0', '--end_index', str(n),
                '--arch', 'drn_d_22', '--dtype', 'bf16', '--pool_mode', 'mean'] + \
               (['--png_encoder', 'device'] if encoder == 'device' else [])
        capsys.readouterr()
        assert cli.main_labelfree(argv) == 0
        printed[encoder] = [l for l in capsys.readouterr().out.splitlines() if l.endswith('.png')]
    # batches (0,2) (2,4) (3,5): image 3 is labelled twice
    want = [os.path.basename(img_fns[i]) for i in (0, 1, 2, 3, 3, 4)]
    assert [os.path.basename(l) for l in printed['pillow']] == want
    assert [os.path.basename(l) for l in printed['device']] == want
    some_road = False
    for fn in img_fns:
        a = read_png(tmp_path / 'pillow' / os.path.basename(fn))
        b = read_png(tmp_path / 'device' / os.path.basename(fn))
        assert a.shape == (2 * H, 2 * W) and a.dtype == b.dtype == np.uint8 and np.array_equal(a, b)
        png_cases.check_file(png, open(tmp_path / 'device' / os.path.basename(fn), 'rb').read(), a)
        some_road = some_road or 0 < a.mean() < 1
    assert some_road


# ------------------------------------------------------------------------------- the demo-video stage
IN_SHAPE, PRED_SHAPE = (32, 64), (64, 128)


def test_label_frames_with_either_encoder(eng, tmp_path):
    root = str(tmp_path)
    rng = np.random.default_rng(90)
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
    for encoder in ('pillow', 'device'):
        stats = {}
        assert dv.label_frames(model, fns, os.path.join(root, encoder), IN_SHAPE, PRED_SHAPE, batchsize=4,
                               stats=stats, png_encoder=encoder) == 6
        assert ('png_payload_bytes' in stats) == (encoder == 'device')
        with dv.MjpegAviWriter(os.path.join(root, encoder + '.avi'), size) as w:
            dv.label_frames(model, fns, os.path.join(root, encoder + '_video'), IN_SHAPE, PRED_SHAPE, batchsize=4,
                            video=w, png_encoder=encoder)
    with pytest.raises(ValueError, match='png_encoder'):
        dv.label_frames(model, fns, os.path.join(root, 'x'), IN_SHAPE, PRED_SHAPE, png_encoder='zlib')
    some_road = False
    for fn in fns:
        name = os.path.basename(fn)
        a = read_png(os.path.join(root, 'pillow', name))
        some_road = some_road or 0 < a.mean() < 1
        for d in ('device', 'pillow_video', 'device_video'):
            assert np.array_equal(read_png(os.path.join(root, d, name)), a), (d, name)
        png_cases.check_file(png, open(os.path.join(root, 'device', name), 'rb').read(), a)
    assert some_road
    # the blended frames do not depend on the encoder, and create_movie.py reads either directory alike
    assert open(os.path.join(root, 'pillow.avi'), 'rb').read() == open(os.path.join(root, 'device.avi'), 'rb').read()
    movies = []
    for encoder in ('pillow', 'device'):
        movie = os.path.join(root, 'movie_%s.avi' % encoder)
        syn.run_python([os.path.join(ROOT, 'utils', 'create_movie.py'), '--pred_label_dir', os.path.join(root, encoder),
                        '--img_dir', os.path.join(root, 'demoVideo'), '--out_video_fn', movie, '--size', str(size[0]),
                        str(size[1])], cwd=root, timeout=120)
        movies.append(open(movie, 'rb').read())
    assert movies[0] == movies[1] == open(os.path.join(root, 'pillow.avi'), 'rb').read()
