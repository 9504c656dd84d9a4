"""The fused DRN stems of csrc/spa_stem.hip (input normalisation + conv1 7x7 + layer 1's 3x3, BN folded, ReLU) against the float64
restatement of tests/stem_ref.py, at image sizes that do not fill the kernels' 16 x 32 output tiles, and the whole DRN forward at
such sizes against the float64 network.

Five entry points, four kernels:
    d32     spa_drn_stem_d, out_dtype 0   k_drn_stem_d (float32 matrix instructions)       DRN-D-22 strict float32
    d_amax  spa_drn_stem_d_amax           k_drn_stem_d_f16x3 (two half-precision planes)    DRN-D-22 float32 (default)
    c_amax  spa_drn_stem_c_amax           k_drn_stem_d_f16x3 + y0                           DRN-C-26 float32 (default)
    d_bf16  spa_drn_stem_d, out_dtype 1   k_drn_stem_d_bf16                                 DRN-D-22 bf16
    c_bf16  spa_drn_stem_c_bf16           k_drn_stem_d_bf16 + y0                            DRN-C-26 bf16
The accuracy checks call the ABI directly with NaN-poisoned outputs (a pixel the kernel does not store cannot pass on what an
earlier call left in a reused allocation) and an amax word pre-filled with 0x7f7fffff; the batch-position checks go through
Engine.drn_stem_d."""
import ctypes
import importlib
import os
import sys
import warnings

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stem_ref  # noqa: E402

SPA_ERR_ARG = -1
FLOAT32 = ('d32', 'd_amax', 'c_amax')
PLANES = ('d_amax', 'c_amax')
BF16 = ('d_bf16', 'c_bf16')
WITH_Y0 = ('c_amax', 'c_bf16')
# (B, H, W): one tile; ragged both ways; one pixel past a tile; smaller than the 7 x 7 halo; a resize shape with a half tile
# row; and 'wrap' (_wrap_shape): more tiles than 3 x CU resident workgroups, so the persistent loop and its one-tile-ahead
# prefetch wrap across images
SHAPES = [(1, 16, 32), (2, 37, 61), (3, 17, 33), (1, 5, 3), (2, 1, 1), (1, 360, 640), 'wrap']
IMAGES = ('random', 'zeros', 'full', 'checker')
WEIGHTS = ('drn_d_22', 'drn_c_26', 'hostile')


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


def _drn():
    return importlib.import_module('superpixel-align_amd.drn')


def _wrap_shape():
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    H, W = 199, 1000                                   # ragged: 13 x 32 tiles, the last row 7 pixels, the last column 8
    per = ((H + 15) // 16) * ((W + 31) // 32)
    B = max(2, 3 * cu // per + 1)
    assert B * per > 3 * cu
    return B, H, W


def _shape(s):
    if s == 'wrap':
        B, H, W = _wrap_shape()
        print('wrap shape for %d CUs: (%d, %d, %d), %d tiles'
              % (torch.cuda.get_device_properties(0).multi_processor_count, B, H, W, B * ((H + 15) // 16) * ((W + 31) // 32)))
        return B, H, W
    return s


def _image(kind, B, H, W, seed=0):
    """(B,3,H,W) float32 0..255 on the CPU: random integers, all 0, all 255, or a 0 / 255 checkerboard (phase per channel)"""
    if kind == 'random':
        return torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(seed)).float()
    if kind in ('zeros', 'full'):
        return torch.full((B, 3, H, W), 0.0 if kind == 'zeros' else 255.0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    c = torch.arange(3).view(3, 1, 1)
    return ((yy + xx + c) % 2 * 255.0).float().unsqueeze(0).expand(B, 3, H, W).contiguous()


_MODELS = {}


def _model(arch, dtype):
    key = (arch, dtype)
    if key not in _MODELS:
        _MODELS[key] = _drn().create_drn(arch, device='cuda', dtype=dtype)
    return _MODELS[key]


def _hostile(w, seed=11, spread=1.5):
    """conv1's output channels scaled by 10^U(-1.5, 1.5), layer 1's input channels divided by the same factors (the rescaling of
    test_gpu_hostile._hostile_state_dict): the same function, channels of layer 0 over three decades"""
    w0, b0, w1p, b1 = (t.detach().cpu().double() for t in w)
    g = torch.Generator().manual_seed(seed)
    s = torch.pow(10.0, (torch.rand(16, generator=g, dtype=torch.float64) * 2 - 1) * spread)
    w0 = w0 * s.view(16, 1)
    b0 = b0 * s
    w1p = (w1p.view(16, 9, 16) / s.view(1, 1, 16)).reshape(16, 144)
    return tuple(t.float().contiguous().cuda() for t in (w0, b0, w1p, b1))


def _weights(which, bf16):
    """the folded stem operands the forward hands to the kernels (the bf16 models' are bfloat16 values), or the hostile set"""
    if which == 'hostile':
        return _hostile(_model('drn_d_22', torch.float32)._stem)
    if which == 'drn_d_22':
        return _model('drn_d_22', torch.bfloat16 if bf16 else torch.float32)._stem
    m = _model('drn_c_26', torch.bfloat16 if bf16 else torch.float32)
    return m._stem_c16 if bf16 else m._front_c['stem']


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


MEAN = (ctypes.c_double * 3)(*stem_ref.MEAN)
STD = (ctypes.c_double * 3)(*stem_ref.STD)


def _run(eng, variant, x, w):
    """One call of the variant's entry point with NaN-poisoned outputs and the amax word pre-filled with 0x7f7fffff.
    Returns the raw (B,H,W,16) buffers y, y0 (or None) and the amax word (or None)."""
    L, ctx = eng._lib, eng._ctx
    B, _, H, W = x.shape
    dt = torch.bfloat16 if variant in BF16 else torch.float32
    y = torch.full((B, H, W, 16), float('nan'), dtype=dt, device='cuda')
    y0 = torch.full((B, H, W, 16), float('nan'), dtype=dt, device='cuda') if variant in WITH_Y0 else None
    am = torch.full((1,), 0x7f7fffff, dtype=torch.int32, device='cuda') if variant in PLANES else None
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = (ctx, _P(x), B, H, W) + tuple(_P(t) for t in w) + (MEAN, STD)
    if variant in ('d32', 'd_bf16'):
        rc = L.spa_drn_stem_d(*a, _P(y), 0 if variant == 'd32' else 1, None, s)
    elif variant == 'd_amax':
        rc = L.spa_drn_stem_d_amax(*a, _P(y), None, _P(am), s)
    elif variant == 'c_amax':
        rc = L.spa_drn_stem_c_amax(*a, _P(y), _P(y0), None, _P(am), s)
    else:
        rc = L.spa_drn_stem_c_bf16(*a, _P(y), _P(y0), None, s)
    torch.cuda.synchronize()
    assert rc == 0, (variant, rc)
    return y, y0, am


def _nchw(t):
    return t.permute(0, 3, 1, 2).double().cpu()


def _no_sign_bit(t):
    """no stored element has its sign bit set (-0.0 included): the amax word is an unsigned maximum of float bit patterns"""
    iv = t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    return not bool((iv < 0).any())


def _bf16_ulp(v):
    """one bfloat16 ulp at |v| (8 significant bits); 0 at 0"""
    _, e = torch.frexp(v.abs())
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), e - 8))


@pytest.mark.parametrize('which', WEIGHTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: s if isinstance(s, str) else 'x'.join(map(str, s)))
def test_float32_stems_match_float64(eng, shape, which):
    """d32, d_amax, c_amax: y (and y0) within 1e-5 of max|ref| at every pixel; on the hostile weights the planes' y within 2x the
    float32-instruction form's error (+ 1e-6); the amax word is the largest stored bit pattern; no sign bit anywhere"""
    B, H, W = _shape(shape)
    w = _weights(which, False)
    worst = {}
    for kind in IMAGES:
        x = _image(kind, B, H, W, seed=B * H * W)
        ref_y, ref_y0 = stem_ref.stem64(stem_ref.normalise(x), *w)
        xd = x.cuda()
        sy, sy0 = float(ref_y.abs().max()), float(ref_y0.abs().max())
        err = {}
        for v in FLOAT32:
            y, y0, am = _run(eng, v, xd, w)
            assert bool(torch.isfinite(y).all()), (v, kind, 'a pixel of y was not stored')
            assert _no_sign_bit(y), (v, kind)
            err[v] = float((_nchw(y) - ref_y).abs().max())
            assert err[v] <= 1e-5 * sy, (v, kind, err[v], sy)
            if y0 is not None:
                assert bool(torch.isfinite(y0).all()), (v, kind, 'a pixel of y0 was not stored')
                assert _no_sign_bit(y0), (v, kind)
                e0 = float((_nchw(y0) - ref_y0).abs().max())
                assert e0 <= 1e-5 * sy0, (v, kind, 'y0', e0, sy0)
                worst[v + '.y0'] = max(worst.get(v + '.y0', 0.0), e0 / sy0 if sy0 else e0)
            if am is not None:
                word = int(am.item())
                assert word >= 0, (v, kind, hex(word & 0xffffffff))
                assert word == int(y.view(torch.int32).max()), (v, kind, hex(word), 'amax word is not the largest stored value')
            worst[v] = max(worst.get(v, 0.0), err[v] / sy if sy else err[v])
        if which == 'hostile':
            for v in PLANES:
                assert err[v] <= 2.0 * err['d32'] + 1e-6 * sy, (v, kind, err[v], err['d32'], sy)
    print('STEM float32 %s %s worst error of max|ref|: %s' % ((B, H, W), which, ' '.join('%s=%.2e' % kv for kv in worst.items())))


@pytest.mark.parametrize('which', WEIGHTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: s if isinstance(s, str) else 'x'.join(map(str, s)))
def test_bf16_stems_match_float64(eng, shape, which):
    """d_bf16, c_bf16 against stem64(bf16=True): y0 within one bf16 ulp (or 2^-20 of max|ref| where the float32 accumulation error
    exceeds a small element's ulp), y within 2^-7 of max|ref|"""
    B, H, W = _shape(shape)
    w = _weights(which, True)
    worst = {}
    for kind in IMAGES:
        x = _image(kind, B, H, W, seed=B * H * W + 1)
        ref_y, ref_y0 = stem_ref.stem64(stem_ref.normalise(x), *w, bf16=True)
        xd = x.cuda()
        sy, sy0 = float(ref_y.abs().max()), float(ref_y0.abs().max())
        for v in BF16:
            y, y0, _ = _run(eng, v, xd, w)
            assert bool(torch.isfinite(y.float()).all()), (v, kind, 'a pixel of y was not stored')
            assert _no_sign_bit(y), (v, kind)
            e = float((_nchw(y) - ref_y).abs().max())
            assert e <= 2.0 ** -7 * sy, (v, kind, e, sy)
            worst[v] = max(worst.get(v, 0.0), e / sy if sy else e)
            if y0 is not None:
                assert bool(torch.isfinite(y0.float()).all()), (v, kind, 'a pixel of y0 was not stored')
                assert _no_sign_bit(y0), (v, kind)
                g0 = _nchw(y0)
                d = (g0 - ref_y0).abs()
                tol = torch.maximum(_bf16_ulp(torch.maximum(g0.abs(), ref_y0.abs())), torch.full_like(d, 2.0 ** -20 * sy0))
                bad = d > tol
                assert not bool(bad.any()), (v, kind, 'y0', int(bad.sum()), float(d.max()), sy0)
                worst[v + '.y0'] = max(worst.get(v + '.y0', 0.0), float((d / tol.clamp_min(1e-300)).max()))
    print('STEM bf16 %s %s worst error (y: of max|ref|, y0: of the tolerance): %s'
          % ((B, H, W), which, ' '.join('%s=%.2e' % kv for kv in worst.items())))


@pytest.mark.parametrize('variant', FLOAT32 + BF16)
def test_stem_result_does_not_depend_on_batch_position(eng, variant):
    """image i of a ragged B = 3 batch is the same image run alone, bit for bit (any difference is a tile-offset or prefetch bug);
    two runs give the same bits; the engine's call is the direct ABI call"""
    B, H, W = 3, 37, 61
    bf16 = variant in BF16
    w = _weights('drn_c_26' if variant.startswith('c') else 'drn_d_22', bf16)
    x = torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(5)).float().cuda()
    dtype = torch.bfloat16 if bf16 else torch.float32
    kw = dict(dtype=dtype, split=variant in PLANES, want_layer0=variant in WITH_Y0)

    def run(xx):
        out = eng.drn_stem_d(xx, *w, **kw)
        out = out if isinstance(out, tuple) else (out,)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    full, again = run(x), run(x)
    for a, b in zip(full, again):
        assert torch.equal(a, b), 'two runs of the same input differ'
    for i in range(B):
        alone = run(x[i:i + 1].contiguous())
        for a, b in zip(full, alone):
            assert torch.equal(a[i:i + 1], b), 'image %d of the batch differs from the same image alone' % i
    y, y0, _ = _run(eng, variant, x, w)
    assert torch.equal(full[0], y.permute(0, 3, 1, 2))
    if y0 is not None:
        assert torch.equal(full[1], y0.permute(0, 3, 1, 2))


def test_normalise_is_the_drn_arithmetic_bit_for_bit(eng):
    """spa_drn_normalise (float32 and bf16 output) = stem_ref.normalise bit for bit (bf16: its round-to-nearest-even value), over
    all 256 integer values in each channel and random non-integer values in [0, 255], at an odd H x W"""
    H, W = 17, 31
    p = torch.arange(H * W)
    ints = torch.stack([(p + 85 * c) % 256 for c in range(3)]).float().view(1, 3, H, W)
    assert all(len(torch.unique(ints[0, c])) == 256 for c in range(3))
    frac = torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(9), dtype=torch.float64).float() * 255.0
    frac[0, :, 0, 0], frac[0, :, 0, 1] = 0.0, 255.0
    x = torch.cat([ints, frac])
    ref = stem_ref.normalise(x)
    xd = x.cuda()
    got = eng.drn_normalise(xd, torch.float32)
    assert torch.equal(got.cpu().contiguous().view(torch.int32), ref.view(torch.int32))
    got16 = eng.drn_normalise(xd, torch.bfloat16)
    assert got16.dtype == torch.bfloat16
    assert torch.equal(got16.cpu().contiguous().view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))


def test_refusals_launch_nothing(eng):
    """H = 0, H x W x 12 >= 2^32 (small valid buffers: the launcher refuses before reading), a null weight pointer and out_dtype 3
    return SPA_ERR_ARG from every entry point, and the poisoned outputs (and amax word) stay untouched"""
    L, ctx = eng._lib, eng._ctx
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.full((1, 3, 8, 8), 100.0, device='cuda')
    w0, w1 = torch.ones((16, 147), device='cuda'), torch.ones((16, 144), device='cuda')
    b = torch.ones(16, device='cuda')
    y = torch.full((1, 8, 8, 16), -7.0, device='cuda')
    y0 = torch.full((1, 8, 8, 16), -7.0, device='cuda')
    yb = torch.full((1, 8, 8, 16), -7.0, dtype=torch.bfloat16, device='cuda')
    y0b = torch.full((1, 8, 8, 16), -7.0, dtype=torch.bfloat16, device='cuda')
    xn = torch.full((1, 8, 8, 3), -7.0, device='cuda')
    am = torch.full((1,), 0x1234567, dtype=torch.int32, device='cuda')
    P = _P

    def calls(B, H, W, ws, dt=0):
        a = (ctx, P(x), B, H, W) + ws + (MEAN, STD)
        return [L.spa_drn_stem_d(*a, P(y), dt, P(xn), s),
                L.spa_drn_stem_d(*a, P(yb), 1, P(xn), s),
                L.spa_drn_stem_d_amax(*a, P(y), P(xn), P(am), s),
                L.spa_drn_stem_c_amax(*a, P(y), P(y0), P(xn), P(am), s),
                L.spa_drn_stem_c_bf16(*a, P(yb), P(y0b), P(xn), s)]
    ws = (P(w0), P(b), P(w1), P(b))
    assert 20000 * 20000 * 12 >= 1 << 32
    rcs = calls(1, 0, 8, ws) + calls(1, 20000, 20000, ws) + calls(1, 8, 8, (P(w0), P(b), None, P(b)))
    rcs.append(L.spa_drn_stem_d(ctx, P(x), 1, 8, 8, *ws, MEAN, STD, P(y), 3, P(xn), s))          # out_dtype 3
    rcs.append(L.spa_drn_normalise(ctx, P(x), 1, 0, 8, P(xn), 0, MEAN, STD, s))
    rcs.append(L.spa_drn_normalise(ctx, P(x), 1, 8, 8, P(xn), 2, MEAN, STD, s))
    torch.cuda.synchronize()
    assert rcs == [SPA_ERR_ARG] * len(rcs), rcs
    for t in (y, y0, yb, y0b, xn):
        assert bool((t == -7.0).all()), 'a refused call wrote its output'
    assert int(am.item()) == 0x1234567, 'a refused call touched the amax word'


# ------------------------------------------------------------------------------------------------------------------------------
# the whole DRN forward at ragged sizes against the float64 network

MODES = ('fp32', 'strict', 'bf16')
NET_SHAPES = [(2, 37, 61), (4, 224, 224), (1, 360, 640)]
# the stem each forward must run: ('stem', dtype, split, want_layer0), or ('normalise',) where there is no stem kernel
ROUTE = {('drn_d_22', 'fp32'): ('stem', torch.float32, True, False),
         ('drn_d_22', 'strict'): ('stem', torch.float32, False, False),
         ('drn_d_22', 'bf16'): ('stem', torch.bfloat16, False, False),
         ('drn_c_26', 'fp32'): ('stem', torch.float32, True, True),
         ('drn_c_26', 'strict'): ('normalise',),
         ('drn_c_26', 'bf16'): ('stem', torch.bfloat16, False, True)}
# forwards that still reach a library convolution (strict float32 DRN-C-26: conv1 and layer 1's 16-channel convolutions): never
# captured into a graph, held to the float64 bound only
LIBRARY = {('drn_c_26', 'strict')}
NET_CASES = [(a, m, s) for s in NET_SHAPES for a in ('drn_d_22', 'drn_c_26') for m in MODES]
_REF64 = {}


def _net_input(shape):
    B, H, W = shape
    return torch.randint(0, 256, (B, 3, H, W), generator=torch.Generator().manual_seed(H * W + B)).float()


def _ref_maps(arch, shape):
    """the float64 network's 8 maps (same seed, BatchNorm folded), computed once per (arch, shape)"""
    key = (arch, shape)
    if key not in _REF64:
        _REF64.clear()                                  # (the cases run shape by shape, arch by arch)
        m64 = _drn().create_drn(arch, device='cpu', dtype=torch.float64)
        _, maps = m64.batch_predict(_net_input(shape))
        _REF64[key] = maps
    return _REF64[key]


def _maps(model, x, mode):
    """mode '0': launch by launch; 'auto': the default rule (small batches are captured when no library convolution is in them)"""
    old = os.environ.pop('SPA_DRN_GRAPH', None)
    if mode != 'auto':
        os.environ['SPA_DRN_GRAPH'] = mode
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('error')              # a capture that fell back must fail the test, not pass by the eager path
            _, maps = model.batch_predict(x)
        torch.cuda.synchronize()
        return [m.clone() for m in maps]
    finally:
        os.environ.pop('SPA_DRN_GRAPH', None)
        if old is not None:
            os.environ['SPA_DRN_GRAPH'] = old


@pytest.mark.parametrize('arch,mode,shape', NET_CASES, ids=['%s-%s-%s' % (a, m, 'x'.join(map(str, s))) for a, m, s in NET_CASES])
def test_drn_forward_at_ragged_sizes(arch, mode, shape):
    drn = _drn()
    E = drn._EPILOGUE
    model = _model(arch, torch.bfloat16 if mode == 'bf16' else torch.float32)
    eng = E['engine']
    x = _net_input(shape).cuda()
    calls = []
    orig_stem, orig_norm = eng.drn_stem_d, eng.drn_normalise

    def stem(*a, **k):
        calls.append(('stem', k.get('dtype', torch.float32), bool(k.get('split', False)), bool(k.get('want_layer0', False))))
        return orig_stem(*a, **k)

    def norm(*a, **k):
        calls.append(('normalise',))
        return orig_norm(*a, **k)
    saved = E['split_gemm']
    eng.drn_stem_d, eng.drn_normalise = stem, norm          # (instance attributes: shadow the methods of this engine only)
    try:
        E['split_gemm'] = mode != 'strict'
        graph = _maps(model, x, 'auto')
        before = E['library_convs']
        eager = _maps(model, x, '0')
        lib = E['library_convs'] - before
        split = E['split_gemm']
    finally:
        E['split_gemm'] = saved
        del eng.drn_stem_d, eng.drn_normalise
    assert calls and set(calls) == {ROUTE[(arch, mode)]}, calls
    ents = [e for k, e in model.__dict__.get('_graphs', {}).items() if k[0] == tuple(x.shape) and k[5] == split]
    assert len(ents) == 1
    if (arch, mode) in LIBRARY:
        assert lib > 0 and ents[0] is False
        print('NET %s %s %s: library convolutions in the forward, not captured; held to the float64 bound only' % (arch, mode, shape))
    else:
        assert lib == 0, 'a library convolution in the %s %s forward at %s' % (arch, mode, shape)
        assert ents[0] is not False, 'the forward was not captured'
        for i in range(8):
            assert torch.equal(graph[i], eager[i]), 'map %d differs between the graph and the eager forward' % i
    ref = _ref_maps(arch, shape)
    errs = []
    for i in (range(8) if mode != 'bf16' else (7,)):
        r = ref[i]
        scale = float(r.abs().max())
        for got in (graph[i], eager[i]):
            assert tuple(got.shape) == tuple(r.shape)
            errs.append(float((got.double().cpu() - r).abs().max()) / scale)
            assert errs[-1] <= (5e-2 if mode == 'bf16' else 2e-5), (i, errs[-1])
    print('NET %s %s %s: worst map error of max|map| %.2e' % (arch, mode, shape, max(errs)))
