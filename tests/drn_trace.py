"""Shared by tests/test_gpu_drn_routes.py and tests/test_drn_routes_cpu.py: the cases of tests/drn_routes.json, the recording
proxy that produced it, and a shape-only walk of the DRN forward for the routing functions of drn.py.

tests/drn_routes.json is this project's own recording (python tests/drn_trace.py on a GPU, made on the commit BEFORE the
dispatch of drn.py was split into choose / count / launch): per case the ordered Engine calls of one batch_predict and
what it added to drn._EPILOGUE's counters (floats as hex, so equality is exact)."""
import collections
import contextlib
import inspect
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'drn_routes.json')
ARCHS = ('drn_d_22', 'drn_c_26')
# mode: (dtype, _EPILOGUE settings, environment, use_fused_stem)
MODES = {
    'fp32': ('float32', {}, {}, True),
    'fp32_strict': ('float32', {'split_gemm': False}, {}, True),
    'fp32_strict_wino2': ('float32', {'split_gemm': False, 'winograd': 2}, {}, True),
    'fp32_strict_nowino': ('float32', {'split_gemm': False, 'winograd': 0}, {}, True),
    'fp32_library': ('float32', {'own_conv32': False}, {}, True),
    'bf16': ('bfloat16', {}, {}, True),
    'bf16_library': ('bfloat16', {'own_conv': False}, {}, True),
    'bf16_nolight': ('bfloat16', {}, {'SPA_BF16_LIGHT': '0'}, True),
    'fp32_unfused': ('float32', {}, {}, False),
}
SHAPES = ((2, 3, 64, 96), (1, 3, 16, 2048))
BIG = (336, 3, 224, 224)                 # the smallest batch with B * 56 * 56 > 2^20: fp32 default only
DEFAULTS = {'own_conv': True, 'own_conv32': True, 'winograd': 4, 'split_gemm': True}


def cases():
    """[(id, arch, mode, shape)]"""
    out = [('%s-%s-%s' % (a, m, 'x'.join(map(str, s))), a, m, s) for a in ARCHS for m in MODES for s in SHAPES]
    return out + [('%s-fp32-%s' % (a, 'x'.join(map(str, BIG))), a, 'fp32', BIG) for a in ARCHS]


@contextlib.contextmanager
def mode_set(drn, model, mode):
    """The process-wide switches of one mode (everything else at its default, SPA_DRN_GRAPH=0), put back afterwards."""
    _, epi, env, fused = MODES[mode]
    env = dict({'SPA_DRN_GRAPH': '0', 'SPA_BF16_LIGHT': None, 'SPA_WINO_MIN_CIN': None}, **env)
    saved_epi = {k: drn._EPILOGUE[k] for k in DEFAULTS}
    saved_env = {k: os.environ.get(k) for k in env}
    saved_fused = model.use_fused_stem
    try:
        drn._EPILOGUE.update(DEFAULTS, **epi)
        for k, v in env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        model.use_fused_stem = fused
        yield
    finally:
        model.use_fused_stem = saved_fused
        drn._EPILOGUE.update(saved_epi)
        for k, v in saved_env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class RecordingEngine(object):
    """A thin proxy around the real Engine: logs every convolution / DRN glue call (method, tensor arguments as shape and
    dtype, scalar arguments, None for an absent residual) and delegates."""
    LOGGED = ('conv', 'drn_', 'bias_act_')

    def __init__(self, eng):
        self._eng = eng
        self.calls = []

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if not name.startswith(self.LOGGED) or not callable(attr):
            return attr

        def call(*args, **kw):
            bound = inspect.signature(attr).bind(*args, **kw)
            self.calls.append([name, {k: _plain(v) for k, v in bound.arguments.items()}])
            return attr(*args, **kw)
        return call


def _plain(v):
    if hasattr(v, 'shape') and hasattr(v, 'dtype'):
        return [list(v.shape), str(v.dtype).replace('torch.', '')]
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return str(v).replace('torch.', '')


def _hex(v):
    return v.hex() if isinstance(v, float) else v


def record(drn, model, mode, shape):
    """One batch_predict of `shape` under `mode` through the recording proxy -> {'calls', 'counters', 'library_convs'}"""
    import torch
    x = torch.full(shape, 127.0, dtype=torch.float32, device='cuda')
    x[..., ::3] = 31.0
    real = drn._EPILOGUE['engine']
    proxy = RecordingEngine(real)
    with mode_set(drn, model, mode):
        before = drn._epi_snapshot()
        drn._EPILOGUE['engine'] = proxy
        try:
            model.batch_predict(x, need=[7])
            torch.cuda.synchronize()
        finally:
            drn._EPILOGUE['engine'] = real
        delta = drn._epi_delta(before)
    counters = {k: _hex(v) for k, v in sorted(delta.items()) if k not in ('c16', 'library_convs')}
    counters['c16'] = {k: [_hex(e) for e in v] for k, v in sorted(delta['c16'].items()) if any(v)}
    return {'calls': proxy.calls, 'counters': counters, 'library_convs': delta['library_convs']}


def mode_flags(drn, mode):
    """the Flags tuple drn._flags() returns under `mode` (an engine at its defaults)"""
    _, epi, env, _ = MODES[mode]
    e = dict(DEFAULTS, **epi)
    return drn.Flags(bf16_light=env.get('SPA_BF16_LIGHT', '1') != '0', wino_min_cin=256, debug=(1, 1, 2), **e)


def walk(drn, model, shape, dtype, flags, fused=True):
    """The decisions of one forward of a raw batch of `shape` on the GPU, from shapes alone (model: an unprepared DRN with
    BatchNorm folded; every tensor channels-last): [(level, layer name, route, shape of the layer's input)]"""
    out = []
    B, _, H, W = shape

    def facts(m, families):
        return drn.Layer(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], m.dilation[0], True, families)

    def conv(name, m, H, W, residual, relu):
        call = drn.Call(dtype, B, H, W, True, True, residual, relu)
        out.append(('conv', name, drn.choose_conv(facts(m, drn.conv_families(m, dtype, True)), call, flags), (B, m.in_channels, H, W)))
        return -(-H // m.stride[0]), -(-W // m.stride[0])

    def block(name, blk, H, W):
        call = drn.Call(dtype, B, H, W, True, True, False, True)
        route = drn.choose_block(facts(blk.conv1, drn.block_families(blk, dtype, True)), call, flags)
        if route == 'separate':
            Ho, Wo = conv(name + '.conv1', blk.conv1, H, W, False, True)
            if blk.residual and blk.downsample is not None:
                conv(name + '.downsample.0', blk.downsample[0], H, W, False, False)
        else:
            out.append(('block', name, route, (B, blk.conv1.in_channels, H, W)))
            Ho, Wo = (H + 1) // 2, (W + 1) // 2
        conv(name + '.conv2', blk.conv2, Ho, Wo, blk.residual, True)
        return Ho, Wo

    def plain(name, seq, H, W):
        for i, m in enumerate(seq):
            if hasattr(m, 'kernel_size'):
                H, W = conv('%s.%d' % (name, i), m, H, W, False, True)
        return H, W

    route = drn.choose_chunk(model.front_families(dtype), fused, dtype, True, flags)
    out.append(('chunk', '', route, tuple(shape)))
    first = {'front_c': 3, 'stem_c16': 2, 'stem_d': 2}.get(route, 1)
    if route == 'front_c':
        H, W = (H + 1) // 2, (W + 1) // 2
    elif route == 'stem_c16':
        conv('layer1.0.conv2', model.layer1[0].conv2, H, W, True, True)
    elif first == 1 and model.arch == 'C':
        conv('conv1', model.conv1, H, W, False, True)
    elif first == 1:
        plain('layer0', model.layer0, H, W)
    for i in range(first, 9):
        layer = getattr(model, 'layer%d' % i)
        if model.arch == 'D' and i in (1, 2, 7, 8):
            H, W = plain('layer%d' % i, layer, H, W)
        else:
            for j, blk in enumerate(layer):
                H, W = block('layer%d.%d' % (i, j), blk, H, W)
    return out


class _Probed(Exception):
    pass


def engine_methods(drn):
    """{(level, route): [Engine methods its launch function calls]}, found by running every launch function against an engine
    whose every method raises its own name (the DRN-C front makes three more calls behind the stem's)."""
    import torch

    class Probe(object):
        def __getattr__(self, name):
            def method(*args, **kw):
                raise _Probed(name)
            return method

    conv = torch.nn.Conv2d(32, 64, 3, padding=1)
    x = torch.zeros((1, 32, 4, 4)).contiguous(memory_format=torch.channels_last)
    holder = type('Holder', (), {'_spa_ops': collections.defaultdict(tuple), 'dilation': (1, 1), 'stride': (1, 1),
                                 '_front_c': collections.defaultdict(tuple), '_stem_c16': (), '_stem': (), 'compute_dtype': torch.float32,
                                 'forward': None, 'forward_maps': None})()
    conv._spa_ops = holder._spa_ops
    found = {('chunk', 'host'): [], ('block', 'separate'): [], ('conv', 'torch'): []}
    saved = drn._epi_snapshot()
    for level, table, args in (('conv', drn._CONV, (conv, x, None, True)), ('block', drn._BLOCK, (holder, x)), ('chunk', drn._CHUNK, (holder, x))):
        for route, (_, launch) in table.items():
            if (level, route) in found:
                continue
            try:
                launch(Probe(), *args) if level != 'chunk' else launch(holder, Probe(), x)
                raise AssertionError('%s launches nothing' % route)
            except _Probed as e:
                found[(level, route)] = [str(e)] + (['conv_small_f16s'] * 3 if route == 'front_c' else [])
    drn._epi_restore(saved)
    return found


def models(drn):
    """{(arch, dtype name): prepared model}, created on first use"""
    import torch

    class Cache(dict):
        def __missing__(self, key):
            self[key] = drn.create_drn(key[0], device='cuda', dtype=getattr(torch, key[1]))
            return self[key]
    return Cache()


def main():
    """Writes the fixture (run from the repository root on a GPU)."""
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    drn = importlib.import_module('superpixel-align_amd.drn')
    cache = models(drn)
    out = {}
    for cid, arch, mode, shape in cases():
        out[cid] = record(drn, cache[(arch, MODES[mode][0])], mode, shape)
        print(cid, len(out[cid]['calls']), 'calls,', out[cid]['library_convs'], 'library convolutions', flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, 'w') as f:
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in out.items()) + '\n}\n')


if __name__ == '__main__':
    main()
