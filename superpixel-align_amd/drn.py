"""Dilated Residual Network feature extractor for the label-generation path (PyTorch-ROCm).

Role in the hot path: `model.batch_predict(imgs)` -> 8 intermediate maps, of which the caller
keeps `maps[i] for i in --use_feature_maps` (default [7] = layer8, 512 x H/8 x W/8)
(reference: batch_spalign_kmeans.py:431-435, models/drn.py:230-325).

What is kept from the reference, because results depend on it
  * architecture C-26 (the reference's create_model, batch_spalign_kmeans.py:524-526) and
    D-22 (BASELINE north star); layer plan [1,1,2,2,2,2,1,1], channels 16..512, dilations
    2 (layer5) / 4 (layer6) / 2 (layer7) / 1 (layer8), layer7/8 of arch C without residual
    (models/drn.py:158-165), arch D plain conv stacks for layers 1,2,7,8 (:134-145,166-170);
  * the map list uses the CHAINER convention: maps[i] is the output of layer(i+1) for both
    archs — Chainer's arch D does not export layer0 (models/drn.py:238-243) although the
    PyTorch file does (models/drn_pytorch.py:216-218);
  * BatchNorm eps 2e-5: load_npz into a fresh Chainer model restores parameters and running
    statistics only, so the published labels were produced with Chainer's default eps, not the
    1e-5 of the PyTorch checkpoint;
  * input normalisation arithmetic of DRN.batch_predict (models/drn.py:319-321): x/255 in
    float32, then (x - mean) and (x / std) evaluated in float64 and stored as float32.

What is designed for MI355X instead of translated
  * inference only: BatchNorm is folded into the preceding convolution at load time
    (`fold_bn=True`), halving the number of memory-bound elementwise passes over the
    16..512-channel full-resolution activations; the unused 1x1 `fc` head
    (models/drn.py:275-276, discarded at batch_spalign_kmeans.py:431) is not evaluated;
  * activations are kept channels-last (NHWC) end to end: that is MIOpen's preferred layout
    for the MFMA implicit-GEMM kernels and it is exactly the layout the pooling kernels of
    libspalign want (C contiguous per feature pixel), so no transpose separates the two;
  * optional bfloat16 execution (`dtype=torch.bfloat16`, BASELINE config 5) with float32
    accumulation inside the convolutions; the pooling kernels read bf16 directly.
Module names follow the upstream checkpoint (conv1/bn1/layerN.M.convK/downsample.0|1/fc) so
`drn_c_26-ddedf421.pth` / `drn_d_22-4bd2f8ea.pth` load with load_state_dict, and
`models/drn_c_26.npz` (Chainer) loads through `load_chainer_npz`.
"""
import collections
import gc
import math
import os
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
CHAINER_BN_EPS = 2e-5

_PLANS = {
    # name: (arch, blocks per layer)
    'drn_c_26': ('C', (1, 1, 2, 2, 2, 2, 1, 1)),
    'drn_d_22': ('D', (1, 1, 2, 2, 2, 2, 1, 1)),
}
_CHANNELS = (16, 32, 64, 128, 256, 512, 512, 512)


def _conv(cin, cout, k, stride=1, dilation=1):
    pad = dilation * (k // 2)
    return nn.Conv2d(cin, cout, k, stride=stride, padding=pad, dilation=dilation, bias=False)


# set by DRN.prepare() on a GPU: libspalign's fused bias/residual/ReLU; 'bytes' accumulates the algorithmic
# HBM bytes of its launches (read y + write y [+ read residual]) for bench.py's roofline entry
_EPILOGUE = {'engine': None, 'bytes': 0, 'launches': 0, 'own_conv': True, 'own_conv32': True, 'winograd': 4, 'wino_saved_flops': 0.0,
             'conv_flops': 0.0, 'light_flops': 0.0, 'light_bytes': 0.0, 'light_launches': 0, 'gemm_flops': 0.0, 'gemm_launches': 0, 'gemm_bytes': 0.0,
             'gemmn_flops': 0.0, 'gemmn_launches': 0, 'gemmn_bytes': 0.0, 'wino_direct_flops': 0.0, 'wino_in_bytes': 0.0,
             'wino_out_bytes': 0.0, 'wino_launches': 0,
             # F(4x4,3x3) GEMMs on the 16-bit matrix cores at float32 accuracy (two half-precision planes per operand, three
             # products: csrc/spa_gemm16.hip); SPA_SPLIT_GEMM=0 keeps the float32 matrix instructions
             'split_gemm': os.environ.get('SPA_SPLIT_GEMM', '1') != '0',
             'gemm16_flops': 0.0, 'gemm16_launches': 0, 'gemm16_bytes': 0.0,
             'gemm16n_flops': 0.0, 'gemm16n_launches': 0, 'gemm16n_bytes': 0.0, 'conv16_flops': 0.0, 'conv16_launches': 0, 'conv16_bytes': 0.0,
             # ... and per kernel instantiation (one `kernels` entry = one rocprofv3 row): c16[kind] = [flops, bytes, launches]
             'c16': {},
             # the layer's OWN bytes of the 256 x 256-tile Winograd layers (X, Y, the residual, the weight planes once): what a
             # convolution that kept V and M on chip would move — bench.py's `algorithmic_bytes` of the GEMM entry
             'gemm16_layer_bytes': 0.0,
             # convolutions handed to MIOpen (F.conv2d) by conv_bias_act: a forward that has any is not captured into a graph
             'library_convs': 0}


def _c16(kind, flops, nbytes, launches=1):
    """per-instantiation counters of the split-plane direct kernels (bench.py prices each against its own rocprofv3 row)"""
    c = _EPILOGUE['c16'].setdefault(kind, [0.0, 0.0, 0])
    c[0] += flops
    c[1] += nbytes
    c[2] += launches


def _epi_snapshot():
    """The numeric counters of _EPILOGUE (bench.py's FLOP / byte accounting), for the graph replay below."""
    snap = {k: v for k, v in _EPILOGUE.items() if isinstance(v, (int, float)) and not isinstance(v, bool)}
    snap['c16'] = {k: list(v) for k, v in _EPILOGUE['c16'].items()}
    return snap


def _epi_restore(snap):
    for k, v in snap.items():
        if k != 'c16':
            _EPILOGUE[k] = v
    _EPILOGUE['c16'] = {k: list(v) for k, v in snap['c16'].items()}


def _epi_delta(before):
    d = {k: _EPILOGUE[k] - v for k, v in before.items() if k != 'c16'}
    d['c16'] = {k: [a - b for a, b in zip(v, before['c16'].get(k, [0.0, 0.0, 0]))] for k, v in _EPILOGUE['c16'].items()}
    return d


def _epi_add(delta):
    for k, v in delta.items():
        if k != 'c16':
            _EPILOGUE[k] += v
    for k, v in delta['c16'].items():
        c = _EPILOGUE['c16'].setdefault(k, [0.0, 0.0, 0])
        for i in range(3):
            c[i] += v[i]


# The forward of a SMALL batch is bound by its ~100 launches, not by the GPU (30 images of 224 x 224, the reference's operating
# point: 9.3 ms of wall clock for 6 ms of kernels; every layer is a few python calls and a ctypes call): such shapes are captured
# once into a HIP graph (torch.cuda.CUDAGraph: the libspalign launches go to torch's current stream, which is the capturing one)
# and replayed — the same kernels with the same arguments, hence the same bits.  SPA_DRN_GRAPH: 1 = every shape, 0 = never,
# unset = batches of at most SPA_DRN_GRAPH_PIXELS pixels (default 4 Mi: full-size batches are GPU bound and keep their
# per-kernel timers).
def _graph_wanted(x):
    mode = os.environ.get('SPA_DRN_GRAPH', '')
    if mode == '0' or not x.is_cuda:
        return False
    if mode == '1':
        return True
    return x.shape[0] * x.shape[2] * x.shape[3] <= int(os.environ.get('SPA_DRN_GRAPH_PIXELS', str(4 << 20)))


# ---- the dispatch of a convolution, a block and a chunk: CHOOSE a route from plain values (no tensor work, no side effect),
# COUNT its FLOPs and bytes into _EPILOGUE (bench.py's roofline rows), LAUNCH the Engine call -------------------------------
F32, BF16 = torch.float32, torch.bfloat16
# what a choice reads from outside its call (debug: spa_debug_set keys 1, 3, 4 of the engine, None without one)
Flags = collections.namedtuple('Flags', 'split_gemm own_conv own_conv32 winograd bf16_light wino_min_cin debug')
# a layer's static facts; folded: BatchNorm folded into its bias; families: the operands prepare() packed for it
Layer = collections.namedtuple('Layer', 'cin cout k stride dilation folded families')
# a call's facts; gpu: an engine and the tensor on the GPU; layout: x and the residual in channels-last storage
Call = collections.namedtuple('Call', 'dtype B H W gpu layout residual relu')


def _flags():
    """Read at EVERY call (the switches are live: bench.py and the tests flip them on prepared models); _graph_forward's key is
    built from the same tuple."""
    E, eng = _EPILOGUE, _EPILOGUE['engine']
    return Flags(E['split_gemm'], E['own_conv'], E['own_conv32'], E['winograd'], os.environ.get('SPA_BF16_LIGHT', '1') != '0',
                 int(os.environ.get('SPA_WINO_MIN_CIN', '256')),
                 None if eng is None else (eng.debug_get(1, 1), eng.debug_get(3, 1), eng.debug_get(4, 2)))


def _nhwc(*tensors):
    """the layout every libspalign kernel wants of its input and (where there is one) of the residual"""
    return all(t is None or t.is_contiguous(memory_format=torch.channels_last) for t in tensors)


def _layer(conv, bn, holder=None):
    return Layer(conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], conv.dilation[0],
                 isinstance(bn, nn.Identity) and conv.bias is not None, tuple(getattr(holder or conv, '_spa_ops', ())))


def _call(x, residual, relu):
    return Call(x.dtype, x.shape[0], x.shape[2], x.shape[3], _EPILOGUE['engine'] is not None and x.is_cuda, _nhwc(x, residual),
                residual is not None, relu)


def _row_fills(W, bn):
    """The direct kernels tile an image ROW into `bn` pixels: on narrow maps most of a tile is padding (28 pixels at the
    reference's 224 x 224 operating point: 403 images/s against 2 113 with MIOpen there).  True where a row fills its tiles to
    80 % (the Winograd kernels flatten the tiles, the split-plane 1x1 form takes the image as one row: neither cares)."""
    return -(-W // bn) * bn <= 1.25 * W


def _out(n, stride):
    return -(-n // stride)


def choose_conv(L, c, f):
    """The route of relu?(conv(x) + bias [+ residual]): one of _CONV's names."""
    if not (c.gpu and L.folded and c.dtype in (F32, BF16)):
        return 'torch'
    fam = L.families
    f32, b16 = c.dtype == F32 and f.own_conv32 and c.layout, c.dtype == BF16 and f.own_conv and c.layout
    if b16 and 'bf16' in fam:
        return 'bf16'
    if b16 and 'light' in fam and f.bf16_light:
        return 'bf16_light'
    bn = 256 if L.cout % 256 == 0 else 128                  # the direct kernel's pixel tile
    wino = ('wino4' if f.winograd == 4 else 'wino2') if f.winograd else None           # 4 (default), 2 or 0 / False
    # with the split-plane kernels the direct form wins below 256 input channels (30 x 128 x 256 pixels, ms Winograd /
    # direct: 128 -> 128 1.10 / 0.99, 128 -> 256 1.85 / 1.61, 256 -> 256 2.65 / 3.09, 256 -> 512 4.28 / 5.35)
    if f32 and wino in fam and not (f.split_gemm and L.cin < f.wino_min_cin and 'direct' in fam and _row_fills(c.W, bn)):
        return 'wino4_f16s' if wino == 'wino4' and f.split_gemm and 'wino4s' in fam else wino + '_f32'
    # (a layer so small that a library convolution's launches cost more than the empty part of the tiles stays direct: the
    # 64-channel layers of a 224 x 224 input; the forward then has no library call left and runs as a captured graph)
    if f32 and 'direct' in fam and (L.k == 1 and f.split_gemm or _row_fills(c.W, bn) or c.B * c.H * c.W <= 1 << 20):
        return ('direct%d_f16s' if f.split_gemm else 'direct%d_f32') % L.k
    if f32 and 'layer2' in fam and c.relu and not c.residual:
        return 'layer2_f16s' if f.split_gemm else 'layer2_f32'
    return 'library'


def choose_block(L, c, f):
    """L: the block's opening convolution, with family 's2' where prepare() packed it together with the projection."""
    if 's2' in L.families and c.gpu and c.dtype == F32 and f.own_conv32 and c.layout:
        if not f.split_gemm:
            return 's2_f32'
        # (narrow maps — 224 x 224 inputs — leave most of a 128-pixel tile empty; the layer is then so small that this costs
        # less than a library convolution and its epilogue pass, and the forward stays capturable)
        if _row_fills(_out(c.W, 2), 128) or c.B * _out(c.H, 2) * _out(c.W, 2) <= 1 << 20:
            return 's2_f16s'
    return 'separate'


def choose_chunk(families, fused, dtype, gpu, f):
    """families: which of the model's front operands ('_front_c', '_stem_c16', '_stem') prepare() packed."""
    if not gpu:
        return 'host'
    if fused and '_front_c' in families and f.split_gemm and f.own_conv32 and dtype == F32:
        return 'front_c'
    if fused and '_stem_c16' in families and f.own_conv and dtype == BF16:
        return 'stem_c16'
    return 'stem_d' if fused and '_stem' in families else 'normalise'


def _flops(px, cout, taps, cin):
    """2 * MACs of a convolution with `px` output pixels"""
    return 2.0 * px * cout * taps * cin


def _work(L, c, proj=0):
    """-> (input pixels, output pixels, 2 * MACs, tensors of the output's size read or written).  proj = 1: a stride-2 opener
    with the block's 1x1 projection in the same pass (a tenth tap, a second output)."""
    opx = c.B * _out(c.H, L.stride) * _out(c.W, L.stride)
    return c.B * c.H * c.W, opx, _flops(opx, L.cout, L.k * L.k + proj, L.cin), (2 if c.residual else 1) + proj


def _add(prefix, flops, nbytes, launches=1):
    _EPILOGUE[prefix + '_flops'] += flops
    _EPILOGUE[prefix + '_bytes'] += nbytes
    _EPILOGUE[prefix + '_launches'] += launches


def _add16(kind, flops, nbytes, launches=1):
    """the split-plane direct kernels (16-bit matrix cores at float32 accuracy): in all and per instantiation"""
    _add('conv16', flops, nbytes, launches)
    _c16(kind, flops, nbytes, launches)


def _count_flops(L, c, proj=0):
    _EPILOGUE['conv_flops'] += _work(L, c, proj)[2]


def _count_light(L, c):
    px, opx, flops, nout = _work(L, c)
    _add('light', flops, 2.0 * (px * L.cin + opx * L.cout * nout))


def _count_f16s(L, c, kind=None, proj=0):
    px, opx, flops, nout = _work(L, c, proj)
    _add16(kind or ('256' if L.cout % 256 == 0 else ('128' if L.cout % 128 == 0 else '64')), flops, 4.0 * (px * L.cin + opx * L.cout * nout))


def _count_gemm1(L, c):
    px, _, flops, _ = _work(L, c)
    _add('gemm' if L.cout % 256 == 0 and not c.residual else 'gemmn', flops, 4.0 * px * (L.cin + L.cout))


def _count_wino(L, c, frac, expand, split):
    """Winograd: F(4x4,3x3) multiplies 36/144 = 1/4 of the direct form's products and expands the activations 2.25x (V, M);
    F(2x2,3x3) 16/36 and 4x.  Executed and direct-equivalent FLOPs are both counted."""
    E, (px, _, direct, nout) = _EPILOGUE, _work(L, c)
    E['wino_direct_flops'] += direct
    E['wino_saved_flops'] += direct * (1.0 - frac)
    wide = L.cout % 256 == 0                                  # the 256 x 256 instance / the narrow tiles
    if split and wide:
        E['gemm16_layer_bytes'] += 4.0 * px * (L.cin + nout * L.cout) + 4.0 * 36 * L.cin * L.cout
    _add(('gemm16' if split else 'gemm') + ('' if wide else 'n'), direct * frac, 4.0 * px * expand * (L.cin + L.cout))  # V read, M written
    E['wino_in_bytes'] += 4.0 * px * (1 + expand) * L.cin                         # k_wino_in reads X and writes V
    E['wino_out_bytes'] += 4.0 * px * (nout + expand) * L.cout                    # M [+ R] read, Y written
    E['wino_launches'] += 1


def _count_library(L, c):
    _EPILOGUE['library_convs'] += 1               # (MIOpen picks its algorithm per call context: such a forward is not captured)


def _amax_on(y, am):
    """the bound on max |y| that scales the next layer's planes travels with the tensor object (in: amax_in=_amax_of(x))"""
    y._spa_amax = am
    return y


def _amax_of(x):
    return getattr(x, '_spa_amax', None)


def _launch_library(eng, conv, x, residual, relu):
    if os.environ.get('SPA_DRN_TRACE_LIBRARY'):
        import sys
        sys.stderr.write('[drn] library convolution: %d -> %d, kernel %s stride %s dilation %s on %s %s\n' % (
            conv.in_channels, conv.out_channels, tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.dilation), tuple(x.shape), x.dtype))
    return _bias_act(eng, conv, F.conv2d(x, conv.weight, None, conv.stride, conv.padding, conv.dilation), residual, relu)


def _count_bias_act(nbytes):
    _EPILOGUE['bytes'] += nbytes                  # read y + write y [+ read residual]
    _EPILOGUE['launches'] += 1


def _bias_act(eng, conv, y, residual, relu):
    """Behind a library convolution, dispatched by the layout the library gave y: libspalign's bias / residual / ReLU as ONE
    in-place pass instead of two or three elementwise kernels."""
    if not (_nhwc(y, residual) and y.shape[1] % (4 if y.dtype == F32 else 8) == 0):
        return _torch_epilogue(y + conv.bias.view(1, -1, 1, 1), residual, relu)
    _count_bias_act(y.numel() * y.element_size() * (3 if residual is not None else 2))
    return eng.bias_act_(y, conv.bias, residual, relu, track_amax=_EPILOGUE['split_gemm'])


def _torch_epilogue(y, residual, relu):
    if residual is not None:
        y = y + residual
    return F.relu_(y) if relu else y


def _launch(method, family, amax=False):
    """eng.method(x, *the family's operands, residual, relu, dilation); amax: a split-plane kernel, which takes the bound on
    max |x| and returns (y, the bound on max |y|)"""
    def launch(eng, m, x, res, relu):
        if not amax:
            return getattr(eng, method)(x, *m._spa_ops[family], res, relu, m.dilation[0])
        return _amax_on(*getattr(eng, method)(x, *m._spa_ops[family], res, relu, m.dilation[0], amax_in=_amax_of(x)))
    return launch


# route: (count(L, c), launch(eng, conv, x, residual, relu))
_CONV = {
    # the bf16 network: the heavy 3x3 stride-1 layers from 64 channels up / the rest (stride 2, 16 / 32 channels, 1x1 projections)
    'bf16': (_count_flops, _launch('conv3x3_bf16', 'bf16')),
    'bf16_light': (_count_light, lambda eng, m, x, res, relu: eng.conv_bf16_light(x, *m._spa_ops['light'], res, relu, m.stride[0], m.dilation[0])),
    # Winograd F(4x4,3x3) on split half-precision planes; F(4x4) and F(2x2) with float32 matrix instructions
    'wino4_f16s': (partial(_count_wino, frac=0.25, expand=2.25, split=True), _launch('conv3x3_wino_f16s', 'wino4s', amax=True)),
    'wino4_f32': (partial(_count_wino, frac=0.25, expand=2.25, split=False), _launch('conv3x3_wino_f32', 'wino4')),
    'wino2_f32': (partial(_count_wino, frac=16.0 / 36.0, expand=4.0, split=False), _launch('conv3x3_wino_f32', 'wino2')),
    # the direct implicit GEMM, 3x3 and (centre tap only) 1x1: on split planes / with float32 matrix instructions (whose 1x1
    # form is counted with the GEMMs)
    'direct3_f16s': (_count_f16s, _launch('conv3x3_f16s', 'direct_s', amax=True)),
    'direct1_f16s': (partial(_count_f16s, kind='1x1'), _launch('conv3x3_f16s', 'direct_s', amax=True)),
    'direct3_f32': (_count_flops, _launch('conv3x3_f32', 'direct')),
    'direct1_f32': (_count_gemm1, _launch('conv3x3_f32', 'direct')),
    # layer 2 of arch D (16 -> 32 channels, stride 2): on split planes / as fmaf chains on the vector pipe
    'layer2_f16s': (partial(_count_f16s, kind='front'), lambda eng, m, x, res, relu: eng.drn_layer2_f16s(x, *m._spa_ops['layer2_s'], amax_in=_amax_of(x))),
    'layer2_f32': (_count_flops, lambda eng, m, x, res, relu: eng.drn_layer2_f32(x, *m._spa_ops['layer2'])),
    'library': (_count_library, _launch_library),                        # MIOpen, then libspalign's bias_act_
}


def _launch_s2_f16s(eng, blk, x):
    y, res, am = eng.conv3x3_s2_f16s(x, *blk._spa_ops['s2_s'], True, amax_in=_amax_of(x))
    return _amax_on(y, am), res


# a block's stride-2 opening convolution and its 1x1 stride-2 projection in ONE pass over x (csrc/spa_conv32.hip):
# route: (count(L, c), launch(eng, block, x) -> (y, the projected residual))
_BLOCK = {'s2_f16s': (partial(_count_f16s, kind='front', proj=1), _launch_s2_f16s),
          's2_f32': (partial(_count_flops, proj=1), lambda eng, blk, x: eng.conv3x3_s2_f32(x, *blk._spa_ops['s2'], True))}


def conv_bias_act(conv, bn, x, residual=None, relu=True):
    """relu?(bn(conv(x)) [+ residual]).  With BatchNorm folded (bn is Identity, conv carries the bias) and the tensors on the
    GPU in channels-last storage this is ONE libspalign kernel with bias, residual and ReLU in its epilogue; the layers no
    kernel takes go to the library's convolution with libspalign's fused epilogue pass behind it."""
    L, c = _layer(conv, bn), _call(x, residual, relu)
    route = choose_conv(L, c, _flags())
    if route == 'torch':
        _EPILOGUE['library_convs'] += 1
        return _torch_epilogue(bn(conv(x)), residual, relu)
    count, launch = _CONV[route]
    count(L, c)
    return launch(_EPILOGUE['engine'], conv, x, residual, relu)


class BasicBlock(nn.Module):
    """conv-bn-relu-conv-bn (+ residual) - relu; `residual=False` for layers 7/8 of arch C."""

    def __init__(self, cin, cout, stride, dilation, residual, eps, project):
        super().__init__()
        self.conv1 = _conv(cin, cout, 3, stride, dilation[0])
        self.bn1 = nn.BatchNorm2d(cout, eps=eps)
        self.conv2 = _conv(cout, cout, 3, 1, dilation[1])
        self.bn2 = nn.BatchNorm2d(cout, eps=eps)
        self.downsample = None
        if project:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(cout, eps=eps))
        self.residual = residual

    def forward(self, x):
        L, c = _layer(self.conv1, self.bn1, self), _call(x, None, True)
        route = choose_block(L, c, _flags())
        if route == 'separate':
            y = conv_bias_act(self.conv1, self.bn1, x, None, True)
            res = None
            if self.residual:
                res = x if self.downsample is None else conv_bias_act(self.downsample[0], self.downsample[1], x, None, False)
        else:
            count, launch = _BLOCK[route]
            count(L, c)
            y, res = launch(_EPILOGUE['engine'], self, x)
        return conv_bias_act(self.conv2, self.bn2, y, res, True)


def _count_front_c(B, _, H, W):
    """layer1's two 16 -> 16 convolutions at full resolution (the first inside the stem kernel, whose 7x7 is not counted), layer2's
    opener 16 -> 32 with its projection and its second convolution 32 -> 32 at half: three launches behind the stem's"""
    px, opx = B * H * W, B * _out(H, 2) * _out(W, 2)
    _add16('front', _flops(px, 16, 9, 16) + _flops(opx, 32, 9 + 1, 16) + _flops(opx, 32, 9, 32),
           4.0 * (px * (16 + 16 + 16) + px * 16 + opx * (32 + 32) + opx * (32 + 32 + 32)), 3)


def _launch_front_c(model, eng, xc):
    """DRN-C: conv1 .. layer2 on libspalign's kernels (no MIOpen convolution, no separate epilogue pass)"""
    fc = model._front_c
    a1, y0 = eng.drn_stem_d(xc.float().contiguous(), *fc['stem'], dtype=F32, split=True, want_layer0=True)
    l1, _ = eng.conv_small_f16s(a1, *fc['l1c2'], 16, 1, 0, y0, True, amax_in=a1._spa_amax)
    a2, proj = eng.conv_small_f16s(l1, *fc['l2c1'], 32, 2, 32, None, True, amax_in=l1._spa_amax)
    l2, _ = eng.conv_small_f16s(a2, *fc['l2c2'], 32, 1, 0, proj, True, amax_in=a2._spa_amax)
    return model.forward_maps(None, front_maps=[l1, l2])


def _launch_stem_c16(model, eng, xc):
    a1, y0 = eng.drn_stem_d(xc.float().contiguous(), *model._stem_c16, dtype=BF16, want_layer0=True)
    b1 = model.layer1[0]
    return model.forward_maps(None, front_maps=[conv_bias_act(b1.conv2, b1.bn2, a1, y0, True)])


def _launch_host(model, eng, xc):
    xi = model.normalise(xc.float())
    return model.forward(xi.to(model.compute_dtype).contiguous(memory_format=torch.channels_last))[1]


# route: (count(B, 3, H, W) or None, launch(model, eng, raw sub-batch) -> the 8 maps)
_CHUNK = {
    'front_c': (_count_front_c, _launch_front_c),
    'stem_c16': (None, _launch_stem_c16),
    'stem_d': (None, lambda model, eng, xc: model.forward_maps(None, layer1_out=eng.drn_stem_d(
        xc.float().contiguous(), *model._stem, dtype=model.compute_dtype, split=_EPILOGUE['split_gemm'] and model.compute_dtype == F32))),
    'normalise': (None, lambda model, eng, xc: model.forward(eng.drn_normalise(xc.float().contiguous(), model.compute_dtype))[1]),
    'host': (None, _launch_host),
}


# ---- what prepare() packs: eligibility is a pure predicate of the layer and the network's dtype ----------------------------
def conv_families(m, dtype, folded):
    """The operand families of convolution `m` in a network of `dtype`.  Winograd where it wins (measured, 30 x 128 x 256
    pixels, ms direct / F(2x2) / F(4x4)):
      512 -> 512  33.2 / 19.8 / 11.9     256 -> 512  16.8 / 11.6 / 7.0     256 -> 256  8.5 / 6.6 / 4.2
      128 -> 256   4.3 /  4.1 /  2.6     128 -> 128   2.4 /  2.4 / 1.6      64 -> 64 (256 x 512)  2.6 / - / 2.7
    so F(4x4,3x3) from 128 input channels up and F(2x2,3x3) (kept as an option) from 256."""
    if not (folded and m.groups == 1 and m.bias is not None and dtype in (F32, BF16)):
        return ()
    k, s, d, pad, ci, co = m.kernel_size, m.stride, m.dilation, m.padding, m.in_channels, m.out_channels
    same3 = k == (3, 3) and pad == d and d[0] == d[1]                  # 3x3, padding = dilation
    one = k == (1, 1) and pad == (0, 0)
    fam = []
    if dtype == F32:
        if same3 and s == (2, 2) and d == (1, 1) and ci == 16 and co == 32:
            fam += ['layer2', 'layer2_s']                             # layer 2 of arch D (_s: as split half-precision planes)
        if same3 and s == (1, 1) and ci % 32 == 0 and co % 64 == 0 and ci >= 128 and co >= 128:
            fam.append('wino4')
            if co % 128 == 0:
                fam.append('wino4s')                                  # ... as split half-precision planes
            if ci >= 256 and co >= 256:
                fam.append('wino2')
        # spa_conv3x3_f32 / _f16s: the 3x3 stride-1 layers from 64 channels up, and the 1x1 stride-1 projections (layers 5, 6)
        # through the same kernel, centre tap only
        if (same3 and d[0] <= 4 or one) and s == (1, 1) and ci % 32 == 0 and co % 64 == 0:
            fam += ['direct', 'direct_s']
    elif same3 and s == (1, 1) and d[0] <= 4 and ci % 64 == 0 and co % 64 == 0:
        fam.append('bf16')                                            # spa_conv3x3_bf16: layers 3-8 of the DRN
    elif (s in ((1, 1), (2, 2)) and (same3 and ci in (16, 32, 64) or one and ci in (16, 32, 64, 128, 256))
          and (co % 64 == 0 and ci >= 32 or co % 32 == 0 and ci <= 32 or co % 16 == 0 and ci == 16)):
        fam.append('light')                                           # spa_conv_bf16_light: every other convolution
    return tuple(fam)


def _pack_conv(m, fam, Engine):
    """{family: operands}; bias float32, weights as (n, tap, c)"""
    if not fam:
        return {}
    ops, bias = {}, m.bias.detach().float().contiguous()
    wt = m.weight.detach().permute(0, 2, 3, 1).reshape(m.out_channels, -1, m.in_channels).contiguous()
    if 'layer2' in fam:     # (the strict float32 network's form: (tap, input channel, output channel) float32)
        ops['layer2'] = (m.weight.detach().float().permute(2, 3, 1, 0).reshape(9, 16, 32).contiguous(), bias)
        ops['layer2_s'] = Engine.layer2_planes(m.weight) + (bias,)
    for name, tile in (('wino4', 4), ('wino2', 2)):
        if name in fam:
            ops[name] = (Engine.winograd_weights(m.weight, tile), bias)
    if 'wino4s' in fam:
        ops['wino4s'] = Engine.winograd_weights_split(m.weight) + (bias,)
    if 'direct' in fam:
        ops['direct'] = (wt.float(), bias)
        ops['direct_s'] = Engine.split_planes(wt.float()) + (bias,)
    if 'bf16' in fam or 'light' in fam:
        ops[fam[0]] = (wt.to(BF16), bias)
    return ops


def block_families(blk, dtype, folded):
    c1, ds = blk.conv1, blk.downsample
    return ('s2', 's2_s') if (dtype == F32 and folded and blk.residual and ds is not None and c1.stride == (2, 2)
                               and c1.kernel_size == (3, 3) and c1.padding == (1, 1) and c1.dilation == (1, 1) and c1.bias is not None
                               and ds[0].kernel_size == (1, 1) and ds[0].stride == (2, 2) and ds[0].bias is not None
                               and c1.in_channels % 32 == 0 and c1.out_channels % 64 == 0) else ()


def _pack_block(blk, fam, Engine):
    """the opener's and (centre tap) the projection's weights as one (2 Cout, 9, Cin) convolution, both biases, Cout"""
    if not fam:
        return {}
    c1, ds = blk.conv1, blk.downsample
    co, ci = c1.out_channels, c1.in_channels
    w = torch.zeros((2 * co, 9, ci), dtype=F32, device=c1.weight.device)
    w[:co] = c1.weight.detach().float().permute(0, 2, 3, 1).reshape(co, 9, ci)
    w[co:, 4] = ds[0].weight.detach().float().reshape(co, ci)
    bias = torch.cat([c1.bias.detach().float(), ds[0].bias.detach().float()]).contiguous()
    return {'s2': (w.contiguous(), bias, co), 's2_s': Engine.split_planes(w) + (bias, co)}


def _pack_stem(c0, c1):
    """operands of the fused stem kernels: the 7x7 and the first 3x3 convolution, weights as (n, ky kx c)"""
    return (c0.weight.detach().float().reshape(16, 147).contiguous(), c0.bias.detach().float().contiguous(),
            c1.weight.detach().float().permute(0, 2, 3, 1).reshape(16, 144).contiguous(), c1.bias.detach().float().contiguous())


class DRN(nn.Module):
    def __init__(self, name='drn_c_26', bn_eps=CHAINER_BN_EPS, num_classes=1000, with_fc=False):
        super().__init__()
        arch, plan = _PLANS[name]
        self.name, self.arch = name, arch
        ch = _CHANNELS
        self._cin = ch[0]
        eps = bn_eps
        stem = [_conv(3, ch[0], 7), nn.BatchNorm2d(ch[0], eps=eps)]
        if arch == 'C':
            self.conv1, self.bn1 = stem
            self.layer1 = self._blocks(ch[0], plan[0], 1, 1, True, True, eps)
            self.layer2 = self._blocks(ch[1], plan[1], 2, 1, True, True, eps)
        else:
            self.layer0 = nn.Sequential(*stem, nn.ReLU(inplace=True))
            self.layer1 = self._plain(ch[0], plan[0], 1, 1, eps)
            self.layer2 = self._plain(ch[1], plan[1], 2, 1, eps)
        self.layer3 = self._blocks(ch[2], plan[2], 2, 1, True, True, eps)
        self.layer4 = self._blocks(ch[3], plan[3], 2, 1, True, True, eps)
        self.layer5 = self._blocks(ch[4], plan[4], 1, 2, False, True, eps)
        self.layer6 = self._blocks(ch[5], plan[5], 1, 4, False, True, eps)
        if arch == 'C':
            self.layer7 = self._blocks(ch[6], plan[6], 1, 2, False, False, eps)
            self.layer8 = self._blocks(ch[7], plan[7], 1, 1, False, False, eps)
        else:
            self.layer7 = self._plain(ch[6], plan[6], 1, 2, eps)
            self.layer8 = self._plain(ch[7], plan[7], 1, 1, eps)
        self.fc = nn.Conv2d(ch[7], num_classes, 1) if with_fc else None
        self.folded = False
        self.compute_dtype = torch.float32
        self.use_fused_stem = True      # arch D, float32, folded BN, on the GPU: libspalign's stem kernel
        self._stem = None
        for m in self.modules():           # the reference's random init (models/drn.py:176-184)
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2.0 / n))
        self.eval()

    # -- builders --------------------------------------------------------------------------
    def _blocks(self, cout, count, stride, dilation, new_level, residual, eps):
        cin = self._cin
        project = stride != 1 or cin != cout
        first = (1, 1) if dilation == 1 else ((dilation // 2 if new_level else dilation), dilation)
        mods = [BasicBlock(cin, cout, stride, first, residual, eps, project)]
        for _ in range(1, count):
            mods.append(BasicBlock(cout, cout, 1, (dilation, dilation), residual, eps, False))
        self._cin = cout
        return nn.Sequential(*mods)

    def _plain(self, cout, count, stride, dilation, eps):
        mods = []
        for i in range(count):
            mods += [_conv(self._cin, cout, 3, stride if i == 0 else 1, dilation),
                     nn.BatchNorm2d(cout, eps=eps), nn.ReLU(inplace=True)]
            self._cin = cout
        return nn.Sequential(*mods)

    # -- inference-time transformations ---------------------------------------------------------
    @torch.no_grad()
    def fold_batchnorm(self):
        """Fold every BatchNorm into the convolution in front of it (eval-mode identity)."""
        def fold(conv, bn):
            scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
            conv.weight.mul_(scale.reshape(-1, 1, 1, 1))
            bias = bn.bias - bn.running_mean * scale
            conv.bias = nn.Parameter(bias if conv.bias is None else conv.bias * scale + bias)
            return nn.Identity()

        def walk(seq):
            mods = list(seq.children())
            for i, m in enumerate(mods[:-1]):
                if isinstance(m, nn.Conv2d) and isinstance(mods[i + 1], nn.BatchNorm2d):
                    seq[i + 1] = fold(m, mods[i + 1])
        if self.folded:
            return self
        if self.arch == 'C':
            self.bn1 = fold(self.conv1, self.bn1)
        for m in self.modules():
            if isinstance(m, BasicBlock):
                m.bn1 = fold(m.conv1, m.bn1)
                m.bn2 = fold(m.conv2, m.bn2)
                if m.downsample is not None:
                    walk(m.downsample)
            elif isinstance(m, nn.Sequential):
                walk(m)
        self.folded = True
        return self

    def prepare(self, device='cuda', dtype=torch.float32, fold_bn=True):
        """Move to the GPU in the layout/dtype the hot path runs in."""
        if fold_bn:
            self.fold_batchnorm()
        self.compute_dtype = dtype
        self.to(device=device, dtype=dtype, memory_format=torch.channels_last)
        self.eval()
        self.__dict__.pop('_graphs', None)              # captured forwards hold the OLD packed operands' addresses
        self._stem = None
        if torch.device(device).type == 'cuda':
            from .engine import default_engine, Engine        # fused glue kernels of libspalign
            _EPILOGUE['engine'] = default_engine()
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    m._spa_ops = _pack_conv(m, conv_families(m, dtype, self.folded), Engine)
                elif isinstance(m, BasicBlock):
                    m._spa_ops = _pack_block(m, block_families(m, dtype, self.folded), Engine)
            fam = self.front_families(dtype)
            f32 = lambda t: t.detach().float().contiguous()
            self._front_c = None
            if '_front_c' in fam:
                # DRN-C's full-resolution front on libspalign's own kernels (csrc/spa_stem.hip, spa_convs.hip): conv1 + layer1's first
                # convolution as the fused stem (which also stores conv1's output, the block's residual), layer1's second convolution,
                # layer2's stride-2 opener together with its 1x1 projection, layer2's second convolution
                c0, b1, b2 = self.conv1, self.layer1[0], self.layer2[0]
                self._front_c = dict(
                    stem=_pack_stem(c0, b1.conv1),
                    l1c2=Engine.small_planes(b1.conv2.weight) + (f32(b1.conv2.bias),),
                    l2c1=Engine.small_planes(b2.conv1.weight, b2.downsample[0].weight)
                    + (torch.cat([f32(b2.conv1.bias), f32(b2.downsample[0].bias)]).contiguous(),),
                    l2c2=Engine.small_planes(b2.conv2.weight) + (f32(b2.conv2.bias),))
            # bf16 DRN-C: conv1 + layer1's first convolution as the fused bf16 stem (which also stores conv1's output, the
            # block's residual); the rest of layers 1 / 2 runs on spa_conv_bf16_light through the modules
            self._stem_c16 = _pack_stem(self.conv1, self.layer1[0].conv1) if '_stem_c16' in fam else None
            # libspalign's fused stem kernel of arch D (normalise + layer0 + layer1)
            self._stem = _pack_stem(self.layer0[0], self.layer1[0]) if '_stem' in fam else None
        return self

    # -- forward ---------------------------------------------------------------------------------
    def forward_maps(self, x, layer1_out=None, front_maps=None):
        """x: normalised (B,3,H,W) (or None with `layer1_out`, the fused stem's output, or `front_maps`, the outputs of the
        first len(front_maps) layers computed by libspalign's front kernels).  Returns the 8 maps of the Chainer convention."""
        def plain(seq, t):
            mods = list(seq.children())            # (conv, bn | Identity, relu) triples
            for i in range(0, len(mods), 3):
                t = conv_bias_act(mods[i], mods[i + 1], t, None, True)
            return t

        first = 1
        maps = []
        if front_maps is not None:
            maps = list(front_maps)
            x = maps[-1]
            first = len(maps) + 1
        elif layer1_out is not None:           # the fused stem already produced layer1's output
            x = layer1_out
            maps.append(x)
            first = 2
        elif self.arch == 'C':
            x = conv_bias_act(self.conv1, self.bn1, x, None, True)
        else:
            x = plain(self.layer0, x)
        for i in range(first, 9):
            layer = getattr(self, 'layer%d' % i)
            x = plain(layer, x) if (self.arch == 'D' and i in (1, 2, 7, 8)) else layer(x)
            maps.append(x)
            hook = self.__dict__.get('_layer_hook')
            if hook is not None:
                hook(i)                            # (LabelPipeline: work for another stream enqueued once layer i is in the queue)
        return maps

    def forward(self, x):
        maps = self.forward_maps(x)
        return (self.fc(maps[-1]) if self.fc is not None else None), maps

    @staticmethod
    def normalise(x):
        """DRN.batch_predict arithmetic (models/drn.py:319-321) without touching the input."""
        mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float64, device=x.device).view(1, 3, 1, 1)
        std = torch.tensor(IMAGENET_STD, dtype=torch.float64, device=x.device).view(1, 3, 1, 1)
        x = x / 255.0
        x = (x.double() - mean).float()
        x = (x.double() / std).float()
        return x

    def front_families(self, dtype):
        """Which front operands prepare() packs for a network of `dtype`: '_front_c', '_stem_c16', '_stem' (the attributes)."""
        if not self.folded:
            return ()
        if self.arch == 'D':
            return ('_stem',) if dtype in (F32, BF16) else ()
        c0, b1, b2 = self.conv1, self.layer1[0], self.layer2[0]
        if dtype == F32 and (len(self.layer1) == 1 and len(self.layer2) == 1 and b1.residual and b1.downsample is None and b2.residual
                             and b2.downsample is not None and b2.conv1.stride == (2, 2) and b2.downsample[0].stride == (2, 2)
                             and all(c.bias is not None for c in (c0, b1.conv1, b1.conv2, b2.conv1, b2.conv2, b2.downsample[0]))):
            return ('_front_c',)
        if dtype == BF16 and (len(self.layer1) == 1 and b1.residual and b1.downsample is None and c0.bias is not None
                              and b1.conv1.bias is not None and b1.conv1.stride == (1, 1) and b1.conv1.dilation == (1, 1)):
            return ('_stem_c16',)
        return ()

    def _forward_chunk(self, xc):
        """One sub-batch: raw (b,3,H,W) float32 0..255 -> the 8 maps."""
        eng = _EPILOGUE['engine']
        fam = tuple(n for n in ('_front_c', '_stem_c16', '_stem') if getattr(self, n, None) is not None)
        route = choose_chunk(fam, self.use_fused_stem, self.compute_dtype, eng is not None and xc.is_cuda, _flags())
        count, launch = _CHUNK[route]
        if count is not None:
            count(*xc.shape)
        return launch(self, eng, xc)

    @torch.no_grad()
    def batch_predict(self, x, sub_batch=None, need=None, streams=1):
        """x: (B,3,H,W) float32 RGB 0..255 (numpy or tensor). -> (logits or None, [8 maps]).

        need: indices of the maps the caller will use (the others come back as None: for the
        default --use_feature_maps 7 that avoids keeping / concatenating 38 GB of activations per
        batch of 30 full-size images).  streams: run that many parts of the batch on side streams
        — the memory-bound epilogue passes of one part then run under the MFMA-bound convolutions
        of another (2 parts of 15: the forward is 2 % shorter than with one part of 30, but in the
        full pipeline the label kernels that follow lose as much, so callers leave it at 1).
        Unlike the reference's --gpu -1 path the input array is never modified (the GPU path
        of the reference copies it too, which is the behaviour the launchers rely on)."""
        dev = next(self.parameters()).device
        x = torch.as_tensor(x)
        if x.device != dev:
            x = x.to(dev, non_blocking=True)
        assert x.ndim == 4 and x.shape[1] == 3
        B = x.shape[0]
        keep = set(range(8)) if need is None else set(int(i) for i in need)

        def pick(maps):
            return [m if i in keep else None for i, m in enumerate(maps)]

        parts = []
        if streams > 1 and x.is_cuda and B >= 2 * streams and not sub_batch:
            if len(getattr(self, '_side', ())) < streams:
                self._side = [torch.cuda.Stream(device=dev) for _ in range(streams)]
            cur = torch.cuda.current_stream(dev)
            per = (B + streams - 1) // streams
            for i in range(streams):
                lo, hi = i * per, min(B, (i + 1) * per)
                if lo >= hi:
                    break
                st = self._side[i]
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    xc = x[lo:hi]
                    xc.record_stream(st)
                    parts.append(pick(self._forward_chunk(xc)))
            for i in range(len(parts)):
                cur.wait_stream(self._side[i])
                for m in parts[i]:
                    if m is not None:
                        m.record_stream(cur)
        elif not sub_batch and _EPILOGUE['engine'] is not None and _graph_wanted(x) and not torch.is_grad_enabled():
            parts.append(self._graph_forward(x, keep, pick))
        else:
            sub = B if not sub_batch else sub_batch
            for s in range(0, B, sub):
                parts.append(pick(self._forward_chunk(x[s:s + sub])))
        maps = []
        for i in range(8):
            col = [p[i] for p in parts]
            maps.append(None if col[0] is None else (col[0] if len(col) == 1 else torch.cat(col, 0)))
        return None, maps

    def _graph_forward(self, x, keep, pick):
        """batch_predict's single-chunk forward as a captured graph (see _graph_wanted).  Falls back to the eager forward for a
        shape whose capture failed (and says so once)."""
        E = _EPILOGUE
        eng = E['engine']
        key = (tuple(x.shape), x.dtype, tuple(x.stride()), self.compute_dtype, tuple(sorted(keep))) + _flags() + (id(eng), self.use_fused_stem)
        cache = self.__dict__.setdefault('_graphs', {})
        # a captured launch holds the addresses of libspalign's workspaces (packed stem weights, the zero line, ...): when one of
        # them has been re-allocated since (another model or a larger shape on the same context), every graph is stale
        gen = eng.ws_generation()
        if self.__dict__.get('_graphs_gen') != gen:
            cache.clear()
            self._graphs_gen = gen
        ent = cache.get(key)
        if ent is None:
            # (a graph keeps its input and every activation of the forward: bound what a stream of odd shapes can pin — at most 8
            # graphs and SPA_DRN_GRAPH_BYTES (default 8 GiB) of pinned activations, estimated at 40 x the input)
            limit = int(os.environ.get('SPA_DRN_GRAPH_BYTES', str(8 << 30)))
            need = 40 * x.numel() * 4
            while cache and (len(cache) >= 8 or sum(e[4] for e in cache.values() if e) + need > limit):
                cache.pop(next(iter(cache)))
            ent = self._graph_capture(x, pick)
            if ent is not False:
                ent = ent + (need,)
            if eng.ws_generation() != gen:          # the capture's warm-up grew a workspace: graphs captured before it are stale
                cache.clear()
                self._graphs_gen = eng.ws_generation()
            cache[key] = ent
        if ent is False:
            return pick(self._forward_chunk(x))
        graph, g_in, g_out, delta, _ = ent
        g_in.copy_(x)
        graph.replay()
        _epi_add(delta)
        # (the graph's outputs are overwritten by the next replay: the caller gets its own copy)
        return [None if m is None else m.clone(memory_format=torch.preserve_format) for m in g_out]

    def _graph_capture(self, x, pick):
        eng = _EPILOGUE['engine']
        dev = x.device
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(device=dev)
        g_in = x.clone(memory_format=torch.preserve_format)
        snap = _epi_snapshot()
        prof_was = eng.prof_is_on()
        try:
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(2):                  # workspaces, kernel attributes, MIOpen's find: nothing of that inside the capture
                    self._forward_chunk(g_in)
            cur.wait_stream(side)
            torch.cuda.synchronize(dev)
            _epi_restore(snap)
            if prof_was:
                eng.prof_enable(False)              # (event records of the per-kernel timers do not belong into a graph)
            graph = torch.cuda.CUDAGraph()
            # A garbage collection inside the capture runs finalisers in this thread, and Engine.__del__ frees device memory
            # (spa_ctx_destroy), which a capturing thread may not do: the capture is invalidated and the stream stays unusable.
            # A driver called several times in one process leaves such engines behind in reference cycles.  So collect them
            # now and let no collection start before the capture has ended.
            gc.collect()
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph, stream=side, capture_error_mode='thread_local'):
                    g_out = pick(self._forward_chunk(g_in))
            finally:
                if gc_was_on:
                    gc.enable()
            delta = _epi_delta(snap)
            _epi_restore(snap)
            if delta.get('library_convs', 0) > 0 and os.environ.get('SPA_DRN_GRAPH') != '1':
                # MIOpen chooses its algorithm (and with it the summation order) differently inside a capture: the bits of an
                # eager forward are the contract, so a forward with library convolutions in it stays eager
                return False
            return graph, g_in, g_out, delta
        except Exception as e:                      # noqa: BLE001 - any capture failure means: run this shape eagerly
            import warnings
            warnings.warn('DRN forward of shape %s not captured into a graph (%s: %s); running it launch by launch'
                          % (tuple(x.shape), type(e).__name__, e))
            _epi_restore(snap)
            return False
        finally:
            if prof_was:
                eng.prof_enable(True)

    class _XP(object):
        """`model.xp` of the reference API (utils/apply_spalign_kmeans.py:30)."""
        @staticmethod
        def asarray(a):
            return torch.as_tensor(a)

    xp = _XP()

    # -- weights ---------------------------------------------------------------------------------
    def load_pth(self, path):
        sd = torch.load(path, map_location='cpu')
        sd = {k: v for k, v in sd.items() if self.fc is not None or not k.startswith('fc.')}
        self.load_state_dict(sd, strict=True)
        return self

    def load_chainer_npz(self, path):
        """models/drn_c_26.npz written by the reference's convert_pth2ch.py (chainer save_npz).

        Key grammar of chainer.serializers.save_npz: a Chain names its children by attribute ("layer3", "conv1",
        "downsample"), the reference's Sequential is a ChainList (models/sequential.py:9, :272-290) and numbers
        ONLY its links, in insertion order — F.relu entries are skipped, so Sequential(conv, bn, relu, conv, bn,
        relu) saves "0/W", "1/gamma", "2/W", "3/gamma" where torch's nn.Sequential has modules 0, 1, 3, 4.  A link
        holds W, b (Convolution2D), gamma, beta, avg_mean, avg_var, N (BatchNormalization)."""
        rename = {'W': 'weight', 'b': 'bias', 'gamma': 'weight', 'beta': 'bias',
                  'avg_mean': 'running_mean', 'avg_var': 'running_var'}
        own = self.state_dict()

        def resolve(parts):
            mod, out = self, []
            for p in parts:
                if isinstance(mod, nn.Sequential) and p.isdigit():
                    links = [i for i, m in enumerate(mod) if any(True for _ in m.parameters())]
                    if int(p) >= len(links):
                        raise KeyError('no link %s under %s' % (p, '.'.join(out)))
                    p = str(links[int(p)])
                out.append(p)
                mod = getattr(mod, p) if not p.isdigit() else mod[int(p)]
            return out
        with np.load(path) as z:
            for key in z.files:
                parts = key.split('/')
                if parts[-1] == 'N' or (parts[0] == 'fc' and self.fc is None):
                    continue
                try:
                    name = '.'.join(resolve(parts[:-1]) + [rename[parts[-1]]])
                except (AttributeError, IndexError, KeyError):
                    raise KeyError('unexpected entry %s in %s' % (key, path))
                if name not in own:
                    raise KeyError('unexpected entry %s in %s' % (key, path))
                own[name].copy_(torch.from_numpy(z[key]).reshape(own[name].shape))
        return self


def flops_per_image(name, H, W):
    """2*MACs of the convolutions (fc excluded) — BASELINE.md section 3."""
    per_full = {'drn_c_26': 1418.6e9, 'drn_d_22': 1089.5e9}[name]
    return per_full * (H * W) / (1024.0 * 2048.0)


def create_drn(name='drn_c_26', weights=None, device='cuda', dtype=torch.float32, fold_bn=True,
               bn_eps=CHAINER_BN_EPS, seed=0):
    """Factory behind create_model(): random init (seeded) unless a weight file is given."""
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    model = DRN(name, bn_eps=bn_eps)
    torch.random.set_rng_state(gen_state)
    if weights:
        if weights.endswith('.npz'):
            model.load_chainer_npz(weights)
        else:
            model.load_pth(weights)
    return model.prepare(device, dtype, fold_bn)
