"""SegNet-Basic training (train_segnet.py --model basic) on libspalign's kernels, without Chainer.

models/segnet_basic.py in train mode, one step:

    y_i = conv7x7(h; W_i)                          no bias; csrc/spa_segnet_train.hip (forward, dgrad, wgrad)
    h, idx_i = maxpool2x2_argmax(relu(bn(y_i)))    conv1 .. conv4 (conv1's input: the LRN-normalised image)
    h = bn(conv7x7(unpool(h, idx_i)))              decode4 .. decode1, indices of pool4 .. pool1
    score = conv_classifier(h)                     1x1, 64 -> 2, with bias
    loss = softmax_cross_entropy | soft-label cross entropy | mean squared error

BatchNorm uses the batch statistics (biased variance + 2e-5; the forward kernel's per-channel sums of y and y^2) and
updates the running averages with decay 0.9 and the unbiased variance.  BatchNorm, ReLU, pooling, the scatter through
the index maps, the classifier and the loss are torch ops; every 7x7 convolution and its two gradients is a kernel.
The optimizers are Chainer's MomentumSGD (v = 0.9 v - lr g; p += v) with WeightDecay and ExponentialShift, and
Chainer's Adam.  `reference_loss` restates the whole step in float64 torch ops (F.conv2d), for the tests.

dtype 'bf16' (SegNetTrainer(..., dtype='bf16'), train_segnet.py --dtype bf16) runs the 7x7 passes on the bf16 matrix
cores (csrc/spa_segnet_train_bf16.hip): every product operand (conv input, weight, output gradient) is rounded to bf16,
the products accumulate in float32, and everything else -- the float32 master weights, BatchNorm, pooling, the
classifier, the loss and the optimizers -- is the float32 path unchanged.  `reference_loss(..., bf16_operands=True)`
restates that step in float64.

split_planes (SegNetTrainer(..., split_planes=True), train_segnet.py --split_planes) runs the 7x7 passes of a float32
step at float32 accuracy on the f16 matrix cores (csrc/spa_segnet_train_f16x3.hip): every operand tensor is scaled by a
power of two and carried as two half-precision planes, three products per float32 product, float32 accumulation.
Everything else is the float32 path unchanged; its float64 restatement is `reference_loss` with unrounded operands.

fused_bn (SegNetTrainer(..., fused_bn=True), train_segnet.py --fused_bn; with any of the three convolution families)
runs what lies between the convolutions on the kernels of csrc/spa_segnet_train_bn.hip instead of torch ops: an encoder
layer's BatchNorm + ReLU + pooling in one pass that stores the pooled map and its index map, a decoder layer's
BatchNorm, their backward (the two per-channel sums in float64, then dy) and the classifier with its backward.  The
batch statistics, the mean / var / rstd arithmetic, bn_update, the losses and the optimizers are the code below
unchanged; `reference_loss` is its float64 restatement too.

Data parallelism (train_segnet.py --data_parallel, SegNetTrainer.set_group(RankGroup())): one rank per GPU under
torchrun, BatchNorm over the union of the ranks' batches and the mean of the ranks' gradients; see RankGroup.
"""
import os
import zipfile

import numpy as np

from . import segnet
from .segnet import BN_EPS, DECODERS, DTYPES, ENCODERS, LAYERS, MEAN, STD

BN_DECAY = 0.9
DTYPE_KEY = 'extensions/dtype'        # the snapshot entry that records the dtype of the run that wrote it
SPLIT_PLANES_KEY = 'extensions/split_planes'   # present (True) only in snapshots of split-plane runs
BETA_INIT = 0.001
PARAM_KEYS = tuple([n + '/W' for n in LAYERS] + ['%s_bn/%s' % (n, p) for n in LAYERS for p in ('gamma', 'beta')]
                   + ['conv_classifier/W', 'conv_classifier/b'])
STAT_KEYS = tuple('%s_bn/%s' % (n, p) for n in LAYERS for p in ('avg_mean', 'avg_var'))


def _torch():
    import torch
    return torch


# ------------------------------------------------------------------------------- parameters
def init_params(seed=0):
    """Chainer's initial state of SegNetBasic(n_class=2): HeNormal (std sqrt(2 / fan_in)) for every convolution and
    the classifier, classifier bias 0, BN gamma 1, beta 0.001, avg_mean 0, avg_var 1.  float32 numpy, Chainer layout."""
    rng = np.random.RandomState(seed)
    p = {}
    for i, name in enumerate(LAYERS):
        cin = 3 if i == 0 else 64
        p[name + '/W'] = (rng.normal(0.0, np.sqrt(2.0 / (cin * 49)), (64, cin, 7, 7))).astype(np.float32)
        p[name + '_bn/gamma'] = np.ones(64, np.float32)
        p[name + '_bn/beta'] = np.full(64, BETA_INIT, np.float32)
        p[name + '_bn/avg_mean'] = np.zeros(64, np.float32)
        p[name + '_bn/avg_var'] = np.ones(64, np.float32)
    p['conv_classifier/W'] = rng.normal(0.0, np.sqrt(2.0 / 64), (2, 64, 1, 1)).astype(np.float32)
    p['conv_classifier/b'] = np.zeros(2, np.float32)
    return p


# ------------------------------------------------------------------------------- shared torch pieces
def conv1_input(img):
    """The conv1 input as the kernels see it, in float64: the dataset's two float32 operations on the 0..255 image
    (B,3,H,W), then Chainer's LRN (n 5 covers all three channels, k 1, alpha 1e-4 / 5, beta 0.75) in float64."""
    torch = _torch()
    x = img.float()
    x = (x - torch.as_tensor(MEAN, device=x.device)[None, :, None, None]) / \
        torch.as_tensor(STD, device=x.device)[None, :, None, None]
    x = x.double()
    return x * (1.0 + 1e-4 / 5 * (x * x).sum(1, keepdim=True)) ** -0.75


def unpool_ref(h, idx):
    """F.upsampling_2d with 2x2 windows: h, idx (B,C,h,w) (idx = ky * 2 + kx) -> (B,C,2h,2w), h at the selected
    position of each block, zero elsewhere (differentiable in h)."""
    torch = _torch()
    B, C, hh, ww = h.shape
    parts = [h * (idx == r).to(h.dtype) for r in range(4)]
    z = torch.stack(parts, -1).view(B, C, hh, ww, 2, 2)
    return z.permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * hh, 2 * ww)


def pool_argmax_nhwc(a):
    """a (B,H,W,C) -> (max over each 2x2 window (B,H/2,W/2,C), the index of its FIRST maximum uint8 (ky * 2 + kx))."""
    torch = _torch()
    B, H, W, C = a.shape
    win = a.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
    idx = torch.argmax(win, -1, keepdim=True)                 # the first maximal value's index
    return win.gather(-1, idx)[..., 0], idx[..., 0].to(torch.uint8)


def softmax_cross_entropy(score, t):
    """chainer.functions.softmax_cross_entropy, normalize=True, ignore_label -1: the summed loss of the labelled
    pixels divided by max(#labelled, 1)."""
    F = _torch().nn.functional
    t = t.long()
    n = int((t != -1).sum())
    return F.cross_entropy(score, t, ignore_index=-1, reduction='sum') / max(n, 1)


def soft_label_loss(score, t):
    """-mean(t * log_softmax(y)) over all B * 2 * H * W elements (train_segnet.py softmax_cross_entropy_with_soft_labels)."""
    F = _torch().nn.functional
    return -(t * F.log_softmax(score, 1)).mean()


def mse_loss(score, t):
    return ((score - t) ** 2).mean()


def loss_function(use_soft_label=False, use_mse=False):
    if use_soft_label:
        return soft_label_loss
    if use_mse:
        return mse_loss
    return softmax_cross_entropy


def bn_update(avg_mean, avg_var, mean, var_biased, m):
    """Chainer's running-average update in place: decay 0.9, the variance unbiased by m / max(m - 1, 1)."""
    adjust = m / max(m - 1.0, 1.0)
    avg_mean *= BN_DECAY
    avg_mean += (1.0 - BN_DECAY) * mean
    avg_var *= BN_DECAY
    avg_var += (1.0 - BN_DECAY) * adjust * var_biased


# ------------------------------------------------------------------------------- float64 restatement
def bf16_round(t):
    """The operand rounding of the bf16 passes: t rounded to bfloat16 (round to nearest even, subnormals kept),
    returned in t's dtype.  It is torch's own conversion, so float64 values are rounded through float32, as the
    kernels round the float32 values of the float32 path."""
    return t.to(_torch().bfloat16).to(t.dtype)


def _rounding_functions():
    torch = _torch()

    class RoundOperand(torch.autograd.Function):
        """forward: bf16_round; backward: the gradient passes unchanged (it reaches the float32 master weights)"""

        @staticmethod
        def forward(ctx, x):
            return bf16_round(x)

        @staticmethod
        def backward(ctx, g):
            return g

    class RoundGradient(torch.autograd.Function):
        """forward: identity; backward: the output gradient rounded, as the dgrad and wgrad passes round dy"""

        @staticmethod
        def forward(ctx, y):
            return y.view_as(y)

        @staticmethod
        def backward(ctx, g):
            return bf16_round(g)

    return RoundOperand, RoundGradient


def conv7_bf16_ref(x, w):
    """F.conv2d(x, w, padding=3) with the bf16 passes' operands: x and w rounded by bf16_round, and in the backward
    the output gradient too; the products and sums in x's dtype."""
    F = _torch().nn.functional
    RoundOperand, RoundGradient = _rounding_functions()
    return RoundGradient.apply(F.conv2d(RoundOperand.apply(x), RoundOperand.apply(w), padding=3))


def reference_loss(P, S, img, t, lossfun, idx_maps=None, acts=None, bf16_operands=False):
    """The training forward in float64 torch ops on (B,C,H,W) tensors: P the parameters (requires_grad float64),
    S the running statistics (updated in place), img (B,3,H,W) 0..255.  idx_maps (the four pooling index maps
    (B,H,W,64) uint8, e.g. the kernels') replace the argmax, so near-ties cannot send the two sides down different
    branches.  acts (a list) receives the pooled activations relu(bn(y)) (B,H,W,64).  bf16_operands: every 7x7
    convolution is conv7_bf16_ref (the bf16 step's operand rounding).  -> (loss, [idx maps used])."""
    torch = _torch()
    F = torch.nn.functional
    conv7 = conv7_bf16_ref if bf16_operands else (lambda x, w: F.conv2d(x, w, padding=3))
    h = conv1_input(img)
    pools = []
    for i, name in enumerate(ENCODERS):
        y = conv7(h, P[name + '/W'])
        h = _bn_ref(P, S, name, y)
        a = F.relu(h).permute(0, 2, 3, 1)
        if acts is not None:
            acts.append(a)
        if idx_maps is not None:
            idx = idx_maps[i]
            B, H, W, C = a.shape
            win = a.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
            p = win.gather(-1, idx.long()[..., None])[..., 0]
        else:
            p, idx = pool_argmax_nhwc(a)
        pools.append(idx)
        h = p.permute(0, 3, 1, 2)
    for name, idx in zip(DECODERS, pools[::-1]):
        y = conv7(unpool_ref(h, idx.permute(0, 3, 1, 2).long()), P[name + '/W'])
        h = _bn_ref(P, S, name, y)
    score = F.conv2d(h, P['conv_classifier/W'], P['conv_classifier/b'])
    return lossfun(score, t), pools


def _bn_ref(P, S, name, y):
    F = _torch().nn.functional
    m = y.numel() / y.shape[1]
    mean = y.detach().mean((0, 2, 3))
    var = y.detach().var((0, 2, 3), unbiased=False)
    bn_update(S[name + '_bn/avg_mean'], S[name + '_bn/avg_var'], mean, var, m)
    return F.batch_norm(y, None, None, P[name + '_bn/gamma'], P[name + '_bn/beta'], training=True, eps=BN_EPS)


# ------------------------------------------------------------------------------- optimizers (Chainer's forms)
class MomentumSGD(object):
    """chainer.optimizers.MomentumSGD(lr, momentum 0.9) with WeightDecay(rate): g += rate * p; v = 0.9 v - lr g;
    p += v."""

    def __init__(self, lr=0.01, momentum=0.9, weight_decay=0.0):
        self.lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.t = 0
        self.state = {}

    def update(self, params, grads):
        self.t += 1
        for k, p in params.items():
            g = grads[k]
            if self.weight_decay > 0:
                g = g + self.weight_decay * p
            v = self.state.setdefault(k, {}).get('v')
            if v is None:
                v = self.state[k]['v'] = p.new_zeros(p.shape)
            v *= self.momentum
            v -= self.lr * g
            p += v

    def state_keys(self):
        return ('v',)


class Adam(object):
    """chainer.optimizers.Adam(alpha 0.001, beta1 0.9, beta2 0.999, eps 1e-8): m += (1 - b1)(g - m); v += (1 - b2)(g^2
    - v); p -= lr_t m / (sqrt(v) + eps), lr_t = alpha sqrt(1 - b2^t) / (1 - b1^t)."""

    def __init__(self, alpha=0.001, beta1=0.9, beta2=0.999, eps=1e-8):
        self.alpha, self.beta1, self.beta2, self.eps = alpha, beta1, beta2, eps
        self.t = 0
        self.state = {}

    @property
    def lr(self):
        fix1 = 1.0 - self.beta1 ** self.t
        fix2 = 1.0 - self.beta2 ** self.t
        return self.alpha * np.sqrt(fix2) / fix1

    def update(self, params, grads):
        self.t += 1
        lr = self.lr
        for k, p in params.items():
            g = grads[k]
            s = self.state.setdefault(k, {})
            if 'm' not in s:
                s['m'] = p.new_zeros(p.shape)
                s['v'] = p.new_zeros(p.shape)
            m, v = s['m'], s['v']
            m += (1.0 - self.beta1) * (g - m)
            v += (1.0 - self.beta2) * (g * g - v)
            p -= lr * m / (v.sqrt() + self.eps)

    def state_keys(self):
        return ('m', 'v')


# ------------------------------------------------------------------------------- the network on the kernels
def pack_w(w):
    """(64,Cin,7,7) torch -> (49,64,Cp) (ky*7+kx, n, c), Cin 3 padded to 4: differentiable, so autograd unpacks dW."""
    torch = _torch()
    cin = w.shape[1]
    wp = w.permute(2, 3, 0, 1).reshape(49, 64, cin)
    if cin == 3:
        wp = torch.cat([wp, wp.new_zeros(49, 64, 1)], 2)
    return wp.contiguous()


def _functions():
    torch = _torch()

    class Conv7(torch.autograd.Function):
        """y = conv7x7(x; wp) on the kernels; backward: dgrad (not for conv1) and split-K wgrad.  family '' (float32),
        '_bf16' (the bf16 matrix cores) or '_f16x3' (split planes on the f16 matrix cores) names the Engine passes;
        all three take the same arguments, float32 in and out."""

        @staticmethod
        def forward(ctx, x, wp, idx, eng, family=''):
            y, stats = getattr(eng, 'segnet_train_forward' + family)(x, wp, idx, MEAN, STD)
            ctx.save_for_backward(x, wp, idx)
            ctx.eng = eng
            ctx.family = family
            ctx.mark_non_differentiable(stats)
            return y, stats

        @staticmethod
        def backward(ctx, gy, _gstats):
            x, wp, idx = ctx.saved_tensors
            eng = ctx.eng
            dgrad = getattr(eng, 'segnet_train_dgrad' + ctx.family)
            wgrad = getattr(eng, 'segnet_train_wgrad' + ctx.family)
            gy = gy.contiguous()
            dx = None
            if ctx.needs_input_grad[0]:
                dx = dgrad(gy, wp, idx)
            dw = wgrad(gy, x, idx, MEAN, STD) if ctx.needs_input_grad[1] else None
            return dx, dw, None, None, None

    class BatchNorm(torch.autograd.Function):
        """BN with given batch statistics over (B,H,W) of a (B,H,W,64) map; the standard backward through them.
        group (a RankGroup, data-parallel runs): the statistics are over the union of every rank's batch, so dy is
        formed from the sums of g and g * xhat over all ranks (m = world size * B*H*W), while gamma and beta get this
        rank's own sums: the gradient all-reduce adds them up once."""

        @staticmethod
        def forward(ctx, y, gamma, beta, mean, rstd, group=None):
            ctx.save_for_backward(y, gamma, mean, rstd)
            ctx.group = group
            return (y - mean) * (rstd * gamma) + beta

        @staticmethod
        def backward(ctx, g):
            y, gamma, mean, rstd = ctx.saved_tensors
            m = y.numel() / y.shape[-1]
            xhat = (y - mean) * rstd
            dbeta = g.sum((0, 1, 2))
            dgamma = (g * xhat).sum((0, 1, 2))
            if ctx.group is None:
                dy = (gamma * rstd / m) * (m * g - dbeta - xhat * dgamma)
            else:
                m *= ctx.group.size
                s = ctx.group.sum_in_rank_order(torch.stack([dbeta, dgamma]))
                dy = (gamma * rstd / m) * (m * g - s[0] - xhat * s[1])
            return dy, dgamma, dbeta, None, None, None

    return Conv7, BatchNorm


def _fused_functions():
    """The layers between the convolutions on the kernels of csrc/spa_segnet_train_bn.hip (fused_bn=True).  Against the
    autograd graph of BatchNorm / relu / pool_argmax_nhwc / matmul, an encoder layer saves y, the pooled map and its
    uint8 index map (not the normalised map, the ReLU output and the windowed copy), a decoder layer y alone."""
    torch = _torch()

    def bn_backward(ctx, g, idx, p):
        y, gamma, mean, rstd = ctx.saved_tensors[:4]
        eng = ctx.eng
        m = y.numel() / y.shape[-1]
        g = g.contiguous()
        sums = eng.segnet_train_bn_backward_sums(g, y, mean, rstd, idx, p)
        total = sums
        if ctx.group is not None:           # as BatchNorm: dy from every rank's sums, gamma and beta from this rank's
            m *= ctx.group.size
            total = ctx.group.sum_in_rank_order(sums)
        dy = eng.segnet_train_bn_backward_dy(g, y, mean, rstd, gamma, total, m, idx, p)
        return dy, sums[1].float(), sums[0].float(), None, None, None, None

    class EncoderBN(torch.autograd.Function):
        """(max over 2x2 of relu(bn(y)), the index of its first maximum) for given batch statistics"""

        @staticmethod
        def forward(ctx, y, gamma, beta, mean, rstd, eng, group=None):
            p, idx = eng.segnet_train_bn_forward(y, mean, rstd, gamma.detach(), beta.detach(), pool=True)
            ctx.save_for_backward(y, gamma, mean, rstd, idx, p)
            ctx.eng, ctx.group = eng, group
            ctx.mark_non_differentiable(idx)
            return p, idx

        @staticmethod
        def backward(ctx, gp, _gidx):
            idx, p = ctx.saved_tensors[4:]
            return bn_backward(ctx, gp, idx, p)

    class DecoderBN(torch.autograd.Function):
        """bn(y) for given batch statistics"""

        @staticmethod
        def forward(ctx, y, gamma, beta, mean, rstd, eng, group=None):
            ctx.save_for_backward(y, gamma, mean, rstd)
            ctx.eng, ctx.group = eng, group
            return eng.segnet_train_bn_forward(y, mean, rstd, gamma.detach(), beta.detach())

        @staticmethod
        def backward(ctx, g):
            return bn_backward(ctx, g, None, None)

    class Classifier(torch.autograd.Function):
        """score (B,H,W,2) = h wc^T + bc for the (2,64,1,1) classifier weight"""

        @staticmethod
        def forward(ctx, h, wc, bc, eng):
            w2 = wc.detach().reshape(2, 64).contiguous()
            ctx.save_for_backward(h, w2)
            ctx.eng = eng
            return eng.segnet_train_classifier_forward(h, w2, bc.detach())

        @staticmethod
        def backward(ctx, g):
            h, w2 = ctx.saved_tensors
            dh, dw, db = ctx.eng.segnet_train_classifier_backward(g.contiguous(), h, w2)
            return dh, dw.view(2, 64, 1, 1), db, None

    return EncoderBN, DecoderBN, Classifier


_FN = []
_FUSED_FN = []


class SegNetTrainer(object):
    """Parameters, running statistics and the optimizer of one SegNetBasic on one GPU.  P: float32 tensors keyed as
    the snapshot (conv1/W, conv1_bn/gamma, ..., conv_classifier/b), S: the running statistics.  dtype 'fp32' or
    'bf16': the operands of the 7x7 passes (see the module docstring); P, S and the optimizer are float32 in both.
    split_planes (float32 only): the 7x7 passes at float32 accuracy on the f16 matrix cores.  fused_bn: BatchNorm, ReLU,
    pooling and the classifier, forward and backward, on the kernels of csrc/spa_segnet_train_bn.hip instead of torch
    ops; it combines with every convolution family and with a RankGroup, and holds no state."""

    def __init__(self, params, optimizer, lossfun, engine=None, device=None, dtype='fp32', split_planes=False,
                 fused_bn=False):
        if dtype not in DTYPES:
            raise ValueError('SegNetTrainer: dtype must be one of %s, got %r' % (DTYPES, dtype))
        if split_planes and dtype != 'fp32':
            raise ValueError("SegNetTrainer: split_planes=True runs the float32 step on split planes; it does not "
                             "combine with dtype=%r" % (dtype,))
        if not isinstance(fused_bn, bool):
            raise ValueError('SegNetTrainer: fused_bn must be True or False, got %r' % (fused_bn,))
        torch = _torch()
        from .engine import Engine
        if not _FN:
            _FN.extend(_functions())
        if fused_bn and not _FUSED_FN:
            _FUSED_FN.extend(_fused_functions())
        self.eng = engine or Engine(device)
        dev = self.eng.device
        self.P = {k: torch.as_tensor(np.asarray(params[k]), dtype=torch.float32).to(dev).contiguous() for k in PARAM_KEYS}
        self.S = {k: torch.as_tensor(np.asarray(params[k]), dtype=torch.float32).to(dev).contiguous() for k in STAT_KEYS}
        self.N = {n: int(np.asarray(params.get(n + '_bn/N', 0))) for n in LAYERS}
        self.opt = optimizer
        self.lossfun = lossfun
        self.dtype = dtype
        self.split_planes = bool(split_planes)
        self.family = '_f16x3' if self.split_planes else ('_bf16' if dtype == 'bf16' else '')
        self.fused_bn = fused_bn
        self.group = None           # a RankGroup: data-parallel steps (set_group)

    def set_group(self, group):
        """Make every step a data-parallel step over `group` (a RankGroup, or None for one process) and give every
        rank rank 0's parameters and running statistics."""
        self.group = group
        if group is not None:
            group.broadcast_(list(self.P.values()) + list(self.S.values()))

    def loss(self, img, t, trace=None):
        """img (B,3,H,W) float32 0..255 on the device (after augmentation, before standardisation), t the labels ->
        the loss (autograd graph to self.P); updates the running statistics.  trace receives the index maps."""
        torch = _torch()
        Conv7, BatchNorm = _FN
        B, C, H, W = img.shape
        if C != 3 or H % 16 or W % 16:
            raise ValueError('SegNet-Basic training input must be (B,3,H,W) with H, W multiples of 16, got %s'
                             % (tuple(img.shape),))
        P = self.P
        h, pools = img.contiguous(), []

        group = self.group
        fused = self.fused_bn
        if fused:
            EncoderBN, DecoderBN, Classifier = _FUSED_FN

        def bn(name, y, stats, layer=None):
            m = float(y.shape[0] * y.shape[1] * y.shape[2])
            if group is not None:
                stats = group.sum_in_rank_order(stats)
                m *= group.size
            mean = stats[0] / m
            var = (stats[1] / m - mean * mean).clamp_min(0.0)
            rstd = (1.0 / torch.sqrt(var + BN_EPS)).float()
            with torch.no_grad():
                bn_update(self.S[name + '_bn/avg_mean'], self.S[name + '_bn/avg_var'], mean.float(), var.float(), m)
            self.N[name] += 1
            if layer is not None:
                return layer.apply(y, P[name + '_bn/gamma'], P[name + '_bn/beta'], mean.float(), rstd, self.eng, group)
            return BatchNorm.apply(y, P[name + '_bn/gamma'], P[name + '_bn/beta'], mean.float(), rstd, group)

        for name in ENCODERS:
            y, stats = Conv7.apply(h, pack_w(P[name + '/W']), None, self.eng, self.family)
            if fused:
                h, idx = bn(name, y, stats, EncoderBN)
            else:
                a = torch.relu(bn(name, y, stats))
                h, idx = pool_argmax_nhwc(a)
                h = h.contiguous()
            pools.append(idx)
        if trace is not None:
            trace.extend(pools)
        for name, idx in zip(DECODERS, pools[::-1]):
            y, stats = Conv7.apply(h, pack_w(P[name + '/W']), idx, self.eng, self.family)
            h = bn(name, y, stats, DecoderBN if fused else None)
        if fused:
            score = Classifier.apply(h, P['conv_classifier/W'], P['conv_classifier/b'], self.eng)
        else:
            score = torch.matmul(h, P['conv_classifier/W'].view(2, 64).t()) + P['conv_classifier/b']
        return self.lossfun(score.permute(0, 3, 1, 2), t)

    def step(self, img, t, trace=None):
        """one update; -> the loss (float)"""
        torch = _torch()
        leaves = {k: v.detach().requires_grad_(True) for k, v in self.P.items()}
        saved, self.P = self.P, leaves
        try:
            loss = self.loss(img, t, trace)
            grads = dict(zip(leaves.keys(), torch.autograd.grad(loss, list(leaves.values()))))
        finally:
            self.P = saved
        if self.group is not None:
            grads = self.group.mean_gradients(grads)
        with torch.no_grad():
            self.opt.update(self.P, grads)
        return float(loss.detach())

    def params_numpy(self):
        out = {k: v.detach().cpu().numpy() for k, v in self.P.items()}
        out.update({k: v.detach().cpu().numpy() for k, v in self.S.items()})
        for n in LAYERS:
            out[n + '_bn/N'] = np.asarray(self.N[n])
        return out

    def predictor(self, pred_shape=None, split_planes=False):
        """The inference network (BN folded from the running statistics) on the same engine: the float32 one whatever
        the training mode, or with split_planes its float32-accurate form on the f16 matrix cores."""
        return segnet.SegNetBasic(self.params_numpy(), pred_shape, engine=self.eng, split_planes=split_planes)


# ------------------------------------------------------------------------------- data parallelism
class RankGroup(object):
    """The collectives of a data-parallel run (train_segnet.py --data_parallel) over torch.distributed's initialised
    default group.  A step on N ranks with b images each computes the gradient of L = (1/N) sum_r L_r, L_r the loss of
    rank r's own batch, with BatchNorm statistics over the union of the N batches (what ChainerMN's
    MultiNodeBatchNormalization and create_multi_node_optimizer intend); with no ignored labels that is the step of
    one process on the N*b images.  Per step:
      * every BN forward: the kernel's (sum y, sum y^2), float64 (2, 64), summed over the ranks (sum_in_rank_order);
        mean, variance and bn_update's unbiased factor use m = N*B*H*W;
      * every BN backward: (sum g, sum g*xhat) summed the same way for dy; gamma and beta get this rank's LOCAL sums
        as their gradients (the global ones would be counted N times by the all-reduce below);
      * all parameter gradients flattened into one float32 bucket, one all_reduce(SUM), divided by N; the optimizer
        (weight decay, ExponentialShift, Adam's bias correction) then runs identically on every rank.
    Collectives run on the backend's device: the rank's GPU for nccl (RCCL), host copies for gloo (the convention of
    dist.gather_records).  Every per-rank computation is the one-process path unchanged, so one rank reproduces the
    one-process bits."""

    def __init__(self):
        import torch.distributed as dist
        torch = _torch()
        self.dist = dist
        self.rank, self.size = dist.get_rank(), dist.get_world_size()
        self.device = (torch.device('cuda', torch.cuda.current_device()) if dist.get_backend() == 'nccl'
                       else torch.device('cpu'))

    def sum_in_rank_order(self, t):
        """t summed over the ranks, on t's device: an all_gather, then parts[0] + parts[1] + ... in rank order, so
        every rank holds the same bits whatever algorithm the collective uses."""
        torch = _torch()
        x = t.detach().to(self.device).contiguous()
        parts = [torch.empty_like(x) for _ in range(self.size)]
        self.dist.all_gather(parts, x)
        total = parts[0]
        for p in parts[1:]:
            total = total + p
        return total.to(t.device)

    def mean_gradients(self, grads):
        """{name: gradient} -> the mean over the ranks: one all_reduce(SUM) of one flat bucket, divided by N."""
        torch = _torch()
        keys = list(grads)
        flat = torch.cat([grads[k].reshape(-1) for k in keys]).to(self.device)
        self.dist.all_reduce(flat, op=self.dist.ReduceOp.SUM)
        flat /= self.size
        flat = flat.to(grads[keys[0]].device)
        out, o = {}, 0
        for k in keys:
            n = grads[k].numel()
            out[k] = flat[o:o + n].view_as(grads[k])
            o += n
        return out

    def broadcast_(self, tensors, src=0):
        """rank src's values into `tensors` (float32, one device) on every rank: one broadcast of a flat copy."""
        torch = _torch()
        flat = torch.cat([t.reshape(-1) for t in tensors]).to(self.device)
        self.dist.broadcast(flat, src)
        o = 0
        for t in tensors:
            n = t.numel()
            t.copy_(flat[o:o + n].view_as(t))
            o += n

    def mean_over_ranks(self, report):
        """{key: number} -> {key: the mean of the ranks' values} (create_multi_node_evaluator: a mean of per-rank
        metrics, not a pooled confusion)."""
        torch = _torch()
        keys = sorted(report)
        total = self.sum_in_rank_order(torch.tensor([float(report[k]) for k in keys], dtype=torch.float64))
        return {k: float(v) / self.size for k, v in zip(keys, total.tolist())}

    def gather_objects(self, obj):
        """one picklable object per rank -> the list over ranks, on every rank"""
        out = [None] * self.size
        self.dist.all_gather_object(out, obj)
        return out

    def barrier(self):
        self.dist.barrier()


def shard_indices(n, n_ranks, rank, shuffle=True, seed=0):
    """The examples of `rank` among n_ranks, as chainermn.scatter_dataset splits a dataset of n: with shuffle, a
    permutation from its own np.random.RandomState(seed) (numpy's global stream is not consumed), else 0..n-1; rank r
    takes order[n*r//N : n*r//N + ceil(n/N)], so the last rank ends at n, every rank gets ceil(n/N) examples and the
    shards overlap where N does not divide n.  One rank keeps the whole set in its order (the one-process run)."""
    if n_ranks == 1:
        return np.arange(n)
    order = np.random.RandomState(seed).permutation(n) if shuffle else np.arange(n)
    lo = n * rank // n_ranks
    return order[lo:lo + -(-n // n_ranks)]


DP_KEY = 'extensions/data_parallel/'      # data-parallel snapshots: world size, every rank's iterator and numpy state


def rank_state(iterator, state=None):
    """this rank's iterator state and numpy random state, as a data-parallel snapshot stores them per rank.  state:
    the (iterator state, numpy state) pair a TrainLoader captured with the batch, instead of the live ones."""
    it_state, st = state if state is not None else (iterator.state(), np.random.get_state())
    out = {'iterator/' + k: np.asarray(v) for k, v in it_state.items()}
    out.update({'np_random/keys': st[1], 'np_random/pos': np.asarray(st[2]), 'np_random/has_gauss': np.asarray(st[3]),
                'np_random/cached_gaussian': np.asarray(st[4])})
    return out


def data_parallel_extra(states):
    """every rank's rank_state (rank order) -> the extra snapshot entries of a data-parallel run"""
    d = {DP_KEY + 'world_size': np.asarray(len(states))}
    for r, s in enumerate(states):
        for k, v in s.items():
            d['%srank%d/%s' % (DP_KEY, r, k)] = v
    return d


def snapshot_world_size(path):
    """The number of ranks that wrote a snapshot, or None for a one-process snapshot."""
    with np.load(path) as z:
        return int(z[DP_KEY + 'world_size']) if DP_KEY + 'world_size' in z.files else None


def load_rank_state(path, rank):
    """-> (iterator state, np random state) of `rank` from a data-parallel snapshot"""
    pre = '%srank%d/' % (DP_KEY, rank)
    with np.load(path) as z:
        it_state = {f[len(pre + 'iterator/'):]: np.asarray(z[f]) for f in z.files if f.startswith(pre + 'iterator/')}
        rnd = ('MT19937', np.asarray(z[pre + 'np_random/keys']), int(z[pre + 'np_random/pos']),
               int(z[pre + 'np_random/has_gauss']), float(z[pre + 'np_random/cached_gaussian']))
    return it_state, rnd


# ------------------------------------------------------------------------------- snapshots
OPT = 'updater/optimizer:main/'


def save_snapshot(path, trainer, iteration, lr, iterator_state, extra=None, np_state=None):
    """A Chainer-style npz: updater/model:main/predictor/<link>/<param> (what segnet.load_snapshot reads), the
    optimizer state under updater/optimizer:main/predictor/<link>/<param>/<state>, the iteration, lr, the iterator,
    numpy's random state (so --resume continues bit for bit), under DTYPE_KEY the trainer's dtype and, for a
    split-plane trainer only, SPLIT_PLANES_KEY = True.  np_state: the numpy state to store instead of the live one
    (the one a TrainLoader captured with the batch of this iteration)."""
    d = {}
    for k, v in trainer.params_numpy().items():
        d[segnet.PREFIX + k] = v
    opt = trainer.opt
    for k, s in opt.state.items():
        for name, v in s.items():
            d['%spredictor/%s/%s' % (OPT, k, name)] = v.detach().cpu().numpy()
    d[OPT + 't'] = np.asarray(opt.t)
    d[OPT + 'lr'] = np.asarray(lr)
    d['updater/iteration'] = np.asarray(iteration)
    for k, v in iterator_state.items():
        d['updater/iterator:main/' + k] = np.asarray(v)
    st = np.random.get_state() if np_state is None else np_state
    d['extensions/np_random/keys'] = st[1]
    d['extensions/np_random/pos'] = np.asarray(st[2])
    d['extensions/np_random/has_gauss'] = np.asarray(st[3])
    d['extensions/np_random/cached_gaussian'] = np.asarray(st[4])
    d[DTYPE_KEY] = np.asarray(getattr(trainer, 'dtype', 'fp32'))
    if getattr(trainer, 'split_planes', False):
        d[SPLIT_PLANES_KEY] = np.asarray(True)
    for k, v in (extra or {}).items():
        d[k] = np.asarray(v)
    tmp = path + '.tmp.npz'
    np.savez(tmp, **d)
    os.replace(tmp, path)


def snapshot_dtype(path):
    """The dtype a snapshot was trained with: 'fp32' or 'bf16' ('fp32' for a snapshot that does not record one).
    Either kind resumes in either dtype: the master weights and the optimizer state are float32 in both."""
    with np.load(path) as z:
        return str(z[DTYPE_KEY]) if DTYPE_KEY in z.files else 'fp32'


def snapshot_split_planes(path):
    """Whether a snapshot was written by a split-plane run (False for one that does not record it).  The state is
    float32 either way, so it resumes with or without --split_planes."""
    with np.load(path) as z:
        return bool(z[SPLIT_PLANES_KEY]) if SPLIT_PLANES_KEY in z.files else False


def load_snapshot_state(path):
    """-> (params dict, optimizer state {param: {name: array}}, t, lr, iteration, iterator state, np random state)"""
    with np.load(path) as z:
        files = set(z.files)
        params = {}
        for k in PARAM_KEYS + STAT_KEYS:
            params[k] = np.asarray(z[segnet.PREFIX + k], np.float32)
        for n in LAYERS:
            key = segnet.PREFIX + n + '_bn/N'
            params[n + '_bn/N'] = int(z[key]) if key in files else 0
        state = {}
        for f in files:
            if f.startswith(OPT + 'predictor/'):
                k, name = f[len(OPT + 'predictor/'):].rsplit('/', 1)
                state.setdefault(k, {})[name] = np.asarray(z[f])
        t = int(z[OPT + 't'])
        lr = float(z[OPT + 'lr'])
        iteration = int(z['updater/iteration'])
        it_state = {f[len('updater/iterator:main/'):]: np.asarray(z[f]) for f in files
                    if f.startswith('updater/iterator:main/')}
        rnd = ('MT19937', np.asarray(z['extensions/np_random/keys']), int(z['extensions/np_random/pos']),
               int(z['extensions/np_random/has_gauss']), float(z['extensions/np_random/cached_gaussian']))
    return params, state, t, lr, iteration, it_state, rnd


# ------------------------------------------------------------------------------- dataset
def pca_lighting_shift(alpha):
    """The three float64 channel shifts pca_lighting adds for the drawn alpha (3,)."""
    eigen_value = np.array((0.2175, 0.0188, 0.0045))
    eigen_vector = np.array(((-0.5675, -0.5808, -0.5836), (0.7192, -0.0045, -0.6948), (0.4009, -0.8140, 0.4203)))
    return eigen_vector.dot(eigen_value * alpha)


def pca_lighting(img, sigma):
    """chainercv.transforms.pca_lighting(img, sigma) with its default eigen decomposition, numpy's global stream."""
    if sigma <= 0:
        return img
    alpha = np.random.normal(0, sigma, size=3)
    img = img.copy()
    img += pca_lighting_shift(alpha).reshape((-1, 1, 1))
    return img


def pil_bicubic_coeffs(n_in, n_out):
    """Pillow's precompute_coeffs (src/libImaging/Resample.c) for BICUBIC (a = -0.5) along one axis, in float64 with
    its operation order -> (bounds (n_out, 2) int32 {first tap, tap count}, taps (n_out, ksize) float64 normalised by
    their sequential sum, unused entries 0).  The tables of a mode 'F' resize, which applies them unrounded
    (Engine.segnet_train_input, pil_resize_float)."""
    scale = float(n_in) / float(n_out)
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in) - xmin
    a = -0.5
    k = np.zeros((n_out, ksize), np.float64)
    ww = np.zeros(n_out, np.float64)
    for x in range(ksize):
        t = np.abs((x + xmin - center + 0.5) * ss)
        near = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
        far = (((t - 5) * t + 8) * t - 4) * a
        wgt = np.where(x < xmax, np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0)), 0.0)
        k[:, x] = wgt
        ww = ww + wgt                                # tap order; the zeros past a row's count change nothing
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    assert ((xmin >= 0) & (xmax >= 0) & (xmin + xmax <= n_in) & (xmax <= ksize)).all()
    return np.stack([xmin, xmax], 1).astype(np.int32), k


def pil_resize_float(img, shape):
    """Pillow's mode 'F' BICUBIC resize of a float32 (C,H,W) image restated in numpy: per output sample a float64 that
    starts at 0 accumulates float64(v) * k in tap order and is stored as float32, the horizontal pass first, the
    vertical pass over its float32 results; a pass whose size does not change is not run.  The arithmetic of
    csrc/spa_segnet_input.hip; equal to resize_bicubic_float's Pillow branch bit for bit."""
    h, w = int(shape[0]), int(shape[1])
    img = np.asarray(img, np.float32)
    if img.shape[2] != w:
        b, k = pil_bicubic_coeffs(img.shape[2], w)
        acc = np.zeros(img.shape[:2] + (w,), np.float64)
        for t in range(k.shape[1]):
            idx = np.minimum(b[:, 0] + t, img.shape[2] - 1)
            term = img[:, :, idx].astype(np.float64) * k[None, None, :, t]
            acc = np.where(t < b[None, None, :, 1], acc + term, acc)
        img = acc.astype(np.float32)
    if img.shape[1] != h:
        b, k = pil_bicubic_coeffs(img.shape[1], h)
        acc = np.zeros((img.shape[0], h, img.shape[2]), np.float64)
        for t in range(k.shape[1]):
            idx = np.minimum(b[:, 0] + t, img.shape[1] - 1)
            term = img[:, idx, :].astype(np.float64) * k[None, :, t, None]
            acc = np.where(t < b[None, :, 1, None], acc + term, acc)
        img = acc.astype(np.float32)
    return img


def nearest_index_table(n_src, n_dst, backend='pil'):
    """The source index of every destination index under resize_nearest_label -> (n_dst,) int32.  'pil': Pillow's
    NEAREST of Image.resize (an affine scale: the source coordinate starts at half a step and grows by repeated
    float64 addition of n_src / n_dst, truncated); 'cv2': cli.nearest_index."""
    if backend == 'cv2':
        from . import cli
        out = cli.nearest_index(n_dst, n_src).astype(np.int32)
    else:
        step = float(n_src) / float(n_dst)
        out = np.empty(n_dst, np.int32)
        xo = step * 0.5
        for x in range(n_dst):
            out[x] = int(xo)
            xo += step
    assert ((out >= 0) & (out < n_src)).all()
    return out


def _cv_cubic_float_taps(n_src, n_dst):
    """OpenCV INTER_CUBIC (A = -0.75) along one axis, float path: clamped source indices (n_dst, 4), float32 taps."""
    scale = float(n_src) / float(n_dst)
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    x = (f - s.astype(np.float32)).astype(np.float32)
    A = np.float32(-0.75)
    c0 = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A
    c1 = ((A + 2) * x - (A + 3)) * x * x + 1
    c2 = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1
    c3 = np.float32(1) - c0 - c1 - c2
    taps = np.stack([c0, c1, c2, c3], 1).astype(np.float32)
    idx = np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, n_src - 1)
    return idx, taps


def resize_bicubic_float(img, shape):
    """chainercv.transforms.resize(img, shape, 3) of a FLOAT32 (C,H,W) image: Pillow's Image.resize(BICUBIC) of each
    channel as a mode 'F' image (not the 8-bit path of cli.resize_bicubic_chw), or with cli.RESIZE_BACKEND 'cv2'
    OpenCV's float INTER_CUBIC (its algorithm restated in float32, not pinned: no cv2 here).  The float counterpart of
    segnet.resize_bilinear_pil."""
    from . import cli
    h, w = int(shape[0]), int(shape[1])
    img = np.asarray(img, np.float32)
    if cli.RESIZE_BACKEND[0] == 'cv2':
        xi, xc = _cv_cubic_float_taps(img.shape[2], w)
        yi, yc = _cv_cubic_float_taps(img.shape[1], h)
        t = np.zeros((img.shape[0], img.shape[1], w), np.float32)
        for k in range(4):
            t += img[:, :, xi[:, k]] * xc[None, None, :, k]
        out = np.zeros((img.shape[0], h, w), np.float32)
        for k in range(4):
            out += t[:, yi[:, k], :] * yc[None, :, k, None]
        return out
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(c, mode='F').resize((w, h), Image.BICUBIC), np.float32)
                     for c in img])


def resize_nearest_label(label, shape):
    """chainercv.transforms.resize(label, shape, 0) of (C,H,W) labels: Pillow NEAREST per channel on the values as
    mode 'F' (exact for labels and scores), or with RESIZE_BACKEND 'cv2' cv.INTER_NEAREST (cli.resize_nearest)."""
    from . import cli
    h, w = int(shape[0]), int(shape[1])
    label = np.asarray(label)
    if cli.RESIZE_BACKEND[0] == 'cv2':
        return np.stack([cli.resize_nearest(c, (h, w)) for c in label])
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(c.astype(np.float32), mode='F').resize((w, h), Image.NEAREST))
                     .astype(label.dtype) for c in label])


class ZippedEstimatedCityscapesDataset(object):
    """datasets/zipped_estimated_cityscapes_dataset.py.  Images from a zip of *leftImg8bit.png, labels from the
    npz-style zip cli.write_label_zip writes (*leftImg8bit.npy road masks, or *leftImg8bit_scores.npy with
    use_soft_label), paired by '<city>_<seq>_<frame>' in the order of whichever side has fewer keys (the label side on a
    tie).  get_example returns (the float32 0..255 image resized and augmented but NOT standardised: conv1 does that in
    its load, label int32 (H,W) or float32 (2,H,W)); standardised() applies the dataset's standardisation on the host."""

    def __init__(self, img_zip_fn, label_zip_fn, resize_shape, random=False, use_soft_label=False):
        for fn in (img_zip_fn, label_zip_fn):
            if not os.path.exists(fn):
                raise ValueError('{} does not exist'.format(fn))
        key = lambda fn: '_'.join(os.path.basename(fn).split('_')[:3])
        postfix = 'leftImg8bit' + ('_scores.npy' if use_soft_label else '.npy')
        with zipfile.ZipFile(label_zip_fn) as zl, zipfile.ZipFile(img_zip_fn) as zi:
            label_fns = {key(fn): fn for fn in zl.namelist() if fn.endswith(postfix)}
            img_fns = {key(fn): fn for fn in zi.namelist() if fn.endswith('leftImg8bit.png')}
        keys = img_fns.keys() if len(img_fns) < len(label_fns) else label_fns.keys()
        self.img_fns = [img_fns[k] for k in keys]
        self.label_fns = [label_fns[k] for k in keys]
        self.resize_shape = tuple(int(v) for v in resize_shape)
        self.random, self.use_soft_label = random, use_soft_label
        self.img_zip_fn, self.label_zip_fn = img_zip_fn, label_zip_fn
        self.img_zf = self.label_zf = None

    def __len__(self):
        return len(self.img_fns)

    def decoded(self, i):
        """-> (the decoded float32 (3,H,W) image, the label member as int32 (H,W) or float32 (2,H,W)), full size"""
        from PIL import Image
        if self.img_zf is None:
            self.img_zf = zipfile.ZipFile(self.img_zip_fn)
        if self.label_zf is None:
            self.label_zf = np.load(self.label_zip_fn)
        with Image.open(self.img_zf.open(self.img_fns[i])) as f:
            img = np.asarray(f.convert('RGB'), dtype=np.float32).transpose(2, 0, 1)
        label = self.label_zf[self.label_fns[i][:-len('.npy')]]
        label = label.astype(np.float32) if self.use_soft_label else label.astype(np.int32)
        return img, label

    def get_example(self, i):
        img, label = self.resized(*self.decoded(i))
        if self.random:
            img = pca_lighting(img, 25.5)
            if np.random.rand() > 0.5:
                img = img[:, :, ::-1]
                label = label[..., ::-1]
        return np.ascontiguousarray(img, np.float32), np.ascontiguousarray(label)

    def resized(self, img, label):
        """get_example's resize of a decoded float32 (3,H,W) image and its converted label, each only where its size
        is not resize_shape"""
        if img.shape[1:] != self.resize_shape:
            img = resize_bicubic_float(img, self.resize_shape)
        if label.shape[-2:] != self.resize_shape:
            label = resize_nearest_label(label if self.use_soft_label else label[None], self.resize_shape)
            if not self.use_soft_label:
                label = label[0]
        return img, label

    @staticmethod
    def augmented(img, label, shift, flip):
        """get_example's --random part with the draws made by the caller (segnet_loader.TrainLoader): shift =
        pca_lighting_shift(np.random.normal(0, 25.5, 3)), flip = np.random.rand() > 0.5, drawn in that order."""
        img = img.copy()
        img += np.asarray(shift, np.float64).reshape((-1, 1, 1))
        if flip:
            img = img[:, :, ::-1]
            label = label[..., ::-1]
        return np.ascontiguousarray(img, np.float32), np.ascontiguousarray(label)

    @staticmethod
    def standardised(img):
        img = np.array(img, np.float32)
        img -= MEAN[:, None, None]
        img /= STD[:, None, None]
        return img

    def __getitem__(self, i):
        return self.get_example(i)


class ShuffledIterator(object):
    """chainer.iterators.SerialIterator(repeat=True, shuffle=True) order: a fresh np.random permutation per epoch, a
    batch that crosses an epoch boundary continues into the next permutation."""

    def __init__(self, n, batchsize):
        self.n, self.batchsize = n, batchsize
        self.order = np.random.permutation(n)
        self.current_position = 0
        self.epoch = 0

    def next_indices(self):
        out = []
        while len(out) < self.batchsize:
            take = min(self.batchsize - len(out), self.n - self.current_position)
            out.extend(self.order[self.current_position:self.current_position + take].tolist())
            self.current_position += take
            if self.current_position >= self.n:
                self.current_position = 0
                self.epoch += 1
                self.order = np.random.permutation(self.n)
        return out

    def state(self):
        return {'order': self.order, 'current_position': self.current_position, 'epoch': self.epoch}

    def load(self, st):
        self.order = np.asarray(st['order']).astype(np.int64)
        self.current_position = int(st['current_position'])
        self.epoch = int(st['epoch'])
