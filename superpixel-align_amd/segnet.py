"""SegNet-Basic inference on libspalign's kernels: what labels_from_segnet.py evaluates between training rounds
(utils/run_train_rounds.py), without Chainer.

models/segnet_basic.py in test mode (BatchNorm with its running statistics, folded into the convolutions here):

    h = LRN(x)                                                 n 5, k 1, alpha 1e-4 / 5, beta 0.75 (Chainer's formula)
    h, idx_i = maxpool2x2_argmax(relu(bn(conv7x7(h))))         conv1 .. conv4
    h = bn(conv7x7(unpool(h, idx_i)))                          decode4 .. decode1, indices of pool4 .. pool1
    score = softmax(conv_classifier(h))                        1x1, 64 -> 2, with bias
    label = argmax(Pillow BILINEAR resize of score to eval_shape)

Every layer is one launch (include/spalign.h: spa_segnet_encode / spa_segnet_decode / spa_segnet_score); the dataset's
standardisation happens inside conv1's load, so the device input is the cubic-resized image as float32 0..255.
SegNetBasic(..., dtype='bf16') runs the convolutions on the bf16 matrix cores instead (spa_segnet_encode_bf16 /
spa_segnet_decode_bf16: every product operand rounded to bf16, float32 accumulation and epilogue); the maps,
probabilities and the score stay float32.  SegNetBasic(..., split_planes=True) (dtype 'fp32' only) keeps float32
accuracy on the f16 matrix cores (spa_segnet_encode_f16x3 / spa_segnet_decode_f16x3: every operand as two scaled
half-precision planes, one scale per image, three products per float32 product).
"""
import glob
import json
import os
import zipfile

import numpy as np

MEAN = np.array([7.315835921071366954e+01, 8.290891754262415247e+01, 7.239239876194160672e+01], dtype=np.float32)
STD = np.array([4.161211675686322309e+01, 4.221582767516605372e+01, 4.048309952494058450e+01], dtype=np.float32)
BN_EPS = 2e-5                        # chainer.links.BatchNormalization's default
PREFIX = 'updater/model:main/predictor/'
ENCODERS = ('conv1', 'conv2', 'conv3', 'conv4')
DECODERS = ('conv_decode4', 'conv_decode3', 'conv_decode2', 'conv_decode1')
LAYERS = ENCODERS + DECODERS
BN_PARAMS = ('gamma', 'beta', 'avg_mean', 'avg_var')
DTYPES = ('fp32', 'bf16')            # the convolutions' operand precisions (inference here, training in segnet_train)


def check_mode(who, dtype, split_planes):
    """The refusals every entry to the network shares: an unknown dtype, and split_planes with a dtype other than
    'fp32' (the split-plane form is a float32-accurate computation; there is no bf16 variant of it)."""
    if dtype not in DTYPES:
        raise ValueError('%s: dtype must be one of %s, got %r' % (who, DTYPES, dtype))
    if split_planes and dtype != 'fp32':
        raise ValueError("%s: split_planes=True needs dtype='fp32', got dtype=%r" % (who, dtype))


# 2 x multiply-adds per 512 x 1024 image, from the layer shapes (tools/segnet_bench.py prices kernel times with it)
def layer_flops(H=512, W=1024):
    out = {}
    for i, name in enumerate(ENCODERS):
        cin = 3 if i == 0 else 64
        out[name] = 2.0 * (H >> i) * (W >> i) * 64 * cin * 49
    for i, name in enumerate(DECODERS):
        s = 3 - i
        out[name] = 2.0 * (H >> s) * (W >> s) * 64 * 64 * 49
    return out


# ------------------------------------------------------------------------------- snapshot
def find_snapshot(param_dir, iteration):
    """labels_from_segnet.py:38-41: the first of sorted(glob(snapshot_*)) whose name CONTAINS 'iter_<iteration>' (a
    substring test: iteration 1 matches iter_1000 when that sorts first), else the last snapshot."""
    snapshots = sorted(glob.glob(os.path.join(param_dir, 'snapshot_*')))
    if not snapshots:
        raise ValueError('no snapshot_* file in %s' % param_dir)
    for snapshot in snapshots:
        if 'iter_{}'.format(iteration) in snapshot:
            break
    return snapshot


def load_train_args(param_dir):
    train_args = json.load(open(os.path.join(param_dir, 'args.txt')))
    model = train_args.get('model')
    if model != 'basic':
        raise ValueError("%s: model '%s' is not supported: only SegNet-Basic ('basic') is implemented%s"
                         % (os.path.join(param_dir, 'args.txt'), model,
                            " (the VGG-style 'normal' SegNet is not)" if model == 'normal' else ''))
    return train_args


def load_snapshot(param_dir, iteration):
    """-> (train_args, snapshot path, {'conv1/W': array, 'conv1_bn/gamma': ..., 'conv_classifier/b': ...}) float32,
    read with numpy from the Chainer npz (keys 'updater/model:main/predictor/<link>/<param>')."""
    train_args = load_train_args(param_dir)
    snapshot = find_snapshot(param_dir, iteration)
    return train_args, snapshot, read_snapshot(snapshot)


def read_snapshot(snapshot):
    """The parameters of one snapshot FILE (utils/create_demovideo.py --snapshot, which the reference loads with
    serializers.load_npz(path='updater/model:main/predictor/')): load_snapshot's dictionary, with its checks of the
    keys and shapes.  There is no args.txt to read beside a bare file: the network is taken to be SegNet-Basic, and a
    snapshot of another model fails those checks."""
    want = {}
    for i, name in enumerate(LAYERS):
        want[name + '/W'] = (64, 3 if i == 0 else 64, 7, 7)
        for p in BN_PARAMS:
            want['%s_bn/%s' % (name, p)] = (64,)
    want['conv_classifier/W'] = (2, 64, 1, 1)
    want['conv_classifier/b'] = (2,)
    params = {}
    with np.load(snapshot) as z:
        for key, shape in want.items():
            if PREFIX + key not in z.files:
                raise KeyError('%s has no %s' % (snapshot, PREFIX + key))
            a = np.asarray(z[PREFIX + key], dtype=np.float32)
            if a.shape != shape:
                raise ValueError('%s: %s has shape %s, expected %s' % (snapshot, PREFIX + key, a.shape, shape))
            params[key] = a
    return params


def fold_bn(params, dtype=np.float32):
    """Test-mode BatchNorm folded into the preceding (bias-free) convolution, computed in float64:
    W' = W * gamma / sqrt(avg_var + eps), b' = beta - avg_mean * gamma / sqrt(avg_var + eps) (as drn.py folds).
    -> {layer: (W' (64,Cin,7,7), b' (64,))} plus 'conv_classifier': (W (2,64), b (2,))."""
    out = {}
    for name in LAYERS:
        g = params[name + '_bn/gamma'].astype(np.float64)
        var = params[name + '_bn/avg_var'].astype(np.float64)
        mu = params[name + '_bn/avg_mean'].astype(np.float64)
        beta = params[name + '_bn/beta'].astype(np.float64)
        scale = g / np.sqrt(var + BN_EPS)
        w = params[name + '/W'].astype(np.float64) * scale[:, None, None, None]
        out[name] = (w.astype(dtype), (beta - mu * scale).astype(dtype))
    out['conv_classifier'] = (params['conv_classifier/W'].reshape(2, 64).astype(dtype),
                              params['conv_classifier/b'].astype(dtype))
    return out


def pack_weight(w):
    """(64,Cin,7,7) -> (49,64,Cp) float32 = (ky*7+kx, n, c), Cin 3 zero-padded to 4 (spa_segnet_encode / _decode)."""
    n, cin = w.shape[:2]
    cp = 4 if cin == 3 else cin
    out = np.zeros((49, n, cp), np.float32)
    out[:, :, :cin] = np.asarray(w, np.float32).transpose(2, 3, 0, 1).reshape(49, n, cin)
    return out


# ------------------------------------------------------------------------------- dataset
def label_mask(label):
    """zipped_cityscapes_road_dataset.py:69-74: ids 0..6 -> -1, 7 -> 1, everything else 0 (int32)."""
    out = np.zeros(label.shape, np.int32)
    out[label <= 6] = -1
    out[label == 7] = 1
    return out


def _decode(fp, gray=False):
    from PIL import Image
    with Image.open(fp) as f:
        a = np.asarray(f.convert('L') if gray else f.convert('RGB'), dtype=np.uint8)
    return a if gray else a.transpose(2, 0, 1)


class ZippedCityscapesRoadDataset(object):
    """datasets/zipped_cityscapes_road_dataset.py.  Pairs as the reference: keys '<city>_<seq>_<frame>' of the members
    ending in leftImg8bit.png / labelIds.png, in the archive order of whichever archive has fewer of them (the label
    side on a tie).  get_example returns what the reference's does (cubic-resized, standardised float32 CHW image, int32
    label); get_raw the decoded uint8 image and the label, for the device path (resize and standardisation on the GPU)."""

    def __init__(self, img_zip_fn, label_zip_fn, resize_shape):
        for fn in (img_zip_fn, label_zip_fn):
            if not os.path.exists(fn):
                raise ValueError('{} does not exist'.format(fn))
        key = lambda fn: '_'.join(os.path.basename(fn).split('_')[:3])
        with zipfile.ZipFile(label_zip_fn) as zl, zipfile.ZipFile(img_zip_fn) as zi:
            label_fns = {key(fn): fn for fn in zl.namelist() if fn.endswith('labelIds.png')}
            img_fns = {key(fn): fn for fn in zi.namelist() if fn.endswith('leftImg8bit.png')}
        keys = img_fns.keys() if len(img_fns) < len(label_fns) else label_fns.keys()
        self.img_fns = [img_fns[k] for k in keys]
        self.label_fns = [label_fns[k] for k in keys]
        self.resize_shape = tuple(int(v) for v in resize_shape)
        self.img_zip_fn, self.label_zip_fn = img_zip_fn, label_zip_fn
        self.img_zf = self.label_zf = None

    def __len__(self):
        return len(self.label_fns)

    def _open(self):
        if self.img_zf is None:
            self.img_zf = zipfile.ZipFile(self.img_zip_fn)
        if self.label_zf is None:
            self.label_zf = zipfile.ZipFile(self.label_zip_fn)

    def get_raw(self, i):
        self._open()
        img = _decode(self.img_zf.open(self.img_fns[i]))
        label = label_mask(_decode(self.label_zf.open(self.label_fns[i]), gray=True))
        return img, label

    def get_example(self, i):
        from importlib import import_module
        cli = import_module(__package__ + '.cli')
        img, label = self.get_raw(i)
        if img.shape[1:] != self.resize_shape:
            img = cli.resize_cvcubic_chw(img, self.resize_shape)
        img = img.astype(np.float32)
        img -= MEAN[:, None, None]
        img /= STD[:, None, None]
        return img, label

    def __getitem__(self, i):
        return self.get_example(i)


# ------------------------------------------------------------------------------- score resize (host form)
def pil_bilinear_coeffs(in_size, out_size):
    """Pillow Resample.c precompute_coeffs for BILINEAR at an upscale: (first index (out,), taps (out, 3) float64)."""
    scale = float(in_size) / float(out_size)
    lo = np.zeros(out_size, np.int64)
    k = np.zeros((out_size, 3), np.float64)
    for o in range(out_size):
        center = (o + 0.5) * scale
        a = max(int(center - 1.0 + 0.5), 0)
        b = min(int(center + 1.0 + 0.5), in_size)
        ww = 0.0
        for j in range(b - a):
            x = abs((float(j + a) - center + 0.5) * 1.0)
            k[o, j] = 1.0 - x if x < 1.0 else 0.0
            ww += k[o, j]
        if ww != 0.0:
            k[o, :] /= ww
        lo[o] = a
    return lo, k


def resize_bilinear_pil(score, shape):
    """score (C,h,w) float32 -> (C,H,W) float32 as chainercv.transforms.resize(score, shape) with the PIL backend
    (Image.resize(BILINEAR) per channel, mode 'F'): a horizontal pass summed in double and stored as float32, then the
    vertical pass.  The host form of spa_segnet_score; upscales only."""
    C, h, w = score.shape
    H, W = int(shape[0]), int(shape[1])
    if H < h or W < w:
        raise ValueError('resize (%d, %d) -> (%d, %d) is a downscale: not supported' % (h, w, H, W))
    xl, xk = pil_bilinear_coeffs(w, W)
    yl, yk = pil_bilinear_coeffs(h, H)
    s = score.astype(np.float64)
    xi = np.minimum(xl[:, None] + np.arange(3)[None, :], w - 1)
    yi = np.minimum(yl[:, None] + np.arange(3)[None, :], h - 1)
    t = np.zeros((C, h, W), np.float64)
    for j in range(3):
        t = t + s[:, :, xi[:, j]] * xk[:, j]
    t = t.astype(np.float32).astype(np.float64)
    o = np.zeros((C, H, W), np.float64)
    for j in range(3):
        o = o + t[:, yi[:, j], :] * yk[:, j][None, :, None]
    return o.astype(np.float32)


# ------------------------------------------------------------------------------- the network
class SegNetBasic(object):
    """The folded, packed network on one GPU.  predict(imgs) takes the images as the device path feeds them: (B,3,H,W)
    float32 0..255 at the training input_shape (the dataset's cubic resize done, its standardisation NOT: conv1 applies
    it in its load, with the same two float32 operations), H and W multiples of 16.  dtype (DTYPES): 'fp32' the
    float32 matrix-core convolutions, 'bf16' the bf16 ones (operands rounded to bf16, float32 accumulation).
    split_planes (with dtype 'fp32' only): the float32-accurate convolutions on the f16 matrix cores."""

    def __init__(self, params, pred_shape=None, device=None, engine=None, dtype='fp32', split_planes=False):
        check_mode('SegNetBasic', dtype, split_planes)
        import torch
        from .engine import Engine
        self.dtype = dtype
        self.split_planes = bool(split_planes)
        self.engine = engine or Engine(device)
        dev = self.engine.device
        folded = fold_bn(params)
        self.w, self.b = {}, {}
        for name in LAYERS:
            w, b = folded[name]
            self.w[name] = torch.from_numpy(pack_weight(w)).to(dev)
            self.b[name] = torch.from_numpy(b).to(dev)
        wc, bc = folded['conv_classifier']
        self.wc = torch.from_numpy(np.ascontiguousarray(wc)).to(dev)
        self.bc = torch.from_numpy(bc).to(dev)
        self.pred_shape = tuple(int(v) for v in pred_shape) if pred_shape is not None else None

    @classmethod
    def from_snapshot(cls, param_dir, iteration, pred_shape=None, device=None, dtype='fp32', split_planes=False):
        check_mode('SegNetBasic', dtype, split_planes)
        train_args, snapshot, params = load_snapshot(param_dir, iteration)
        model = cls(params, pred_shape, device, dtype=dtype, split_planes=split_planes)
        model.train_args, model.snapshot = train_args, snapshot
        return model

    @classmethod
    def from_snapshot_file(cls, snapshot, pred_shape=None, device=None, dtype='fp32', split_planes=False):
        """The network of one snapshot file (read_snapshot), as utils/create_demovideo.py --snapshot names it."""
        check_mode('SegNetBasic', dtype, split_planes)
        model = cls(read_snapshot(snapshot), pred_shape, device, dtype=dtype, split_planes=split_planes)
        model.snapshot = snapshot
        return model

    def forward(self, x, timer=None, trace=None, logits=False):
        """x (B,3,H,W) float32 0..255 on the device -> softmax probabilities (B,2,H,W) float32, or with logits=True the
        classifier's raw scores (the values that softmax consumes).  timer(name) is called before each layer and at the
        end (per-layer event timing, tools/segnet_bench.py); trace (a list) receives the encoders' (pooled, idx)
        pairs."""
        e = self.engine
        B, C, H, W = x.shape
        if C != 3 or H % 16 or W % 16:
            raise ValueError('SegNet-Basic input must be (B,3,H,W) with H, W multiples of 16, got %s' % (tuple(x.shape),))
        if self.dtype == 'bf16':
            encode, decode = e.segnet_encode_bf16, e.segnet_decode_bf16
        elif self.split_planes:
            encode, decode = e.segnet_encode_f16x3, e.segnet_decode_f16x3
        else:
            encode, decode = e.segnet_encode, e.segnet_decode
        h, pools = x, []
        for name in ENCODERS:
            timer and timer(name)
            h, idx = encode(h, self.w[name], self.b[name], MEAN, STD)
            pools.append(idx)
            if trace is not None:
                trace.append((h, idx))
        for name, idx in zip(DECODERS, pools[::-1]):
            timer and timer(name)
            if name == 'conv_decode1':
                h = decode(h, idx, self.w[name], self.b[name], self.wc, self.bc, logits=logits)
            else:
                h = decode(h, idx, self.w[name], self.b[name])
        timer and timer(None)
        return h

    def predict(self, imgs, return_score=False):
        """segnet_basic.py:84-113, batched: imgs (B,3,H,W) float32 0..255 (torch tensor on the device, or numpy) ->
        list of labels (int32 (H',W')), or of (label, score float32 (2,H',W')) with return_score, (H',W') = pred_shape
        (the probabilities resized with Pillow's BILINEAR) or the input size."""
        import torch
        x = torch.as_tensor(imgs, dtype=torch.float32).to(self.engine.device).contiguous()
        prob = self.forward(x)
        shape = self.pred_shape or tuple(prob.shape[2:])
        mask, sc = self.engine.segnet_score(prob, shape, want_scores=return_score)
        mask = mask.cpu().numpy().astype(np.int32)
        if not return_score:
            return list(mask)
        sc = sc.cpu().numpy()
        return [(mask[i], sc[i]) for i in range(mask.shape[0])]

    def predict_labels(self, imgs):
        """What the reference's predict(imgs) returns WITHOUT return_score (segnet_basic.py:96-114,
        utils/create_demovideo.py): the argmax of the classifier's raw scores resized to pred_shape with Pillow's
        BILINEAR -- no softmax before the resize, where predict() above resizes probabilities.  The two differ where
        the resize mixes pixels of different confidence.  imgs as for predict -> list of int32 (H',W') labels."""
        import torch
        x = torch.as_tensor(imgs, dtype=torch.float32).to(self.engine.device).contiguous()
        z = self.forward(x, logits=True)
        mask, _ = self.engine.segnet_score(z, self.pred_shape or tuple(z.shape[2:]))
        return list(mask.cpu().numpy().astype(np.int32))
