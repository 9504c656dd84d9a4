"""CPU tests of the fused BatchNorm training mode (train_segnet.py --fused_bn, SegNetTrainer(fused_bn=True)): the flag
is read in front of and among the reference flags, args.txt records it only when given, utils/run_train_rounds.py
forwards it, and a non-bool fused_bn is refused before an Engine exists.

The second half is the float64 restatement of the kernels of csrc/spa_segnet_train_bn.hip that
tests/test_gpu_segnet_train_fused.py compares them with, and the seeded inputs of those tests.  Here the restatement is
checked against autograd: the three layers, written with the kernels' explicit backward formulas, give
segnet_train.reference_loss's loss and gradients when they replace its torch ops, and the inputs leave fewer than
UNDECIDED_CAP of their pooling windows without a decided index."""
import importlib
import json
import os
import sys

import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402

segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
engine = importlib.import_module('superpixel-align_amd.engine')
train_segnet = importlib.import_module('train_segnet')
rtr = importlib.import_module('utils.run_train_rounds')

F = torch.nn.functional


# ------------------------------------------------------------------------------- the command line
def test_pre_parser_reads_fused_bn():
    pre, rest = train_segnet.get_pre_args([])
    assert pre.fused_bn is False and rest == []
    pre, rest = train_segnet.get_pre_args(['--fused_bn', '--batchsize', '2', '--lr', '0.1'])
    assert pre.fused_bn is True and rest == ['--batchsize', '2', '--lr', '0.1']
    pre, rest = train_segnet.get_pre_args(['--batchsize', '2', '--fused_bn', '--lr', '0.1', '--random'])
    assert pre.fused_bn is True and pre.dtype == 'fp32' and rest == ['--batchsize', '2', '--lr', '0.1', '--random']
    with pytest.raises(SystemExit):                       # the reference parser does not take it
        train_segnet.get_args(['--fused_bn'])
    assert 'fused_bn' not in vars(train_segnet.get_args([]))
    # with every other mode of this implementation
    pre, rest = train_segnet.get_pre_args(['--dtype', 'bf16', '--fused_bn', '--data_parallel', '--loader_procs', '3',
                                           '--resume', 'x'])
    assert pre.fused_bn and pre.dtype == 'bf16' and pre.data_parallel and pre.loader_procs == 3
    assert rest == ['--resume', 'x']
    pre, rest = train_segnet.get_pre_args(['--split_planes', '--fused_bn'])
    assert pre.fused_bn and pre.split_planes and rest == []


def test_run_args_record_fused_bn_only_when_given():
    reference = vars(train_segnet.get_parser().parse_args([]))
    pre, args = train_segnet.run_args([])
    assert vars(args) == dict(reference, dtype='fp32')                 # a default run's args.txt entries
    pre, args = train_segnet.run_args(['--fused_bn'])
    assert vars(args) == dict(reference, dtype='fp32', fused_bn=True)
    assert '"fused_bn": true' in json.dumps(vars(args), indent=4, sort_keys=True)
    pre, args = train_segnet.run_args(['--split_planes', '--fused_bn', '--data_parallel'])
    assert args.fused_bn is True and args.split_planes is True and args.data_parallel is True
    pre, args = train_segnet.run_args(['--dtype', 'bf16', '--fused_bn'])
    assert vars(args) == dict(reference, dtype='bf16', fused_bn=True)


def _train_argvs(argv):
    a = rtr.get_args(argv)
    steps = [s for s in rtr.plan(a, 'R/train_round1_x_0') if s['kind'] == 'train']
    dirs = {i + 1: 'D%d' % (i + 1) for i in range(len(steps))}
    return [rtr.train_argv(a, s, 'D%d' % (i + 1), dirs) for i, s in enumerate(steps)]


def test_rounds_driver_forwards_the_flag_only_when_given():
    base = ['--n_round', '3', '--iteration', '100', '--val_iteration', '50', '--n_use_data', '40', '--random']
    plain = _train_argvs(base)
    flagged = _train_argvs(base + ['--fused_bn'])
    assert len(plain) == len(flagged) > 1
    for a, b in zip(plain, flagged):
        assert '--fused_bn' not in a
        assert b == a + ['--fused_bn']
    assert rtr.get_args(base).fused_bn is False
    both = _train_argvs(base + ['--fused_bn', '--split_planes', '--loader_procs', '2'])
    for a in both:
        assert '--fused_bn' in a and '--split_planes' in a and '--loader_procs' in a
    for a in _train_argvs(base + ['--fused_bn', '--dtype', 'bf16']):
        assert '--fused_bn' in a and a[a.index('--dtype') + 1] == 'bf16'
    # train_segnet.py takes the child command line with the flag
    pre, rest = train_segnet.get_pre_args(flagged[1])
    assert pre.fused_bn and pre.data_parallel and '--fused_bn' not in rest
    train_segnet.get_args(rest)


class _NoEngine(object):
    def __init__(self, *a, **k):
        raise AssertionError('an Engine was created')


def test_trainer_rejects_a_non_bool_fused_bn(monkeypatch):
    monkeypatch.setattr(engine, 'Engine', _NoEngine)
    for bad in (1, 0, 'yes', None, 'True'):
        with pytest.raises(ValueError, match='fused_bn'):
            st.SegNetTrainer(st.init_params(0), st.MomentumSGD(), st.softmax_cross_entropy, fused_bn=bad)
    for ok in (True, False):
        with pytest.raises(AssertionError, match='Engine'):          # the patch is what a trainer would reach
            st.SegNetTrainer(st.init_params(0), st.MomentumSGD(), st.softmax_cross_entropy, fused_bn=ok)


def test_engine_and_library_name_the_five_entry_points(spa):
    for name in ('bn_forward', 'bn_backward_sums', 'bn_backward_dy', 'classifier_forward', 'classifier_backward'):
        assert callable(getattr(engine.Engine, 'segnet_train_' + name))
        assert 'spa_segnet_train_' + name in spa._lib.PROTOTYPES
        assert hasattr(spa._lib.lib(), 'spa_segnet_train_' + name)


# ------------------------------------------------------------------------------- the float64 restatement
# Every function takes channels-last (B,H,W,64) maps and (64) vectors of one dtype on one device and uses torch ops
# only; the GPU tests call them with float64 copies of exactly the float32 operands the kernels get.
def windows(a):
    """(B,H,W,C) -> (B,H/2,W/2,C,4), window position ky * 2 + kx last"""
    B, H, W, C = a.shape
    return a.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)


def unwindows(w):
    """the inverse of windows"""
    B, Hh, Wh, C, _ = w.shape
    return w.reshape(B, Hh, Wh, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * Hh, 2 * Wh, C)


def bn_forward(y, mean, rstd, gamma, beta):
    return (y - mean) * (rstd * gamma) + beta


def pool_forward(o):
    """-> (the 2x2 maximum of relu(o), the index of its first maximum)"""
    win = windows(torch.relu(o))
    idx = win.argmax(-1, keepdim=True)
    return win.gather(-1, idx)[..., 0], idx[..., 0].to(torch.uint8)


def full_gradient(gp, idx, p):
    """the full-resolution gradient of the encoder form: gp at the position idx selects where p > 0, zero elsewhere"""
    g = torch.where(p > 0, gp, torch.zeros_like(gp))
    sel = torch.arange(4, device=gp.device) == idx.long()[..., None]
    return unwindows(g[..., None] * sel.to(gp.dtype))


def backward_terms(g, y, mean, rstd):
    """-> the elementwise terms (g, g * xhat) whose sums over (B,H,W) the sums kernel forms"""
    return g, g * ((y - mean) * rstd)


def backward_sums(g, y, mean, rstd):
    t0, t1 = backward_terms(g, y, mean, rstd)
    return torch.stack([t0.sum((0, 1, 2)), t1.sum((0, 1, 2))])


def backward_dy(g, y, mean, rstd, gamma, sums, m):
    return (gamma * rstd / m) * (m * g - sums[0] - (y - mean) * rstd * sums[1])


def classifier_forward(h, wc, bc):
    return h @ wc.t() + bc


def classifier_backward(ds, h, wc):
    """-> (dh, dwc (2,64), db (2))"""
    return ds @ wc, ds.reshape(-1, 2).t() @ h.reshape(-1, 64), ds.sum((0, 1, 2))


def _layers():
    class EncoderBN(torch.autograd.Function):
        @staticmethod
        def forward(ctx, y, gamma, beta, mean, rstd):
            p, idx = pool_forward(bn_forward(y, mean, rstd, gamma, beta))
            ctx.save_for_backward(y, gamma, mean, rstd, idx, p)
            ctx.mark_non_differentiable(idx)
            return p, idx

        @staticmethod
        def backward(ctx, gp, _gi):
            y, gamma, mean, rstd, idx, p = ctx.saved_tensors
            g = full_gradient(gp, idx, p)
            s = backward_sums(g, y, mean, rstd)
            m = y.numel() / 64
            return backward_dy(g, y, mean, rstd, gamma, s, m), s[1], s[0], None, None

    class DecoderBN(torch.autograd.Function):
        @staticmethod
        def forward(ctx, y, gamma, beta, mean, rstd):
            ctx.save_for_backward(y, gamma, mean, rstd)
            return bn_forward(y, mean, rstd, gamma, beta)

        @staticmethod
        def backward(ctx, g):
            y, gamma, mean, rstd = ctx.saved_tensors
            s = backward_sums(g, y, mean, rstd)
            return backward_dy(g, y, mean, rstd, gamma, s, y.numel() / 64), s[1], s[0], None, None

    class Classifier(torch.autograd.Function):
        @staticmethod
        def forward(ctx, h, wc, bc):
            ctx.save_for_backward(h, wc)
            return classifier_forward(h, wc, bc)

        @staticmethod
        def backward(ctx, g):
            h, wc = ctx.saved_tensors
            return classifier_backward(g, h, wc)

    return EncoderBN, DecoderBN, Classifier


def fused_reference_loss(P, img, t, lossfun):
    """segnet_train.reference_loss's network (float64, F.conv2d) with the three restated layers in place of its
    batch_norm / relu / pooling / classifier ops.  -> (loss, the four index maps)"""
    EncoderBN, DecoderBN, Classifier = _layers()

    def statistics(y):
        mean = y.detach().mean((0, 1, 2))
        var = y.detach().var((0, 1, 2), unbiased=False)
        return mean, 1.0 / torch.sqrt(var + segnet.BN_EPS)

    def conv7(h, w):                                   # channels-last in and out
        return F.conv2d(h.permute(0, 3, 1, 2), w, padding=3).permute(0, 2, 3, 1)

    h = st.conv1_input(img).permute(0, 2, 3, 1)
    pools = []
    for name in segnet.ENCODERS:
        y = conv7(h, P[name + '/W'])
        h, idx = EncoderBN.apply(y, P[name + '_bn/gamma'], P[name + '_bn/beta'], *statistics(y))
        pools.append(idx)
    for name, idx in zip(segnet.DECODERS, pools[::-1]):
        up = st.unpool_ref(h.permute(0, 3, 1, 2), idx.permute(0, 3, 1, 2).long()).permute(0, 2, 3, 1)
        y = conv7(up, P[name + '/W'])
        h = DecoderBN.apply(y, P[name + '_bn/gamma'], P[name + '_bn/beta'], *statistics(y))
    score = Classifier.apply(h, P['conv_classifier/W'].view(2, 64), P['conv_classifier/b'])
    return lossfun(score.permute(0, 3, 1, 2), t), pools


@pytest.mark.parametrize('lossfun', ['softmax_cross_entropy', 'soft_label_loss', 'mse_loss'])
def test_restatement_matches_reference_loss_gradients(lossfun):
    B, H, W = 2, 16, 32
    p = sref.random_params(11)                         # gammas and betas away from their initial 1 and 0.001
    g = torch.Generator().manual_seed(12)
    img = torch.rand((B, 3, H, W), generator=g, dtype=torch.float64) * 255
    if lossfun == 'softmax_cross_entropy':
        t = torch.randint(-1, 2, (B, H, W), generator=g)
    else:
        t = torch.rand((B, 2, H, W), generator=g, dtype=torch.float64)
    fn = getattr(st, lossfun)
    out = []
    for fused in (False, True):
        P = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in st.PARAM_KEYS}
        S = {k: torch.tensor(p[k], dtype=torch.float64) for k in st.STAT_KEYS}
        loss, pools = fused_reference_loss(P, img, t, fn) if fused else st.reference_loss(P, S, img, t, fn)
        out.append((loss, pools, dict(zip(P, torch.autograd.grad(loss, list(P.values()))))))
    (l0, m0, g0), (l1, m1, g1) = out
    assert abs(l0.item() - l1.item()) < 1e-12 * abs(l0.item())
    for a, b in zip(m0, m1):
        assert torch.equal(a, b)
    for k in st.PARAM_KEYS:
        e = float((g0[k] - g1[k]).abs().max() / g0[k].abs().max())
        assert e < 1e-9, '%s: %.3g' % (k, e)


# ------------------------------------------------------------------------------- the GPU tests' inputs
SHAPES = [(1, 2, 2), (2, 6, 10), (1, 16, 16), (3, 64, 128), (2, 256, 512)]
# (1,2,2): one window per channel; (2,6,10): conv4's partial tiles; (2,256,512): 64 MB per map, the capped grid of
# 2048 workgroups x 16 pixels walks it 8 times
POOL_TOL = 1e-5           # a window is decided by this fraction of max|o|
UNDECIDED_CAP = 1e-3      # the share of windows that may be left out of the index comparison
ZERO_CH, NEG_CH = 5, 9    # the channels whose gamma is 0 and negative


def kernel_inputs(shape, seed=21):
    """float32 CPU operands of every kernel at (B,H,W): y = randn * 1.5 + 0.3, gradients randn, gamma in [0.5, 1.5]
    with channel ZERO_CH at 0 and NEG_CH negated, beta in [-0.2, 0.2], mean and rstd the float32 batch statistics of
    y.  beta[ZERO_CH] is -0.1: that channel's o is beta everywhere, so its windows are all-negative (pooled 0, index
    0) and decided; a positive beta there would make 1/64 of all windows four-way ties."""
    B, H, W = shape
    g = torch.Generator().manual_seed(seed + B * 1000003 + H * 1009 + W)
    d = {}
    d['y'] = torch.randn((B, H, W, 64), generator=g) * 1.5 + 0.3
    d['g'] = torch.randn((B, H, W, 64), generator=g)
    d['gp'] = torch.randn((B, H // 2, W // 2, 64), generator=g)
    d['gamma'] = torch.rand(64, generator=g) + 0.5
    d['gamma'][ZERO_CH] = 0.0
    d['gamma'][NEG_CH] *= -1.0
    d['beta'] = torch.rand(64, generator=g) * 0.4 - 0.2
    d['beta'][ZERO_CH] = -0.1
    y64 = d['y'].double()
    d['mean'] = y64.mean((0, 1, 2)).float()
    d['rstd'] = (1.0 / torch.sqrt(y64.var((0, 1, 2), unbiased=False) + segnet.BN_EPS)).float()
    d['wc'] = torch.randn((2, 64), generator=g) / 4
    d['bc'] = torch.rand(2, generator=g) * 0.2 - 0.1
    d['ds'] = torch.randn((B, H, W, 2), generator=g)
    return d


def decided(o, tol):
    """o (B,H,W,C) the float64 pre-ReLU map -> (all four below -tol, the maximum above 0 and the runner-up by more
    than tol, argmax), each (B,H/2,W/2,C)"""
    win = windows(o)
    srt = win.sort(-1, descending=True).values
    neg = (win < -tol).all(-1)
    lead = (srt[..., 0] > tol) & (srt[..., 0] - srt[..., 1] > tol)
    return neg, lead, win.argmax(-1)


@pytest.mark.parametrize('shape', SHAPES)
def test_inputs_leave_few_windows_undecided(shape):
    d = {k: v.double() for k, v in kernel_inputs(shape).items()}
    o = bn_forward(d['y'], d['mean'], d['rstd'], d['gamma'], d['beta'])
    neg, lead, _ = decided(o, POOL_TOL * float(o.abs().max()))
    share = 1.0 - float((neg | lead).double().mean())
    print('%s: undecided windows %.3g' % (shape, share))
    assert share < UNDECIDED_CAP
    assert bool(neg[..., ZERO_CH].all()) and float(neg.double().mean()) > 0.01      # both kinds occur
    assert float(lead.double().mean()) > 0.5
