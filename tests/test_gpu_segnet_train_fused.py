"""GPU tests of the fused BatchNorm training mode (csrc/spa_segnet_train_bn.hip, SegNetTrainer(fused_bn=True),
train_segnet.py --fused_bn).  Every kernel is compared with the float64 torch restatement of
tests/test_segnet_train_fused_cpu.py, evaluated on the device on float64 copies of exactly the float32 operands the
kernel gets (the float32 mean and rstd included), so only the kernel's own roundings count.  Outputs are NaN- or
255-poisoned with a guard past the end, every call is repeated for equal bits, refused calls write nothing.  Then one
whole step per convolution family and one two-rank step against segnet_train.reference_loss, and train_segnet.py
--fused_bn -> --resume -> labels_from_segnet.py on synthetic zips."""
import ctypes
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402
import test_segnet_train_fused_cpu as fref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
st = importlib.import_module('superpixel-align_amd.segnet_train')
SpalignError = importlib.import_module('superpixel-align_amd._lib').SpalignError

SHAPES = fref.SHAPES
# Elementwise outputs, as a fraction of max|ref|.  The forward expression is four float32 roundings of 6e-8 each on
# values no larger than max|ref| for these inputs: 2.4e-7, a factor of 4 below the bound.
BN_FWD_TOL = 1e-6
ELEM_TOL = 1e-5           # dy, score, dh: FWD_TOL's convention in test_gpu_segnet_train.py
SUM_TOL = 1e-6            # every reduction, as a fraction of sum |term|: BN_TOL's convention in test_gpu_segnet_train.py


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


_CASES = {}


def case(shape):
    """the float32 device operands of fref.kernel_inputs(shape) and, computed once per shape, their float64 copies and
    the float64 references: o, the pooled map and its decided windows, the full-resolution encoder gradient, the sums"""
    if shape in _CASES:
        return _CASES[shape]
    d = {k: v.cuda().contiguous() for k, v in fref.kernel_inputs(shape).items()}
    r = {k: v.double() for k, v in d.items()}
    r['o'] = fref.bn_forward(r['y'], r['mean'], r['rstd'], r['gamma'], r['beta'])
    r['p'], r['idx'] = fref.pool_forward(r['o'])
    # the backward of the encoder form gets what the forward kernel stores; its reference the same values
    c = dict(d=d, r=r)
    _CASES.clear()                                      # one shape's references at a time (64 MB maps)
    _CASES[shape] = c
    return c


def byte_poisoned(shape, guard=1024):
    n = int(np.prod(shape))
    buf = torch.full((n + guard,), 255, dtype=torch.uint8, device='cuda')
    return buf[:n].view(shape), buf


def err(got, ref):
    """max |got - ref| / max |ref|"""
    return float((got.double() - ref).abs().max() / ref.abs().max())


def sum_err(got, terms):
    """the per-channel sums `got` against the float64 sums of `terms` over all but the last axis, as a fraction of the
    sums of |terms|; the worst channel"""
    t = terms.reshape(-1, terms.shape[-1])
    scale = t.abs().sum(0).clamp_min(1e-300)
    return float(((got.double() - t.sum(0)).abs() / scale).max())


# ------------------------------------------------------------------------------- forward
@pytest.mark.parametrize('shape', SHAPES)
def test_forward_decoder_form(eng, shape):
    c = case(shape)
    d, r = c['d'], c['r']
    B, H, W = shape
    out, buf = sref.poisoned((B, H, W, 64))
    o = eng.segnet_train_bn_forward(d['y'], d['mean'], d['rstd'], d['gamma'], d['beta'], out=out)
    torch.cuda.synchronize()
    sref.check_guard(buf, B * H * W * 64)
    assert not torch.isnan(o).any().item(), 'an output was not stored'
    e = err(o, r['o'])
    print('bn forward %s: %.3g of max|ref|' % (shape, e))
    assert e < BN_FWD_TOL
    assert torch.equal(eng.segnet_train_bn_forward(d['y'], d['mean'], d['rstd'], d['gamma'], d['beta']), o)


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_encoder_form(eng, shape):
    c = case(shape)
    d, r = c['d'], c['r']
    B, H, W = shape
    n = B * (H // 2) * (W // 2) * 64
    out, buf = sref.poisoned((B, H // 2, W // 2, 64))
    oi, ibuf = byte_poisoned((B, H // 2, W // 2, 64))
    p, idx = eng.segnet_train_bn_forward(d['y'], d['mean'], d['rstd'], d['gamma'], d['beta'], pool=True, out=out,
                                         out_idx=oi)
    torch.cuda.synchronize()
    sref.check_guard(buf, n)
    assert bool((ibuf[n:] == 255).all()), 'a kernel wrote past the end of its index map'
    assert not torch.isnan(p).any().item() and int(idx.max()) <= 3, 'an output was not stored'
    scale = float(r['o'].abs().max())
    e = float((p.double() - r['p']).abs().max()) / scale
    neg, lead, arg = fref.decided(r['o'], fref.POOL_TOL * scale)
    share = 1.0 - float((neg | lead).double().mean())
    print('bn + relu + pool %s: pooled %.3g of max|ref|, undecided windows %.3g' % (shape, e, share))
    assert e < BN_FWD_TOL
    assert share < fref.UNDECIDED_CAP
    assert bool((p[neg] == 0.0).all()), 'an all-negative window is not exactly 0'
    assert int((idx[neg] != 0).sum()) == 0, 'an all-negative window has a non-zero index'
    assert int((idx.long()[lead] != arg[lead]).sum()) == 0, 'a decided window has another index'
    # the gamma = 0 channel: beta < 0 everywhere
    assert bool((p[..., fref.ZERO_CH] == 0).all()) and bool((idx[..., fref.ZERO_CH] == 0).all())
    p2, idx2 = eng.segnet_train_bn_forward(d['y'], d['mean'], d['rstd'], d['gamma'], d['beta'], pool=True)
    assert torch.equal(p2, p) and torch.equal(idx2, idx)


# ------------------------------------------------------------------------------- backward
def encoder_operands(eng, c):
    """(gp, idx, p) of the encoder backward: the forward kernel's own pooled map and indices, and the float64
    full-resolution gradient they define"""
    d, r = c['d'], c['r']
    if 'kp' not in c:
        c['kp'], c['kidx'] = eng.segnet_train_bn_forward(d['y'], d['mean'], d['rstd'], d['gamma'], d['beta'], pool=True)
        c['gfull'] = fref.full_gradient(r['gp'], c['kidx'], c['kp'].double())
    return d['gp'], c['kidx'], c['kp'], c['gfull']


@pytest.mark.parametrize('shape', SHAPES)
def test_backward_sums(eng, shape):
    c = case(shape)
    d, r = c['d'], c['r']
    gp, idx, p, gfull = encoder_operands(eng, c)
    for form, g, kw, g64 in (('decoder', d['g'], {}, r['g']), ('encoder', gp, dict(idx=idx, p=p), gfull)):
        out, buf = sref.poisoned((2, 64), torch.float64)
        s = eng.segnet_train_bn_backward_sums(g, d['y'], d['mean'], d['rstd'], out=out, **kw)
        torch.cuda.synchronize()
        sref.check_guard(buf, 128)
        assert not torch.isnan(s).any().item()
        t0, t1 = fref.backward_terms(g64, r['y'], r['mean'], r['rstd'])
        e0, e1 = sum_err(s[0], t0), sum_err(s[1], t1)
        print('bn backward sums %s %s: %.3g, %.3g of sum|term|' % (form, shape, e0, e1))
        assert e0 < SUM_TOL and e1 < SUM_TOL
        assert torch.equal(eng.segnet_train_bn_backward_sums(g, d['y'], d['mean'], d['rstd'], **kw), s)
    # nothing flows through a window whose pooled output is 0: another gradient there, the same bits
    gp2 = torch.where(p > 0, gp, gp + 100.0)
    assert not torch.equal(gp2, gp)
    assert torch.equal(eng.segnet_train_bn_backward_sums(gp2, d['y'], d['mean'], d['rstd'], idx=idx, p=p), s)


@pytest.mark.parametrize('shape', SHAPES)
def test_backward_dy(eng, shape):
    c = case(shape)
    d, r = c['d'], c['r']
    B, H, W = shape
    m = float(B * H * W)
    gp, idx, p, gfull = encoder_operands(eng, c)
    for form, g, kw, g64 in (('decoder', d['g'], {}, r['g']), ('encoder', gp, dict(idx=idx, p=p), gfull)):
        own = eng.segnet_train_bn_backward_sums(g, d['y'], d['mean'], d['rstd'], **kw)
        exact = fref.backward_sums(g64, r['y'], r['mean'], r['rstd'])
        for what, sums in (("the kernel's sums", own), ('float64 sums', exact)):
            out, buf = sref.poisoned((B, H, W, 64))
            dy = eng.segnet_train_bn_backward_dy(g, d['y'], d['mean'], d['rstd'], d['gamma'], sums, m, out=out, **kw)
            torch.cuda.synchronize()
            sref.check_guard(buf, B * H * W * 64)
            assert not torch.isnan(dy).any().item(), 'an output was not stored'
            ref = fref.backward_dy(g64, r['y'], r['mean'], r['rstd'], r['gamma'], sums, m)
            e = err(dy, ref)
            print('bn backward dy %s %s, %s: %.3g of max|ref|' % (form, shape, what, e))
            assert e < ELEM_TOL
            assert torch.equal(eng.segnet_train_bn_backward_dy(g, d['y'], d['mean'], d['rstd'], d['gamma'], sums, m,
                                                               **kw), dy)
    assert bool((dy[..., fref.ZERO_CH] == 0).all())              # gamma = 0: no gradient reaches y
    gp2 = torch.where(p > 0, gp, gp + 100.0)
    assert torch.equal(eng.segnet_train_bn_backward_dy(gp2, d['y'], d['mean'], d['rstd'], d['gamma'], sums, m, idx=idx,
                                                       p=p), dy)
    # a data-parallel step passes the ranks' total and the union's pixel count
    dy2 = eng.segnet_train_bn_backward_dy(g, d['y'], d['mean'], d['rstd'], d['gamma'], sums * 2, 2 * m, **kw)
    assert err(dy2, fref.backward_dy(g64, r['y'], r['mean'], r['rstd'], r['gamma'], sums * 2, 2 * m)) < ELEM_TOL


# ------------------------------------------------------------------------------- classifier
@pytest.mark.parametrize('shape', SHAPES)
def test_classifier(eng, shape):
    c = case(shape)
    d, r = c['d'], c['r']
    B, H, W = shape
    h, h64 = d['y'], r['y']
    out, buf = sref.poisoned((B, H, W, 2))
    score = eng.segnet_train_classifier_forward(h, d['wc'], d['bc'], out=out)
    torch.cuda.synchronize()
    sref.check_guard(buf, B * H * W * 2)
    assert not torch.isnan(score).any().item()
    e = err(score, fref.classifier_forward(h64, r['wc'], r['bc']))
    assert torch.equal(eng.segnet_train_classifier_forward(h, d['wc'], d['bc']), score)
    odh, bdh = sref.poisoned((B, H, W, 64))
    odw, bdw = sref.poisoned((2, 64))
    odb, bdb = sref.poisoned((2,))
    dh, dw, db = eng.segnet_train_classifier_backward(d['ds'], h, d['wc'], out=odh, out_dw=odw, out_db=odb)
    torch.cuda.synchronize()
    sref.check_guard(bdh, B * H * W * 64)
    sref.check_guard(bdw, 128)
    sref.check_guard(bdb, 2)
    assert not (torch.isnan(dh).any().item() or torch.isnan(dw).any().item() or torch.isnan(db).any().item())
    rdh, _, _ = fref.classifier_backward(r['ds'], h64, r['wc'])
    eh = err(dh, rdh)
    ew = max(sum_err(dw[k], r['ds'][..., k:k + 1] * h64) for k in range(2))
    eb = sum_err(db, r['ds'])
    print('classifier %s: score %.3g, dh %.3g of max|ref|; dWc %.3g, db %.3g of sum|term|' % (shape, e, eh, ew, eb))
    assert e < ELEM_TOL and eh < ELEM_TOL and ew < SUM_TOL and eb < SUM_TOL
    dh2, dw2, db2 = eng.segnet_train_classifier_backward(d['ds'], h, d['wc'])
    assert torch.equal(dh2, dh) and torch.equal(dw2, dw) and torch.equal(db2, db)


# ------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(eng):
    lib, ctx, s = eng._lib, eng._ctx, eng._s()
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)
    B, H, W = 1, 6, 8
    y = torch.randn((B, H, W, 64), device='cuda')
    half = torch.randn((B, H // 2, W // 2, 64), device='cuda')
    v = torch.rand(64, device='cuda') + 0.5
    ix = torch.zeros((B, H // 2, W // 2, 64), dtype=torch.uint8, device='cuda')
    ds = torch.randn((B, H, W, 2), device='cuda')
    wc = torch.randn((2, 64), device='cuda')
    sums = torch.zeros((2, 64), dtype=torch.float64, device='cuda')
    out, buf = sref.poisoned((B, H, W, 64))
    out64, buf64 = sref.poisoned((2, 64), torch.float64)
    oi, ibuf = byte_poisoned((B, H // 2, W // 2, 64))
    dw, dwbuf = sref.poisoned((2, 64))
    db, dbbuf = sref.poisoned((2,))
    fwd, bsum, bdy = (lib.spa_segnet_train_bn_forward, lib.spa_segnet_train_bn_backward_sums,
                      lib.spa_segnet_train_bn_backward_dy)
    cf, cb = lib.spa_segnet_train_classifier_forward, lib.spa_segnet_train_classifier_backward
    null = None
    codes = [
        # odd H, odd W
        fwd(ctx, P(y), P(v), P(v), P(v), P(v), 1, 5, 8, P(out), null, s),
        fwd(ctx, P(y), P(v), P(v), P(v), P(v), 1, 6, 7, P(out), P(oi), s),
        bsum(ctx, P(y), null, null, P(y), P(v), P(v), 1, 5, 8, P(out64), s),
        bdy(ctx, P(y), null, null, P(y), P(v), P(v), P(v), P(sums), 48.0, 1, 6, 7, P(out), s),
        cf(ctx, P(y), P(wc), P(v), 1, 5, 8, P(out), s),
        cb(ctx, P(ds), P(y), P(wc), 1, 6, 7, P(out), P(dw), P(db), s),
        # an empty batch
        fwd(ctx, P(y), P(v), P(v), P(v), P(v), 0, 6, 8, P(out), null, s),
        # null pointers: an input, a parameter vector, an output; idx without p and p without idx; no context
        fwd(ctx, null, P(v), P(v), P(v), P(v), B, H, W, P(out), null, s),
        fwd(ctx, P(y), P(v), null, P(v), P(v), B, H, W, P(out), P(oi), s),
        bsum(ctx, P(half), P(ix), null, P(y), P(v), P(v), B, H, W, P(out64), s),
        bsum(ctx, P(half), null, P(half), P(y), P(v), P(v), B, H, W, P(out64), s),
        bdy(ctx, P(y), null, null, P(y), P(v), P(v), P(v), null, 48.0, B, H, W, P(out), s),
        bdy(ctx, P(half), P(ix), null, P(y), P(v), P(v), P(v), P(sums), 48.0, B, H, W, P(out), s),
        bdy(ctx, P(y), null, null, P(y), P(v), P(v), P(v), P(sums), 0.0, B, H, W, P(out), s),       # m = 0
        cf(ctx, P(y), null, P(v), B, H, W, P(out), s),
        cb(ctx, P(ds), P(y), P(wc), B, H, W, P(out), null, P(db), s),
        cb(None, P(ds), P(y), P(wc), B, H, W, P(out), P(dw), P(db), s),
        # a map that is not 16-byte aligned
        fwd(ctx, P(y.view(-1)[1:]), P(v), P(v), P(v), P(v), B, H, W - 2, P(out), null, s),
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in codes), codes
    # the Engine refuses before the library is called: a wrong dtype, a mismatched index shape, an odd size
    bad = [
        lambda: eng.segnet_train_bn_forward(y.double(), v, v, v, v, out=out),
        lambda: eng.segnet_train_bn_forward(y, v, v, v.double(), v, out=out),
        lambda: eng.segnet_train_bn_forward(y, v, v, v, v, pool=True, out=half, out_idx=ix.int()),
        lambda: eng.segnet_train_bn_forward(y, v, v, v, v, pool=True, out=out[:, :H // 2, :W // 2].contiguous(),
                                            out_idx=ix[:, :, :3].contiguous()),
        lambda: eng.segnet_train_bn_forward(y[:, :5].contiguous(), v, v, v, v),
        lambda: eng.segnet_train_bn_backward_sums(half, y, v, v, idx=ix[:, :2].contiguous(), p=half, out=out64),
        lambda: eng.segnet_train_bn_backward_sums(half, y, v, v, idx=ix, out=out64),
        lambda: eng.segnet_train_bn_backward_sums(y, y, v, v, idx=ix, p=half, out=out64),
        lambda: eng.segnet_train_bn_backward_dy(y, y, v, v, v, sums.float(), 48.0, out=out),
        lambda: eng.segnet_train_bn_backward_dy(half, y, v, v, v, sums, 48.0, idx=ix.long(), p=half, out=out),
        lambda: eng.segnet_train_classifier_forward(y, wc.t().contiguous(), v[:2].contiguous(), out=out[..., :2]),
        lambda: eng.segnet_train_classifier_backward(ds.half(), y, wc, out=out, out_dw=dw, out_db=db),
        lambda: eng.segnet_train_classifier_backward(ds[:, :4].contiguous(), y, wc, out=out, out_dw=dw, out_db=db),
    ]
    for call in bad:
        with pytest.raises(SpalignError):
            call()
    torch.cuda.synchronize()
    assert torch.isnan(buf).all().item() and torch.isnan(buf64).all().item()
    assert torch.isnan(dwbuf).all().item() and torch.isnan(dbbuf).all().item() and bool((ibuf == 255).all())


# ------------------------------------------------------------------------------- one whole step per family
# (loss, update, running statistics) bounds of the unfused step of each family, copied from
# test_gpu_segnet_train.py (test_full_training_step_against_float64: 1e-5, STEP_TOL, STAT_TOL),
# test_gpu_segnet_train_bf16.py (test_full_bf16_training_step_against_float64: 1e-2, STEP_TOL, STAT_TOL) and
# test_gpu_segnet_train_f16x3.py (LOSS_TOL, STEP_TOL, STAT_TOL)
STEP_BOUNDS = {'fp32': (1e-5, 5e-3, 3e-5), 'bf16': (1e-2, 2e-2, 3e-2), 'f16x3': (1e-5, 5e-3, 3e-5)}
FAMILY_KW = {'fp32': {}, 'bf16': dict(dtype='bf16'), 'f16x3': dict(split_planes=True)}


@pytest.mark.parametrize('family', ['fp32', 'bf16', 'f16x3'])
def test_full_fused_step_against_float64(eng, family):
    r = sref.step_against_float64(eng, dict(fused_bn=True, **FAMILY_KW[family]), bf16_operands=family == 'bf16')
    loss_tol, step_tol, stat_tol = STEP_BOUNDS[family]
    worst, es = r['updates'], r['stats']
    ku, ks = max(worst, key=worst.get), max(es, key=es.get)
    el = abs(r['loss'] - r['l64']) / abs(r['l64'])
    print('fused %s step: loss %.3g, worst update %.3g (%s), worst statistic %.3g (%s)'
          % (family, el, worst[ku], ku, es[ks], ks))
    assert el < loss_tol, 'loss %.9g vs float64 %.9g' % (r['loss'], r['l64'])
    assert worst[ku] < step_tol, '%s: update error %.3g' % (ku, worst[ku])
    assert es[ks] < stat_tol, '%s: running statistic error %.3g' % (ks, es[ks])
    assert len(r['maps']) == 4 and all(m.dtype == torch.uint8 and int(m.max()) <= 3 for m in r['maps'])


@pytest.mark.parametrize('family', ['fp32', 'bf16', 'f16x3'])
def test_fused_step_repeats_bit_for_bit(eng, family):
    sref.check_step_repeats(eng, fused_bn=True, **FAMILY_KW[family])


def test_unfused_trainer_is_the_default(eng):
    tr = st.SegNetTrainer(st.init_params(0), st.MomentumSGD(), st.softmax_cross_entropy, engine=eng)
    assert tr.fused_bn is False


# ------------------------------------------------------------------------------- two ranks
TIMEOUT = 900
SHARED = {'SPA_DIST_BACKEND': 'gloo', 'SPA_BENCH_SAME_DEVICE': '1'}

_STEP_RANK = r'''
import importlib, os, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
st = importlib.import_module('superpixel-align_amd.segnet_train')
dist = importlib.import_module('superpixel-align_amd.dist')
rank, ws, _ = dist.init()
eng = importlib.import_module('superpixel-align_amd.engine').default_engine()
g = torch.Generator().manual_seed(6)
img = torch.rand((4, 3, 64, 128), generator=g) * 255
t = torch.randint(0, 2, (4, 64, 128), generator=g)          # no ignored labels: the 2-rank step is the batch-4 step
p = st.init_params(5)
if rank == 1:
    p['conv1/W'] = p['conv1/W'] + 1.0                        # overwritten by rank 0's parameters (set_group)
tr = st.SegNetTrainer(p, st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy, engine=eng,
                      fused_bn=True)
tr.set_group(st.RankGroup())
trace = []
loss = tr.step(img[2 * rank:2 * rank + 2].cuda(), t[2 * rank:2 * rank + 2].cuda(), trace)
out = {k: v.cpu().numpy() for k, v in list(tr.P.items()) + list(tr.S.items())}
out.update({'trace%d' % i: m.cpu().numpy() for i, m in enumerate(trace)})
out['loss'] = np.asarray(loss)
np.savez(os.path.join(sys.argv[2], 'rank%d.npz' % rank), **out)
'''

# test_gpu_segnet_dp.py's TOLS['fp32'] (update, running statistics) and its loss bound
DP_STEP_TOL, DP_STAT_TOL, DP_LOSS_TOL = 5e-3, 3e-5, 1e-5


def test_two_rank_fused_step_against_float64(tmp_path):
    port = str(syn.free_port())
    procs = []
    for r in range(2):
        env = syn.env(RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1', MASTER_PORT=port,
                      **SHARED)
        procs.append(subprocess.Popen([sys.executable, '-c', _STEP_RANK, ROOT, str(tmp_path)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=TIMEOUT)[0].decode())
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    a, b = [dict(np.load(str(tmp_path / ('rank%d.npz' % r)))) for r in range(2)]
    for k in st.PARAM_KEYS + st.STAT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), '%s differs between the ranks' % k
    p = st.init_params(5)
    g = torch.Generator().manual_seed(6)
    img = torch.rand((4, 3, 64, 128), generator=g) * 255
    t = torch.randint(0, 2, (4, 64, 128), generator=g)
    maps = [torch.from_numpy(np.concatenate([a['trace%d' % i], b['trace%d' % i]])) for i in range(4)]
    P64 = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in st.PARAM_KEYS}
    S64 = {k: torch.tensor(p[k], dtype=torch.float64) for k in st.STAT_KEYS}
    l64, _ = st.reference_loss(P64, S64, img.double(), t, st.softmax_cross_entropy, idx_maps=maps)
    grads = dict(zip(P64.keys(), torch.autograd.grad(l64, list(P64.values()))))
    with torch.no_grad():
        Q = {k: v.detach().clone() for k, v in P64.items()}
        st.MomentumSGD(0.01, weight_decay=0.0005).update(Q, grads)
    mean_loss = 0.5 * (float(a['loss']) + float(b['loss']))
    assert abs(mean_loss - l64.item()) < DP_LOSS_TOL * abs(l64.item())
    worst = {}
    for k in st.PARAM_KEYS:
        d_gpu = a[k].astype(np.float64) - p[k].astype(np.float64)
        d_ref = (Q[k] - P64[k].detach()).numpy()
        worst[k] = float(np.abs(d_gpu - d_ref).max() / np.abs(d_ref).max())
    kmax = max(worst, key=worst.get)
    print('fused 2-rank step: worst update error %.3g (%s)' % (worst[kmax], kmax))
    assert worst[kmax] < DP_STEP_TOL, '%s: update error %.3g' % (kmax, worst[kmax])
    for k in st.STAT_KEYS:
        ref = S64[k].numpy()
        e = float(np.abs(a[k].astype(np.float64) - ref).max() / np.abs(ref).max())
        assert e < DP_STAT_TOL, '%s: running statistic error %.3g' % (k, e)


# ------------------------------------------------------------------------------- end to end
# the constants of test_gpu_segnet_train.py's test_train_then_label_end_to_end
E2E_ITERS = 40
E2E_LOSS_FRACTION = 0.35
E2E_MIN_IOU = 0.6


def test_train_fused_then_label_end_to_end(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = ['--fused_bn'] + syn.train_args(z, E2E_ITERS, 20, 10, extra=['--decay_iteration', '30'])
    d1, d2 = str(tmp_path / 'run'), str(tmp_path / 'resumed')
    syn.run_python([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d1], ROOT)
    log = json.load(open(os.path.join(d1, 'log')))
    assert [e['iteration'] for e in log] == [10, 20, 30, 40]
    assert log[-1]['main/loss'] < E2E_LOSS_FRACTION * log[0]['main/loss'], [e['main/loss'] for e in log]
    assert log[-1]['val/main/iou/road'] > E2E_MIN_IOU, log[-1]
    args = json.load(open(os.path.join(d1, 'args.txt')))
    assert args['fused_bn'] is True and args['dtype'] == 'fp32' and 'split_planes' not in args
    # --resume from the middle reaches the same snapshot, bit for bit; the snapshot has no entry for the mode
    syn.run_python([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d2, '--resume',
                                                                      os.path.join(d1, 'snapshot_iter_20')], ROOT)
    keys = syn.same_snapshot(os.path.join(d1, 'snapshot_iter_40'), os.path.join(d2, 'snapshot_iter_40'), bitwise=True)
    assert not [k for k in keys if 'fused' in k]
    # labels_from_segnet.py on the trainer's snapshot predicts what the trainer's validation predicted
    out = str(tmp_path / 'labels')
    syn.run_python([os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', d1, '--iteration', str(E2E_ITERS),
                    '--img_zip_fn', z[2], '--label_zip_fn', z[3], '--out_dir', out, '--start_index', '0',
                    '--end_index', '3', '--eval_shape', '64', '128', '--no_figure'], ROOT)
    res = [json.loads(l) for l in open(os.path.join(out, 'result.json')) if l.strip()]
    FP, FN, TP = (sum(r[k] for r in res) for k in ('FP', 'FN', 'TP'))
    assert (FP, FN) == (log[-1]['val_/main/FP'], log[-1]['val_/main/FN'])
    assert TP / float(TP + FP + FN) == log[-1]['val/main/iou/road']
