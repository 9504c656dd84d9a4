"""GPU tests of the SegNet-Basic training kernels (csrc/spa_segnet_train.hip, segnet_train.py): every forward, input
gradient and weight gradient form against float64 torch convolutions and their autograd, the BatchNorm partial sums,
NaN-poisoned outputs with a guard past the end, bit-identical repeats, refusals that write nothing, one whole training
step against the float64 restatement, and train_segnet.py -> labels_from_segnet.py end to end on synthetic zips.
The pass checks are the shared bodies of tests/segnet_ref.py, called with this file's family and bounds."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_ref as sref  # noqa: E402
import segnet_train_synth as syn  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 16, 16), (2, 48, 80), (3, 64, 128), (2, 6, 10)]
# (2, 6, 10): a conv4 / decode4 resolution (1/8 of the input): a partial row tile; conv1 needs multiples of 16

# Bounds, as a fraction of max|ref|.  Measured worst over the first three SHAPES: forward 2.4e-6 (conv1's float32 LRN
# load), dgrad 2.7e-6, wgrad 2.9e-7; decode1's wgrad at (4,512,1024) 1.4e-6.  Forward and dgrad forms keep the
# inference tests' 1e-5; wgrad sums up to K = B*H*W products per output (float32 within a chunk, float64 across the
# chunks), so it gets 1e-5 at the small shapes and 2e-5 at decode1's K = 2.1e6.
FWD_TOL = 1e-5
WGRAD_TOL = 1e-5
WGRAD_BIG_TOL = 2e-5
BN_TOL = 1e-6             # the BatchNorm partial sums against float64 sums of the kernel's own y
# float32 entry points; float32 operands enter the reference as they are; conv1's input is restated in float64
MODE = dict(family='', operand=sref.d64)
CONV1 = dict(device_conv1=False, check_conv1=False)


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_forms_and_bn_sums(eng, shape):
    sref.check_forward(eng, shape, 1, fwd_tol=FWD_TOL, bn_tol=BN_TOL, **MODE, **CONV1)


@pytest.mark.parametrize('shape', SHAPES)
def test_dgrad_forms(eng, shape):
    sref.check_dgrad(eng, shape, 2, fwd_tol=FWD_TOL, **MODE)


@pytest.mark.parametrize('shape', SHAPES)
def test_wgrad_forms(eng, shape):
    sref.check_wgrad(eng, shape, 3, wgrad_tol=WGRAD_TOL, **MODE, **CONV1)


def test_wgrad_decode1_full_size(eng):
    sref.check_wgrad_decode1_full_size(eng, big_tol=WGRAD_BIG_TOL, **MODE)


def test_refusals_write_nothing(eng):
    sref.check_train_refusals(eng, '', unaligned_weights=False)


# ------------------------------------------------------------------------------- one whole training step
# every parameter's update, relative to its max |update|: measured worst 1.4e-3, on the BN gammas (their gradient
# sum(g * xhat) cancels heavily in float32); the convolution weights are far tighter
STEP_TOL = 5e-3
STAT_TOL = 3e-5          # running statistics, relative to max |value|; measured worst 3.9e-6


def test_full_training_step_against_float64(eng):
    r = sref.step_against_float64(eng, {})
    assert abs(r['loss'] - r['l64']) < 1e-5 * abs(r['l64'])
    for k, e in r['updates'].items():
        assert e < STEP_TOL, '%s: update error %.3g' % (k, e)
    for k, e in r['stats'].items():
        assert e < STAT_TOL, '%s: running statistic error %.3g' % (k, e)
    # the kernels' index maps are the first maximum wherever the float64 window is not a near-tie
    for m, a in zip(r['maps'], r['acts']):
        Bq, Hq, Wq, C = a.shape
        win = a.detach().reshape(Bq, Hq // 2, 2, Wq // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(Bq, Hq // 2, Wq // 2,
                                                                                                 C, 4)
        top2 = win.topk(2, -1).values
        clear = (top2[..., 0] - top2[..., 1]) > 1e-4 * float(a.abs().max())
        first = torch.argmax(win, -1)
        assert torch.equal(first[clear], m.long()[clear])
        assert float(clear.double().mean()) > 0.5


# ------------------------------------------------------------------------------- end to end
# Chosen from the float64 restatement of this task run on the CPU (same data, 40 iterations of MomentumSGD): the loss
# fell from 1.09 to 0.078 (first 10-iteration mean 0.6, last 0.07), and the validation road IoU was 0.65 after 10
# iterations and 0.785 after 40.
E2E_ITERS = 40
E2E_LOSS_FRACTION = 0.35
E2E_MIN_IOU = 0.6


def test_train_then_label_end_to_end(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = syn.train_args(z, E2E_ITERS, 20, 10, extra=['--decay_iteration', '30'])
    d1, d2 = str(tmp_path / 'run'), str(tmp_path / 'resumed')
    syn.run_python([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d1], ROOT)
    log = json.load(open(os.path.join(d1, 'log')))
    assert [e['iteration'] for e in log] == [10, 20, 30, 40]
    assert log[-1]['main/loss'] < E2E_LOSS_FRACTION * log[0]['main/loss'], [e['main/loss'] for e in log]
    assert log[-1]['val/main/iou/road'] > E2E_MIN_IOU, log[-1]
    assert log[-1]['lr'] == pytest.approx(0.001) and log[0]['lr'] == 0.01
    args = json.load(open(os.path.join(d1, 'args.txt')))
    assert args['model'] == 'basic' and args['input_shape'] == [64, 128]
    # --resume from the middle reaches the same snapshot, bit for bit
    syn.run_python([os.path.join(ROOT, 'train_segnet.py')] + common + ['--result_dir', d2, '--resume',
                                                             os.path.join(d1, 'snapshot_iter_20')], ROOT)
    with np.load(os.path.join(d1, 'snapshot_iter_40')) as a, np.load(os.path.join(d2, 'snapshot_iter_40')) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k
    # labels_from_segnet.py on the trainer's snapshot predicts what the trainer's validation predicted
    out = str(tmp_path / 'labels')
    syn.run_python([os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir', d1, '--iteration', str(E2E_ITERS),
          '--img_zip_fn', z[2], '--label_zip_fn', z[3], '--out_dir', out, '--start_index', '0', '--end_index', '3',
          '--eval_shape', '64', '128', '--no_figure'], ROOT)
    res = [json.loads(l) for l in open(os.path.join(out, 'result.json')) if l.strip()]
    FP = sum(r['FP'] for r in res)
    FN = sum(r['FN'] for r in res)
    TP = sum(r['TP'] for r in res)
    assert (FP, FN) == (log[-1]['val_/main/FP'], log[-1]['val_/main/FN'])
    assert TP / float(TP + FP + FN) == log[-1]['val/main/iou/road']
