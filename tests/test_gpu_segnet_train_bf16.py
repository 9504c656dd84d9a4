"""GPU tests of SegNet-Basic training on the bf16 matrix cores (csrc/spa_segnet_train_bf16.hip, SegNetTrainer(...,
dtype='bf16'), train_segnet.py --dtype bf16): the eight pass forms against float64 torch convolutions and their
autograd on the same bf16-rounded operands, the BatchNorm partial sums, NaN-poisoned outputs with a guard past the end,
bit-identical repeats, refusals that write nothing, one whole bf16 step against the float64 restatement with operand
rounding, and train_segnet.py --dtype bf16 -> --resume -> labels_from_segnet.py end to end on synthetic zips.
The pass checks are the shared bodies of tests/segnet_ref.py, called with this file's family, operand rounding and
bounds."""
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
st = importlib.import_module('superpixel-align_amd.segnet_train')

SHAPES = [(1, 16, 16), (2, 48, 80), (3, 64, 128), (2, 6, 10)]
# (2, 6, 10): a conv4 / decode4 resolution (1/8 of the input): a partial row tile; conv1 needs multiples of 16

# Bounds, as a fraction of max|ref|, the float32 forms' bounds.  The reference multiplies the kernels' own bf16
# operands in float64, so the products agree exactly and only the float32 accumulation order differs.  Measured worst
# over SHAPES: forward 8.8e-7, dgrad 9.6e-7, wgrad 1.1e-7; decode1's wgrad at (4,512,1024) 7.3e-7.
FWD_TOL = 1e-5
WGRAD_TOL = 1e-5
WGRAD_BIG_TOL = 2e-5
BN_TOL = 1e-6             # the BatchNorm partial sums against float64 sums of the kernel's own y
# bf16 entry points; every operand enters the reference rounded to bf16; conv1's input is the float32 kernels' own
# operand (checked against the float64 restatement), rounded
MODE = dict(family='_bf16', operand=sref.r16)
CONV1 = dict(device_conv1=True, check_conv1=True)


@pytest.fixture(scope='module')
def eng():
    engine = importlib.import_module('superpixel-align_amd.engine')
    e = engine.Engine()
    yield e
    e.close()


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_forms_and_bn_sums(eng, shape):
    worst = sref.check_forward(eng, shape, 1, fwd_tol=FWD_TOL, bn_tol=BN_TOL, **MODE, **CONV1)
    print('bf16 forward %s: worst %.3g' % (shape, worst))


@pytest.mark.parametrize('shape', SHAPES)
def test_dgrad_forms(eng, shape):
    print('bf16 dgrad %s: worst %.3g' % (shape, sref.check_dgrad(eng, shape, 2, fwd_tol=FWD_TOL, **MODE)))


@pytest.mark.parametrize('shape', SHAPES)
def test_wgrad_forms(eng, shape):
    worst = sref.check_wgrad(eng, shape, 3, wgrad_tol=WGRAD_TOL, **MODE, **CONV1)
    print('bf16 wgrad %s: worst %.3g' % (shape, worst))


def test_wgrad_decode1_full_size(eng):
    sref.check_wgrad_decode1_full_size(eng, big_tol=WGRAD_BIG_TOL, label='bf16', **MODE)


def test_refusals_write_nothing(eng):
    sref.check_train_refusals(eng, '_bf16', unaligned_weights=True)


# ------------------------------------------------------------------------------- one whole training step
# Every parameter's update against the float64 restatement with the same operand rounding (reference_loss(...,
# bf16_operands=True)), relative to its max |update|.  The kernels round float32 values, the restatement float64 ones:
# wherever the two differ across a bf16 rounding boundary an operand lands one bf16 ulp (2^-8 relative) apart, and the
# output gradients behind BatchNorm (whose weight gradients cancel heavily) differ in float32 vs float64 by far more
# than one float32 ulp.  Measured worst 9.0e-3 (conv2/W).  That gap is the rounding's, not the kernels': the same step
# restated in float32 torch ops on the CPU, with the same rounding, differs from the float64 one by 7.3e-3 (conv2/W),
# and by 5.0e-3 even with the output gradients left unrounded.
STEP_TOL = 2e-2
# Running statistics, relative to max |value|: measured worst 1.4e-2 (conv_decode1_bn/avg_mean, a batch mean that
# cancels); the float32 CPU restatement with the same rounding is 9.7e-3 from the float64 one there.
STAT_TOL = 3e-2
LOSS_VS_FP32 = 1e-2      # the bf16 step's loss against the float32 step's, relative


def test_full_bf16_training_step_against_float64(eng):
    r = sref.step_against_float64(eng, dict(dtype='bf16'), bf16_operands=True)
    loss, l64, worst, es = r['loss'], r['l64'], r['updates'], r['stats']
    kmax = max(worst, key=worst.get)
    print('bf16 step: loss %.6g (float64 %.6g), worst update error %.3g (%s)' % (loss, l64, worst[kmax], kmax))
    assert worst[kmax] < STEP_TOL, '%s: update error %.3g' % (kmax, worst[kmax])
    kmax = max(es, key=es.get)
    print('bf16 step: worst running statistic error %.3g (%s)' % (es[kmax], kmax))
    assert es[kmax] < STAT_TOL, '%s: running statistic error %.3g' % (kmax, es[kmax])
    # against the float32 step on the same parameters and batch
    tr32 = st.SegNetTrainer(r['p'], st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy, engine=eng)
    loss32 = tr32.step(r['img'].cuda(), r['t'].cuda())
    print('bf16 step: loss %.6g, float32 step %.6g' % (loss, loss32))
    assert abs(loss - loss32) < LOSS_VS_FP32 * abs(loss32)
    assert abs(loss - l64) < LOSS_VS_FP32 * abs(l64)


def test_bf16_step_repeats_bit_for_bit(eng):
    sref.check_step_repeats(eng, dtype='bf16')


# ------------------------------------------------------------------------------- end to end
# The float32 end-to-end test's settings and bounds (tests/test_gpu_segnet_train.py).
E2E_ITERS = 40
E2E_LOSS_FRACTION = 0.35
E2E_MIN_IOU = 0.6


def test_train_bf16_then_label_end_to_end(tmp_path):
    z = syn.write(str(tmp_path / 'data'), 8, 3, 64, 128)
    common = syn.train_args(z, E2E_ITERS, 20, 10, extra=['--decay_iteration', '30'])
    d1, d2, d3 = str(tmp_path / 'run'), str(tmp_path / 'resumed'), str(tmp_path / 'resumed_fp32')
    script = os.path.join(ROOT, 'train_segnet.py')
    syn.run_python([script, '--dtype', 'bf16'] + common + ['--result_dir', d1], ROOT)
    log = json.load(open(os.path.join(d1, 'log')))
    print('bf16 end to end: loss %s, road IoU %.4f' % ([round(e['main/loss'], 4) for e in log],
                                                      log[-1]['val/main/iou/road']))
    assert [e['iteration'] for e in log] == [10, 20, 30, 40]
    assert log[-1]['main/loss'] < E2E_LOSS_FRACTION * log[0]['main/loss'], [e['main/loss'] for e in log]
    assert log[-1]['val/main/iou/road'] > E2E_MIN_IOU, log[-1]
    assert log[-1]['lr'] == pytest.approx(0.001) and log[0]['lr'] == 0.01
    args = json.load(open(os.path.join(d1, 'args.txt')))
    assert args['dtype'] == 'bf16' and args['model'] == 'basic' and args['input_shape'] == [64, 128]
    snap20 = os.path.join(d1, 'snapshot_iter_20')
    assert st.snapshot_dtype(snap20) == 'bf16'
    # --resume from the middle in the same dtype reaches the same snapshot, bit for bit
    syn.run_python([script, '--dtype', 'bf16'] + common + ['--result_dir', d2, '--resume', snap20], ROOT)
    with np.load(os.path.join(d1, 'snapshot_iter_40')) as a, np.load(os.path.join(d2, 'snapshot_iter_40')) as b:
        assert set(a.files) == set(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k
    # a bf16 snapshot resumes in float32 too (float32 master weights and optimizer state)
    r = syn.run_python([script] + common + ['--result_dir', d3, '--resume', snap20], ROOT)
    assert 'resuming a bf16 snapshot in fp32' in r.stdout
    assert st.snapshot_dtype(os.path.join(d3, 'snapshot_iter_40')) == 'fp32'
    log3 = json.load(open(os.path.join(d3, 'log')))
    assert log3[-1]['val/main/iou/road'] > E2E_MIN_IOU, log3[-1]
    # labels_from_segnet.py on the bf16 trainer's snapshot predicts what the trainer's validation predicted
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
