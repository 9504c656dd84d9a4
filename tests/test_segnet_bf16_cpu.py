"""CPU tests of bf16 SegNet-Basic inference: the library exports the bf16 entry points and the engine wraps them,
labels_from_segnet.py's --dtype and save_labels' dtype default to fp32, SegNetBasic refuses an unknown dtype before it
touches a device, and utils/run_train_rounds.py's --label_dtype is independent of --dtype and reaches every labelling
worker's spec."""
import importlib
import inspect
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
lfs = importlib.import_module('labels_from_segnet')
rtr = importlib.import_module('utils.run_train_rounds')

BF16_SYMBOLS = ('spa_segnet_encode_bf16', 'spa_segnet_decode_bf16')


def test_library_exports_bf16_entry_points(spa):
    L = spa._lib.lib()
    for name in BF16_SYMBOLS:
        assert hasattr(L, name), name
        assert name in spa._lib.PROTOTYPES
    # the same C signatures as the float32 stages
    for name in BF16_SYMBOLS:
        assert spa._lib.PROTOTYPES[name] == spa._lib.PROTOTYPES[name[:-len('_bf16')]]
    engine = importlib.import_module('superpixel-align_amd.engine')
    for m in ('segnet_encode_bf16', 'segnet_decode_bf16'):
        assert callable(getattr(engine.Engine, m))
        f32 = inspect.signature(getattr(engine.Engine, m[:-len('_bf16')]))
        assert inspect.signature(getattr(engine.Engine, m)) == f32


def test_one_list_of_dtypes():
    assert segnet.DTYPES == ('fp32', 'bf16')
    assert st.DTYPES is segnet.DTYPES


def test_labels_parser_dtype():
    base = ['--param_dir', 'p', '--iteration', '1']
    assert lfs.get_parser().parse_args(base).dtype == 'fp32'
    assert lfs.get_parser().parse_args(base + ['--dtype', 'bf16']).dtype == 'bf16'
    assert lfs.get_parser().parse_args(base + ['--dtype', 'fp32']).dtype == 'fp32'
    for bad in ('fp16', 'float32', 'BF16'):
        with pytest.raises(SystemExit):
            lfs.get_parser().parse_args(base + ['--dtype', bad])


def test_save_labels_dtype_default():
    sig = inspect.signature(lfs.save_labels)
    assert sig.parameters['dtype'].default == 'fp32'
    assert list(sig.parameters)[-1] == 'dtype'                 # a trailing keyword: positional callers unchanged


def test_save_labels_refuses_unknown_dtype(tmp_path):
    with pytest.raises(ValueError, match='dtype'):
        lfs.save_labels(str(tmp_path), 1, 0, 'img.zip', 'label.zip', str(tmp_path / 'out'), 0, 1, False, [64, 128],
                        dtype='fp16')


def test_segnet_refuses_unknown_dtype_before_device_work(monkeypatch):
    engine = importlib.import_module('superpixel-align_amd.engine')

    def no_engine(*a, **k):
        raise AssertionError('an Engine was created for a refused dtype')

    monkeypatch.setattr(engine, 'Engine', no_engine)
    for bad in ('fp16', 'float32', 'BF16', None):
        with pytest.raises(ValueError, match='dtype'):
            segnet.SegNetBasic({}, dtype=bad)
        with pytest.raises(ValueError, match='dtype'):
            segnet.SegNetBasic.from_snapshot('/nonexistent', 1, dtype=bad)
    assert inspect.signature(segnet.SegNetBasic).parameters['dtype'].default == 'fp32'
    assert inspect.signature(segnet.SegNetBasic.from_snapshot).parameters['dtype'].default == 'fp32'


def test_run_train_rounds_label_dtype_flag():
    assert rtr.get_args([]).label_dtype == 'fp32'
    assert rtr.get_args(['--dtype', 'bf16']).label_dtype == 'fp32'        # --dtype is the training dtype only
    a = rtr.get_args(['--label_dtype', 'bf16'])
    assert a.label_dtype == 'bf16' and a.dtype == 'fp32'
    with pytest.raises(SystemExit):
        rtr.get_args(['--label_dtype', 'fp16'])


@pytest.mark.parametrize('label_dtype', [None, 'fp32', 'bf16'])
def test_run_train_rounds_label_dtype_reaches_every_worker(monkeypatch, tmp_path, label_dtype):
    seen = []

    def fake_run_workers(target, specs, timeout, names=None):
        assert target is rtr.label_worker
        seen.extend(specs)
        for s in specs:                                        # what a worker leaves: an empty spool
            os.makedirs(s['spool'], exist_ok=True)
            open(os.path.join(s['spool'], 'names'), 'w').close()

    monkeypatch.setattr(rtr, 'run_workers', fake_run_workers)
    argv = ['--n_gpus', '3', '--n_labels', '7', '--dtype', 'bf16']
    if label_dtype:
        argv += ['--label_dtype', label_dtype]
    args = rtr.get_args(argv)
    out_dir = str(tmp_path / 'labels')
    rtr.create_label_from_model(args, str(tmp_path / 'run'), 10, out_dir, str(tmp_path / 'labels.zip'))
    assert len(seen) == 3
    assert [s['dtype'] for s in seen] == [label_dtype or 'fp32'] * 3


def test_label_worker_passes_dtype(monkeypatch, tmp_path):
    got = {}

    def fake_save_labels(*a, **k):
        got.update(k)

    monkeypatch.setattr(lfs, 'save_labels', fake_save_labels)
    spec = {'param_dir': 'p', 'iteration': 1, 'device': 0, 'img_zip_fn': 'i', 'label_zip_fn': 'l', 'out_dir': 'o',
            'start': 0, 'end': 1, 'soft_label': False, 'eval_shape': [64, 128], 'save_each': False, 'figure': False,
            'dtype': 'bf16', 'spool': str(tmp_path / 'spool')}
    rtr.label_worker(spec)
    assert got['dtype'] == 'bf16'
