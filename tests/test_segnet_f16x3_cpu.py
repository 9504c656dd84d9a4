"""CPU tests of split-plane (float32-accurate, f16 matrix cores) SegNet-Basic inference: the library exports the two
entry points with the float32 stages' C signatures and the engine wraps them; SegNetBasic, labels_from_segnet.py,
utils/run_train_rounds.py and train_segnet.py carry the mode as a flag that is off by default, refused together with
bf16 before any device work, and leaves every default output unchanged."""
import importlib
import inspect
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
engine = importlib.import_module('superpixel-align_amd.engine')
lfs = importlib.import_module('labels_from_segnet')
rtr = importlib.import_module('utils.run_train_rounds')
train_segnet = importlib.import_module('train_segnet')

STAGES = ('encode', 'decode')


# ------------------------------------------------------------------------------- library, header, engine
def test_abi_rows_equal_float32_rows(spa):
    P = spa._lib.PROTOTYPES
    for s in STAGES:
        assert P['spa_segnet_%s_f16x3' % s] == P['spa_segnet_%s' % s]


def test_declared_in_header_with_float32_arguments():
    header = open(os.path.join(ROOT, 'include', 'spalign.h')).read()
    for s in STAGES:
        assert syn.declaration(header, 'spa_segnet_%s_f16x3' % s) == syn.declaration(header, 'spa_segnet_%s' % s)


def test_library_exports_f16x3_entry_points(spa):
    L = spa._lib.lib()
    for s in STAGES:
        assert hasattr(L, 'spa_segnet_%s_f16x3' % s)


def test_engine_methods_have_float32_signatures():
    for s in STAGES:
        m = getattr(engine.Engine, 'segnet_%s_f16x3' % s)
        assert callable(m)
        assert inspect.signature(m) == inspect.signature(getattr(engine.Engine, 'segnet_%s' % s))


# ------------------------------------------------------------------------------- segnet.SegNetBasic
def test_dtypes_tuple_unchanged():
    assert segnet.DTYPES == ('fp32', 'bf16')                   # the mode is a flag, not a third dtype


def _no_engine(*a, **k):
    raise AssertionError('an Engine was created for a refused combination')


def test_segnet_split_planes_default_and_refusal(monkeypatch):
    for f in (segnet.SegNetBasic, segnet.SegNetBasic.from_snapshot):
        sig = inspect.signature(f)
        assert sig.parameters['split_planes'].default is False
        assert sig.parameters['dtype'].default == 'fp32'
    assert list(inspect.signature(segnet.SegNetBasic).parameters) == [
        'params', 'pred_shape', 'device', 'engine', 'dtype', 'split_planes']
    monkeypatch.setattr(engine, 'Engine', _no_engine)
    with pytest.raises(ValueError) as e:
        segnet.SegNetBasic({}, dtype='bf16', split_planes=True)
    assert 'split_planes' in str(e.value) and 'bf16' in str(e.value)
    with pytest.raises(ValueError) as e:
        segnet.SegNetBasic.from_snapshot('/nonexistent', 1, dtype='bf16', split_planes=True)
    assert 'split_planes' in str(e.value) and 'bf16' in str(e.value)


def test_trainer_predictor_signature():
    sig = inspect.signature(st.SegNetTrainer.predictor)
    assert list(sig.parameters) == ['self', 'pred_shape', 'split_planes']
    assert sig.parameters['split_planes'].default is False and sig.parameters['pred_shape'].default is None


# ------------------------------------------------------------------------------- labels_from_segnet.py
def test_labels_parser_flag():
    base = ['--param_dir', 'p', '--iteration', '1']
    assert lfs.get_parser().parse_args(base).split_planes is False
    a = lfs.get_parser().parse_args(base + ['--split_planes'])
    assert a.split_planes is True and a.dtype == 'fp32'


def test_save_labels_signature():
    sig = inspect.signature(lfs.save_labels)
    assert list(sig.parameters)[-1] == 'dtype'                 # still the trailing keyword
    assert list(sig.parameters)[-2] == 'split_planes'
    assert sig.parameters['split_planes'].default is False


def test_save_labels_refuses_split_planes_with_bf16(tmp_path):
    param_dir = tmp_path / 'never_read'                        # no args.txt: reading it would raise another error
    with pytest.raises(ValueError) as e:
        lfs.save_labels(str(param_dir), 1, 0, 'img.zip', 'label.zip', str(tmp_path / 'out'), 0, 1, False, [64, 128],
                        split_planes=True, dtype='bf16')
    assert 'split_planes' in str(e.value) and 'bf16' in str(e.value)
    assert not (tmp_path / 'out').exists()


def test_labels_cli_refuses_split_planes_with_bf16(tmp_path):
    out = tmp_path / 'out'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'labels_from_segnet.py'), '--param_dir',
                        str(tmp_path / 'never_read'), '--iteration', '1', '--img_zip_fn', 'i.zip', '--label_zip_fn',
                        'l.zip', '--out_dir', str(out), '--start_index', '0', '--end_index', '1', '--split_planes',
                        '--dtype', 'bf16'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT, timeout=300)
    assert r.returncode != 0
    assert b'split_planes' in r.stderr
    assert not out.exists()


# ------------------------------------------------------------------------------- utils/run_train_rounds.py
def test_run_train_rounds_label_split_planes_flag():
    assert rtr.get_args([]).label_split_planes is False
    assert rtr.get_args(['--split_planes']).label_split_planes is False     # the training rounds' flag only
    assert rtr.get_args(['--dtype', 'bf16']).label_split_planes is False
    a = rtr.get_args(['--label_split_planes'])
    assert a.label_split_planes is True and a.split_planes is False and a.label_dtype == 'fp32'
    a = rtr.get_args(['--label_split_planes', '--dtype', 'bf16'])           # bf16 training, float32-accurate labels
    assert a.label_split_planes is True and a.dtype == 'bf16'
    with pytest.raises(SystemExit):
        rtr.get_args(['--label_split_planes', '--label_dtype', 'bf16'])


@pytest.mark.parametrize('flag', [False, True])
def test_run_train_rounds_label_split_planes_reaches_every_worker(monkeypatch, tmp_path, flag):
    seen = []

    def fake_run_workers(target, specs, timeout, names=None):
        assert target is rtr.label_worker
        seen.extend(specs)
        for s in specs:                                        # what a worker leaves: an empty spool
            os.makedirs(s['spool'], exist_ok=True)
            open(os.path.join(s['spool'], 'names'), 'w').close()

    monkeypatch.setattr(rtr, 'run_workers', fake_run_workers)
    args = rtr.get_args(['--n_gpus', '3', '--n_labels', '7', '--split_planes']
                        + (['--label_split_planes'] if flag else []))
    rtr.create_label_from_model(args, str(tmp_path / 'run'), 10, str(tmp_path / 'labels'), str(tmp_path / 'labels.zip'))
    assert len(seen) == 3
    assert [s['split_planes'] for s in seen] == [flag] * 3
    assert [s['dtype'] for s in seen] == ['fp32'] * 3


def test_label_worker_passes_split_planes(monkeypatch, tmp_path):
    got = []

    def fake_save_labels(*a, **k):
        got.append(k)

    monkeypatch.setattr(lfs, 'save_labels', fake_save_labels)
    spec = {'param_dir': 'p', 'iteration': 1, 'device': 0, 'img_zip_fn': 'i', 'label_zip_fn': 'l', 'out_dir': 'o',
            'start': 0, 'end': 1, 'soft_label': False, 'eval_shape': [64, 128], 'save_each': False, 'figure': False,
            'dtype': 'fp32', 'spool': str(tmp_path / 'spool')}
    rtr.label_worker(dict(spec, split_planes=True))
    rtr.label_worker(spec)                                     # a spec without the key: off
    assert got[0]['split_planes'] is True and got[0]['dtype'] == 'fp32'
    assert got[1]['split_planes'] is False


def _train_argvs(argv):
    a = rtr.get_args(argv)
    steps = [s for s in rtr.plan(a, 'R/train_round1_x_0') if s['kind'] == 'train']
    dirs = {i + 1: 'D%d' % (i + 1) for i in range(len(steps))}
    return [rtr.train_argv(a, s, 'D%d' % (i + 1), dirs) for i, s in enumerate(steps)]


def test_training_children_unchanged_by_label_split_planes():
    base = ['--n_round', '3', '--iteration', '100', '--val_iteration', '50', '--n_use_data', '40', '--random']
    assert _train_argvs(base + ['--label_split_planes']) == _train_argvs(base)
    assert _train_argvs(base + ['--split_planes', '--label_split_planes']) == _train_argvs(base + ['--split_planes'])
    for argv in _train_argvs(base + ['--label_split_planes']):
        assert '--val_split_planes' not in argv and '--split_planes' not in argv


# ------------------------------------------------------------------------------- train_segnet.py
def test_pre_parser_reads_val_split_planes():
    pre, rest = train_segnet.get_pre_args([])
    assert pre.val_split_planes is False and rest == []
    pre, rest = train_segnet.get_pre_args(['--split_planes'])
    assert pre.val_split_planes is False                       # a split-plane run's validation stays float32
    pre, rest = train_segnet.get_pre_args(['--batchsize', '2', '--val_split_planes', '--lr', '0.1'])
    assert pre.val_split_planes is True and pre.split_planes is False
    assert rest == ['--batchsize', '2', '--lr', '0.1']
    with pytest.raises(SystemExit):                            # the reference parser does not take it
        train_segnet.get_args(['--val_split_planes'])


def test_run_args_record_val_split_planes_only_when_given():
    reference = vars(train_segnet.get_parser().parse_args([]))
    pre, args = train_segnet.run_args([])
    assert vars(args) == dict(reference, dtype='fp32')
    pre, args = train_segnet.run_args(['--split_planes'])
    assert vars(args) == dict(reference, dtype='fp32', split_planes=True)
    pre, args = train_segnet.run_args(['--val_split_planes'])
    assert vars(args) == dict(reference, dtype='fp32', val_split_planes=True)
    assert json.loads(json.dumps(vars(args), sort_keys=True))['val_split_planes'] is True
    pre, args = train_segnet.run_args(['--val_split_planes', '--dtype', 'bf16'])     # bf16 steps, validation is its own
    assert vars(args) == dict(reference, dtype='bf16', val_split_planes=True)


def test_evaluate_asks_the_predictor_for_the_mode():
    """evaluate() builds its predictor without the keyword unless the mode is asked for (trainer doubles of earlier
    tests take pred_shape only)."""
    calls = []

    class Stop(Exception):
        pass

    class Trainer(object):
        eng = None

        def predictor(self, *a, **k):
            calls.append((a, k))
            raise Stop()

    class Valid(object):
        resize_shape = (32, 64)

        def __len__(self):
            return 0

    for kw in ({}, {'split_planes': False}, {'split_planes': True}):
        with pytest.raises(Stop):
            train_segnet.evaluate(Trainer(), Valid(), [64, 128], 2, **kw)
    assert calls == [(([64, 128],), {}), (([64, 128],), {}), (([64, 128],), {'split_planes': True})]
