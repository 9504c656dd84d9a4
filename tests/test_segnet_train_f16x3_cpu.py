"""CPU tests of the split-plane SegNet-Basic training mode (train_segnet.py --split_planes): the flag is read in front
of the reference flag set, --split_planes with --dtype bf16 is refused before an Engine exists, a default run's
args.txt and snapshot entries are unchanged, the new C entry points are declared and bound exactly as the float32
ones, and utils/run_train_rounds.py passes the flag to the training children only when given."""
import importlib
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

segnet = importlib.import_module('superpixel-align_amd.segnet')
st = importlib.import_module('superpixel-align_amd.segnet_train')
engine = importlib.import_module('superpixel-align_amd.engine')
train_segnet = importlib.import_module('train_segnet')
rtr = importlib.import_module('utils.run_train_rounds')

PASSES = ('forward', 'dgrad', 'wgrad')


def test_pre_parser_reads_split_planes():
    pre, rest = train_segnet.get_pre_args([])
    assert pre.split_planes is False and rest == []
    pre, rest = train_segnet.get_pre_args(['--batchsize', '2', '--split_planes', '--lr', '0.1'])
    assert pre.split_planes is True and pre.dtype == 'fp32' and rest == ['--batchsize', '2', '--lr', '0.1']
    with pytest.raises(SystemExit):                       # the reference parser does not take it
        train_segnet.get_args(['--split_planes'])
    assert 'split_planes' not in vars(train_segnet.get_args([]))
    # get_dtype_args' return value is unchanged: it leaves the flag to the caller
    assert train_segnet.get_dtype_args(['--split_planes']) == ('fp32', ['--split_planes'])


def test_run_args_record_split_planes_only_when_given():
    reference = vars(train_segnet.get_parser().parse_args([]))
    pre, args = train_segnet.run_args([])
    assert vars(args) == dict(reference, dtype='fp32')                 # a default run's args.txt entries
    pre, args = train_segnet.run_args(['--split_planes'])
    assert vars(args) == dict(reference, dtype='fp32', split_planes=True)
    assert json.loads(json.dumps(vars(args), sort_keys=True))['split_planes'] is True
    pre, args = train_segnet.run_args(['--split_planes', '--data_parallel'])
    assert args.split_planes is True and args.data_parallel is True


class _NoEngine(object):
    def __init__(self, *a, **k):
        raise AssertionError('an Engine was created')


def test_bf16_refusal_before_any_engine(monkeypatch):
    monkeypatch.setattr(engine, 'Engine', _NoEngine)
    with pytest.raises(ValueError, match='split_planes'):
        st.SegNetTrainer(st.init_params(0), st.MomentumSGD(), st.softmax_cross_entropy, dtype='bf16',
                         split_planes=True)
    for argv in (['--split_planes', '--dtype', 'bf16'], ['--dtype', 'bf16', '--split_planes', '--batchsize', '2']):
        with pytest.raises(ValueError) as e:
            train_segnet.main(argv)
        assert '--split_planes' in str(e.value) and '--dtype bf16' in str(e.value)
    with pytest.raises(AssertionError, match='Engine'):              # the patch is what a trainer would reach
        st.SegNetTrainer(st.init_params(0), st.MomentumSGD(), st.softmax_cross_entropy, split_planes=True)


def _keys(path):
    with np.load(path) as z:
        return set(z.files)


def test_snapshot_entries(tmp_path):
    it = st.ShuffledIterator(5, 2)
    paths = {}
    for tag, sp in (('plain', None), ('off', False), ('on', True)):
        d = tmp_path / tag
        d.mkdir()
        json.dump({'model': 'basic', 'input_shape': [32, 64], 'dtype': 'fp32'}, open(str(d / 'args.txt'), 'w'))
        paths[tag] = str(d / 'snapshot_iter_10')
        attrs = dict(dtype='fp32') if sp is None else dict(dtype='fp32', split_planes=sp)
        st.save_snapshot(paths[tag], syn.FakeTrainer(st.init_params(1), 3, 2, **attrs), 10, 0.01, it.state())
    assert _keys(paths['off']) == _keys(paths['plain'])               # a default run keeps today's entries
    assert st.SPLIT_PLANES_KEY not in _keys(paths['plain'])
    assert _keys(paths['on']) == _keys(paths['plain']) | {st.SPLIT_PLANES_KEY}
    assert st.SPLIT_PLANES_KEY == 'extensions/split_planes'
    assert st.snapshot_split_planes(paths['on']) and not st.snapshot_split_planes(paths['off'])
    assert st.snapshot_dtype(paths['on']) == 'fp32'
    # --resume and labels_from_segnet.py's reader take it unchanged
    ref = st.load_snapshot_state(paths['plain'])
    got = st.load_snapshot_state(paths['on'])
    for k in st.PARAM_KEYS:
        assert np.array_equal(got[0][k], ref[0][k]), k
    args, snap, params = segnet.load_snapshot(str(tmp_path / 'on'), 10)
    for k in st.PARAM_KEYS:
        assert np.array_equal(params[k], ref[0][k]), k


def test_abi_rows_equal_float32_rows(spa):
    P = spa._lib.PROTOTYPES
    for p in PASSES:
        assert P['spa_segnet_train_%s_f16x3' % p] == P['spa_segnet_train_%s' % p]
    for p in PASSES:
        assert callable(getattr(engine.Engine, 'segnet_train_%s_f16x3' % p))


def test_declared_in_header_with_float32_arguments():
    header = open(os.path.join(ROOT, 'include', 'spalign.h')).read()
    for p in PASSES:
        assert syn.declaration(header, 'spa_segnet_train_%s_f16x3' % p) == \
            syn.declaration(header, 'spa_segnet_train_%s' % p)


def test_library_exports_f16x3_entry_points(spa):
    L = spa._lib.lib()
    for p in PASSES:
        assert hasattr(L, 'spa_segnet_train_%s_f16x3' % p)


def _first_train_argv(argv):
    a = rtr.get_args(argv)
    steps = [s for s in rtr.plan(a, 'R/train_round1_x_0') if s['kind'] == 'train']
    dirs = {i + 1: 'D%d' % (i + 1) for i in range(len(steps))}
    return [rtr.train_argv(a, s, 'D%d' % (i + 1), dirs) for i, s in enumerate(steps)]


def test_rounds_driver_passes_the_flag_only_when_given():
    base = ['--n_round', '3', '--iteration', '100', '--val_iteration', '50', '--n_use_data', '40', '--random']
    plain = _first_train_argv(base)
    flagged = _first_train_argv(base + ['--split_planes'])
    for a, b in zip(plain, flagged):
        assert '--split_planes' not in a
        assert b == a + ['--split_planes']
    assert rtr.get_args(base).split_planes is False
    with pytest.raises(SystemExit):
        rtr.get_args(base + ['--split_planes', '--dtype', 'bf16'])
    # train_segnet.py takes the child command line with the flag
    pre, rest = train_segnet.get_pre_args(flagged[1])
    assert pre.split_planes and pre.data_parallel and '--split_planes' not in rest
    train_segnet.get_args(rest)
