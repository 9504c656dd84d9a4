"""GPU tests of data-parallel SegNet training (train_segnet.py --data_parallel, segnet_train.RankGroup) and of
utils/run_train_rounds.py on one MI355X: two ranks share the GPU over gloo (SPA_DIST_BACKEND=gloo,
SPA_BENCH_SAME_DEVICE=1), one rank runs RCCL (SPA_DIST_FORCE=1).  One 2-rank step against the float64 restatement on
the concatenated batch, fp32 and bf16; one RCCL rank against the one-process run, bit for bit; torchrun with 2 ranks:
rank 0's files only, validation in the log, resume bit for bit and the refusal of another world size; the driver for
two rounds on synthetic zips, and its stop at a failing child.  Every child runs under a time limit; a failing child
ends the test."""
import glob
import importlib
import io
import json
import os
import subprocess
import sys
import zipfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

st = importlib.import_module('superpixel-align_amd.segnet_train')

TIMEOUT = 900
SHARED = {'SPA_DIST_BACKEND': 'gloo', 'SPA_BENCH_SAME_DEVICE': '1'}


def _ranks(script, args, n, env_extra, tmp_path):
    """n processes of `script` as ranks 0..n-1 of one gloo group; every one must exit with 0"""
    port = str(syn.free_port())
    procs = []
    for r in range(n):
        env = syn.env(RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1', MASTER_PORT=port,
                      **env_extra)
        procs.append(subprocess.Popen([sys.executable, '-c', script] + args, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
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
    return outs


# ------------------------------------------------------------------------------- one step on 2 ranks vs float64
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
                      dtype=sys.argv[3])
tr.set_group(st.RankGroup())
trace = []
loss = tr.step(img[2 * rank:2 * rank + 2].cuda(), t[2 * rank:2 * rank + 2].cuda(), trace)
out = {k: v.cpu().numpy() for k, v in list(tr.P.items()) + list(tr.S.items())}
out.update({'trace%d' % i: m.cpu().numpy() for i, m in enumerate(trace)})
out['loss'] = np.asarray(loss)
if rank == 0:                                                # the one-process step on all 4 images, same kernels
    one = st.SegNetTrainer(st.init_params(5), st.MomentumSGD(0.01, weight_decay=0.0005), st.softmax_cross_entropy,
                           engine=eng, dtype=sys.argv[3])
    trace = []
    one.step(img.cuda(), t.cuda(), trace)
    out.update({'one/' + k: v.cpu().numpy() for k, v in one.P.items()})
    out.update({'one/trace%d' % i: m.cpu().numpy() for i, m in enumerate(trace)})
np.savez(os.path.join(sys.argv[2], 'rank%d.npz' % rank), **out)
'''

# (update, running statistics) bounds, relative to max |value|: those of test_full_training_step_against_float64 (fp32)
# and test_full_bf16_training_step_against_float64 (bf16).  The bf16 update bound there is set at a batch of 2; on this
# batch of 4 the bf16 step is further from its float64 restatement (measured 0.125 on conv4/W, for the 2-rank step and
# the one-process bf16 step on the same 4 images alike; the restatement itself run in float32 is 0.124 away,
# tools/segnet_bf16_restatement_gap.py), so bf16 is held to that one-process step: no further from float64 than it,
# plus the update bound.
TOLS = {'fp32': (5e-3, 3e-5), 'bf16': (2e-2, 3e-2)}


def _update_errors(P, p, Q, P64):
    out = {}
    for k in st.PARAM_KEYS:
        d_gpu = P[k].astype(np.float64) - p[k].astype(np.float64)
        d_ref = (Q[k] - P64[k].detach()).numpy()
        out[k] = float(np.abs(d_gpu - d_ref).max() / np.abs(d_ref).max())
    return out


def _float64_step(p, img, t, maps, bf16):
    P64 = {k: torch.tensor(p[k], dtype=torch.float64, requires_grad=True) for k in st.PARAM_KEYS}
    S64 = {k: torch.tensor(p[k], dtype=torch.float64) for k in st.STAT_KEYS}
    l64, _ = st.reference_loss(P64, S64, img.double(), t, st.softmax_cross_entropy, idx_maps=maps, bf16_operands=bf16)
    grads = dict(zip(P64.keys(), torch.autograd.grad(l64, list(P64.values()))))
    with torch.no_grad():
        Q = {k: v.detach().clone() for k, v in P64.items()}
        st.MomentumSGD(0.01, weight_decay=0.0005).update(Q, grads)
    return P64, S64, Q, l64


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_two_rank_step_against_float64(tmp_path, dtype):
    _ranks(_STEP_RANK, [ROOT, str(tmp_path), dtype], 2, SHARED, tmp_path)
    a, b = [dict(np.load(str(tmp_path / ('rank%d.npz' % r)))) for r in range(2)]
    for k in st.PARAM_KEYS + st.STAT_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), '%s differs between the ranks' % k
    p = st.init_params(5)
    g = torch.Generator().manual_seed(6)
    img = torch.rand((4, 3, 64, 128), generator=g) * 255
    t = torch.randint(0, 2, (4, 64, 128), generator=g)
    maps = [torch.from_numpy(np.concatenate([a['trace%d' % i], b['trace%d' % i]])) for i in range(4)]
    P64, S64, Q, l64 = _float64_step(p, img, t, maps, dtype == 'bf16')
    step_tol, stat_tol = TOLS[dtype]
    mean_loss = 0.5 * (float(a['loss']) + float(b['loss']))
    assert abs(mean_loss - l64.item()) < (1e-5 if dtype == 'fp32' else 1e-2) * abs(l64.item())
    worst = _update_errors(a, p, Q, P64)
    kmax = max(worst, key=worst.get)
    print('%s 2-rank step: worst update error %.3g (%s)' % (dtype, worst[kmax], kmax))
    if dtype == 'fp32':
        assert worst[kmax] < step_tol, '%s: update error %.3g' % (kmax, worst[kmax])
    else:
        one_maps = [torch.from_numpy(a['one/trace%d' % i]) for i in range(4)]
        _, _, Q1, _ = _float64_step(p, img, t, one_maps, True)
        one = _update_errors({k: a['one/' + k] for k in st.PARAM_KEYS}, p, Q1, P64)
        print('bf16 one-process step on the 4 images: worst update error %.3g (%s)' % (max(one.values()),
                                                                                      max(one, key=one.get)))
        for k in st.PARAM_KEYS:
            assert worst[k] < one[k] + step_tol, '%s: update error %.3g, one process %.3g' % (k, worst[k], one[k])
    for k in st.STAT_KEYS:
        ref = S64[k].numpy()
        e = float(np.abs(a[k].astype(np.float64) - ref).max() / np.abs(ref).max())
        assert e < stat_tol, '%s: running statistic error %.3g' % (k, e)


# ------------------------------------------------------------------------------- train_segnet.py
def _synth(tmp_path, n_train=8, n_val=3):
    return syn.write(str(tmp_path / 'data'), n_train, n_val, 64, 128)


def _common(z, iters, every):
    return syn.train_args(z, iters, every, every, extra=['--random'])


def _run(cmd, env, ok=True):
    return syn.run(cmd, env, ROOT, TIMEOUT, ok)


def _torchrun(n, argv, env):
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
            '--master-addr', '127.0.0.1', '--master-port', str(syn.free_port()),
            os.path.join(ROOT, 'train_segnet.py')] + argv


def test_rccl_one_rank_matches_one_process(tmp_path):
    z = _synth(tmp_path)
    common = _common(z, 4, 2)
    d1, d2 = str(tmp_path / 'single'), str(tmp_path / 'rccl')
    script = os.path.join(ROOT, 'train_segnet.py')
    _run([sys.executable, script] + common + ['--result_dir', d1], syn.env())
    _run([sys.executable, script, '--data_parallel'] + common + ['--result_dir', d2],
         syn.env(SPA_DIST_FORCE='1', RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1',
                 MASTER_PORT=str(syn.free_port())))
    keys = syn.same_snapshot(os.path.join(d1, 'snapshot_iter_4'), os.path.join(d2, 'snapshot_iter_4'), 'common')
    assert len(keys) > 60
    assert st.snapshot_world_size(os.path.join(d2, 'snapshot_iter_4')) == 1
    args = json.load(open(os.path.join(d2, 'args.txt')))
    assert args['data_parallel'] is True and args['world_size'] == 1
    assert 'data_parallel' not in json.load(open(os.path.join(d1, 'args.txt')))
    la, lb = json.load(open(os.path.join(d1, 'log'))), json.load(open(os.path.join(d2, 'log')))
    assert [e['main/loss'] for e in la] == [e['main/loss'] for e in lb]
    assert [e['val/main/iou/road'] for e in la] == [e['val/main/iou/road'] for e in lb]


def test_torchrun_two_ranks_resume_and_refusal(tmp_path):
    z = _synth(tmp_path)
    env = syn.env(**SHARED)
    runs = tmp_path / 'runs'
    da, db, dc = str(runs / 'straight'), str(runs / 'resumed'), str(runs / 'refused')
    _run(_torchrun(2, ['--data_parallel'] + _common(z, 4, 2) + ['--result_dir', da], env), env)
    assert sorted(os.listdir(da)) == ['args.txt', 'log', 'snapshot_iter_2', 'snapshot_iter_4']
    assert os.listdir(str(runs)) == ['straight']                 # the other rank wrote nothing
    args = json.load(open(os.path.join(da, 'args.txt')))
    assert args['data_parallel'] is True and args['world_size'] == 2
    log = json.load(open(os.path.join(da, 'log')))
    assert [e['iteration'] for e in log] == [2, 4]
    for e in log:
        for k in ('main/loss', 'val/main/iou/road', 'val/main/miou', 'val_/main/precision', 'val_/main/FP'):
            assert k in e and np.isfinite(e[k]), (k, e)
    assert st.snapshot_world_size(os.path.join(da, 'snapshot_iter_4')) == 2
    # 2 steps + --resume + 2 steps == 4 steps, bit for bit
    _run(_torchrun(2, ['--data_parallel'] + _common(z, 4, 2) +
                   ['--result_dir', db, '--resume', os.path.join(da, 'snapshot_iter_2')], env), env)
    syn.same_snapshot(os.path.join(da, 'snapshot_iter_4'), os.path.join(db, 'snapshot_iter_4'))
    # another world size is refused
    r = _run(_torchrun(1, ['--data_parallel'] + _common(z, 4, 2) +
                       ['--result_dir', dc, '--resume', os.path.join(da, 'snapshot_iter_2')], env), env, ok=False)
    assert r.returncode != 0
    assert 'written by 2 rank(s), this run has 1' in r.stdout + r.stderr
    assert not os.path.exists(dc)                                  # refused before anything is written


# ------------------------------------------------------------------------------- utils/run_train_rounds.py
def _gt_zip(z, path):
    """gtFine labelIds PNGs (7 road, 21 elsewhere) of the synthetic training images, from their road masks"""
    from PIL import Image
    with zipfile.ZipFile(z[1]) as zl, zipfile.ZipFile(path, 'w') as zo:
        for name in zl.namelist():
            key = os.path.basename(name).split('_leftImg8bit')[0]
            m = np.load(io.BytesIO(zl.read(name)))
            buf = io.BytesIO()
            Image.fromarray(np.where(m, 7, 21).astype(np.uint8)).save(buf, format='PNG')
            zo.writestr('gtFine/train/synth/%s_gtFine_labelIds.png' % key, buf.getvalue())
    return path


def test_run_train_rounds_two_rounds(tmp_path):
    z = _synth(tmp_path, 16, 3)
    gt = _gt_zip(z, str(tmp_path / 'data' / 'train_gt.zip'))
    base = str(tmp_path / 'results')
    cmd = [sys.executable, os.path.join(ROOT, 'utils', 'run_train_rounds.py'), '--n_gpus', '2', '--n_round', '2',
           '--iteration', '10', '--val_iteration', '10', '--n_labels', '16', '--use_soft_label', '--batchsize', '2',
           '--input_shape', '64', '128', '--eval_shape', '64', '128', '--val_eval_shape', '64', '128',
           '--img_zip_fn', z[0], '--label_zip_fn', gt, '--estimated_label_zip_fn', z[1],
           '--val_img_zip', z[2], '--val_label_zip', z[3],
           '--result_base_dir', base, '--no_figure', '--child_timeout', str(TIMEOUT)]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=syn.env(**SHARED), capture_output=True, text=True,
                       timeout=3 * TIMEOUT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    firsts = glob.glob(os.path.join(base, 'train_round1_*'))
    assert len(firsts) == 1
    first = firsts[0]
    seconds = glob.glob(os.path.join(first, 'train_round2_*'))
    assert len(seconds) == 1
    assert os.path.exists(os.path.join(first, 'snapshot_iter_10'))
    assert os.path.exists(os.path.join(seconds[0], 'snapshot_iter_20'))
    a2 = json.load(open(os.path.join(seconds[0], 'args.txt')))
    assert a2['resume'] == os.path.join(first, 'snapshot_iter_10') and a2['use_soft_label']
    assert a2['world_size'] == 2 and a2['train_limit'] == ['20', 'iteration']
    assert a2['train_label_zip'] == os.path.join(first, 'iter-10_eval-train.0.zip')
    for it in (10, 20):
        out_dir = os.path.join(first, 'iter-%d_eval-train' % it)
        zfn = out_dir + '.0.zip'
        with np.load(zfn) as zz:
            assert len(zz.files) == 32
            sc = zz[os.path.join(out_dir, 'synth_000003_000019_leftImg8bit_scores')]
            mk = zz[os.path.join(out_dir, 'synth_000003_000019_leftImg8bit')]
            assert sc.shape == (2, 64, 128) and sc.dtype == np.float32 and mk.dtype == bool
            assert float((mk == (sc[1] > sc[0])).mean()) > 0.99
        for soft in (False, True):
            ds = st.ZippedEstimatedCityscapesDataset(z[0], zfn, (64, 128), use_soft_label=soft)
            assert len(ds) == 16
            ds.get_example(15)
        lines = [json.loads(l) for l in open(os.path.join(out_dir, 'result.json'))]
        assert len(lines) == 16
        assert [l['img_fn'] for l in lines] == sorted(l['img_fn'] for l in lines)
        assert sorted({(l['start_index'], l['end_index']) for l in lines}) == [(0, 8), (8, 16)]   # worker ranges
        assert not os.path.exists(out_dir + '.spool')


def test_run_train_rounds_stops_at_failing_child(tmp_path):
    z = _synth(tmp_path, 4, 1)
    base = str(tmp_path / 'results')
    cmd = [sys.executable, os.path.join(ROOT, 'utils', 'run_train_rounds.py'), '--n_gpus', '2', '--n_round', '2',
           '--iteration', '2', '--val_iteration', '2', '--n_labels', '4', '--batchsize', '2',
           '--input_shape', '64', '128', '--eval_shape', '64', '128', '--val_eval_shape', '64', '128',
           '--img_zip_fn', str(tmp_path / 'missing.zip'),
           '--label_zip_fn', z[1], '--estimated_label_zip_fn', z[1], '--val_img_zip', z[2], '--val_label_zip', z[3],
           '--result_base_dir', base, '--no_figure', '--child_timeout', str(TIMEOUT)]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=syn.env(**SHARED), capture_output=True, text=True, timeout=TIMEOUT)
    assert r.returncode != 0
    assert 'no further process is started' in r.stderr
    first = glob.glob(os.path.join(base, 'train_round1_*'))
    assert len(first) == 1
    assert not glob.glob(os.path.join(first[0], 'iter-*'))            # no labeller started
    assert not glob.glob(os.path.join(first[0], 'train_round2_*'))
