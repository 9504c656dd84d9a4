#!/usr/bin/env python
"""Train SegNet-Basic on generated labels, relabel the training split with it, and repeat (same CLI, defaults, round
arithmetic, result directories and label zips as the reference script of this name), on libspalign's kernels.

  round 1    train_segnet.py on --estimated_label_zip_fn      -> {result_base_dir}/train_round1_<time>_<i>
             labels from its snapshot_iter_{iteration}         -> {first}/iter-{iteration}_eval-{split}.0.zip
  round k>1  train_segnet.py --resume {previous}/snapshot_iter_{resume_iteration} on the previous round's labels,
             up to iteration * k (with --use_soft_label or --use_mse) -> {first}/train_round{k}_<time>_<i>
             labels from its snapshot_iter_{iteration * k}    -> {first}/iter-{iteration * k}_eval-{split}.0.zip
(Trash/train_round1 under --test_mode, train_extra_round{k} when the image zip is the train_extra split.)

Training: each round is one child process, `python -m torch.distributed.run --nnodes=1 --nproc-per-node n_gpus
--master-addr 127.0.0.1 --master-port <free port> train_segnet.py --data_parallel ...` (the reference's mpiexec and
ChainerMN).  Labelling: n_gpus spawned child processes, worker i on device i (device 0 under SPA_BENCH_SAME_DEVICE=1)
over the reference's range [i*step, min(n, (i+1)*step)), step = ceil(n_labels / n_gpus), through
labels_from_segnet.save_labels.  Each worker spools its arrays as .npy files and its result.json lines in a file of its
own; the driver then appends the lines to {out_dir}/result.json in index order and streams the arrays into the label
zip (stored, Zip64, one member at a time), with the member names and contents np.savez gives the reference's dict:
<out_dir>/<base>.npy (bool mask) and <out_dir>/<base>_scores.npy (float32 (2, H, W)).  The driver itself never
initialises the GPU and never holds more than one image's arrays.

Failure: the driver stops at the first child that fails (non-zero exit, signal or --child_timeout), stops its
siblings, starts no further process and exits non-zero (the reference ignores the status).  No child outlives the
driver: SIGTERM, SIGINT and SIGHUP to the driver stop the running children (torchrun and its ranks, or the labellers)
before it exits, and every child is started with the parent-death signal SIGTERM, so a driver that is killed outright
takes its children with it (torchrun answers SIGTERM by stopping its ranks).

Additions, defaulting to what the reference hard-codes: --input_shape, --val_img_zip, --val_label_zip,
--val_eval_shape (the training rounds' validation shape: train_segnet.py's --eval_shape, whose default the reference
leaves in place; the driver's own --eval_shape is the labelling shape only), --dtype (the training rounds' dtype
only), --label_dtype (the labelling passes' convolution precision, labels_from_segnet.py --dtype; fp32 unless given,
whatever --dtype is), --split_planes (the training rounds' train_segnet.py --split_planes: float32 steps with their
convolution passes on split f16 planes; passed to the training children only when given), --label_split_planes (the
labelling passes' labels_from_segnet.py --split_planes: float32-accurate inference on the f16 matrix cores;
independent of --split_planes and --dtype, refused with --label_dtype bf16), --fused_bn (the training rounds'
train_segnet.py --fused_bn: BatchNorm, ReLU, pooling and the classifier on fused kernels; passed to the training children
only when given, with any --dtype and with --split_planes), --loader_procs (the training rounds'
train_segnet.py --loader_procs: decode workers per rank and the input stage on the GPU, passed only when given; the
job needs n_gpus x loader_procs CPUs for them; they also feed those rounds' validation), --device_cache_gb (the
training rounds' train_segnet.py --device_cache_gb, passed only when given), --label_loader_procs (the
labelling passes' labels_from_segnet.py --loader_procs: decode workers per labelling process, independent of
--loader_procs; the job needs n_gpus x label_loader_procs CPUs for them), --n_labels (overrides the
split's constant), --no_figure (the labellers' 3-panel figures), --figure_renderer (labels_from_segnet.py's: matplotlib,
the default, or device: the labelling processes compose and JPEG-encode the figures on the GPU), --child_timeout.
plan() computes the rounds, their commands, resume paths, result-directory prefixes and zip names without launching
anything.
"""
import argparse
import glob
import json
import math
import multiprocessing
import os
import shutil
import signal
import socket
import subprocess
import sys
import time
import zipfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from train_segnet import create_result_dir  # noqa: E402  (numpy only: the driver never touches the GPU)

TRAIN_SCRIPT = os.path.join(ROOT, 'train_segnet.py')
STOP_GRACE = 60             # seconds a child gets to stop after SIGTERM (torchrun stops its ranks) before SIGKILL


def get_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--n_round', type=int, default=1)
    parser.add_argument('--iteration', type=int, default=2000)
    parser.add_argument('--val_iteration', type=int, default=100)
    parser.add_argument('--n_use_data', type=int, default=None)
    parser.add_argument('--use_soft_label', action='store_true', default=False)
    parser.add_argument('--use_mse', action='store_true', default=False)
    parser.add_argument('--random', action='store_true', default=False)
    parser.add_argument('--test_mode', action='store_true', default=False)
    parser.add_argument('--save_each', action='store_true', default=False)
    parser.add_argument('--n_gpus', type=int, default=8)
    parser.add_argument('--batchsize', type=int, default=8)
    parser.add_argument('--result_base_dir', type=str, default='results')
    parser.add_argument('--resume_round', type=int, default=2, help='The default is 2')
    parser.add_argument('--first_result_dir', type=str, default=None, help='For resuming')
    parser.add_argument('--out_zip_fn', type=str, default=None, help='For resuming')
    parser.add_argument('--eval_shape', type=int, nargs=2, default=[1024, 2048])
    parser.add_argument('--img_zip_fn', type=str, default='data/cityscapes_train_imgs.0.zip')
    parser.add_argument('--label_zip_fn', type=str, default='data/cityscapes_train_labels.0.zip')
    parser.add_argument('--estimated_label_zip_fn', type=str, default='results/estimated_train_labels.0.zip')
    # additions
    parser.add_argument('--input_shape', type=int, nargs=2, default=[512, 1024])
    parser.add_argument('--val_img_zip', type=str, default='data/cityscapes_val_imgs.0.zip')
    parser.add_argument('--val_label_zip', type=str, default='data/cityscapes_val_labels.0.zip')
    parser.add_argument('--val_eval_shape', type=int, nargs=2, default=[1024, 2048],
                        help="train_segnet.py's --eval_shape: the shape of the training rounds' validation")
    parser.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    parser.add_argument('--label_dtype', type=str, default='fp32', choices=['fp32', 'bf16'],
                        help="labels_from_segnet.py's --dtype for the labelling passes (independent of --dtype)")
    parser.add_argument('--split_planes', action='store_true', default=False,
                        help="train_segnet.py --split_planes for the training rounds (float32 only)")
    parser.add_argument('--label_split_planes', action='store_true', default=False,
                        help="labels_from_segnet.py --split_planes for the labelling passes (--label_dtype fp32 only)")
    parser.add_argument('--fused_bn', action='store_true', default=False,
                        help="train_segnet.py --fused_bn for the training rounds")
    parser.add_argument('--loader_procs', type=int, default=0,
                        help="train_segnet.py --loader_procs for the training rounds: decode workers PER RANK "
                             "(keep n_gpus x loader_procs within the CPUs the job has); 0: none")
    parser.add_argument('--device_cache_gb', type=float, default=0.0,
                        help="train_segnet.py --device_cache_gb for the training rounds (needs --loader_procs): GB of "
                             "decoded examples every rank keeps in device memory; the labelling passes do not take it")
    parser.add_argument('--label_loader_procs', type=int, default=0,
                        help="labels_from_segnet.py --loader_procs for the labelling passes: decode workers PER "
                             "LABELLING PROCESS; the job needs n_gpus x label_loader_procs CPUs for the decode workers; "
                             "0: none")
    parser.add_argument('--n_labels', type=int, default=None, help='images to relabel (default: the split size)')
    parser.add_argument('--no_figure', action='store_true', default=False)
    parser.add_argument('--figure_renderer', type=str, default='matplotlib', choices=['matplotlib', 'device'],
                        help="the labelling processes' save_labels(figure_renderer=...)")
    parser.add_argument('--child_timeout', type=float, default=0,
                        help='seconds one child (a training round or a labelling pass) may take; 0: no limit')
    return parser


def get_args(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    if args.split_planes and args.dtype != 'fp32':
        parser.error('--split_planes (float32 steps on split planes) does not combine with --dtype %s' % args.dtype)
    if args.label_split_planes and args.label_dtype != 'fp32':
        parser.error('--label_split_planes (float32-accurate labelling on split planes) does not combine with '
                     '--label_dtype %s' % args.label_dtype)
    n_labels = args.n_labels
    if args.test_mode:
        args.iteration = 10
        args.val_iteration = 10
        args.n_labels = 16
        args.n_use_data = 16
        args.n_round = 3
    elif 'train_extra' in args.img_zip_fn:
        args.n_labels = 22973
    else:
        args.n_labels = 2975
    if n_labels is not None:
        args.n_labels = n_labels
    return args


def split_of(img_zip_fn):
    return 'train_extra' if 'train_extra' in img_zip_fn else 'train'


def first_round_prefix(args):
    if args.test_mode:
        return '{}/Trash/train_round1'.format(args.result_base_dir)
    if 'train_extra' in args.img_zip_fn:
        return '{}/train_extra_round1'.format(args.result_base_dir)
    return '{}/train_round1'.format(args.result_base_dir)


def next_round_prefix(first_result_dir, n_round, img_zip_fn):
    if 'train_extra' in img_zip_fn:
        return '{}/train_extra_round{}'.format(first_result_dir, n_round)
    return '{}/train_round{}'.format(first_result_dir, n_round)


def label_out_dir(first_result_dir, iteration, split):
    return '{}/iter-{}_eval-{}'.format(first_result_dir, iteration, split)


def label_ranges(n_labels, n_gpus):
    """the reference's labelling ranges: [i, min(n, i + step)) for i = 0, step, ..., step = ceil(n_labels / n_gpus)"""
    step = int(math.ceil(n_labels / float(n_gpus)))
    return [(i, n_labels if i + step >= n_labels else i + step) for i in range(0, n_labels, step)]


def plan(args, first_result_dir):
    """The steps this invocation runs, in order, without launching anything:
      {'kind': 'train', 'round': k, 'prefix' (None for round 1: its directory is first_result_dir),
       'train_limit', 'train_label_zip', 'resume': None or (round whose directory to resume from, iteration)}
      {'kind': 'label', 'round': k (whose directory holds the snapshot), 'iteration', 'out_dir', 'out_zip'}"""
    split = split_of(args.img_zip_fn)
    steps = []
    if args.first_result_dir is None:
        steps.append({'kind': 'train', 'round': 1, 'prefix': None, 'train_limit': args.iteration,
                      'train_label_zip': args.estimated_label_zip_fn, 'resume': None})
    if args.out_zip_fn is None:
        out_dir = label_out_dir(first_result_dir, args.iteration, split)
        steps.append({'kind': 'label', 'round': 1, 'iteration': args.iteration, 'out_dir': out_dir,
                      'out_zip': out_dir + '.0.zip'})
        out_zip = out_dir + '.0.zip'
    else:
        out_zip = args.out_zip_fn
    prev = 1
    end_iteration = args.iteration
    for n_round in range(args.resume_round, args.n_round + 1):
        resume_iteration = end_iteration
        end_iteration = args.iteration * n_round
        steps.append({'kind': 'train', 'round': n_round,
                      'prefix': next_round_prefix(first_result_dir, n_round, args.img_zip_fn),
                      'train_limit': end_iteration, 'train_label_zip': out_zip, 'resume': (prev, resume_iteration)})
        out_dir = label_out_dir(first_result_dir, end_iteration, split)
        out_zip = out_dir + '.0.zip'
        steps.append({'kind': 'label', 'round': n_round, 'iteration': end_iteration, 'out_dir': out_dir,
                      'out_zip': out_zip})
        prev = n_round
    return steps


def train_argv(args, step, result_dir, dirs):
    """train_segnet.py's arguments for a 'train' step; dirs: {round: result directory} of the rounds before it"""
    a = ['--data_parallel', '--dtype', args.dtype, '--model', 'basic', '--optimizer', 'Adam',
         '--train_limit', str(step['train_limit']), 'iteration',
         '--val_interval', str(args.val_iteration), 'iteration',
         '--log_interval', str(args.val_iteration), 'iteration',
         '--batchsize', str(args.batchsize),
         '--input_shape', str(args.input_shape[0]), str(args.input_shape[1]),
         '--eval_shape', str(args.val_eval_shape[0]), str(args.val_eval_shape[1]),
         '--train_img_zip', args.img_zip_fn, '--train_label_zip', step['train_label_zip'],
         '--val_img_zip', args.val_img_zip, '--val_label_zip', args.val_label_zip,
         '--result_dir', result_dir]
    if step['resume'] is not None:
        prev, it = step['resume']
        a += ['--resume', '{}/snapshot_iter_{}'.format(dirs[prev], it)]
        if args.use_soft_label:
            a.append('--use_soft_label')
        elif args.use_mse:
            a.append('--use_mse')
    if args.n_use_data is not None:
        a += ['--n_use_data', str(args.n_use_data)]
    if args.random:
        a.append('--random')
    if args.split_planes:
        a.append('--split_planes')
    if args.fused_bn:
        a.append('--fused_bn')
    if args.loader_procs:
        a += ['--loader_procs', str(args.loader_procs)]
    if args.device_cache_gb:
        a += ['--device_cache_gb', repr(float(args.device_cache_gb))]
    return a


def free_port():
    """a TCP port nobody listens on now (bound to port 0), so concurrent jobs on one machine do not collide"""
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def torchrun_command(n_gpus, argv, port):
    return [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n_gpus),
            '--master-addr', '127.0.0.1', '--master-port', str(port), TRAIN_SCRIPT] + list(argv)


class ChildFailed(RuntimeError):
    pass


class Interrupted(BaseException):
    """SIGTERM, SIGINT or SIGHUP to the driver, raised where it waits, so that the waits' cleanup stops the children"""

    def __init__(self, signum):
        BaseException.__init__(self, signum)
        self.signum = signum


def _raise_interrupted(signum, frame):
    for sig in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        signal.signal(sig, signal.SIG_IGN)                      # the cleanup that follows is not interrupted again
    raise Interrupted(signum)


def install_signal_handlers():
    for sig in (signal.SIGTERM, signal.SIGINT, signal.SIGHUP):
        signal.signal(sig, _raise_interrupted)


def _prctl():
    try:
        import ctypes
        return ctypes.CDLL(None, use_errno=True).prctl
    except (OSError, AttributeError):
        return None


def _die_with_parent(parent_pid, prctl=None):
    """in a child: SIGTERM once the parent is gone (Linux PR_SET_PDEATHSIG), and at once if it already is"""
    prctl = prctl or _prctl()
    if prctl is not None:
        prctl(1, int(signal.SIGTERM), 0, 0, 0)                     # PR_SET_PDEATHSIG = 1
    if os.getppid() != parent_pid:
        os.kill(os.getpid(), signal.SIGTERM)


def run_training(cmd, timeout):
    """one training round as a child in its own session (killpg reaches torchrun and whatever it has not moved to
    sessions of its own).  On a time limit, or an Interrupted raised while waiting, it is stopped: SIGTERM (torchrun
    stops its ranks), then SIGKILL after STOP_GRACE seconds.  Raises ChildFailed unless it exits with 0."""
    env = dict(os.environ, MPLBACKEND='Agg')
    parent, prctl = os.getpid(), _prctl()                           # resolved before the fork
    p = subprocess.Popen(cmd, env=env, start_new_session=True, preexec_fn=lambda: _die_with_parent(parent, prctl))
    try:
        rc = p.wait(timeout=timeout or None)
    except subprocess.TimeoutExpired:
        raise ChildFailed('training timed out after %g s: %s' % (timeout, ' '.join(cmd)))
    finally:
        if p.poll() is None:
            _stop_session(p)
    if rc != 0:
        raise ChildFailed('training exited with %s: %s' % (_status(rc), ' '.join(cmd)))


def _stop_session(p):
    for sig, wait in ((signal.SIGTERM, STOP_GRACE), (signal.SIGKILL, 20)):
        try:
            os.killpg(p.pid, sig)
        except ProcessLookupError:
            return
        try:
            p.wait(timeout=wait)
            return
        except subprocess.TimeoutExpired:
            pass


def _status(rc):
    return 'signal %d' % -rc if rc < 0 else 'status %d' % rc


# ------------------------------------------------------------------------------- labelling
def label_worker(spec):
    """One labelling child: one save_labels call over [start, end); with save_each=False every array it hands over is
    spooled at once as <spool>/<n>.npy (np.save writes the bytes np.savez stores for a member) and its key appended
    to <spool>/names, so the worker holds one batch at a time."""
    import numpy as np
    sys.path.insert(0, ROOT)
    from labels_from_segnet import save_labels
    spool = spec['spool']
    os.makedirs(spool, exist_ok=True)
    count = [0]
    with open(os.path.join(spool, 'names'), 'w') as names:
        def spool_one(key, value):
            np.save(os.path.join(spool, '%d.npy' % count[0]), value)
            names.write(json.dumps(key) + '\n')
            count[0] += 1

        save_labels(spec['param_dir'], spec['iteration'], spec['device'], spec['img_zip_fn'], spec['label_zip_fn'],
                    spec['out_dir'], spec['start'], spec['end'], spec['soft_label'], spec['eval_shape'],
                    spec['save_each'], figure=spec['figure'], result_fn=os.path.join(spool, 'result.json'),
                    on_labels=None if spec['save_each'] else spool_one,
                    split_planes=spec.get('split_planes', False), dtype=spec['dtype'],
                    loader_procs=spec.get('loader_procs', 0),
                    figure_renderer=spec.get('figure_renderer', 'matplotlib'))


def _child_main(target, arg, parent_pid):
    """the entry of every spawned child: die with the driver, then target(arg)"""
    _die_with_parent(parent_pid)
    target(arg)


def run_workers(target, args, timeout, names=None):
    """target(a) for every a in args, each in a spawned child; returns once all exited with 0.  At the first failure,
    the time limit, or an Interrupted raised while waiting, the others are stopped (SIGTERM, then SIGKILL) and the
    exception propagates (ChildFailed for the first two)."""
    ctx = multiprocessing.get_context('spawn')
    procs = [ctx.Process(target=_child_main, args=(target, a, os.getpid()),
                         name=names[i] if names else 'w%d' % i) for i, a in enumerate(args)]
    try:
        for p in procs:
            p.start()
        deadline = time.time() + timeout if timeout else None
        pending = list(procs)
        while pending:
            for p in list(pending):
                if p.exitcode is None:
                    continue
                pending.remove(p)
                if p.exitcode != 0:
                    raise ChildFailed('labelling worker %s exited with %s' % (p.name, _status(p.exitcode)))
            if pending and deadline is not None and time.time() > deadline:
                raise ChildFailed('labelling timed out after %g s' % timeout)
            time.sleep(0.1)
    finally:
        _stop_all([p for p in procs if p.pid is not None and p.exitcode is None])


def _stop_all(procs):
    for p in procs:
        p.terminate()
    deadline = time.time() + STOP_GRACE
    for p in procs:
        p.join(max(0.0, deadline - time.time()))
        if p.exitcode is None:
            p.kill()
            p.join()


def stream_label_zip(out_zip, items, remove=True):
    """items: (key, .npy file) in order -> out_zip as np.savez(out_zip, **{key: array}) would write it (members
    key + '.npy', stored, Zip64), copying one file at a time; remove: delete each file once stored."""
    tmp = out_zip + '.tmp'
    with zipfile.ZipFile(tmp, 'w', zipfile.ZIP_STORED, allowZip64=True) as zf:
        for key, fn in items:
            with open(fn, 'rb') as src, zf.open(key + '.npy', 'w', force_zip64=True) as dst:
                shutil.copyfileobj(src, dst, 1 << 20)
            if remove:
                os.remove(fn)
    os.replace(tmp, out_zip)
    return out_zip


def spooled_items(spools):
    for spool in spools:
        with open(os.path.join(spool, 'names')) as fp:
            for n, line in enumerate(fp):
                yield json.loads(line), os.path.join(spool, '%d.npy' % n)


def label_specs(args, param_dir, iteration, out_dir):
    """the labelling workers' arguments (label_worker): one contiguous range of the first n_labels images per GPU"""
    soft_label = args.use_soft_label or args.use_mse
    same_device = os.environ.get('SPA_BENCH_SAME_DEVICE') == '1'
    spool_root = out_dir + '.spool'
    specs = []
    for i, (start, end) in enumerate(label_ranges(args.n_labels, args.n_gpus)):
        specs.append({'device': 0 if same_device else i, 'param_dir': param_dir, 'iteration': iteration,
                      'img_zip_fn': args.img_zip_fn, 'label_zip_fn': args.label_zip_fn, 'out_dir': out_dir,
                      'start': start, 'end': end, 'soft_label': soft_label, 'eval_shape': list(args.eval_shape),
                      'save_each': args.save_each, 'figure': not args.no_figure, 'dtype': args.label_dtype,
                      'split_planes': args.label_split_planes, 'loader_procs': args.label_loader_procs,
                      'figure_renderer': getattr(args, 'figure_renderer', 'matplotlib'), 'spool': os.path.join(spool_root, 'w%d' % i)})
    return specs


def create_label_from_model(args, param_dir, iteration, out_dir, out_zip):
    """labels_from_segnet.save_labels over the first n_labels images of the split, sharded over n_gpus spawned
    workers -> out_zip"""
    spool_root = out_dir + '.spool'
    os.makedirs(out_dir, exist_ok=True)
    specs = label_specs(args, param_dir, iteration, out_dir)
    run_workers(label_worker, specs, args.child_timeout)
    spools = [s['spool'] for s in specs]
    with open(os.path.join(out_dir, 'result.json'), 'a') as out:
        for spool in spools:
            fn = os.path.join(spool, 'result.json')
            if os.path.exists(fn):
                with open(fn) as fp:
                    shutil.copyfileobj(fp, out)
    if args.save_each:
        print('zipping files...')
        with zipfile.ZipFile(out_zip, 'w') as zf:
            for fn in sorted(glob.glob(os.path.join(out_dir, '*.npy'))):
                zf.write(fn)
    else:
        stream_label_zip(out_zip, spooled_items(spools))
    shutil.rmtree(spool_root, ignore_errors=True)
    return out_zip


# ------------------------------------------------------------------------------- driver
def run(args):
    first_result_dir = args.first_result_dir
    if first_result_dir is None:
        first_result_dir = create_result_dir(first_round_prefix(args))
    dirs = {1: first_result_dir}
    for step in plan(args, first_result_dir):
        k = step['round']
        if step['kind'] == 'train':
            if k not in dirs:
                dirs[k] = create_result_dir(step['prefix'])
            cmd = torchrun_command(args.n_gpus, train_argv(args, step, dirs[k], dirs), free_port())
            print('train_img_zip:', args.img_zip_fn)
            print('train_label_zip:', step['train_label_zip'])
            print('-' * 20)
            print(' '.join(cmd))
            print('=' * 20)
            sys.stdout.flush()
            run_training(cmd, args.child_timeout)
        else:
            out_zip = create_label_from_model(args, dirs[k], step['iteration'], step['out_dir'], step['out_zip'])
            print('{} round finished'.format('First' if k == 1 else '%dth' % k))
            print('result_dir:', dirs[k])
            print('out_zip_fn:', out_zip)
            print('-' * 20)
            sys.stdout.flush()
    return dirs


def main(argv=None):
    args = get_args(argv)
    install_signal_handlers()
    try:
        run(args)
    except ChildFailed as e:
        print('run_train_rounds: %s; no further process is started' % e, file=sys.stderr)
        return 1
    except Interrupted as e:
        print('run_train_rounds: signal %d, the running children were stopped' % e.signum, file=sys.stderr)
        return 128 + e.signum
    return 0


if __name__ == '__main__':
    sys.exit(main())
