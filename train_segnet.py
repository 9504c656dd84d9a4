#!/usr/bin/env python
"""Train SegNet-Basic on estimated road labels (same CLI, defaults and outputs as the reference script of this name,
which utils/run_train_rounds.py runs between labelling rounds), on libspalign's kernels instead of Chainer.  See
superpixel-align_amd/segnet_train.py for the network, the optimizers and the dataset.

Outputs in the result directory (create_result_dir(prefix), or --result_dir):
  args.txt               the arguments, JSON (sort_keys, indent 4)
  log                    LogReport's JSON list, one entry per --log_interval: iteration, epoch, main/loss (mean over
                         the interval), lr, elapsed_time and, where validation ran, val/main/iou/road,
                         val/main/iou/non_road, val/main/miou, val_/main/precision, val_/main/recall, val_/main/FP, FN
  snapshot_iter_<N>      every --val_interval: the npz labels_from_segnet.py reads (updater/model:main/predictor/...)
                         plus the optimizer, iteration, lr and iterator state that --resume reads
Only --model basic; one process unless --data_parallel is given.  An 'epoch' interval is converted to iterations
with the size of the (per-rank) training set.

--dtype {fp32,bf16} (this implementation's addition, parsed in front of the reference flags; default fp32): bf16 runs
every 7x7 convolution pass of a training step on the bf16 matrix cores, with float32 accumulation, float32 master
weights, BatchNorm and optimizer.  The dtype goes into args.txt and every snapshot.  --resume continues bit for bit in
the snapshot's own dtype, and a float32 snapshot may also be resumed in bf16 or the other way round (the weights and the
optimizer state are float32 in both).  Validation runs the float32 inference network in every training mode unless
--val_split_planes is given (its float32-accurate form on the f16 matrix cores, segnet.SegNetBasic split_planes;
recorded in args.txt only when given), and labels_from_segnet.py reads the snapshots of either dtype.

--split_planes (also parsed in front of the reference flags): run every 7x7 convolution pass of the float32 step at
float32 accuracy on the f16 matrix cores (each operand as two power-of-two-scaled half-precision planes, three products
per float32 product).  Everything else is the float32 path.  It does not combine with --dtype bf16.  Only when given,
args.txt records "split_planes": true and every snapshot an extensions/split_planes entry; --resume follows the
command-line flag (the state is float32 either way), and labels_from_segnet.py reads the snapshots unchanged.

--fused_bn (also parsed in front of the reference flags): run what lies between the 7x7 convolutions -- BatchNorm, ReLU,
2x2 pooling with its index maps, the classifier, forward and backward -- on the kernels of
csrc/spa_segnet_train_bn.hip instead of torch ops (SegNetTrainer(fused_bn=True)).  It combines with --dtype bf16,
--split_planes, --data_parallel, --loader_procs and --resume.  The losses and the optimizers stay in torch.  The mode
holds no state: a snapshot gets no new entry, --resume follows the command line, and a resumed fused run continues a
fused run bit for bit.  args.txt records "fused_bn": true only when the flag is given.  Validation is untouched.

--data_parallel (also parsed in front of the reference flags): run as one rank of a torchrun launch (RANK, WORLD_SIZE,
LOCAL_RANK; dist.init binds the rank's GPU), what the reference does under mpiexec with ChainerMN.  A step computes
the gradient of the mean of the ranks' losses with BatchNorm over all ranks' batches (segnet_train.RankGroup).  Rank
r seeds random, numpy and torch with r; the training set is split by segnet_train.shard_indices (chainermn's
scatter_dataset with shuffle), the validation set into contiguous shards, and every reported validation metric is the
mean of the ranks' values.  Only rank 0 writes args.txt (with data_parallel and world_size), the log (main/loss is its
own) and the snapshots, which add the world size and every rank's iterator and numpy state; --resume continues bit
for bit with the same world size and refuses another one.  One rank computes the one-process run's bits.

--loader_procs N (also parsed in front of the reference flags; default 0: the loop decodes, resizes and augments every
batch itself, one image after the other, between two steps).  With N > 0, N worker processes decode the PNGs and read
the labels a few batches ahead into pinned shared-memory slabs, and the GPU resizes and augments them on a side stream
(superpixel-align_amd/segnet_loader.py).  The run computes the bits of the default run: the same losses, the same
snapshots (they store the iterator and numpy state that belong to their iteration, not the prefetching loader's), and
--resume continues bit for bit from either kind of run with or without the flag.  args.txt records loader_procs only
when it is given.  Under --data_parallel every rank has its own N workers: keep ranks x N within the CPUs the job has.
A batch whose frames are not of the first frame's size takes the host path, and so does the whole run (it says so
once) where /dev/shm cannot hold the slabs.  The same workers feed the validation passes (segnet_loader.LabelLoader): the
validation images go through the predictor in batches of --batchsize, the confusion counts come from
spa_segnet_label_eval and are summed on the device, and every report entry is the default run's.

--device_cache_gb G (pre-parser, float, default 0; needs --loader_procs > 0, refused otherwise before anything is
written).  With G > 0 every decoded training frame and label array, and every staged validation batch, stays in device
memory once it has been seen (superpixel-align_amd/frame_cache.py), first come first kept up to G GB per rank, no
eviction; an example that is kept is never decoded or uploaded again, and the input kernels read it where it lies.  The
draws, the losses, the validation entries, the snapshots and --resume are the run's without the flag.  args.txt records
device_cache_gb only when it is given; at close the run prints one line with the cache's counters to stderr.
"""
import argparse
import importlib
import json
import os
import random
import re
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def get_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument(
        '--train_img_zip', type=str, default='data/cityscapes_train_imgs.0.zip',
        help='If it\'s given, ZippedEstimatedCityscapesDataset will be used.')
    parser.add_argument(
        '--train_label_zip', type=str, default='results/estimated_train_labels.0.zip',
        help='If it\'s given, ZippedEstimatedCityscapesDataset will be used.')
    parser.add_argument(
        '--val_img_zip', type=str, default='data/cityscapes_val_imgs.0.zip',
        help='If it\'s given, ZippedCityscapesRoadDataset will be used.')
    parser.add_argument(
        '--val_label_zip', type=str, default='data/cityscapes_gtFine_val_labels.0.zip',
        help='If it\'s given, ZippedCityscapesRoadDataset will be used.')
    parser.add_argument('--model', type=str, default='basic', choices=['normal', 'basic'])
    parser.add_argument('--batchsize', type=int, default=4)
    parser.add_argument('--lr', type=float, default=0.01)
    parser.add_argument('--decay_iteration', type=int, default=300)
    parser.add_argument('--weight_decay', type=float, default=0.0005)
    parser.add_argument('--train_limit', type=str, nargs=2, default=['1000', 'iteration'])
    parser.add_argument('--optimizer', type=str, default='MomentumSGD', choices=['Adam', 'MomentumSGD'])
    parser.add_argument('--input_shape', type=int, nargs=2, default=[512, 1024])
    parser.add_argument('--random', action='store_true', default=False)
    parser.add_argument('--communicator', type=str, default='single_node')
    parser.add_argument('--prefix', type=str, default='results/round_1')
    parser.add_argument('--resume', type=str, default=None)
    parser.add_argument('--log_interval', type=str, nargs=2, default=['50', 'iteration'])
    parser.add_argument('--val_interval', type=str, nargs=2, default=['50', 'iteration'])
    parser.add_argument('--eval_shape', type=int, nargs=2, default=[1024, 2048])
    parser.add_argument('--result_dir', type=str, default=None)
    parser.add_argument(
        '--use_soft_label', action='store_true', default=False,
        help='If True, softmax cross entorpy with soft labels is used as loss function')
    parser.add_argument(
        '--use_mse', action='store_true', default=False,
        help='If True, mean squared error is used as loss function')
    parser.add_argument('--n_use_data', type=int, default=None)
    return parser


def get_args(argv=None):
    return get_parser().parse_args(argv)


def get_dtype_args(argv=None):
    """-> (--dtype, the remaining arguments for get_args): the flag is read by a pre-parser, in front of the
    reference flag set of get_parser."""
    argv = list(sys.argv[1:] if argv is None else argv)
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'],
                     help='operands of the 7x7 convolution passes: float32 or bf16 (float32 accumulation)')
    known, rest = pre.parse_known_args(argv)
    return known.dtype, rest


def get_pre_args(argv=None):
    """-> (namespace of this implementation's flags, the remaining arguments for get_args): --dtype (get_dtype_args),
    --split_planes, --val_split_planes, --fused_bn, --data_parallel, --loader_procs and --device_cache_gb, read by one
    pre-parser in front of the reference flag set of get_parser."""
    argv = list(sys.argv[1:] if argv is None else argv)
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'],
                     help='operands of the 7x7 convolution passes: float32 or bf16 (float32 accumulation)')
    pre.add_argument('--split_planes', action='store_true', default=False,
                     help='float32 step with its 7x7 passes at float32 accuracy on the f16 matrix cores')
    pre.add_argument('--val_split_planes', action='store_true', default=False,
                     help='validation passes at float32 accuracy on the f16 matrix cores (SegNetBasic split_planes)')
    pre.add_argument('--fused_bn', action='store_true', default=False,
                     help='BatchNorm, ReLU, pooling and the classifier of the step on fused kernels instead of torch ops')
    pre.add_argument('--data_parallel', action='store_true', default=False,
                     help='run as one rank of a torchrun launch (RANK / WORLD_SIZE / LOCAL_RANK)')
    pre.add_argument('--loader_procs', type=int, default=0,
                     help='decode worker processes of the input stage (per rank); 0: the loop prepares its batches itself')
    pre.add_argument('--device_cache_gb', type=float, default=0.0,
                     help='with --loader_procs: keep up to this many GB of decoded training and validation examples in '
                          'device memory (per rank) and decode each of them once; 0: decode every time')
    return pre.parse_known_args(argv)


def check_split_planes(pre):
    """The refusal of --split_planes with --dtype bf16 (the mode is the float32 step on split planes)."""
    if pre.split_planes and pre.dtype != 'fp32':
        raise ValueError('--split_planes runs the float32 step on split f16 planes and does not combine with '
                         '--dtype %s' % pre.dtype)


def run_args(argv=None):
    """-> (the pre-parser's namespace, the run's arguments as args.txt records them, before a data-parallel run adds
    its world size): the reference flags plus dtype, and split_planes / val_split_planes / fused_bn / data_parallel /
    loader_procs / device_cache_gb only where they are given.  --device_cache_gb without --loader_procs is refused
    here, before anything is written."""
    pre, argv = get_pre_args(argv)
    check_split_planes(pre)
    args = get_args(argv)
    args.dtype = pre.dtype
    if pre.split_planes:
        args.split_planes = True                   # args.txt records it; a default run's args.txt is unchanged
    if pre.val_split_planes:
        args.val_split_planes = True               # likewise: recorded only when given
    if pre.fused_bn:
        args.fused_bn = True                       # likewise
    if pre.data_parallel:
        args.data_parallel = True                  # args.txt records it with the world size; one-process runs unchanged
    if pre.loader_procs < 0:
        raise ValueError('--loader_procs must be >= 0, got %d' % pre.loader_procs)
    if pre.loader_procs:
        args.loader_procs = pre.loader_procs       # recorded only when given
    if not pre.device_cache_gb >= 0:
        raise ValueError('--device_cache_gb must be >= 0, got %r' % pre.device_cache_gb)
    if pre.device_cache_gb > 0:
        if not pre.loader_procs:
            raise ValueError('--device_cache_gb keeps what the decode workers of --loader_procs deliver: give '
                             '--loader_procs N > 0 with it')
        args.device_cache_gb = pre.device_cache_gb # likewise
    return pre, args


def create_result_dir(prefix):
    """<prefix>_<time>_<i> for the first i >= 0 that does not exist yet; copies this script into it."""
    stamp = time.strftime('%Y-%m-%d_%H-%M-%S')
    i = 0
    result_dir = '{}_{}_{}'.format(prefix, stamp, i)
    while os.path.exists(result_dir):
        i += 1
        result_dir = re.sub('_[0-9]+$', '_{}'.format(i), result_dir)
    os.makedirs(result_dir)
    shutil.copy(os.path.abspath(__file__), os.path.join(result_dir, os.path.basename(__file__)))
    return result_dir


def check_supported(args):
    """The refusals: the VGG-style 'normal' SegNet (segnet.load_train_args' message) and multi-rank launches without
    --data_parallel."""
    if args.model != 'basic':
        raise ValueError("--model '%s' is not supported: only SegNet-Basic ('basic') is implemented%s"
                         % (args.model, " (the VGG-style 'normal' SegNet is not)" if args.model == 'normal' else ''))
    ws = int(os.environ.get('WORLD_SIZE', os.environ.get('OMPI_COMM_WORLD_SIZE', '1')))
    if ws > 1 and not getattr(args, 'data_parallel', False):
        raise RuntimeError('train_segnet.py runs in one process only unless --data_parallel is given (WORLD_SIZE=%d): '
                           'a multi-rank launch needs the cross-rank BatchNorm and gradient all-reduce of '
                           '--data_parallel' % ws)


def _iterations(interval, n_data, batchsize):
    n, unit = int(interval[0]), interval[1]
    if unit == 'iteration':
        return n
    if unit == 'epoch':
        return max(1, int(np.ceil(n * n_data / float(batchsize))))
    raise ValueError('unknown interval unit %r' % unit)


def evaluate(trainer, valid, eval_shape, batchsize, indices=None, split_planes=False, loader=None):
    """SemanticSegmentationEvaluator + PrecisionRecallEvaluator over the validation set (or its examples `indices`)
    with the inference network (BN folded from the running statistics), predicting as labels_from_segnet.py does ->
    the report entries.  split_planes: the predictor's float32-accurate convolutions on the f16 matrix cores
    (--val_split_planes) instead of the float32 ones.  loader: a segnet_loader.LabelLoader over the same indices
    (--loader_procs): its batches of `batchsize` images go through the predictor together, segnet_label_eval's counts
    are summed on the device and downloaded once; an image has the same bits in any batch and the counts are
    integers, so the entries are the same.  Batches the loader marks for the host path take the per-image body."""
    import torch
    model = trainer.predictor(eval_shape, split_planes=True) if split_planes else trainer.predictor(eval_shape)
    eng = trainer.eng
    in_shape = tuple(int(v) for v in valid.resize_shape)
    indices = list(range(len(valid))) if indices is None else [int(i) for i in indices]
    conf = np.zeros(4, np.int64)                                    # TN, FP, FN, TP

    def host_images(ids):
        raws = [valid.get_raw(i) for i in ids]
        for img, label in raws:
            u8 = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 2, 0))[None]).to(eng.device)
            x = eng.resize_cvcubic_u8(u8.contiguous(), in_shape)
            mask, _ = eng.segnet_score(model.forward(x), tuple(eval_shape))
            gt = torch.from_numpy(np.ascontiguousarray(label[None])).to(eng.device)
            conf[...] += eng.confusion(mask, gt).cpu().numpy()[0]

    if loader is None:
        for lo in range(0, len(indices), batchsize):
            host_images(indices[lo:lo + batchsize])
    else:
        if list(loader.indices) != indices:
            raise ValueError('evaluate: the loader was opened over other indices than the ones to evaluate')
        shape = tuple(int(v) for v in eval_shape)
        total = torch.zeros(4, dtype=torch.int64, device=eng.device)
        for batch in loader.batches():
            if batch.host or tuple(batch.label_ids.shape[1:]) != shape:
                host_images(batch.indices)
                continue
            x = eng.resize_cvcubic_u8(batch.frames, in_shape)
            _, _, counts = eng.segnet_label_eval(model.forward(x), shape, batch.label_ids)
            total += counts.sum(0)
        conf += total.cpu().numpy()                                 # the one download of a validation
    TN, FP, FN, TP = [int(v) for v in conf]
    with np.errstate(divide='ignore', invalid='ignore'):
        iou_road = TP / float(TP + FP + FN) if TP + FP + FN else float('nan')
        iou_non = TN / float(TN + FN + FP) if TN + FN + FP else float('nan')
        prec = TP / float(TP + FP) if TP + FP else float('nan')
        rec = TP / float(TP + FN) if TP + FN else float('nan')
    return {'val/main/iou/road': iou_road, 'val/main/iou/non_road': iou_non,
            'val/main/miou': float(np.nanmean([iou_road, iou_non])),
            'val/main/class_accuracy/road': rec,
            'val_/main/precision': prec, 'val_/main/recall': rec, 'val_/main/FP': FP, 'val_/main/FN': FN}


def resume_check(snapshot_world_size, world_size):
    """The refusal of a resume across world sizes: a data-parallel snapshot records its world size and every rank's
    iterator, a one-process snapshot (None) only one iterator."""
    if (snapshot_world_size or 1) != world_size:
        raise RuntimeError('--resume: the snapshot was written by %s, this run has %d rank(s); resume with the world '
                           'size that wrote it' % ('%d rank(s)' % snapshot_world_size if snapshot_world_size
                                                   else 'one process', world_size))


def open_loader(n_procs, train, train_ids, it, stage, cache=None):
    """-> the run's segnet_loader.TrainLoader on n_procs workers, or None where /dev/shm cannot hold its slabs: the
    run says so once and prepares its batches itself (nothing has been drawn, so the bits are the same).  cache: the
    run's frame_cache (--device_cache_gb); without a loader it stays unused."""
    sl = importlib.import_module('superpixel-align_amd.segnet_loader')
    return sl.open_or_none(lambda: sl.TrainLoader(train, train_ids, it, n_procs, stage, cache=cache),
                           '--loader_procs: %s; the batches are prepared on the host')


def open_label_loader(n_procs, valid, valid_ids, batchsize, stage, pool=None, cache=None):
    """-> the run's segnet_loader.LabelLoader over the rank's validation indices (on the training loader's workers
    where `pool` is given), or None where /dev/shm cannot hold its slabs: one line, and validation decodes on the host"""
    sl = importlib.import_module('superpixel-align_amd.segnet_loader')
    return sl.open_or_none(lambda: sl.LabelLoader(valid, valid_ids, batchsize, n_procs, stage, pool=pool, cache=cache),
                           '--loader_procs: %s; the validation images are decoded on the host')


def main(argv=None):
    import torch
    pre, args = run_args(argv)
    dp = pre.data_parallel
    check_supported(args)
    st = importlib.import_module('superpixel-align_amd.segnet_train')
    segnet = importlib.import_module('superpixel-align_amd.segnet')

    group = None
    rank, ws = 0, 1
    eng = None
    if dp:
        dist = importlib.import_module('superpixel-align_amd.dist')
        rank, ws, _ = dist.init()                  # binds this rank's GPU; a process group for ws > 1 or SPA_DIST_FORCE
        import torch.distributed
        if torch.distributed.is_initialized():
            group = st.RankGroup()
        eng = importlib.import_module('superpixel-align_amd.engine').default_engine()
        args.world_size = ws
    else:
        torch.cuda.set_device(0)

    snap_ws = None
    if args.resume is not None:
        snap_ws = st.snapshot_world_size(args.resume)
        resume_check(snap_ws, ws)                  # before anything is written

    random.seed(rank)                              # the reference seeds by intra_rank
    np.random.seed(rank)
    torch.manual_seed(rank)
    if rank == 0:
        print(json.dumps(vars(args), indent=4, sort_keys=True))

    soft_label = args.use_soft_label or args.use_mse
    train = st.ZippedEstimatedCityscapesDataset(args.train_img_zip, args.train_label_zip, args.input_shape,
                                                args.random, soft_label)
    n_train = len(train) if args.n_use_data is None else min(args.n_use_data, len(train))
    valid = segnet.ZippedCityscapesRoadDataset(args.val_img_zip, args.val_label_zip, args.input_shape)
    # scatter_dataset: the training set shuffled into ws shards, the validation set in contiguous ones
    train_ids = st.shard_indices(n_train, ws, rank, shuffle=True)
    valid_ids = st.shard_indices(len(valid), ws, rank, shuffle=False)
    if rank == 0:
        print('train dataset:', n_train)
        print('valid dataset:', len(valid))

    lossfun = st.loss_function(args.use_soft_label, args.use_mse)
    if args.optimizer == 'Adam':
        opt = st.Adam()
    else:
        opt = st.MomentumSGD(args.lr, weight_decay=args.weight_decay)
    device = torch.cuda.current_device()
    trainer = st.SegNetTrainer(st.init_params(0), opt, lossfun, engine=eng, device=device, dtype=args.dtype,
                               split_planes=pre.split_planes, fused_bn=pre.fused_bn)
    it = st.ShuffledIterator(len(train_ids), args.batchsize)

    result_dir = None
    if rank == 0:
        result_dir = args.result_dir if args.result_dir is not None else create_result_dir(args.prefix)
        os.makedirs(result_dir, exist_ok=True)
        with open(os.path.join(result_dir, 'args.txt'), 'w') as fp:
            json.dump(vars(args), fp, indent=4, sort_keys=True)

    iteration = 0
    log = []
    if args.resume is not None:
        params, state, t, lr, iteration, it_state, rnd = st.load_snapshot_state(args.resume)
        if snap_ws is not None:
            it_state, rnd = st.load_rank_state(args.resume, rank)
        snap_dtype = st.snapshot_dtype(args.resume)
        if snap_dtype != args.dtype and rank == 0:
            print('resuming a %s snapshot in %s' % (snap_dtype, args.dtype))
        if st.snapshot_split_planes(args.resume) != pre.split_planes and rank == 0:
            print('resuming a %s snapshot %s --split_planes' % (snap_dtype, 'with' if pre.split_planes else 'without'))
        trainer = st.SegNetTrainer(params, opt, lossfun, engine=trainer.eng, dtype=args.dtype,
                                   split_planes=pre.split_planes, fused_bn=pre.fused_bn)
        opt.t = t
        if args.optimizer == 'MomentumSGD':
            opt.lr = lr
        opt.state = {k: {n: torch.as_tensor(v).to(trainer.eng.device) for n, v in s.items()} for k, s in state.items()}
        it.load(it_state)
        np.random.set_state(rnd)
        log_fn = os.path.join(os.path.dirname(os.path.abspath(args.resume)), 'log')
        if rank == 0 and os.path.exists(log_fn):
            log = [e for e in json.load(open(log_fn)) if e['iteration'] <= iteration]
    trainer.set_group(group)                       # every rank starts from rank 0's parameters

    # epoch units count the examples of this rank's shard, as the reference's per-rank iterator does
    stop = _iterations(args.train_limit, len(train_ids), args.batchsize)
    log_every = _iterations(args.log_interval, len(train_ids), args.batchsize)
    val_every = _iterations(args.val_interval, len(train_ids), args.batchsize)
    decay = args.decay_iteration if args.optimizer == 'MomentumSGD' else 0
    dev = trainer.eng.device
    loader = val_loader = cache = None
    if pre.device_cache_gb > 0:                    # this rank's cache of its own shards; nothing is allocated yet
        fc = importlib.import_module('superpixel-align_amd.frame_cache')
        cache = fc.DeviceFrameCache(int(pre.device_cache_gb * (1 << 30)), dev)
    if pre.loader_procs:                           # after --resume has set the iterator and numpy's state
        sl = importlib.import_module('superpixel-align_amd.segnet_loader')
        loader = open_loader(pre.loader_procs, train, train_ids, it, sl.DeviceStage(train, trainer.eng), cache)
    # loader None: every batch is prepared here; else loader.next() hands out the same batches, each with the (iterator
    # state, numpy state) the plain loop has after it, which the log and the snapshots then use
    try:
        if pre.loader_procs and len(valid_ids):    # validation reads from the same workers
            val_loader = open_label_loader(pre.loader_procs, valid, valid_ids, args.batchsize,
                                           sl.DeviceLabelStage(trainer.eng),
                                           pool=loader.workers if loader is not None else None, cache=cache)
        losses = []
        t0 = time.time()
        while iteration < stop:
            if loader is None:
                ids = train_ids[it.next_indices()]
                batch = [train.get_example(i) for i in ids]
                img = torch.from_numpy(np.stack([b[0] for b in batch])).to(dev)
                lab = torch.from_numpy(np.stack([b[1] for b in batch])).to(dev)
                it_state, np_state = it.state(), None                    # the live states are this iteration's
            else:
                img, lab, (it_state, np_state) = loader.next()
            losses.append(trainer.step(img, lab))
            lr_used = opt.lr                                             # observe_lr: Adam's is alpha_t of this step
            iteration += 1
            if decay > 0 and iteration % decay == 0:
                opt.lr *= 0.1                                            # ExponentialShift('lr', 0.1)
            report = {}
            if iteration % val_every == 0:
                report.update(evaluate(trainer, valid, args.eval_shape, args.batchsize, valid_ids,
                                       split_planes=pre.val_split_planes, loader=val_loader))
                if group is not None:
                    report = group.mean_over_ranks(report)               # create_multi_node_evaluator: mean over ranks
            if iteration % log_every == 0:
                entry = {'epoch': int(it_state['epoch']), 'iteration': iteration, 'main/loss': float(np.mean(losses)),
                         'lr': lr_used, 'elapsed_time': time.time() - t0}
                entry.update(report)
                losses = []
                if rank == 0:
                    log.append(entry)
                    with open(os.path.join(result_dir, 'log'), 'w') as fp:
                        json.dump(log, fp, indent=4)
                    print(json.dumps({k: entry.get(k) for k in ('iteration', 'main/loss', 'val/main/iou/road',
                                                                'val_/main/precision', 'val_/main/recall', 'lr',
                                                                'elapsed_time')}))
            if iteration % val_every == 0:
                extra = None
                if dp:
                    mine = st.rank_state(it, None if np_state is None else (it_state, np_state))
                    states = group.gather_objects(mine) if group is not None else [mine]
                    extra = st.data_parallel_extra(states)
                if rank == 0:
                    st.save_snapshot(os.path.join(result_dir, 'snapshot_iter_{}'.format(iteration)), trainer, iteration,
                                     opt.lr, it_state, extra, np_state)
    finally:
        if val_loader is not None:
            val_loader.close()
        if loader is not None:
            loader.close()
        if cache is not None:                      # after the loaders that can name its entries
            cache.close()
            print(('rank %d ' % rank if dp else '') + fc.summary_line(cache, loader, val_loader), file=sys.stderr,
                  flush=True)
    if group is not None:
        group.barrier()                            # no rank leaves before rank 0's last snapshot is written
    return result_dir


if __name__ == '__main__':
    main()
