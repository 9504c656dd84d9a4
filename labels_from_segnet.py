#!/usr/bin/env python
"""Labels from a trained SegNet-Basic snapshot (same CLI, outputs and save_labels() as the reference script of this
name, which utils/run_train_rounds.py imports between training rounds), on libspalign's kernels instead of Chainer.
See superpixel-align_amd/segnet.py for the network.

Outputs per image, in --out_dir:
  <basename>.npy          bool mask of shape eval_shape (argmax of the probabilities resized to eval_shape)
  <basename>_scores.npy   THE MASK AGAIN: the reference's CLI path (save_each=True, labels_from_segnet.py:90-92) saves
                          `pred` under this name too; kept byte-compatible.  save_labels(..., save_each=False) returns
                          the float32 (2, H, W) scores instead, as run_train_rounds.py expects.
  <basename>.png          the 3-panel figure (unless --no_figure)
  <stem>.jpg              instead of it with --figure_renderer device: the three panels (the frame under the mask, the
                          ground truth's road, the mask) composed and JPEG-encoded on the device,
                          superpixel-align_amd/figure.py; everything else is the same byte for byte
  result.json             one JSON line per image, the reference's keys in its order (with --dtype bf16 one more key
                          after them, "dtype": "bf16"; with --split_planes one more, "split_planes": true; plain float32
                          lines are the reference's keys only)
Additions: --loader_procs N (default 0: the loop decodes every PNG itself and scores every image with a launch and a
synchronisation of its own; N > 0: N worker processes decode the frames and the labelIds images a few batches ahead into
pinned shared-memory slabs, superpixel-align_amd/segnet_loader.py LabelLoader, the mask, the scores and the confusion
counts of a batch come from one launch, spa_segnet_label_eval, and the files of a batch are written while the next one
is on the device; the outputs are the same, byte for byte), --no_figure, --batchsize (images per launch chain), --dtype {fp32,bf16} (the precision of the convolutions'
operands: fp32, the default, the float32 matrix cores; bf16 every product operand rounded to bf16 with float32
accumulation, see include/spalign.h spa_segnet_encode_bf16), --split_planes (float32 accuracy on the f16 matrix cores:
every operand as two scaled half-precision planes, three products per float32 product, spa_segnet_encode_f16x3; the
counterpart of train_segnet.py --split_planes, refused with --dtype bf16).  --gpu -1 (the reference's CPU mode) runs on device 0:
there is no CPU path.  Only model 'basic' in the snapshot's args.txt is supported.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _save_figure(d, i, pred, label, out_dir):
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from PIL import Image
    d._open()
    with Image.open(d.img_zf.open(d.img_fns[i])) as f:        # the archive member (the reference opens it as a path)
        img = np.array(f.convert('RGB'), dtype=np.uint8)
    plt.clf()
    fig, axes = plt.subplots(1, 3)
    fig.set_dpi(300)
    for a in axes:
        a.axis('off')
    axes[0].imshow(img)
    axes[0].imshow(pred, alpha=0.4, cmap=plt.cm.Set1_r)
    axes[0].set_title('Estimated road mask (input image overlayed)', fontsize=4)
    axes[1].imshow(label == 1)
    axes[1].set_title('Ground truth road mask', fontsize=4)
    axes[2].imshow(pred)
    axes[2].set_title('Estimated road mask', fontsize=4)
    plt.savefig(os.path.join(out_dir, os.path.basename(d.img_fns[i])), bbox_inches='tight')
    plt.close()


class _DeviceFigures(object):
    """--figure_renderer device: the 1x3 figures of batches whose frames are of eval_shape, through figure.DeviceFigures
    (created with the first such batch).  encode -> a slot, or None for a batch that matplotlib has to draw."""

    def __init__(self, eng, eval_shape_t, batchsize):
        self.figure = importlib.import_module('superpixel-align_amd.figure')
        self.eng, self.shape, self.batch, self.figs = eng, eval_shape_t, batchsize, None
        self.overlay, self.on_1, self.on_7 = self.figure.overlay(), self.figure.two_colour([1]), self.figure.two_colour([7])

    def encode(self, frames, mask, truth, truth_is_ids):
        """frames (n,H,W,3), mask (n,H,W) 0 / 1 and truth (n,H,W), all uint8 on the device; truth_is_ids: truth holds
        the raw labelIds bytes (road is 7), otherwise 1 where the label mask is 1"""
        if tuple(frames.shape[1:3]) != self.shape or tuple(truth.shape[1:]) != self.shape:
            return None
        if self.figs is None:
            self.figs = self.figure.DeviceFigures(self.eng, self.shape, self.batch, (1, 3))
        mask = mask.contiguous()
        return self.figs.encode(frames.contiguous(), [mask, truth.contiguous(), mask],
                                [self.overlay, self.on_7 if truth_is_ids else self.on_1, self.on_1],
                                [self.figure.BLEND, self.figure.TABLE, self.figure.TABLE])

    def files(self, slot, n):
        """once the host knows that the stream got past encode(): the n JPEG files of the slot"""
        self.figs.fetch(slot)
        return [self.figs.file_bytes(slot, j) for j in range(n)]


def _loader_run(torch, segnet, eng, model, loader, in_shape, eval_shape_t, save_each, emit, host_batch, result_path,
                times, figures=None):
    """save_labels with --loader_procs: batch k goes slab -> resize -> network -> segnet_label_eval -> non-blocking
    copies into one of two pinned host buffer sets, and while it is on the device the host writes batch k-1's outputs
    (one event wait and one open of the result file per batch).  A batch the loader marks for the host path, or whose
    labels are not of eval_shape (the plain loop's ValueError), goes through host_batch after the batch before it has
    been written, so files, on_labels calls and JSON lines keep the index order.  -> the number of such batches.
    times: seconds spent waiting for the loader, waiting for the device and writing the outputs are added to its
    'loader_wait_s', 'device_wait_s' and 'output_s'."""
    clock = time.perf_counter
    B = loader.B
    ring = []
    for _ in range(2):
        ring.append({'mask': torch.empty((B,) + eval_shape_t, dtype=torch.uint8).pin_memory(),
                     'scores': None if save_each else torch.empty((B, 2) + eval_shape_t,
                                                                  dtype=torch.float32).pin_memory(),
                     'counts': torch.empty((B, 4), dtype=torch.int64).pin_memory()})
    pending = [None]

    def flush():
        rec, pending[0] = pending[0], None
        if rec is None:
            return
        t0 = clock()
        rec['event'].synchronize()
        t1 = clock()
        buf = rec['buf']
        mask_h, counts_h = buf['mask'].numpy(), buf['counts'].numpy()
        sc_h = buf['scores'].numpy() if buf['scores'] is not None else None
        jpgs = figures.files(rec['fig'], len(rec['indices'])) if rec['fig'] is not None else None
        with open(result_path, 'a') as fp:
            for j, i in enumerate(rec['indices']):
                label = segnet.label_mask(rec['ids_host'][j]) if rec['ids_host'] is not None else None
                emit(i, mask_h[j], sc_h[j] if sc_h is not None else None, label, counts_h[j], fp,
                     None if jpgs is None else jpgs[j])
        times['device_wait_s'] += t1 - t0
        times['output_s'] += clock() - t1

    n_host = k = 0
    batches = loader.batches()
    while True:
        t0 = clock()
        batch = next(batches, None)
        times['loader_wait_s'] += clock() - t0
        if batch is None:
            break
        if batch.host or tuple(batch.label_ids.shape[1:]) != eval_shape_t:
            flush()
            n_host += 1
            host_batch(batch.indices)
            continue
        n = len(batch.indices)
        x = eng.resize_cvcubic_u8(batch.frames, in_shape)
        prob = model.forward(x)
        mask, sc, counts = eng.segnet_label_eval(prob, eval_shape_t, batch.label_ids, want_scores=not save_each)
        buf = ring[k % 2]
        k += 1
        buf['mask'][:n].copy_(mask, non_blocking=True)
        buf['counts'][:n].copy_(counts, non_blocking=True)
        if sc is not None:
            buf['scores'][:n].copy_(sc, non_blocking=True)
        fig = figures.encode(batch.frames, mask, batch.label_ids, True) if figures is not None else None
        event = torch.cuda.Event()
        event.record()
        rec = {'indices': batch.indices, 'ids_host': batch.ids_host, 'buf': buf, 'event': event, 'fig': fig}
        flush()                                          # batch k-1's files while batch k is on the device
        pending[0] = rec
    flush()
    return n_host


def save_labels(param_dir, iteration, gpu, img_zip_fn, label_zip_fn, out_dir,
                start_index, end_index, soft_label, eval_shape,
                save_each=False, figure=True, batchsize=4, result_fn=None, on_labels=None,
                loader_procs=0, loader_stats=None, figure_renderer='matplotlib', split_planes=False, dtype='fp32'):
    """labels_from_segnet.py:24-153.  With save_each=False returns {<out_dir>/<basename>: bool mask,
    <out_dir>/<basename>_scores: float32 (2, H, W) probabilities at eval_shape}.  result_fn: the file the JSON lines
    are appended to (default <out_dir>/result.json; utils/run_train_rounds.py gives each labelling process its own).
    on_labels (save_each=False): called with (key, array) for the mask and then the scores of every image, in index
    order, instead of collecting them in the returned dict (which stays empty), so a long range needs the memory of
    one batch only.  dtype: 'fp32' (default) or 'bf16', the network's convolution precision (segnet.SegNetBasic);
    bf16 adds "dtype": "bf16" to every JSON line.  split_planes (dtype 'fp32' only): the float32-accurate
    convolutions on the f16 matrix cores; adds "split_planes": true to every JSON line.  loader_procs N > 0: N worker
    processes decode the frames and labelIds images ahead of the network and everything after it is one launch per batch
    (_loader_run); the outputs are the plain loop's.  loader_stats: a dict that receives loop_s (the wall time of the
    batch loop) and, from a loader run, n_host_batches (batches that took the plain loop's path), pinned, worker_pids and
    the loop's loader_wait_s, device_wait_s and output_s.  figure_renderer: 'matplotlib' (<basename>.png, as the
    reference draws it) or 'device' (<stem>.jpg, composed and encoded on the device, figure.py; a batch whose frames are
    not of eval_shape, and a batch the loader hands to the host path, are drawn by matplotlib); everything else that is
    written or returned is the same under either."""
    import torch
    if figure_renderer not in ('matplotlib', 'device'):
        raise ValueError('save_labels: figure_renderer must be matplotlib or device, got %r' % (figure_renderer,))
    segnet = importlib.import_module('superpixel-align_amd.segnet')
    cli = importlib.import_module('superpixel-align_amd.cli')
    segnet.check_mode('save_labels', dtype, split_planes)
    train_args = segnet.load_train_args(param_dir)

    if not os.path.exists(out_dir):
        try:
            os.makedirs(out_dir)
        except Exception:
            pass

    device = max(int(gpu), 0)
    torch.cuda.set_device(device)
    model = segnet.SegNetBasic.from_snapshot(param_dir, iteration, pred_shape=eval_shape, device=device, dtype=dtype,
                                             split_planes=split_planes)
    eng = model.engine
    in_shape = tuple(int(v) for v in train_args['input_shape'])
    eval_shape_t = tuple(int(v) for v in eval_shape)

    d = segnet.ZippedCityscapesRoadDataset(img_zip_fn, label_zip_fn, train_args['input_shape'])
    if end_index > len(d):
        raise ValueError(
            'end_index option should be less than the length of dataset '
            '{} but {} was given.'.format(len(d), end_index))

    pred_and_scores = {} if not save_each else None
    batchsize = max(int(batchsize), 1)
    result_path = result_fn or os.path.join(out_dir, 'result.json')
    figures = _DeviceFigures(eng, eval_shape_t, batchsize) if figure and figure_renderer == 'device' else None

    def emit(i, pred, score, label, conf, fp, jpg=None):
        """one image's outputs: pred uint8 (H,W), score float32 (2,H,W) or None, label int32 (H,W) (matplotlib's
        figure), conf (TN, FP, FN, TP), jpg: the figure's file made on the device; the JSON line goes to fp"""
        sc = cli.score_from_counts(*[int(v) for v in conf])
        pred = pred.astype(bool)
        fn_base = os.path.splitext(os.path.basename(d.img_fns[i]))[0]
        save_fn = os.path.join(out_dir, fn_base)
        if save_each:
            np.save(save_fn, pred)
            np.save(save_fn + '_scores', pred)       # sic: the reference saves the mask under this name too
        elif on_labels is not None:
            on_labels(save_fn, pred)
            on_labels(save_fn + '_scores', score.astype(np.float32))
        else:
            pred_and_scores[save_fn] = pred
            pred_and_scores[save_fn + '_scores'] = score.astype(np.float32)
        if figure and jpg is not None:
            with open(save_fn + '.jpg', 'wb') as f:
                f.write(jpg)
        elif figure:
            _save_figure(d, i, pred, label, out_dir)
        result_info = {
            'img_fn': d.img_fns[i],
            'label_fn': d.label_fns[i],
            'road_iou': sc['road_iou'],
            'non_road_iou': sc['non_road_iou'],
            'precision': sc['precision'],
            'recall': sc['recall'],
            'TP': sc['TP'],
            'FP': sc['FP'],
            'FN': sc['FN'],
        }
        result_info.update({
            'param_dir': param_dir,
            'iteration': iteration,
            'gpu': gpu,
            'img_zip_fn': img_zip_fn,
            'label_zip_fn': label_zip_fn,
            'out_dir': out_dir,
            'start_index': start_index,
            'end_index': end_index,
            'soft_label': soft_label,
            'eval_shape': eval_shape,
            'save_each': save_each,
        })
        result_info.update({'train_args': train_args})
        if dtype != 'fp32':
            result_info['dtype'] = dtype
        if split_planes:
            result_info['split_planes'] = True
        print(json.dumps(result_info), file=fp)

    def host_batch(ids, device_figures=True):
        """the plain loop's batch: decoded here, one confusion launch and one synchronisation per image.
        device_figures False: a batch the loader left to the host path, drawn by matplotlib under either renderer"""
        raws = [d.get_raw(i) for i in ids]
        # images of one size go through one launch chain (Cityscapes: all of them)
        groups = {}
        for j, (img, _) in enumerate(raws):
            groups.setdefault(img.shape, []).append(j)
        preds, scores, jpgs = [None] * len(ids), [None] * len(ids), [None] * len(ids)
        for shape, js in groups.items():
            u8 = torch.from_numpy(np.stack([raws[j][0].transpose(1, 2, 0) for j in js])).to(eng.device)
            x = eng.resize_cvcubic_u8(u8.contiguous(), in_shape)     # (B,3,h,w) float32 0..255, the dataset's cv2 resize
            prob = model.forward(x)
            mask, sc = eng.segnet_score(prob, eval_shape_t, want_scores=not save_each)
            slot = None
            if figures is not None and device_figures and all(raws[j][1].shape == eval_shape_t for j in js):
                truth = torch.from_numpy(np.stack([raws[j][1] == 1 for j in js]).astype(np.uint8)).to(eng.device)
                slot = figures.encode(u8, mask, truth, False)
            mask_h = mask.cpu().numpy()
            sc_h = sc.cpu().numpy() if sc is not None else None
            files = figures.files(slot, len(js)) if slot is not None else None
            for t, j in enumerate(js):
                preds[j] = mask_h[t]
                scores[j] = sc_h[t] if sc_h is not None else None
                jpgs[j] = files[t] if files is not None else None
        for j, i in enumerate(ids):
            label = raws[j][1]
            pred = preds[j]
            if label.shape != pred.shape:
                raise ValueError('label %s has shape %s, the prediction %s (eval_shape)'
                                 % (d.label_fns[i], label.shape, pred.shape))
            conf = eng.confusion(torch.from_numpy(pred[None]).to(eng.device),
                                 torch.from_numpy(np.ascontiguousarray(label[None])).to(eng.device)).cpu().numpy()[0]
            with open(result_path, 'a') as fp:
                emit(i, pred, scores[j], label, conf, fp, jpgs[j])

    loader = None
    if int(loader_procs) > 0 and end_index > start_index:
        sl = importlib.import_module('superpixel-align_amd.segnet_loader')
        # the label ids on the host are matplotlib's: not needed where every loader batch is drawn on the device
        keep_ids = figure and not (figures is not None and sl._first_png_shapes(d)[0][:2] == eval_shape_t)
        loader = sl.open_or_none(lambda: sl.LabelLoader(d, range(start_index, end_index), batchsize, int(loader_procs),
                                                        sl.DeviceLabelStage(eng), keep_ids=keep_ids),
                                 '--loader_procs: %s; the images are decoded on the host')
    times = {'loader_wait_s': 0.0, 'device_wait_s': 0.0, 'output_s': 0.0}
    t_loop = time.perf_counter()
    if loader is None:
        for lo in range(start_index, end_index, batchsize):
            host_batch(list(range(lo, min(lo + batchsize, end_index))))
    else:
        try:
            n_host = _loader_run(torch, segnet, eng, model, loader, in_shape, eval_shape_t, save_each, emit,
                                 lambda ids: host_batch(ids, False), result_path, times, figures)
        finally:
            if loader_stats is not None:
                loader_stats.update(pinned=loader.pinned, worker_pids=list(loader.worker_pids))
            loader.close()
        if loader_stats is not None:
            loader_stats['n_host_batches'] = n_host
            loader_stats.update(times)
    if loader_stats is not None:
        loader_stats['loop_s'] = time.perf_counter() - t_loop       # the batches only: no model load, no worker start
    del model
    if not save_each:
        return pred_and_scores


def _non_negative(v):
    n = int(v)
    if n < 0:
        raise argparse.ArgumentTypeError('must be >= 0, got %d' % n)
    return n


def get_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--param_dir', type=str)
    parser.add_argument('--iteration', type=int)
    parser.add_argument('--gpu', type=int, default=-1)
    parser.add_argument('--img_zip_fn', type=str)
    parser.add_argument('--label_zip_fn', type=str)
    parser.add_argument('--out_dir', type=str)
    parser.add_argument('--start_index', type=int)
    parser.add_argument('--end_index', type=int)
    parser.add_argument('--soft_label', action='store_true', default=False)
    parser.add_argument('--eval_shape', type=int, nargs=2, default=[1024, 2048])
    parser.add_argument('--no_figure', action='store_true', default=False)
    parser.add_argument('--figure_renderer', type=str, default='matplotlib', choices=['matplotlib', 'device'],
                        help='matplotlib: <basename>.png as the reference draws it; device: <stem>.jpg, the three panels '
                             'composed and JPEG-encoded on the device')
    parser.add_argument('--batchsize', type=int, default=4)
    parser.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    parser.add_argument('--split_planes', action='store_true', default=False)
    parser.add_argument('--loader_procs', type=_non_negative, default=0,
                        help='decode worker processes that feed the network; 0: the loop decodes every image itself')
    return parser


if __name__ == '__main__':
    parser = get_parser()
    args = parser.parse_args()
    if args.split_planes and args.dtype != 'fp32':
        parser.error('--split_planes is the float32-accurate mode: it cannot be combined with --dtype %s' % args.dtype)
    if args.figure_renderer == 'device' and args.no_figure:
        parser.error('--figure_renderer device draws figures: not with --no_figure')
    save_labels(
        args.param_dir, args.iteration, args.gpu, args.img_zip_fn,
        args.label_zip_fn, args.out_dir, args.start_index, args.end_index,
        args.soft_label, args.eval_shape, True, figure=not args.no_figure, batchsize=args.batchsize,
        split_planes=args.split_planes, dtype=args.dtype, loader_procs=args.loader_procs,
        figure_renderer=args.figure_renderer)
