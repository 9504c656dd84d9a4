"""GPU test of cli.ProcessDecoder on its own (--decode_procs; the driver comparison in test_gpu_pipeline.py reaches it
only end to end): every batch against Pillow's decode of its files, a reused slab, the short last batch, the batch
with a frame of another size, the host label copies, and what close() leaves behind."""
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segnet_train_synth as syn  # noqa: E402

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def test_process_decoder_batches_reuse_and_fallback(tmp_path):
    from PIL import Image
    cli = importlib.import_module('superpixel-align_amd.cli')
    rng = np.random.default_rng(7)
    frames, labels, img_fns, lab_fns = [], [], [], []
    for i in range(7):
        h, w = (20, 30) if i == 5 else (24, 40)
        frames.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        labels.append(rng.integers(0, 34, (24, 40), dtype=np.uint8))
        img_fns.append(str(tmp_path / ('f%d.png' % i)))
        lab_fns.append(str(tmp_path / ('l%d.png' % i)))
        Image.fromarray(frames[i]).save(img_fns[i])
        Image.fromarray(labels[i]).save(lab_fns[i])
        assert Image.open(lab_fns[i]).mode == 'L'
    before = syn.shm_names()
    dec = cli.ProcessDecoder(cli.ImageList(img_fns, None, np.uint8), cli.ImageList(lab_fns, None, np.uint8), 2, 2,
                             torch.device('cuda', 0), depth=3, host_labels=True)
    try:
        pids = dec.worker_pids
        assert 1 <= len(pids) <= 2 and all(syn.alive(p) for p in pids)
        got = [dec.take(idx) for idx in ([0, 1], [2, 3], [4, 5], [6])]     # the fourth comes back to the first slab
        torch.cuda.synchronize()
        assert got[2] is None                               # frame 5 has another size: the caller's threads take it
        for idx, g in zip(([0, 1], [2, 3], None, [6]), got):
            if idx is None:
                continue
            imgs, gts, host = g
            assert imgs.is_cuda and imgs.dtype == torch.uint8 and tuple(imgs.shape) == (len(idx), 24, 40, 3)
            assert gts.is_cuda and gts.dtype == torch.uint8 and tuple(gts.shape) == (len(idx), 24, 40)
            for j, i in enumerate(idx):
                assert np.array_equal(imgs[j].cpu().numpy(), np.asarray(Image.open(img_fns[i])))
                assert np.array_equal(gts[j].cpu().numpy(), np.asarray(Image.open(lab_fns[i])))
                assert host[j].flags.owndata and np.array_equal(host[j], labels[i])     # the first batch's: after reuse
    finally:
        dec.close()
        dec.close()
    assert syn.shm_names() == before and not any(syn.alive(p) for p in pids)
