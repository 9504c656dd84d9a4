#!/usr/bin/env python3
"""Development aid: SHA-256 digests of the outputs of every SegNet entry point, in every operand type and input form,
on seeded inputs, so that two builds can be compared bit for bit from two processes:
    SPA_LIB_PATH=$PWD/ab/libspalign_old.so python tools/segnet_digest.py ; python tools/segnet_digest.py
Inference x {fp32, bf16, f16x3}: encode conv1 (B = 3, 48 x 80), encode 64-channel and decode (36 x 80), decode1
(32 x 80; none of them fills the 8 x 32 tiles) and SegNetBasic.forward + segnet_score at B = 2, 512 x 1024 ->
1024 x 2048.  Training x the same: forward in its three input forms with the BN statistics, dgrad full and pooled,
wgrad in its three input forms, at the small shapes and at B = 2, 256 x 512 (several wgrad chunks per workgroup)."""
import hashlib, importlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
segnet = importlib.import_module('superpixel-align_amd.segnet')
engine = importlib.import_module('superpixel-align_amd.engine')
from segnet_bench import random_params  # noqa: E402

SFX = (('fp32', ''), ('bf16', '_bf16'), ('f16x3', '_f16x3'))


def dig(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()[:16] if t is not None else '-'


def show(*key_and_tensors):
    n = sum(1 for v in key_and_tensors if isinstance(v, str))
    print(' '.join(key_and_tensors[:n]), ' '.join(dig(t) for t in key_and_tensors[n:]), flush=True)


def main():
    torch.cuda.set_device(0)
    eng = engine.Engine(0)
    g = torch.Generator(device='cuda').manual_seed(7)
    rnd = lambda *s: torch.randn(s, generator=g, device='cuda')
    w1, w64 = rnd(49, 64, 4) * 0.05, rnd(49, 64, 64) * 0.02
    w1[:, :, 3] = 0
    bias, wc, bc = rnd(64) * 0.1, rnd(2, 64) * 0.1, rnd(2) * 0.1
    for tag, B, H1, W1, H, W in (('small', 3, 48, 80, 36, 80), ('large', 2, 256, 512, 128, 256)):
        img = torch.rand((B, 3, H1, W1), generator=g, device='cuda') * 255
        x = rnd(B, H, W, 64)                                       # a 64-channel map, channels-last storage
        xh = rnd(B, H // 2, W // 2, 64)                            # a decoder's pooled input and its index map
        idx = torch.randint(0, 4, (B, H // 2, W // 2, 64), generator=g, device='cuda', dtype=torch.uint8)
        dy1, dy = rnd(B, H1, W1, 64), rnd(B, H, W, 64)
        xh1 = rnd(B, 16, 40, 64)                                   # decode1 writes the network's size: a multiple of 16
        idx1 = torch.randint(0, 4, (B, 16, 40, 64), generator=g, device='cuda', dtype=torch.uint8)
        for mode, sfx in SFX:
            if tag == 'small':
                enc, dec = getattr(eng, 'segnet_encode' + sfx), getattr(eng, 'segnet_decode' + sfx)
                show('infer', mode, 'encode_conv1', *enc(img, w1, bias, segnet.MEAN, segnet.STD))
                show('infer', mode, 'encode_64', *enc(x.permute(0, 3, 1, 2), w64, bias))
                show('infer', mode, 'decode', dec(xh.permute(0, 3, 1, 2), idx.permute(0, 3, 1, 2), w64, bias))
                show('infer', mode, 'decode1', dec(xh1.permute(0, 3, 1, 2), idx1.permute(0, 3, 1, 2), w64, bias, wc, bc))
            fwd, dgrad, wgrad = (getattr(eng, 'segnet_train_' + k + sfx) for k in ('forward', 'dgrad', 'wgrad'))
            show('train', mode, tag, 'forward_conv1', *fwd(img, w1, None, segnet.MEAN, segnet.STD))
            show('train', mode, tag, 'forward_64', *fwd(x, w64))
            show('train', mode, tag, 'forward_dec', *fwd(xh, w64, idx))
            show('train', mode, tag, 'forward_nostats', *fwd(x, w64, stats=False))
            show('train', mode, tag, 'dgrad_full', dgrad(dy, w64))
            show('train', mode, tag, 'dgrad_pooled', dgrad(dy, w64, idx))
            show('train', mode, tag, 'wgrad_conv1', wgrad(dy1, img, None, segnet.MEAN, segnet.STD))
            show('train', mode, tag, 'wgrad_64', wgrad(dy, x))
            show('train', mode, tag, 'wgrad_dec', wgrad(dy, xh, idx))
    p = random_params()
    img = torch.randint(0, 256, (2, 3, 512, 1024), generator=g, device='cuda').float()
    for mode, _ in SFX:
        m = segnet.SegNetBasic(p, pred_shape=(1024, 2048), engine=eng, dtype='bf16' if mode == 'bf16' else 'fp32',
                               split_planes=mode == 'f16x3')
        trace = []
        prob = m.forward(img, trace=trace)
        mask, sc = eng.segnet_score(prob, (1024, 2048), want_scores=True)
        show('chain', mode, 'encoders', *[t for pair in trace for t in pair])
        show('chain', mode, 'prob_mask_scores', prob, mask, sc)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
