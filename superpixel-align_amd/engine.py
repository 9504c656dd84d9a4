"""Device-level front end: torch tensors in, torch tensors out, every call a C-ABI call.

PyTorch is used here only for device memory and streams (the plumbing); the arithmetic of
every method below runs in libspalign.so (hand-written HIP for gfx950).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import FmapDesc, SpalignError, check


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _req(t, dtype, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise SpalignError('%s must be a contiguous CUDA tensor of dtype %s' % (what, dtype))
    return t


def _out(out, shape, dtype, device):
    """the output of a convolution wrapper: a new channels-last tensor, or the caller's (tests hand in poisoned buffers)"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device, memory_format=torch.channels_last)
    if not (out.is_cuda and out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous(memory_format=torch.channels_last)):
        raise SpalignError('out must be a channels-last CUDA tensor of dtype %s and shape %s' % (dtype, tuple(shape)))
    return out


def _scratch(scratch, v_shape, m_shape, device):
    """(v, m) scratch of the Winograd wrappers: new tensors, or the caller's pair"""
    if scratch is None:
        return (torch.empty(v_shape, dtype=torch.float32, device=device), torch.empty(m_shape, dtype=torch.float32, device=device))
    v, m = scratch
    for t, shape in ((v, v_shape), (m, m_shape)):
        if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
            raise SpalignError('scratch must be two contiguous float32 CUDA tensors of shapes %s, %s' % (v_shape, m_shape))
    return v, m


class Engine(object):
    """One spa_ctx (one GPU). Not thread safe; make one per process/GPU."""

    def __init__(self, device=None):
        if not torch.cuda.is_available():
            raise SpalignError('no GPU visible: the superpixel-align hot path has no CPU fallback')
        self.device = torch.device('cuda', torch.cuda.current_device() if device is None else device)
        self._lib = _lib.lib()
        h = ctypes.c_void_p()
        check(self._lib.spa_ctx_create(self.device.index, ctypes.byref(h)))
        self._ctx = h
        self._in_tables = {}           # segnet_train_input / _label: device tables per (kind, n_in, n_out, backend)
        self._stream_own = {}          # png_deflate / jpeg_encode: the engine's own out and meta (_stream_out)

    def _s(self):
        """The launch stream: torch's current stream of THIS engine's device (a spa_ctx is bound to one
        device; torch's current device may be another one)."""
        return _stream(self.device)

    def close(self):
        if getattr(self, '_ctx', None):
            self._lib.spa_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ status
    def status(self):
        """Read and clear the latched device status bits (synchronises the stream)."""
        v = ctypes.c_uint32(0)
        check(self._lib.spa_status(self._ctx, ctypes.byref(v), self._s()))
        return v.value

    def status_peek_async(self, word=None):
        """Enqueue a copy of the latched status bits into a pinned one-element int32 tensor on the current stream
        (nothing is cleared or synchronised); check it with `raise_on_word` once the stream got that far."""
        if word is None:
            word = torch.zeros(1, dtype=torch.int32).pin_memory()
        check(self._lib.spa_status_peek_async(self._ctx, ctypes.c_void_p(word.data_ptr()), self._s()))
        return word

    def status_take_async(self, word=None):
        """status_peek_async followed, in stream order, by the clear of the latch: the word holds the bits of the work
        enqueued since the previous take (per batch in the drivers' asynchronous loop)."""
        if word is None:
            word = torch.zeros(1, dtype=torch.int32).pin_memory()
        check(self._lib.spa_status_take_async(self._ctx, ctypes.c_void_p(word.data_ptr()), self._s()))
        return word

    def raise_on_word(self, word, ignore=_lib.INFO_BITS):
        st = int(word.item()) & 0xffffffff
        self.last_info = st & _lib.INFO_BITS
        st &= ~ignore
        if st:
            self.status()                                            # clear the latch, then report
            msgs = [m for bit, m in _lib.STATUS_BITS.items() if st & bit]
            raise SpalignError('device status 0x%x: %s' % (st, '; '.join(msgs)))

    def raise_on_status(self, ignore=_lib.INFO_BITS):
        """Raise on latched error bits.  Informational bits (a starved SLIC seed, an oversize
        component: both handled as scikit-image handles them) are collected in `self.last_info`."""
        st = self.status()
        self.last_info = st & _lib.INFO_BITS
        st &= ~ignore
        if st:
            msgs = [m for bit, m in _lib.STATUS_BITS.items() if st & bit]
            raise SpalignError('device status 0x%x: %s' % (st, '; '.join(msgs)))

    def ws_generation(self):
        """re-allocations of the context's workspaces so far (a captured graph is valid while this does not change)"""
        return int(self._lib.spa_ws_generation(self._ctx))

    def debug_set(self, key, value):
        """diagnostic kernel-selection switches (include/spalign.h: spa_debug_set); key 1 = planes-in-LDS kernel for the narrow
        split-plane 3x3 layers (1, default) or the kernel it replaced (0); key 3 = the 2-D tile kernel for the stride-2 openers
        (conv3x3_s2_f16s; 1, default) or the generic kernel for every shape (0); key 4 = the Winograd layers' operand path:
        0 = sub-grid-major tile numbering and float32 V, 1 = the sub-grids of a pixel row interleaved in the numbering (layers of
        dilation > 2), 2 (default) = that numbering and V written as the GEMM's planes (Cout a multiple of 256 from 512 on)"""
        check(self._lib.spa_debug_set(self._ctx, int(key), int(value)))
        self.__dict__.setdefault('_debug', {})[int(key)] = int(value)

    def debug_get(self, key, default):
        """the value debug_set last gave `key` on this engine (`default`: the library's own)"""
        return self.__dict__.get('_debug', {}).get(int(key), default)

    # ------------------------------------------------------------------ per-kernel timing
    def prof_enable(self, on=True):
        check(self._lib.spa_prof_enable(self._ctx, 1 if on else 0))
        self._prof_on = bool(on)

    def prof_is_on(self):
        return bool(getattr(self, '_prof_on', False))

    def prof_read(self):
        """{kernel name: (total ms, launches)} since prof_enable (synchronises)."""
        out = {}
        for slot in range(self._lib.spa_prof_slots()):
            ms, n = ctypes.c_double(0), ctypes.c_int(0)
            check(self._lib.spa_prof_read(self._ctx, slot, ctypes.byref(ms), ctypes.byref(n)))
            if n.value:
                out[self._lib.spa_prof_name(slot).decode()] = (ms.value, n.value)
        return out

    # ------------------------------------------------------------------ DRN glue
    def drn_normalise(self, x, dtype=torch.float32):
        """(B,3,H,W) float32 0..255 -> normalised channels-last tensor of `dtype` (one pass)."""
        x = _req(x, torch.float32, 'x')
        B, C, H, W = x.shape
        assert C == 3
        out = torch.empty((B, 3, H, W), dtype=dtype, device=x.device, memory_format=torch.channels_last)
        mean = (ctypes.c_double * 3)(0.485, 0.456, 0.406)
        std = (ctypes.c_double * 3)(0.229, 0.224, 0.225)
        check(self._lib.spa_drn_normalise(self._ctx, _ptr(x), B, H, W, _ptr(out),
                                          0 if dtype == torch.float32 else 1, mean, std, self._s()))
        return out

    def drn_stem_d(self, x, w0, b0, w1p, b1, dtype=torch.float32, split=False, want_layer0=False):
        """DRN-D stem in one kernel: raw (B,3,H,W) float32 0..255 -> layer1 output (B,16,H,W) of
        `dtype` (float32 arithmetic) in channels-last storage.  w0 (16,147), w1p (16,144) in
        (n, ky, kx, c) order.  split (float32 only): the 16-bit matrix cores with two half-precision planes per operand
        (float32 accuracy, csrc/spa_stem.hip) instead of the float32 matrix instructions."""
        x = _req(x, torch.float32, 'x')
        B, C, H, W = x.shape
        assert C == 3
        for t, shape in ((w0, (16, 147)), (b0, (16,)), (w1p, (16, 144)), (b1, (16,))):
            _req(t, torch.float32, 'stem weights')
            assert tuple(t.shape) == shape
        out = torch.empty((B, 16, H, W), dtype=dtype, device=x.device, memory_format=torch.channels_last)
        mean = (ctypes.c_double * 3)(0.485, 0.456, 0.406)
        std = (ctypes.c_double * 3)(0.229, 0.224, 0.225)
        # normalised channels-last copy of the image (float32, or bfloat16 for the bf16 kernel): per call, so calls
        # on different streams (DRN.batch_predict(streams > 1)) never share the context-wide workspace
        scratch = torch.empty((B, H, W, 3), dtype=dtype, device=x.device)
        if split and dtype == torch.float32:
            am = torch.empty(1, dtype=torch.int32, device=x.device)      # the largest value stored: layer 2's scale
            if want_layer0:
                # DRN-C: layer0's output as well (the residual of layer1's BasicBlock)
                out0 = torch.empty((B, 16, H, W), dtype=dtype, device=x.device, memory_format=torch.channels_last)
                check(self._lib.spa_drn_stem_c_amax(self._ctx, _ptr(x), B, H, W, _ptr(w0), _ptr(b0), _ptr(w1p), _ptr(b1),
                                                    mean, std, _ptr(out), _ptr(out0), _ptr(scratch), _ptr(am), self._s()))
                out._spa_amax = am
                return out, out0
            check(self._lib.spa_drn_stem_d_amax(self._ctx, _ptr(x), B, H, W, _ptr(w0), _ptr(b0), _ptr(w1p), _ptr(b1),
                                                mean, std, _ptr(out), _ptr(scratch), _ptr(am), self._s()))
            out._spa_amax = am
            return out
        if want_layer0:
            # DRN-C in the bf16 network: conv1's output as well (the residual of layer1's BasicBlock)
            assert dtype == torch.bfloat16, 'want_layer0: the split-plane float32 kernel or the bf16 kernel'
            out0 = torch.empty((B, 16, H, W), dtype=dtype, device=x.device, memory_format=torch.channels_last)
            check(self._lib.spa_drn_stem_c_bf16(self._ctx, _ptr(x), B, H, W, _ptr(w0), _ptr(b0), _ptr(w1p), _ptr(b1),
                                                mean, std, _ptr(out), _ptr(out0), _ptr(scratch), self._s()))
            return out, out0
        check(self._lib.spa_drn_stem_d(self._ctx, _ptr(x), B, H, W, _ptr(w0), _ptr(b0), _ptr(w1p), _ptr(b1),
                                       mean, std, _ptr(out), 0 if dtype == torch.float32 else 1, _ptr(scratch),
                                       self._s()))
        return out

    @staticmethod
    def layer2_planes(weight):
        """(32,16,3,3) -> (wp, inv_t) for drn_layer2_f16s: the MFMA A fragments of the two half-precision planes of t * w,
        [2 channel tiles][2 planes][5 steps][64 lanes][8]: lane = (channel n = lane & 15, k group g = lane >> 4), k group
        (step s, g) = tap 2s + g // 2 (tap 9: zero pad), input channels 8 (g & 1) .. + 7 (csrc/spa_stem.hip)."""
        assert tuple(weight.shape) == (32, 16, 3, 3)
        w = weight.detach().float()
        amax = float(w.abs().max().clamp_min(1e-30))
        t = 2.0 ** (14 - int(np.floor(np.log2(amax))))
        ws = (w.double() * t).float().reshape(32, 16, 9)                      # (n, c, tap)
        frag = torch.zeros((2, 5, 64, 8), dtype=torch.float32, device=w.device)
        for s_ in range(5):
            for g in range(4):
                tap = 2 * s_ + g // 2
                if tap > 8:
                    continue
                c0 = 8 * (g & 1)
                for ct in range(2):
                    frag[ct, s_, g * 16:(g + 1) * 16, :] = ws[ct * 16:(ct + 1) * 16, c0:c0 + 8, tap]
        h = frag.half()
        l = (frag - h.float()).half()
        return torch.stack([h, l], dim=1).contiguous(), float(1.0 / t)        # (2, 2, 5, 64, 8)

    def drn_layer2_f16s(self, x, wp, inv_t, bias, amax_in=None, out=None):
        """relu(conv3x3(x; 16 -> 32 channels, stride 2, padding 1) + bias) on the 16-bit matrix cores at float32 accuracy.
        Returns y with the device word of its largest value attached as `_spa_amax`."""
        B, C, H, W = x.shape
        assert C == 16 and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        assert wp.dtype == torch.float16 and tuple(wp.shape) == (2, 2, 5, 64, 8) and wp.is_contiguous()
        assert bias.dtype == torch.float32 and bias.numel() == 32 and bias.is_contiguous()
        if amax_in is None:
            amax_in = self.amax(x)
        y = _out(out, (B, 32, (H + 1) // 2, (W + 1) // 2), torch.float32, x.device)
        am = torch.empty(1, dtype=torch.int32, device=x.device)
        check(self._lib.spa_drn_layer2_f16s(self._ctx, _ptr(x), B, H, W, _ptr(wp), ctypes.c_float(inv_t), _ptr(bias), _ptr(amax_in),
                                            _ptr(am), _ptr(y), self._s()))
        y._spa_amax = am
        return y

    def drn_layer2_f32(self, x, w9, bias):
        """relu(conv3x3(x; 16 -> 32 channels, stride 2, padding 1) + bias) in plain float32 (the strict float32 network);
        w9 (9,16,32) float32 = (tap, input channel, output channel)"""
        B, C, H, W = x.shape
        assert C == 16 and x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        assert w9.dtype == torch.float32 and tuple(w9.shape) == (9, 16, 32) and w9.is_contiguous()
        assert bias.dtype == torch.float32 and bias.numel() == 32 and bias.is_contiguous()
        y = torch.empty((B, 32, (H + 1) // 2, (W + 1) // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        check(self._lib.spa_drn_layer2_f32(self._ctx, _ptr(x), B, H, W, _ptr(w9), _ptr(bias), _ptr(y), self._s()))
        return y

    def conv3x3_s2_f32(self, x, wt, bias, csplit, relu=True, out=None, out2=None):
        """conv3x3_s2_f16s with float32 matrix instructions: wt (Cout,9,Cin) float32 (the projection's rows hold its weights at
        tap 4).  Returns (y, y2 or None)."""
        B, Cin, Hi, Wi = x.shape
        Cout = wt.shape[0]
        assert x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        assert wt.dtype == torch.float32 and wt.is_contiguous() and tuple(wt.shape) == (Cout, 9, Cin)
        assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Cout
        Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
        y = _out(out, (B, csplit, Ho, Wo), torch.float32, x.device)
        y2 = _out(out2, (B, Cout - csplit, Ho, Wo), torch.float32, x.device) if csplit < Cout else None
        check(self._lib.spa_conv3x3_s2_f32(self._ctx, _ptr(x), B, Hi, Wi, Cin, _ptr(wt), Cout, int(csplit), _ptr(bias),
                                           1 if relu else 0, _ptr(y), _ptr(y2), self._s()))
        return y, y2

    @staticmethod
    def small_planes(weight, proj_weight=None):
        """(Cout,Cin,3,3) [+ the block's 1x1 projection (Cp,Cin,1,1)] -> (wp, inv_t) for conv_small_f16s: the MFMA A fragments of
        the two half-precision planes of t * w.  Main tiles [Cout/16][2 planes][steps][64 lanes][8]: lane = (channel n = lane & 15
        of the tile, k group g = lane >> 4); Cin 16: 5 steps, k group (s, g) = tap 2s + g // 2 (tap 9: zero pad), input channels
        8 (g & 1) .. + 7; Cin 32: 9 steps, k group (s, g) = tap s, channels 8 g .. + 7.  Projection tiles [Cp/16][2][64][8]: the
        fragment of the step holding the centre tap (csrc/spa_convs.hip)."""
        Cout, Cin = int(weight.shape[0]), int(weight.shape[1])
        assert tuple(weight.shape[2:]) == (3, 3) and Cin in (16, 32) and Cout % 16 == 0
        w = weight.detach().float()
        amax = float(w.abs().max())
        if proj_weight is not None:
            assert tuple(proj_weight.shape[1:]) == (Cin, 1, 1) and proj_weight.shape[0] % 16 == 0 and Cin == 16
            amax = max(amax, float(proj_weight.detach().float().abs().max()))
        t = 2.0 ** (14 - int(np.floor(np.log2(max(amax, 1e-30)))))
        ws = (w.double() * t).float().reshape(Cout, Cin, 9)
        steps = 5 if Cin == 16 else 9
        frag = torch.zeros((Cout // 16, steps, 64, 8), dtype=torch.float32, device=w.device)
        for s_ in range(steps):
            for g in range(4):
                tap, c0 = (2 * s_ + g // 2, 8 * (g & 1)) if Cin == 16 else (s_, 8 * g)
                if tap > 8:
                    continue
                for ct in range(Cout // 16):
                    frag[ct, s_, g * 16:(g + 1) * 16, :] = ws[ct * 16:(ct + 1) * 16, c0:c0 + 8, tap]
        h = frag.half()
        parts = [torch.stack([h, (frag - h.float()).half()], dim=1).reshape(-1)]          # (tiles, 2, steps, 64, 8)
        if proj_weight is not None:
            Cp = int(proj_weight.shape[0])
            ps = (proj_weight.detach().double() * t).float().reshape(Cp, Cin)
            pf = torch.zeros((Cp // 16, 64, 8), dtype=torch.float32, device=w.device)
            for g in range(2):                                                            # tap 4 = step 2, k groups 0 and 1
                for pt in range(Cp // 16):
                    pf[pt, g * 16:(g + 1) * 16, :] = ps[pt * 16:(pt + 1) * 16, 8 * g:8 * g + 8]
            ph = pf.half()
            parts.append(torch.stack([ph, (pf - ph.float()).half()], dim=1).reshape(-1))  # (tiles, 2, 64, 8)
        return torch.cat(parts).contiguous(), float(1.0 / t)

    def conv_small_f16s(self, x, wp, inv_t, bias, cout, stride=1, n_proj=0, residual=None, relu=True, amax_in=None, out=None, out2=None):
        """relu?(conv3x3(x; Cin 16 | 32 -> cout 16 | 32, stride 1 | 2, padding 1) + bias [+ residual]) on the 16-bit matrix cores
        at float32 accuracy, optionally with the block's 1x1 stride-2 projection as a second output (n_proj = 32).
        -> (y, y2 or None); y carries the device word of its largest value as `_spa_amax`."""
        B, Cin, H, W = x.shape
        assert x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        assert wp.dtype == torch.float16 and wp.is_contiguous() and bias.dtype == torch.float32 and bias.numel() == cout + n_proj
        Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
        if amax_in is None:
            amax_in = self.amax(x)
        y = _out(out, (B, cout, Ho, Wo), torch.float32, x.device)
        y2 = _out(out2, (B, n_proj, Ho, Wo), torch.float32, x.device) if n_proj else None
        if residual is not None:
            assert residual.dtype == torch.float32 and residual.shape == y.shape and residual.is_contiguous(memory_format=torch.channels_last)
        am = torch.empty(1, dtype=torch.int32, device=x.device)
        check(self._lib.spa_conv_small_f16s(self._ctx, _ptr(x), B, H, W, Cin, _ptr(wp), ctypes.c_float(inv_t), int(cout), int(stride),
                                            int(n_proj), _ptr(bias), _ptr(residual), 1 if relu else 0, _ptr(amax_in), _ptr(am),
                                            _ptr(y), _ptr(y2), self._s()))
        y._spa_amax = am
        return y, y2

    def bias_act_(self, y, bias, residual=None, relu=True, track_amax=False):
        """In place y = relu?(y + bias [+ residual]) on a channels-last (B,C,H,W) activation.  track_amax (float32): the
        pass also records the largest magnitude it stores; the device word is attached to y as `_spa_amax`."""
        B, C, H, W = y.shape
        if track_amax and y.dtype == torch.float32:
            am = torch.empty(1, dtype=torch.int32, device=y.device)
            check(self._lib.spa_bias_act_amax(self._ctx, _ptr(y), B * H * W, C, _ptr(bias), _ptr(residual), 1 if relu else 0,
                                              _ptr(am), self._s()))
            y._spa_amax = am
            return y
        check(self._lib.spa_bias_act(self._ctx, _ptr(y), 0 if y.dtype == torch.float32 else 1, B * H * W, C,
                                     _ptr(bias), _ptr(residual), 1 if relu else 0, self._s()))
        return y

    def conv3x3_f32(self, x, wt, bias, residual=None, relu=True, dilation=1, out=None):
        """relu?(conv3x3(x; stride 1, padding = dilation) + bias [+ residual]) on the float32 matrix cores.
        x (B,Cin,H,W) float32 in channels-last storage, wt (Cout,9,Cin) float32, bias (Cout) float32."""
        B, Cin, H, W = x.shape
        Cout = wt.shape[0]
        assert x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        taps = wt.shape[1]
        assert wt.dtype == torch.float32 and wt.is_contiguous() and tuple(wt.shape) == (Cout, taps, Cin) and taps in (1, 9)
        assert bias.dtype == torch.float32 and bias.is_contiguous()
        y = _out(out, (B, Cout, H, W), torch.float32, x.device)
        if residual is not None:
            assert residual.dtype == torch.float32 and residual.shape == y.shape and \
                residual.is_contiguous(memory_format=torch.channels_last)
        if taps == 1:           # (Cout, 1, Cin): the 1x1 projection
            check(self._lib.spa_conv1x1_f32(self._ctx, _ptr(x), B, H, W, Cin, _ptr(wt), Cout, _ptr(bias),
                                            _ptr(residual), 1 if relu else 0, _ptr(y), self._s()))
        else:
            check(self._lib.spa_conv3x3_f32(self._ctx, _ptr(x), B, H, W, Cin, _ptr(wt), Cout, _ptr(bias),
                                            _ptr(residual), 1 if relu else 0, int(dilation), _ptr(y), self._s()))
        return y

    @staticmethod
    def split_planes(wt):
        """(Cout,taps,Cin) float32 -> (wt2, inv_t) for conv3x3_f16s: wt2 (Cout,taps,Cin/32,2,32) float16 = the planes
        h = rn(t w), l = rn(t w - h) of the weights scaled by the power of two t that brings the largest magnitude into
        [2^14, 2^15); inv_t = 1 / t."""
        Cout, taps, Cin = wt.shape
        amax = float(wt.abs().max().clamp_min(1e-30))
        t = 2.0 ** (14 - int(np.floor(np.log2(amax))))
        ws = (wt.double() * t).float()                                        # exact
        h = ws.half()
        l = (ws - h.float()).half()
        wt2 = torch.stack([h.view(Cout, taps, Cin // 32, 32), l.view(Cout, taps, Cin // 32, 32)], dim=3).contiguous()
        return wt2, float(1.0 / t)

    def conv3x3_f16s(self, x, wt2, inv_t, bias, residual=None, relu=True, dilation=1, amax_in=None, track_amax=True, out=None):
        """conv3x3_f32 (3x3 or, with one tap, the 1x1 projection) on the 16-bit matrix cores at float32 accuracy: weights as
        two half-precision planes (split_planes), pixels split in the kernel.  Returns (y, amax of y or None)."""
        B, Cin, H, W = x.shape
        Cout, taps = wt2.shape[0], wt2.shape[1]
        assert x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        assert wt2.dtype == torch.float16 and wt2.is_contiguous() and tuple(wt2.shape) == (Cout, taps, Cin // 32, 2, 32) and taps in (1, 9)
        assert bias.dtype == torch.float32 and bias.is_contiguous()
        y = _out(out, (B, Cout, H, W), torch.float32, x.device)
        if residual is not None:
            assert residual.dtype == torch.float32 and residual.shape == y.shape and \
                residual.is_contiguous(memory_format=torch.channels_last)
        if amax_in is None:
            amax_in = self.amax(x)
        amax_out = torch.empty(1, dtype=torch.int32, device=x.device) if track_amax else None
        if taps == 1:
            # (a 1x1 convolution does not see rows: the image goes in as ONE row of H * W pixels, so the kernel's 128- / 256-pixel
            # tiles are full whatever the width — the same sums per pixel, hence the same bits)
            H, W = 1, H * W
            check(self._lib.spa_conv1x1_f16s(self._ctx, _ptr(x), B, H, W, Cin, _ptr(wt2), ctypes.c_float(inv_t), Cout, _ptr(bias),
                                             _ptr(residual), 1 if relu else 0, _ptr(amax_in), _ptr(amax_out), _ptr(y), self._s()))
        else:
            check(self._lib.spa_conv3x3_f16s(self._ctx, _ptr(x), B, H, W, Cin, _ptr(wt2), ctypes.c_float(inv_t), Cout, _ptr(bias),
                                             _ptr(residual), 1 if relu else 0, int(dilation), _ptr(amax_in), _ptr(amax_out),
                                             _ptr(y), self._s()))
        return y, amax_out

    def conv3x3_s2_f16s(self, x, wt2, inv_t, bias, csplit, relu=True, amax_in=None, out=None, out2=None):
        """3x3 stride-2 padding-1 convolution (+ the block's 1x1 stride-2 projection as output channels csplit..) on the
        16-bit matrix cores at float32 accuracy: one pass over x.  wt2 = split_planes of the (Cout,9,Cin) weights (the
        projection's rows hold its weights at tap 4).  Returns (y, y2 or None, amax of y)."""
        B, Cin, Hi, Wi = x.shape
        Cout = wt2.shape[0]
        assert x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        assert wt2.dtype == torch.float16 and wt2.is_contiguous() and tuple(wt2.shape) == (Cout, 9, Cin // 32, 2, 32)
        assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == Cout
        Ho, Wo = (Hi + 1) // 2, (Wi + 1) // 2
        y = _out(out, (B, csplit, Ho, Wo), torch.float32, x.device)
        y2 = _out(out2, (B, Cout - csplit, Ho, Wo), torch.float32, x.device) if csplit < Cout else None
        if amax_in is None:
            amax_in = self.amax(x)
        amax_out = torch.empty(1, dtype=torch.int32, device=x.device)
        check(self._lib.spa_conv3x3_s2_f16s(self._ctx, _ptr(x), B, Hi, Wi, Cin, _ptr(wt2), ctypes.c_float(inv_t), Cout, int(csplit),
                                            _ptr(bias), 1 if relu else 0, _ptr(amax_in), _ptr(amax_out), _ptr(y), _ptr(y2), self._s()))
        return y, y2, amax_out

    @staticmethod
    def winograd_weights(weight, tile=2):
        """(Cout,Cin,3,3) -> (n*n,Cout,Cin) float32: G g G^T of F(tile x tile, 3x3), computed in float64, position-major.
        tile 2: points 0, 1, -1, inf (n = 4); tile 4: points 0, 1, -1, 1/2, -2, inf (n = 6; csrc/spa_wino.hip)."""
        if tile == 2:
            G, den = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], 1.0
        else:
            # 30 G, an integer matrix, and ONE division by 900 at the end: the thirds and fifteenths of G = (1/2, 0, 0), (1/6, 1/6, 1/6),
            # (1/6, -1/6, 1/6), (16/15, 8/15, 4/15), (1/30, -1/15, 2/15), (0, 0, 1/2) are not float64 numbers, and with them as factors
            # taps that cancel exactly left 1e-15 where U is zero (tests/wino_exact.py, premise (a))
            G, den = [[15, 0, 0], [5, 5, 5], [5, -5, 5], [32, 16, 8], [1, -2, 4], [0, 0, 15]], 900.0
        G = torch.tensor(G, dtype=torch.float64, device=weight.device)
        u = torch.einsum('ij,kcjl,ml->imkc', G, weight.detach().double(), G)
        if den != 1.0:
            u.div_(den)
        return u.reshape(G.shape[0] ** 2, weight.shape[0], weight.shape[1]).float().contiguous()

    def conv3x3_wino_f32(self, x, u, bias, residual=None, relu=True, dilation=1, out=None, scratch=None):
        """relu?(conv3x3(x; stride 1, padding = dilation) + bias [+ residual]) by Winograd F(2x2,3x3) (u of 16
        positions) or F(4x4,3x3) (36 positions) on the float32 matrix cores.  x (B,Cin,H,W) float32 channels-last,
        u = winograd_weights(weight, tile), bias (Cout) float32."""
        B, Cin, H, W = x.shape
        npos, Cout = u.shape[0], u.shape[1]
        assert npos in (16, 36)
        assert x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        assert u.dtype == torch.float32 and u.is_contiguous() and tuple(u.shape) == (npos, Cout, Cin)
        assert bias.dtype == torch.float32 and bias.is_contiguous()
        y = _out(out, (B, Cout, H, W), torch.float32, x.device)
        if residual is not None:
            assert residual.dtype == torch.float32 and residual.shape == y.shape and \
                residual.is_contiguous(memory_format=torch.channels_last)
        tiles, fn = (self._lib.spa_wino_tiles, self._lib.spa_conv3x3_wino_f32) if npos == 16 else \
            (self._lib.spa_wino4_tiles, self._lib.spa_conv3x3_wino4_f32)
        T = int(tiles(B, H, W, int(dilation)))
        v, m = _scratch(scratch, (npos, T, Cin), (npos, T, Cout), x.device)       # per call: stream safe
        check(fn(self._ctx, _ptr(x), B, H, W, Cin, _ptr(u), Cout, _ptr(bias), _ptr(residual),
                 1 if relu else 0, int(dilation), _ptr(v), _ptr(m), _ptr(y), self._s()))
        return y

    @staticmethod
    def winograd_weights_split(weight):
        """(Cout,Cin,3,3) -> (u2, cs) for conv3x3_wino_f16s: u2 (36,Cout,Cin/32,2,32) float16 = the two half-precision
        planes h = rn(t U), l = rn(t U - h) of the F(4x4,3x3) weights U = G g G^T (float64 -> float32) scaled per position by
        the power of two t that brings the largest magnitude into [2^14, 2^15); cs = 36 float32 2^(p_i + p_j) / t_ij
        (csrc/spa_wino.hip)."""
        u = Engine.winograd_weights(weight, 4)                                # (36, Cout, Cin) float32
        Cout, Cin = u.shape[1], u.shape[2]
        amax = u.abs().amax(dim=(1, 2)).double().clamp_min(1e-30)
        t = torch.exp2(14.0 - torch.floor(torch.log2(amax)))                  # per position, exact powers of two
        us = (u.double() * t.view(36, 1, 1)).float()                          # exact
        h = us.half()
        l = (us - h.float()).half()
        u2 = torch.stack([h.view(36, Cout, Cin // 32, 32), l.view(36, Cout, Cin // 32, 32)], dim=3).contiguous()
        p = torch.tensor([4, 4, 4, 3, 3, 4], dtype=torch.float64, device=u.device)
        cs = (torch.exp2(p.view(6, 1) + p.view(1, 6)).reshape(36) / t).float().cpu().numpy().copy()
        return u2, cs

    def amax(self, x):
        """device word with the bit pattern of max |x| (the scale input of conv3x3_wino_f16s)"""
        assert x.dtype == torch.float32 and x.numel() % 4 == 0
        a = torch.empty(1, dtype=torch.int32, device=x.device)
        check(self._lib.spa_amax_f32(self._ctx, _ptr(x), x.numel(), _ptr(a), self._s()))
        return a

    def conv3x3_wino_f16s(self, x, u2, cs, bias, residual=None, relu=True, dilation=1, amax_in=None, track_amax=True, _keep=None,
                          out=None, scratch=None):
        """conv3x3_wino_f32's F(4x4,3x3) with the GEMMs on the 16-bit matrix cores at float32 accuracy (two half-precision
        planes per operand, three products).  (u2, cs) = winograd_weights_split(weight).  Returns (y, amax of y or None);
        amax_in: the amax the producing call returned for x (computed here when None)."""
        B, Cin, H, W = x.shape
        Cout = u2.shape[1]
        assert x.dtype == torch.float32 and x.is_contiguous(memory_format=torch.channels_last)
        assert u2.dtype == torch.float16 and u2.is_contiguous() and tuple(u2.shape) == (36, Cout, Cin // 32, 2, 32)
        assert bias.dtype == torch.float32 and bias.is_contiguous() and cs.dtype == np.float32 and cs.shape == (36,)
        y = _out(out, (B, Cout, H, W), torch.float32, x.device)
        if residual is not None:
            assert residual.dtype == torch.float32 and residual.shape == y.shape and \
                residual.is_contiguous(memory_format=torch.channels_last)
        if amax_in is None:
            amax_in = self.amax(x)
        amax_out = torch.empty(1, dtype=torch.int32, device=x.device) if track_amax else None
        T = int(self._lib.spa_wino4_tiles(B, H, W, int(dilation)))
        v, m = _scratch(scratch, (36, T, Cin), (36, T, Cout), x.device)       # v: two float16 planes = 4 bytes per element
        if _keep is not None:                    # tools / tests: look at the transformed operands
            _keep['v'], _keep['m'] = v, m
        check(self._lib.spa_conv3x3_wino4_f16s(self._ctx, _ptr(x), B, H, W, Cin, _ptr(u2), cs.ctypes.data, Cout, _ptr(bias),
                                               _ptr(residual), 1 if relu else 0, int(dilation), _ptr(amax_in), _ptr(amax_out),
                                               _ptr(v), _ptr(m), _ptr(y), self._s()))
        return y, amax_out

    def conv3x3_bf16(self, x, wt, bias, residual=None, relu=True, dilation=1):
        """relu?(conv3x3(x; stride 1, padding = dilation) + bias [+ residual]) on the bf16 matrix cores.
        x (B,Cin,H,W) bfloat16 in channels-last storage, wt (Cout,9,Cin) bfloat16, bias (Cout) float32."""
        B, Cin, H, W = x.shape
        Cout = wt.shape[0]
        assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
        assert wt.dtype == torch.bfloat16 and wt.is_contiguous() and tuple(wt.shape) == (Cout, 9, Cin)
        assert bias.dtype == torch.float32 and bias.is_contiguous()
        y = torch.empty((B, Cout, H, W), dtype=torch.bfloat16, device=x.device, memory_format=torch.channels_last)
        if residual is not None:
            assert residual.dtype == torch.bfloat16 and residual.shape == y.shape and \
                residual.is_contiguous(memory_format=torch.channels_last)
        check(self._lib.spa_conv3x3_bf16(self._ctx, _ptr(x), B, H, W, Cin, _ptr(wt), Cout, _ptr(bias),
                                         _ptr(residual), 1 if relu else 0, int(dilation), _ptr(y), self._s()))
        return y

    def conv_bf16_light(self, x, wt, bias, residual=None, relu=True, stride=1, dilation=1, out=None):
        """The light layers of the bf16 DRN (models/drn.py:134-151, 195-203) on libspalign's kernel: x (B,Cin,H,W) bf16
        channels-last, wt (Cout,taps,Cin) bf16 with taps 9 (3x3, padding = dilation) or 1 (1x1), stride 1 or 2."""
        B, Cin, H, W = x.shape
        Cout, taps = wt.shape[0], wt.shape[1]
        assert x.dtype == torch.bfloat16 and x.is_contiguous(memory_format=torch.channels_last)
        assert wt.dtype == torch.bfloat16 and wt.is_contiguous() and tuple(wt.shape) == (Cout, taps, Cin) and taps in (1, 9)
        assert bias.dtype == torch.float32 and bias.is_contiguous()
        Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
        y = _out(out, (B, Cout, Ho, Wo), torch.bfloat16, x.device)
        if residual is not None:
            assert residual.dtype == torch.bfloat16 and residual.shape == y.shape and \
                residual.is_contiguous(memory_format=torch.channels_last)
        check(self._lib.spa_conv_bf16_light(self._ctx, _ptr(x), B, H, W, Cin, _ptr(wt), int(taps), int(stride), Cout, _ptr(bias),
                                            _ptr(residual), 1 if relu else 0, int(dilation), _ptr(y), self._s()))
        return y

    def resize_bicubic_u8(self, src, shape):
        """Decoded 8-bit images (B,H,W,C) uint8 -> (B,C,h,w) float32, bicubic exactly as Pillow's 8-bit
        Image.resize(..., BICUBIC) per channel (datasets/resize_image_dataset.py:31-34)."""
        src = _req(src, torch.uint8, 'src')
        B, H, W, C = src.shape
        h, w = int(shape[0]), int(shape[1])
        out = torch.empty((B, C, h, w), dtype=torch.float32, device=src.device)
        check(self._lib.spa_resize_bicubic_u8(self._ctx, _ptr(src), B, H, W, C, h, w, _ptr(out), self._s()))
        return out

    def resize_cvcubic_u8(self, src, shape):
        """Decoded 8-bit images (B,H,W,C) uint8 -> (B,C,h,w) float32 holding the bytes of OpenCV's 8-bit INTER_CUBIC resize
        (the cv2 branch of chainercv.transforms.resize on the uint8 image: what the reference environment ran; not pinned,
        see include/spalign.h)."""
        src = _req(src, torch.uint8, 'src')
        B, H, W, C = src.shape
        h, w = int(shape[0]), int(shape[1])
        out = torch.empty((B, C, h, w), dtype=torch.float32, device=src.device)
        check(self._lib.spa_resize_cvcubic_u8(self._ctx, _ptr(src), B, H, W, C, h, w, _ptr(out), self._s()))
        return out

    def resize_u8(self, src, shape, backend='pil'):
        return self.resize_cvcubic_u8(src, shape) if backend == 'cv2' else self.resize_bicubic_u8(src, shape)

    # ------------------------------------------------------------------ SLIC
    def rgb2lab(self, rgb, ratio=0.1):
        rgb = _req(rgb, torch.float32, 'rgb')
        B, C, H, W = rgb.shape
        assert C == 3
        lab = torch.empty_like(rgb)
        check(self._lib.spa_rgb2lab(self._ctx, _ptr(rgb), B, H, W, ratio, _ptr(lab), self._s()))
        return lab

    def slic_core(self, lab, n_segments, max_iter=10, want_centres=False):
        lab = _req(lab, torch.float32, 'lab')
        B, C, H, W = lab.shape
        assert C == 3
        labels = torch.empty((B, H, W), dtype=torch.int32, device=lab.device)
        centres = None
        if want_centres:
            nC = _lib.make_plan(H, W, n_segments).n_centroids
            centres = torch.empty((B, nC, 6), dtype=torch.float32, device=lab.device)
        check(self._lib.spa_slic_core(self._ctx, _ptr(lab), B, H, W, n_segments, max_iter,
                                      _ptr(labels), _ptr(centres), self._s()))
        return (labels, centres) if want_centres else labels

    def enforce_connectivity(self, labels, min_size, max_size):
        labels = _req(labels, torch.int32, 'labels')
        B, H, W = labels.shape
        out = torch.empty_like(labels)
        n_labels = torch.empty((B,), dtype=torch.int32, device=labels.device)
        check(self._lib.spa_enforce_connectivity(self._ctx, _ptr(labels), B, H, W, min_size, max_size,
                                                 _ptr(out), _ptr(n_labels), self._s()))
        return out, n_labels

    def slic(self, rgb, n_segments, compactness=10.0, max_iter=10):
        """slic(img, n_segments) for a batch: (B,3,H,W) f32 0..255 -> labels (B,H,W) i32, n_labels (B)."""
        rgb = _req(rgb, torch.float32, 'rgb')
        B, C, H, W = rgb.shape
        assert C == 3
        labels = torch.empty((B, H, W), dtype=torch.int32, device=rgb.device)
        n_labels = torch.empty((B,), dtype=torch.int32, device=rgb.device)
        check(self._lib.spa_slic(self._ctx, _ptr(rgb), B, H, W, n_segments, compactness, max_iter,
                                 _ptr(labels), _ptr(n_labels), self._s()))
        return labels, n_labels

    def slic_u8(self, rgb, n_segments, compactness=10.0, max_iter=10):
        """slic(uint8 image, n_segments) as superpixel_overlaps.py:303 calls it: scikit-image's float64 core.
        rgb (B,3,H,W) f32 holding the uint8 values -> labels (B,H,W) i32, n_labels (B)."""
        rgb = _req(rgb, torch.float32, 'rgb')
        B, C, H, W = rgb.shape
        assert C == 3
        labels = torch.empty((B, H, W), dtype=torch.int32, device=rgb.device)
        n_labels = torch.empty((B,), dtype=torch.int32, device=rgb.device)
        check(self._lib.spa_slic_u8(self._ctx, _ptr(rgb), B, H, W, n_segments, float(compactness), max_iter,
                                    _ptr(labels), _ptr(n_labels), self._s()))
        return labels, n_labels

    def rgb2lab_u8_f64(self, rgb, compactness=10.0):
        """rgb2lab(img_as_float(uint8 image)) * (1/compactness), float64 planar (B,3,H,W)."""
        rgb = _req(rgb, torch.float32, 'rgb')
        B, C, H, W = rgb.shape
        lab = torch.empty((B, 3, H, W), dtype=torch.float64, device=rgb.device)
        check(self._lib.spa_rgb2lab_u8_f64(self._ctx, _ptr(rgb), B, H, W, 1.0 / float(compactness), _ptr(lab), self._s()))
        return lab

    def slic_core_f64(self, lab, n_segments, max_iter=10, want_centres=False):
        """_slic_cython[double] on a scaled float64 Lab image (B,3,H,W) -> labels (B,H,W) i32 [, centres (B,nC,6)]."""
        lab = _req(lab, torch.float64, 'lab')
        B, C, H, W = lab.shape
        labels = torch.empty((B, H, W), dtype=torch.int32, device=lab.device)
        cen = None
        if want_centres:
            cen = torch.empty((B, _lib.make_plan(H, W, n_segments).n_centroids, 6), dtype=torch.float64, device=lab.device)
        check(self._lib.spa_slic_core_f64(self._ctx, _ptr(lab), B, H, W, n_segments, max_iter, _ptr(labels),
                                          _ptr(cen), self._s()))
        return (labels, cen) if want_centres else labels

    def felzenszwalb(self, rgb, scale=300.0, sigma=0.8, min_size=20, uint8_image=False, out=None):
        """felzenszwalb(img/255, scale, sigma, min_size) for a batch -> labels (B,H,W) i32, n_labels (B).
        uint8_image: the reference passed a uint8 image, so /255. happens in float64
        (superpixel_overlaps.py:294-300) instead of float32 (batch_spalign_kmeans.py:301-307).
        out: (labels, n_labels) tensors of the caller's to write into."""
        rgb = _req(rgb, torch.float32, 'rgb')
        B, C, H, W = rgb.shape
        assert C == 3
        if out is not None:
            labels, n_labels = _req(out[0], torch.int32, 'labels'), _req(out[1], torch.int32, 'n_labels')
            assert labels.shape == (B, H, W) and n_labels.shape == (B,)
        else:
            labels = torch.empty((B, H, W), dtype=torch.int32, device=rgb.device)
            n_labels = torch.empty((B,), dtype=torch.int32, device=rgb.device)
        fn = self._lib.spa_felzenszwalb_u8 if uint8_image else self._lib.spa_felzenszwalb
        check(fn(self._ctx, _ptr(rgb), B, H, W, scale, sigma, min_size, _ptr(labels), _ptr(n_labels), self._s()))
        return labels, n_labels

    def overlap_refine(self, labels, road, max_labels, threshold):
        """superpixel_overlaps.py:353-361 -> refined (B,H,W) u8 (1 = road)."""
        labels = _req(labels, torch.int32, 'labels')
        road = _req(road, torch.uint8, 'road')
        B = labels.shape[0]
        npix = labels[0].numel()
        assert road.shape == labels.shape
        out = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
        check(self._lib.spa_overlap_refine(self._ctx, _ptr(labels), _ptr(road), B, npix, int(max_labels),
                                           float(threshold), _ptr(out), self._s()))
        return out

    # ------------------------------------------------------------------ descriptors
    def segment_offsets(self, n_labels):
        n_labels = _req(n_labels, torch.int32, 'n_labels')
        B = n_labels.numel()
        off = torch.empty((B + 1,), dtype=torch.int32, device=n_labels.device)
        check(self._lib.spa_segment_offsets(self._ctx, _ptr(n_labels), B, _ptr(off), self._s()))
        return off

    def segment_stats(self, labels, offsets, ncap, prior_params=None, want_centroid=True):
        """-> count (ncap) i32, centroid (ncap,2) f64 or None, prior (ncap) f64 or None."""
        labels = _req(labels, torch.int32, 'labels')
        offsets = _req(offsets, torch.int32, 'offsets')
        B, H, W = labels.shape
        dev = labels.device
        count = torch.empty((ncap,), dtype=torch.int32, device=dev)
        centroid = torch.zeros((ncap, 2), dtype=torch.float64, device=dev) if want_centroid else None
        prior = torch.zeros((ncap,), dtype=torch.float64, device=dev) if prior_params else None
        yp, xp, ys, xs = prior_params if prior_params else (0.75, 0.5, 0.1, 0.1)
        check(self._lib.spa_segment_stats(self._ctx, _ptr(labels), B, H, W, _ptr(offsets), ncap,
                                          yp, xp, ys, xs, _ptr(count), _ptr(centroid), _ptr(prior),
                                          self._s()))
        return count, centroid, prior

    # device-resident CPython `random` stream (random.seed(1111) of the reference's module scope)
    def pyrandom_seed(self, seed=1111):
        check(self._lib.spa_pyrandom_dev_seed(self._ctx, int(seed), self._s()))

    def pyrandom_generate(self, want):
        """Make `want` outputs of the stream available (asynchronous on the current stream)."""
        check(self._lib.spa_pyrandom_dev_generate(self._ctx, int(want), self._s()))

    def anchor_ranks(self, count, n_ptr, ncap, n_anchors, total_pixels):
        """random.shuffle(pixel list)[:n_anchors] of every superpixel, on the device:
        -> ranks (ncap, n_anchors) int32 (raster rank of the chosen pixels), n_valid (ncap) int32."""
        count = _req(count, torch.int32, 'count')
        ranks = torch.empty((ncap, n_anchors), dtype=torch.int32, device=count.device)
        n_valid = torch.zeros((ncap,), dtype=torch.int32, device=count.device)
        check(self._lib.spa_anchor_ranks_dev(self._ctx, _ptr(count), _ptr(n_ptr), ncap, n_anchors, int(total_pixels),
                                             _ptr(ranks), _ptr(n_valid), self._s()))
        return ranks, n_valid

    def select_anchor_pixels(self, labels, offsets, ncap, ranks, n_valid):
        labels = _req(labels, torch.int32, 'labels')
        ranks = _req(ranks, torch.int32, 'ranks')
        n_valid = _req(n_valid, torch.int32, 'n_valid')
        B, H, W = labels.shape
        A = ranks.shape[1]
        anchors = torch.zeros((ncap, A, 2), dtype=torch.int32, device=labels.device)
        check(self._lib.spa_select_anchor_pixels(self._ctx, _ptr(labels), B, H, W, _ptr(offsets), ncap,
                                                 _ptr(ranks), _ptr(n_valid), A, _ptr(anchors),
                                                 self._s()))
        return anchors

    @staticmethod
    def fmap_desc(fmap):
        """fmap: (B, C, fh, fw) tensor in channels_last memory format (float32 or bfloat16)."""
        if fmap.dtype not in (torch.float32, torch.bfloat16):
            raise SpalignError('feature map dtype must be float32 or bfloat16')
        B, C, fh, fw = fmap.shape
        sb, sc, sy, sx = fmap.stride()
        return FmapDesc(C, fh, fw, sb, sc, sy, sx, 0 if fmap.dtype == torch.float32 else 1)

    @staticmethod
    def as_channels_last(fmap):
        """NCHW-shaped tensor stored NHWC; a no-op for the DRN module of this package."""
        if fmap.stride(1) == 1 and fmap.is_contiguous(memory_format=torch.channels_last):
            return fmap
        return fmap.contiguous(memory_format=torch.channels_last)

    def _new_x(self, ncap, C, append_pos, x_dtype, dev):
        D = C + (2 if append_pos else 0)
        return torch.zeros((ncap, D), dtype=x_dtype, device=dev), D

    def pool_anchor(self, fmap, img_h, offsets, ncap, anchors, n_valid, n_neighbors=4,
                    centroid=None, append_pos=True):
        fmap = self.as_channels_last(fmap)
        d = self.fmap_desc(fmap)
        B = fmap.shape[0]
        x_dtype = torch.float64 if append_pos else torch.float32
        X, D = self._new_x(ncap, d.C, append_pos, x_dtype, fmap.device)
        A = anchors.shape[1]
        check(self._lib.spa_pool_anchor(self._ctx, _ptr(fmap), ctypes.byref(d), B, img_h,
                                        _ptr(offsets), ncap, _ptr(anchors), _ptr(n_valid), A,
                                        n_neighbors, _ptr(centroid), 1 if append_pos else 0, _ptr(X),
                                        1 if append_pos else 0, D, self._s()))
        return X

    def pool_mean(self, fmap, labels, offsets, ncap, count, sampling='nearest', centroid=None,
                  append_pos=True):
        fmap = self.as_channels_last(fmap)
        d = self.fmap_desc(fmap)
        B, H, W = labels.shape
        x_dtype = torch.float64 if append_pos else torch.float32
        X, D = self._new_x(ncap, d.C, append_pos, x_dtype, fmap.device)
        check(self._lib.spa_pool_mean(self._ctx, _ptr(fmap), ctypes.byref(d), _ptr(labels), B, H, W,
                                      _ptr(offsets), ncap, _ptr(count),
                                      {'nearest': 0, 'bilinear': 1}[sampling], _ptr(centroid),
                                      1 if append_pos else 0, _ptr(X), 1 if append_pos else 0, D,
                                      self._s()))
        return X

    # ------------------------------------------------------------------ k-means + paint
    def kmeans(self, X, w, n_ptr, k, max_iter=1000, init_other=None, gate=None):
        """-> assign (ncap) i32, info (4) i32 {iterations, status, N, -} (both on the device).
        gate: device int32 word — the launch runs only if it holds a positive number (outputs stay zero otherwise)."""
        if X.dtype not in (torch.float32, torch.float64) or not X.is_contiguous():
            raise SpalignError('X must be contiguous float32/float64')
        w = _req(w, torch.float64, 'weights')
        ncap, D = X.shape
        assign = torch.zeros((ncap,), dtype=torch.int32, device=X.device)
        info = torch.zeros((4,), dtype=torch.int32, device=X.device)
        check(self._lib.spa_kmeans_weighted_gated(self._ctx, _ptr(X), 0 if X.dtype == torch.float32 else 1,
                                                  D, D, _ptr(w), _ptr(n_ptr), ncap, k, max_iter,
                                                  _ptr(init_other), _ptr(gate), _ptr(assign), _ptr(info), self._s()))
        return assign, info

    def retry_update(self, assign, offsets, B, counters, gate=None):
        """Retry bookkeeping of one k-means run on the device (spa_kmeans_retry_update): counters (2) int32 = [pending, made]."""
        check(self._lib.spa_kmeans_retry_update(self._ctx, _ptr(assign), _ptr(offsets), int(B), _ptr(gate), _ptr(counters[0:1]),
                                                _ptr(counters[1:2]), None, self._s()))

    NP_INIT_MAX = 65536          # csrc/spa_nprng.hip: the index vector lives in LDS, one byte per point

    def np_kmeans_init(self, state, w, n_ptr, k, gate=None):
        """The k > 2 initial assignment (batch_spalign_kmeans.py:141-149) drawn on the device from numpy's stream.
        state: (628,) int32 device tensor holding the generator (NpRandom.state() uploaded once; advanced in place);
        -> init_other (ncap) int64 for kmeans().  gate as in kmeans(): nothing is drawn unless it is positive."""
        w = _req(w, torch.float64, 'weights')
        ncap = w.shape[0]
        assert state.dtype == torch.int32 and state.numel() == 628 and state.is_contiguous() and ncap <= self.NP_INIT_MAX
        init = torch.zeros((ncap,), dtype=torch.int64, device=w.device)
        check(self._lib.spa_np_kmeans_init_dev(self._ctx, _ptr(state), _ptr(w), _ptr(n_ptr), ncap, k, _ptr(gate), _ptr(init),
                                               None, self._s()))
        return init

    def paint(self, labels, assign, offsets):
        labels = _req(labels, torch.int32, 'labels')
        B, H, W = labels.shape
        cluster = torch.empty((B, H, W), dtype=torch.uint8, device=labels.device)
        road = torch.empty((B, H, W), dtype=torch.uint8, device=labels.device)
        check(self._lib.spa_paint(self._ctx, _ptr(labels), _ptr(assign), _ptr(offsets), B, H, W,
                                  _ptr(cluster), _ptr(road), self._s()))
        return cluster, road

    # ------------------------------------------------------------------ SegNet-Basic (labels_from_segnet.py)
    LAYOUT_NHWC, LAYOUT_NCHW = 0, 1

    @classmethod
    def _layout(cls, x):
        """Storage of a (B,C,H,W) float32 / uint8 tensor: plain contiguous -> planar, channels-last -> NHWC."""
        if x.is_contiguous():
            return cls.LAYOUT_NCHW
        if x.is_contiguous(memory_format=torch.channels_last):
            return cls.LAYOUT_NHWC
        raise SpalignError('segnet: the input is neither contiguous nor channels-last')

    def segnet_encode(self, x, wt, bias, mean=None, std=None):
        """One encoder stage, maxpool2x2_argmax(relu(conv7x7(x) + bias)): x (B,3,H,W) float32 planar image 0..255
        (conv1: standardised with mean / std and LRN-normalised in the load; wt (49,64,4)) or (B,64,H,W) channels-last
        (wt (49,64,64)) -> (pooled (B,64,H/2,W/2) float32, idx (B,64,H/2,W/2) uint8), both channels-last."""
        return self._segnet_encode(self._lib.spa_segnet_encode, x, wt, bias, mean, std)

    def segnet_encode_bf16(self, x, wt, bias, mean=None, std=None):
        """segnet_encode on the bf16 matrix cores: the same float32 arguments and outputs, every product operand
        rounded to bf16 (round to nearest even), float32 accumulation and epilogue."""
        return self._segnet_encode(self._lib.spa_segnet_encode_bf16, x, wt, bias, mean, std)

    def segnet_encode_f16x3(self, x, wt, bias, mean=None, std=None):
        """segnet_encode at float32 accuracy on the f16 matrix cores: the same float32 arguments and outputs, every
        operand as two scaled half-precision planes (one scale per image), three products per float32 product."""
        return self._segnet_encode(self._lib.spa_segnet_encode_f16x3, x, wt, bias, mean, std)

    def _segnet_encode(self, fn, x, wt, bias, mean, std):
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
        B, C, H, W = x.shape
        _req(wt, torch.float32, 'wt')
        _req(bias, torch.float32, 'bias')
        pooled = torch.empty((B, 64, H // 2, W // 2), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        idx = torch.empty((B, 64, H // 2, W // 2), dtype=torch.uint8, device=x.device, memory_format=torch.channels_last)
        m = (ctypes.c_float * 3)(*mean) if mean is not None else None
        s = (ctypes.c_float * 3)(*std) if std is not None else None
        check(fn(self._ctx, _ptr(x), self._layout(x), B, H, W, C, _ptr(wt), _ptr(bias), m, s, _ptr(pooled), _ptr(idx),
                 self._s()))
        return pooled, idx

    def segnet_decode(self, x, idx, wt, bias, wc=None, bc=None, logits=False, out=None):
        """One decoder stage, conv7x7(unpool(x, idx)) + bias: x (B,64,h,w) float32 and idx (B,64,h,w) uint8
        channels-last -> (B,64,2h,2w) float32 channels-last; with the classifier wc (2,64), bc (2) (decode1): softmax
        probabilities (B,2,2h,2w) float32 planar, or with logits=True the classifier's two sums before the softmax
        (spa_segnet_decode_logits; wc and bc required).  out: the caller's (B,2,2h,2w) buffer for a classifier form."""
        return self._segnet_decode('spa_segnet_decode%s', x, idx, wt, bias, wc, bc, logits, out)

    def segnet_decode_bf16(self, x, idx, wt, bias, wc=None, bc=None, logits=False, out=None):
        """segnet_decode on the bf16 matrix cores: the same float32 arguments and outputs, every product operand
        rounded to bf16 (round to nearest even), float32 accumulation, bias, classifier and softmax."""
        return self._segnet_decode('spa_segnet_decode%s_bf16', x, idx, wt, bias, wc, bc, logits, out)

    def segnet_decode_f16x3(self, x, idx, wt, bias, wc=None, bc=None, logits=False, out=None):
        """segnet_decode at float32 accuracy on the f16 matrix cores: the same float32 arguments and outputs, every
        operand as two scaled half-precision planes (one scale per image), float32 bias, classifier and softmax."""
        return self._segnet_decode('spa_segnet_decode%s_f16x3', x, idx, wt, bias, wc, bc, logits, out)

    def _segnet_decode(self, name, x, idx, wt, bias, wc, bc, logits=False, out=None):
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and idx.dtype == torch.uint8
        B, C, h, w = x.shape
        assert C == 64 and tuple(idx.shape) == tuple(x.shape)
        _req(wt, torch.float32, 'wt')
        _req(bias, torch.float32, 'bias')
        if logits and (wc is None or bc is None):
            raise SpalignError('segnet_decode: logits=True needs the classifier wc and bc')
        fn = getattr(self._lib, name % ('_logits' if logits else ''))
        if wc is None:
            if out is not None:
                raise SpalignError('segnet_decode: out is for the classifier forms only')
            y = torch.empty((B, 64, 2 * h, 2 * w), dtype=torch.float32, device=x.device, memory_format=torch.channels_last)
        else:
            _req(wc, torch.float32, 'wc')
            _req(bc, torch.float32, 'bc')
            y = out if out is not None else torch.empty((B, 2, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
            if tuple(_req(y, torch.float32, 'out').shape) != (B, 2, 2 * h, 2 * w):
                raise SpalignError('segnet_decode: out must be %s float32' % ((B, 2, 2 * h, 2 * w),))
        layout = self._layout(x)
        if self._layout(idx) != layout:
            raise SpalignError('segnet_decode: x and idx have different layouts')
        check(fn(self._ctx, _ptr(x), _ptr(idx), layout, B, h, w, _ptr(wt), _ptr(bias), _ptr(wc), _ptr(bc), _ptr(y),
                 self._s()))
        return y

    def segnet_score(self, prob, shape, want_scores=False):
        """prob (B,2,h,w) float32 -> (mask (B,H,W) uint8, scores (B,2,H,W) float32 or None): Pillow's BILINEAR upscale
        of each channel to shape = (H, W), then the argmax (ties: class 0)."""
        prob = _req(prob, torch.float32, 'prob')
        B, C, h, w = prob.shape
        assert C == 2
        H, W = int(shape[0]), int(shape[1])
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=prob.device)
        sc = torch.empty((B, 2, H, W), dtype=torch.float32, device=prob.device) if want_scores else None
        check(self._lib.spa_segnet_score(self._ctx, _ptr(prob), B, h, w, H, W, _ptr(mask), _ptr(sc), self._s()))
        return mask, sc

    def segnet_label_eval(self, prob, shape, label_ids=None, want_scores=False):
        """segnet_score and, with label_ids (B,H,W) uint8 (the raw labelIds bytes), the confusion of the mask against
        segnet.label_mask(label_ids), in one launch -> (mask (B,H,W) uint8, scores (B,2,H,W) float32 or None, counts
        (B,4) int64 {TN, FP, FN, TP} or None).  mask and scores have segnet_score's bits, counts are
        confusion(mask, label_mask(ids))."""
        prob = _req(prob, torch.float32, 'prob')
        B, C, h, w = prob.shape
        assert C == 2
        H, W = int(shape[0]), int(shape[1])
        counts = None
        if label_ids is not None:
            label_ids = _req(label_ids, torch.uint8, 'label_ids')
            if tuple(label_ids.shape) != (B, H, W):
                raise SpalignError('segnet_label_eval: label_ids must be %s uint8, got %s'
                                   % ((B, H, W), tuple(label_ids.shape)))
            counts = torch.empty((B, 4), dtype=torch.int64, device=prob.device)
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=prob.device)
        sc = torch.empty((B, 2, H, W), dtype=torch.float32, device=prob.device) if want_scores else None
        check(self._lib.spa_segnet_label_eval(self._ctx, _ptr(prob), B, h, w, H, W, _ptr(label_ids), _ptr(mask),
                                              _ptr(sc), _ptr(counts), self._s()))
        return mask, sc, counts

    def segnet_overlay(self, score, frames, color=(128, 64, 128), alpha=0.5, out_mask=None, out_blended=None):
        """segnet_score's mask of score (B,2,h,w) float32 at the frames' size and utils/create_movie.py's blend of the
        road colour into frames (B,H,W,3) uint8, in one launch -> (mask (B,H,W) uint8, blended (B,H,W,3) uint8): where
        the mask is 1 a channel is uint8(alpha * color[c] + (1 - alpha) * v) as numpy computes it (demovideo.blend_host),
        elsewhere the frame's byte.  frames may be any view with contiguous (H,W,3) images packed one after the other;
        out_mask / out_blended: the caller's buffers."""
        score = _req(score, torch.float32, 'score')
        frames = _req(frames, torch.uint8, 'frames')
        B, C, h, w = score.shape
        if C != 2 or frames.dim() != 4 or frames.shape[0] != B or frames.shape[3] != 3:
            raise SpalignError('segnet_overlay: score must be (B,2,h,w) and frames (B,H,W,3), got %s and %s'
                               % (tuple(score.shape), tuple(frames.shape)))
        H, W = int(frames.shape[1]), int(frames.shape[2])
        color = [int(v) for v in color]
        if len(color) != 3 or min(color) < 0 or max(color) > 255:
            raise SpalignError('segnet_overlay: color must be three values 0..255, got %r' % (color,))
        mask = out_mask if out_mask is not None else torch.empty((B, H, W), dtype=torch.uint8, device=score.device)
        blended = out_blended if out_blended is not None else torch.empty_like(frames)
        if tuple(_req(mask, torch.uint8, 'out_mask').shape) != (B, H, W) or \
                tuple(_req(blended, torch.uint8, 'out_blended').shape) != (B, H, W, 3):
            raise SpalignError('segnet_overlay: out_mask must be %s and out_blended %s uint8' % ((B, H, W), (B, H, W, 3)))
        check(self._lib.spa_segnet_overlay(self._ctx, _ptr(score), B, h, w, H, W, _ptr(frames),
                                           (ctypes.c_uint8 * 3)(*color), float(alpha), _ptr(mask), _ptr(blended),
                                           self._s()))
        return mask, blended

    # ---- SegNet-Basic training input stage (segnet_loader.py): get_example's arithmetic on decoded batches
    def _input_tables(self, kind, n_in, n_out, backend):
        """Device tables of one axis, uploaded once per (kind, n_in, n_out, backend): 'cubic' -> (bounds, taps, ksize)
        of segnet_train.pil_bicubic_coeffs or _cv_cubic_float_taps, 'nearest' -> segnet_train.nearest_index_table."""
        from . import segnet_train as st
        cache = self._in_tables
        key = (kind, int(n_in), int(n_out), backend)
        if key not in cache:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            if kind == 'nearest':
                cache[key] = up(st.nearest_index_table(n_in, n_out, backend))
            elif backend == 'cv2':
                idx, taps = st._cv_cubic_float_taps(n_in, n_out)
                assert ((idx >= 0) & (idx < n_in)).all()
                cache[key] = (up(idx.astype(np.int32)), up(taps.astype(np.float32)), 4)
            else:
                bounds, taps = st.pil_bicubic_coeffs(n_in, n_out)
                cache[key] = (up(bounds), up(taps), int(taps.shape[1]))
        return cache[key]

    @staticmethod
    def _input_backend(backend):
        if backend is None:
            from . import cli
            backend = cli.RESIZE_BACKEND[0]
        if backend not in ('pil', 'cv2'):
            raise SpalignError("resize backend must be 'pil' or 'cv2', got %r" % (backend,))
        return backend

    def _flip(self, flip, B):
        if flip is None:
            return None
        flip = _req(flip, torch.uint8, 'flip')
        if tuple(flip.shape) != (B,):
            raise SpalignError('flip must be (B,) uint8, got %s' % (tuple(flip.shape),))
        return flip

    @staticmethod
    def _input_out(out, shape, dtype, device):
        """the output of an input-stage wrapper: a new tensor, or the caller's (tests hand in poisoned buffers)"""
        if out is None:
            return torch.empty(shape, dtype=dtype, device=device)
        _req(out, dtype, 'out')
        if tuple(out.shape) != tuple(shape):
            raise SpalignError('out must be %s, got %s' % (tuple(shape), tuple(out.shape)))
        return out

    def _segnet_train_input(self, fn, src, B, H, W, shape, shift, flip, backend, out):
        """segnet_train_input and segnet_train_input_ptrs below: src is the batch or the table of its addresses"""
        B, H, W = int(B), int(H), int(W)
        h, w = int(shape[0]), int(shape[1])
        backend = self._input_backend(backend)
        if shift is not None:
            shift = _req(shift, torch.float64, 'shift')
            if tuple(shift.shape) != (B, 3):
                raise SpalignError('shift must be (B,3) float64, got %s' % (tuple(shift.shape),))
        flip = self._flip(flip, B)
        out = self._input_out(out, (B, 3, h, w), torch.float32, self.device if src is None else src.device)
        xb = xk = yb = yk = tmp = None
        ksx = ksy = 0
        if (H, W) != (h, w) and B > 0:
            cv = backend == 'cv2'
            if cv or W != w:
                xb, xk, ksx = self._input_tables('cubic', W, w, backend)
            if cv or H != h:
                yb, yk, ksy = self._input_tables('cubic', H, h, backend)
            if xb is not None and yb is not None:
                tmp = torch.empty((B, 3, H, w), dtype=torch.float32, device=out.device)
        check(fn(self._ctx, _ptr(src), B, H, W, h, w, 1 if backend == 'cv2' else 0, _ptr(xb), _ptr(xk), ksx, _ptr(yb),
                 _ptr(yk), ksy, _ptr(shift), _ptr(flip), _ptr(tmp), _ptr(out), self._s()))
        return out

    def segnet_train_input(self, src, shape, shift=None, flip=None, backend=None, out=None):
        """Decoded frames (B,H,W,3) uint8 -> the training images (B,3,h,w) float32 0..255 with the bits of
        ZippedEstimatedCityscapesDataset.get_example: each channel resized as a float image (Pillow's mode 'F' BICUBIC,
        or with backend 'cv2' resize_bicubic_float's OpenCV form; backend None: cli.RESIZE_BACKEND), then shift (B,3)
        float64 (pca_lighting_shift of each image's draw) added as numpy's float32 += float64, then the images with
        flip (B,) uint8 != 0 mirrored.  Equal sizes: widened only.  out: the caller's (B,3,h,w) float32 tensor."""
        src = _req(src, torch.uint8, 'src')
        if src.dim() != 4 or src.shape[3] != 3:
            raise SpalignError('segnet_train_input: src must be (B,H,W,3) uint8, got %s' % (tuple(src.shape),))
        B, H, W, _ = src.shape
        return self._segnet_train_input(self._lib.spa_segnet_train_input, src, B, H, W, shape, shift, flip, backend,
                                        out)

    @staticmethod
    def _address_table(table, B):
        """a _ptrs wrapper's table: (B,) int64 device addresses; None is handed on as NULL (the library refuses it)"""
        if table is not None:
            _req(table, torch.int64, 'table')
            if tuple(table.shape) != (int(B),):
                raise SpalignError('table must be (B,) int64 device addresses, got %s' % (tuple(table.shape),))
        return table

    def segnet_train_input_ptrs(self, table, B, src_shape, shape, shift=None, flip=None, backend=None, out=None):
        """segnet_train_input over frames that lie anywhere in device memory: table (B,) int64 on the device, the
        address of every example's decoded frame (H,W,3) uint8, src_shape = (H, W).  The addresses need no alignment
        and may repeat; whoever builds the table keeps the frames alive until the launch has run.  Same bits."""
        table = self._address_table(table, B)
        return self._segnet_train_input(self._lib.spa_segnet_train_input_ptrs, table, B, src_shape[0], src_shape[1],
                                        shape, shift, flip, backend, out)

    def _segnet_train_label(self, fn, src, is_float, B, C, H, W, lead, shape, flip, backend, out):
        B, C, H, W = int(B), int(C), int(H), int(W)
        h, w = int(shape[0]), int(shape[1])
        backend = self._input_backend(backend)
        flip = self._flip(flip, B)
        yi = self._input_tables('nearest', H, h, backend)
        xi = self._input_tables('nearest', W, w, backend)
        out = self._input_out(out, tuple(lead) + (h, w), torch.float32 if is_float else torch.int32,
                              self.device if src is None else src.device)
        check(fn(self._ctx, _ptr(src), is_float, B, C, H, W, h, w, _ptr(yi), _ptr(xi), _ptr(flip), _ptr(out),
                 self._s()))
        return out

    def segnet_train_label(self, src, shape, flip=None, backend=None, out=None):
        """The labels of the same examples: uint8 masks (B,H,W) -> int32 (B,h,w), or float32 scores (B,C,H,W) ->
        float32 (B,C,h,w), resized as resize_nearest_label does (Pillow's NEAREST, or cli.resize_nearest with backend
        'cv2') and mirrored where flip (B,) uint8 != 0.  out: the caller's tensor of that shape and dtype."""
        if src.dtype == torch.uint8 and src.dim() == 3:
            src = _req(src, torch.uint8, 'src')
            is_float, C = 0, 1
        elif src.dtype == torch.float32 and src.dim() == 4:
            src = _req(src, torch.float32, 'src')
            is_float, C = 1, int(src.shape[1])
        else:
            raise SpalignError('segnet_train_label: src must be (B,H,W) uint8 or (B,C,H,W) float32')
        B, (H, W) = src.shape[0], src.shape[-2:]
        return self._segnet_train_label(self._lib.spa_segnet_train_label, src, is_float, B, C, H, W, src.shape[:-2],
                                        shape, flip, backend, out)

    def segnet_train_label_ptrs(self, table, B, src_shape, dtype, shape, flip=None, backend=None, out=None):
        """segnet_train_label over label arrays that lie anywhere in device memory: table (B,) int64 on the device,
        the address of every example's array; src_shape (H,W) with dtype uint8 (masks -> int32 (B,h,w)) or (C,H,W)
        with dtype float32 (scores -> float32 (B,C,h,w)).  The addresses need no alignment and may repeat."""
        src_shape = tuple(int(v) for v in src_shape)
        dtype = np.dtype(dtype)
        if dtype == np.uint8 and len(src_shape) == 2:
            is_float, C, lead = 0, 1, (int(B),)
        elif dtype == np.float32 and len(src_shape) == 3:
            is_float, C, lead = 1, src_shape[0], (int(B), src_shape[0])
        else:
            raise SpalignError('segnet_train_label_ptrs: the arrays must be (H,W) uint8 or (C,H,W) float32')
        table = self._address_table(table, B)
        return self._segnet_train_label(self._lib.spa_segnet_train_label_ptrs, table, is_float, B, C, src_shape[-2],
                                        src_shape[-1], lead, shape, flip, backend, out)

    # ---- SegNet-Basic training (segnet_train.py).  Maps are (B,H,W,64) contiguous tensors (channels-last storage);
    # conv1's input is the planar (B,3,H,W) float32 image 0..255.
    def _train_input(self, x, idx):
        """-> (layout, Cin, H, W at the convolution's resolution) of a training input form (see spalign.h)."""
        if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
            raise SpalignError('segnet_train: x must be a contiguous (B,3,H,W) or (B,H,W,64) float32 CUDA tensor')
        if idx is not None:
            _req(idx, torch.uint8, 'idx')
            if x.shape[3] != 64 or tuple(idx.shape) != tuple(x.shape):
                raise SpalignError('segnet_train: the decoder input and its index map must both be (B,h,w,64)')
            return self.LAYOUT_NHWC, 64, 2 * x.shape[1], 2 * x.shape[2]
        if x.shape[1] == 3:
            return self.LAYOUT_NCHW, 3, x.shape[2], x.shape[3]
        if x.shape[3] != 64:
            raise SpalignError('segnet_train: x must be (B,3,H,W) or (B,H,W,64), got %s' % (tuple(x.shape),))
        return self.LAYOUT_NHWC, 64, x.shape[1], x.shape[2]

    def segnet_train_forward(self, x, wt, idx=None, mean=None, std=None, stats=True, out=None):
        """y = conv7x7(x; wt), no bias, at full resolution: x the planar image (conv1, wt (49,64,4), standardised with
        mean / std and LRN-normalised in the load), a (B,H,W,64) map, or a decoder's (B,H/2,W/2,64) input with its
        index map idx.  -> (y (B,H,W,64) float32, (sum y, sum y^2) (2,64) float64 or None)."""
        return self._segnet_train_forward(self._lib.spa_segnet_train_forward, x, wt, idx, mean, std, stats, out)

    def segnet_train_forward_bf16(self, x, wt, idx=None, mean=None, std=None, stats=True, out=None):
        """segnet_train_forward on the bf16 matrix cores: the same float32 arguments and outputs, every product
        operand rounded to bf16 (round to nearest even), float32 accumulation."""
        return self._segnet_train_forward(self._lib.spa_segnet_train_forward_bf16, x, wt, idx, mean, std, stats, out)

    def segnet_train_forward_f16x3(self, x, wt, idx=None, mean=None, std=None, stats=True, out=None):
        """segnet_train_forward at float32 accuracy on the f16 matrix cores: the same float32 arguments and outputs,
        every operand split into two scaled half-precision planes, three products per float32 product."""
        return self._segnet_train_forward(self._lib.spa_segnet_train_forward_f16x3, x, wt, idx, mean, std, stats, out)

    def _segnet_train_forward(self, fn, x, wt, idx, mean, std, stats, out):
        layout, cin, H, W = self._train_input(x, idx)
        _req(wt, torch.float32, 'wt')
        B = x.shape[0]
        y = out if out is not None else torch.empty((B, H, W, 64), dtype=torch.float32, device=x.device)
        _req(y, torch.float32, 'out')
        st = torch.empty((2, 64), dtype=torch.float64, device=x.device) if stats else None
        m = (ctypes.c_float * 3)(*mean) if mean is not None else None
        s = (ctypes.c_float * 3)(*std) if std is not None else None
        check(fn(self._ctx, _ptr(x), _ptr(idx), layout, B, H, W, cin, _ptr(wt), m, s, _ptr(y), _ptr(st), self._s()))
        return y, st

    def segnet_train_dgrad(self, dy, wt, idx=None, out=None):
        """The input gradient of a 64-channel layer: dy (B,H,W,64), wt (49,64,64) the forward weight.  idx None ->
        (B,H,W,64); idx (B,H/2,W/2,64) (decoder layers) -> the gradient at the pooled input (B,H/2,W/2,64)."""
        return self._segnet_train_dgrad(self._lib.spa_segnet_train_dgrad, dy, wt, idx, out)

    def segnet_train_dgrad_bf16(self, dy, wt, idx=None, out=None):
        """segnet_train_dgrad with dy and the weight rounded to bf16, float32 accumulation."""
        return self._segnet_train_dgrad(self._lib.spa_segnet_train_dgrad_bf16, dy, wt, idx, out)

    def segnet_train_dgrad_f16x3(self, dy, wt, idx=None, out=None):
        """segnet_train_dgrad at float32 accuracy: dy and the weight as split planes on the f16 matrix cores."""
        return self._segnet_train_dgrad(self._lib.spa_segnet_train_dgrad_f16x3, dy, wt, idx, out)

    def _segnet_train_dgrad(self, fn, dy, wt, idx, out):
        dy = _req(dy, torch.float32, 'dy')
        _req(wt, torch.float32, 'wt')
        B, H, W, C = dy.shape
        if idx is not None:
            _req(idx, torch.uint8, 'idx')
            shape = (B, H // 2, W // 2, 64)
            if tuple(idx.shape) != shape:
                raise SpalignError('segnet_train_dgrad: idx must be %s, got %s' % (shape, tuple(idx.shape)))
        else:
            shape = (B, H, W, 64)
        dx = out if out is not None else torch.empty(shape, dtype=torch.float32, device=dy.device)
        _req(dx, torch.float32, 'out')
        check(fn(self._ctx, _ptr(dy), _ptr(wt), _ptr(idx), B, H, W, _ptr(dx), self._s()))
        return dx

    def segnet_train_wgrad(self, dy, x, idx=None, mean=None, std=None, out=None):
        """dw (49,64,Cp) = the weight gradient of conv7x7 for the output gradient dy (B,H,W,64) and the layer's input
        form (x, idx) as segnet_train_forward takes it (Cp 4 for conv1, channel 3 zero)."""
        return self._segnet_train_wgrad(self._lib.spa_segnet_train_wgrad, dy, x, idx, mean, std, out)

    def segnet_train_wgrad_bf16(self, dy, x, idx=None, mean=None, std=None, out=None):
        """segnet_train_wgrad with dy and the input form rounded to bf16, float32 accumulation."""
        return self._segnet_train_wgrad(self._lib.spa_segnet_train_wgrad_bf16, dy, x, idx, mean, std, out)

    def segnet_train_wgrad_f16x3(self, dy, x, idx=None, mean=None, std=None, out=None):
        """segnet_train_wgrad at float32 accuracy: dy and the input form as split planes on the f16 matrix cores."""
        return self._segnet_train_wgrad(self._lib.spa_segnet_train_wgrad_f16x3, dy, x, idx, mean, std, out)

    def _segnet_train_wgrad(self, fn, dy, x, idx, mean, std, out):
        dy = _req(dy, torch.float32, 'dy')
        layout, cin, H, W = self._train_input(x, idx)
        B = x.shape[0]
        if tuple(dy.shape) != (B, H, W, 64):
            raise SpalignError('segnet_train_wgrad: dy must be %s, got %s' % ((B, H, W, 64), tuple(dy.shape)))
        dw = out if out is not None else torch.empty((49, 64, 4 if cin == 3 else 64), dtype=torch.float32,
                                                     device=dy.device)
        _req(dw, torch.float32, 'out')
        m = (ctypes.c_float * 3)(*mean) if mean is not None else None
        s = (ctypes.c_float * 3)(*std) if std is not None else None
        check(fn(self._ctx, _ptr(dy), _ptr(x), _ptr(idx), layout, B, H, W, cin, m, s, _ptr(dw), self._s()))
        return dw

    # ---- SegNet-Basic training between the convolutions (SegNetTrainer(fused_bn=True); csrc/spa_segnet_train_bn.hip).
    # y is the layer's (B,H,W,64) convolution output; mean, rstd, gamma, beta are (64) float32.  The encoder forms take
    # the (B,H/2,W/2,64) pooled map p, its index map idx and the gradient g at the pooled map, the decoder forms the
    # full-resolution gradient g alone.
    @staticmethod
    def _bn_map(y, what='y'):
        _req(y, torch.float32, what)
        if y.dim() != 4 or y.shape[3] != 64 or y.shape[1] % 2 or y.shape[2] % 2 or y.numel() == 0:
            raise SpalignError('segnet_train_bn: %s must be (B,H,W,64) with even H, W, got %s' % (what, tuple(y.shape)))
        return tuple(y.shape)

    @staticmethod
    def _bn_vectors(**vectors):
        for name, v in vectors.items():
            _req(v, torch.float32, name)
            if tuple(v.shape) != (64,):
                raise SpalignError('segnet_train_bn: %s must be (64,), got %s' % (name, tuple(v.shape)))

    @staticmethod
    def _bn_out(out, shape, dtype, device, what='out'):
        if out is None:
            return torch.empty(shape, dtype=dtype, device=device)
        _req(out, dtype, what)
        if tuple(out.shape) != tuple(shape):
            raise SpalignError('segnet_train_bn: %s must be %s, got %s' % (what, tuple(shape), tuple(out.shape)))
        return out

    def _bn_gradient(self, g, idx, p, y):
        """checks the gradient form (g, idx, p) of a backward call against y -> (B, H, W)"""
        B, H, W, _ = self._bn_map(y)
        _req(g, torch.float32, 'g')
        if (idx is None) != (p is None):
            raise SpalignError('segnet_train_bn: idx and p come together (the encoder form) or not at all')
        shape = (B, H, W, 64) if idx is None else (B, H // 2, W // 2, 64)
        if tuple(g.shape) != shape:
            raise SpalignError('segnet_train_bn: g must be %s, got %s' % (shape, tuple(g.shape)))
        if idx is not None:
            _req(idx, torch.uint8, 'idx')
            _req(p, torch.float32, 'p')
            if tuple(idx.shape) != shape or tuple(p.shape) != shape:
                raise SpalignError('segnet_train_bn: idx and p must be %s, got %s and %s'
                                   % (shape, tuple(idx.shape), tuple(p.shape)))
        return B, H, W

    def segnet_train_bn_forward(self, y, mean, rstd, gamma, beta, pool=False, out=None, out_idx=None):
        """o = (y - mean) * (rstd * gamma) + beta.  pool False (decoder): -> o (B,H,W,64).  pool True (encoder): ->
        (the 2x2 maximum of relu(o) (B,H/2,W/2,64), the uint8 index ky*2+kx of its first maximum)."""
        B, H, W, _ = self._bn_map(y)
        self._bn_vectors(mean=mean, rstd=rstd, gamma=gamma, beta=beta)
        if not pool:
            if out_idx is not None:
                raise SpalignError('segnet_train_bn_forward: out_idx belongs to pool=True')
            o = self._bn_out(out, (B, H, W, 64), torch.float32, y.device)
            idx = None
        else:
            o = self._bn_out(out, (B, H // 2, W // 2, 64), torch.float32, y.device)
            idx = self._bn_out(out_idx, (B, H // 2, W // 2, 64), torch.uint8, y.device, 'out_idx')
        check(self._lib.spa_segnet_train_bn_forward(self._ctx, _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta),
                                                    B, H, W, _ptr(o), _ptr(idx), self._s()))
        return (o, idx) if pool else o

    def segnet_train_bn_backward_sums(self, g, y, mean, rstd, idx=None, p=None, out=None):
        """-> (2,64) float64: (sum g, sum g * xhat) over (B,H,W), xhat = (y - mean) * rstd, g in either form."""
        B, H, W = self._bn_gradient(g, idx, p, y)
        self._bn_vectors(mean=mean, rstd=rstd)
        s = self._bn_out(out, (2, 64), torch.float64, y.device)
        check(self._lib.spa_segnet_train_bn_backward_sums(self._ctx, _ptr(g), _ptr(idx), _ptr(p), _ptr(y), _ptr(mean),
                                                          _ptr(rstd), B, H, W, _ptr(s), self._s()))
        return s

    def segnet_train_bn_backward_dy(self, g, y, mean, rstd, gamma, sums, m, idx=None, p=None, out=None):
        """-> dy (B,H,W,64) = (gamma * rstd / m) * (m * g - sums[0] - xhat * sums[1]); sums (2,64) float64 on the
        device (segnet_train_bn_backward_sums, summed over the ranks in a data-parallel step), m the pixel count."""
        B, H, W = self._bn_gradient(g, idx, p, y)
        self._bn_vectors(mean=mean, rstd=rstd, gamma=gamma)
        _req(sums, torch.float64, 'sums')
        if tuple(sums.shape) != (2, 64) or not float(m) >= 1.0:
            raise SpalignError('segnet_train_bn_backward_dy: sums must be (2,64) and m >= 1')
        dy = self._bn_out(out, (B, H, W, 64), torch.float32, y.device)
        check(self._lib.spa_segnet_train_bn_backward_dy(self._ctx, _ptr(g), _ptr(idx), _ptr(p), _ptr(y), _ptr(mean),
                                                        _ptr(rstd), _ptr(gamma), _ptr(sums), float(m), B, H, W,
                                                        _ptr(dy), self._s()))
        return dy

    def segnet_train_classifier_forward(self, h, wc, bc, out=None):
        """score (B,H,W,2) = h (B,H,W,64) * wc (2,64)^T + bc (2)."""
        B, H, W, _ = self._bn_map(h, 'h')
        _req(wc, torch.float32, 'wc')
        _req(bc, torch.float32, 'bc')
        if tuple(wc.shape) != (2, 64) or tuple(bc.shape) != (2,):
            raise SpalignError('segnet_train_classifier_forward: wc must be (2,64) and bc (2,)')
        score = self._bn_out(out, (B, H, W, 2), torch.float32, h.device)
        check(self._lib.spa_segnet_train_classifier_forward(self._ctx, _ptr(h), _ptr(wc), _ptr(bc), B, H, W,
                                                            _ptr(score), self._s()))
        return score

    def segnet_train_classifier_backward(self, dscore, h, wc, out=None, out_dw=None, out_db=None):
        """-> (dh (B,H,W,64) = dscore * wc, dwc (2,64), db (2)) for dscore (B,H,W,2)."""
        B, H, W, _ = self._bn_map(h, 'h')
        _req(dscore, torch.float32, 'dscore')
        _req(wc, torch.float32, 'wc')
        if tuple(dscore.shape) != (B, H, W, 2) or tuple(wc.shape) != (2, 64):
            raise SpalignError('segnet_train_classifier_backward: dscore must be %s and wc (2,64)' % ((B, H, W, 2),))
        dh = self._bn_out(out, (B, H, W, 64), torch.float32, h.device)
        dw = self._bn_out(out_dw, (2, 64), torch.float32, h.device, 'out_dw')
        db = self._bn_out(out_db, (2,), torch.float32, h.device, 'out_db')
        check(self._lib.spa_segnet_train_classifier_backward(self._ctx, _ptr(dscore), _ptr(h), _ptr(wc), B, H, W,
                                                             _ptr(dh), _ptr(dw), _ptr(db), self._s()))
        return dh, dw, db

    def confusion(self, road, gt):
        """road (B,H,W) u8, gt (B,H,W) i32 in {-1,0,1} -> (B,4) i64 {TN, FP, FN, TP}."""
        road = _req(road, torch.uint8, 'road')
        gt = _req(gt, torch.int32, 'gt')
        B = road.shape[0]
        out = torch.zeros((B, 4), dtype=torch.int64, device=road.device)
        check(self._lib.spa_confusion(self._ctx, _ptr(road), _ptr(gt), B, road[0].numel(), _ptr(out),
                                      self._s()))
        return out

    # ---- label PNGs (png.py)
    def png_deflate(self, src, out_shape=None, out=None, nbytes=None, adler=None):
        """src (B,Hs,Ws) uint8 -> (out (B,stride) uint8, nbytes (B) int32, adler (B) int32), all on the device: row b of
        out begins with the raw deflate stream of image b's label PNG (nbytes[b] bytes; nothing at or past them is
        written) and adler[b] holds the bits of the Adler-32 of its filtered scanlines; png.assemble makes the file.
        out_shape (Ho, Wo): the image is first resized as cv.INTER_NEAREST does it (png.nearest_tables), inside the
        encoder's loads.  out / nbytes / adler: the caller's buffers (stride >= spa_png_deflate_bound(Ho, Wo));
        without them the engine's own, which the next call without them overwrites."""
        from . import png
        src = _req(src, torch.uint8, 'src')
        if src.dim() != 3:
            raise SpalignError('png_deflate: src must be (B,Hs,Ws) uint8, got %s' % (tuple(src.shape),))
        B, Hs, Ws = (int(v) for v in src.shape)
        Ho, Wo = (Hs, Ws) if out_shape is None else (int(out_shape[0]), int(out_shape[1]))
        rows = cols = None
        if (Ho, Wo) != (Hs, Ws):
            key = ('png', Hs, Ws, Ho, Wo)
            if key not in self._in_tables:
                if min(Hs, Ws, Ho, Wo) <= 0:
                    raise SpalignError('png_deflate: %s -> %s' % ((Hs, Ws), (Ho, Wo)))
                self._in_tables[key] = tuple(torch.from_numpy(t.astype(np.int32)).to(self.device)
                                             for t in png.nearest_tables((Hs, Ws), (Ho, Wo)))
            rows, cols = self._in_tables[key]
        out, (nbytes, adler), stride = self._stream_out(
            'png_deflate', B, int(self._lib.spa_png_deflate_bound(Ho, Wo)), 'spa_png_deflate_bound(%d, %d)' % (Ho, Wo),
            out, (('nbytes', nbytes), ('adler', adler)))
        check(self._lib.spa_png_deflate_u8(self._ctx, _ptr(src), B, Hs, Ws, _ptr(rows), _ptr(cols), Ho, Wo, _ptr(out),
                                           stride, _ptr(nbytes), _ptr(adler), self._s()))
        return out, nbytes, adler

    def _stream_out(self, name, B, bound, bound_name, out, meta):
        """What png_deflate and jpeg_encode share: the caller's out (B,stride) uint8 and int32 meta vectors (B), checked,
        or, where one is None, the engine's own for `name`: allocated once, overwritten by the next call without.
        bound: the bytes a row must hold; meta: ((what, tensor or None), ...) -> (out, the meta vectors, the row stride
        to pass down)."""
        own = self._stream_own.setdefault(name, {})
        if out is None:
            stride = max((bound + 15) // 16 * 16, 16)
            if 'out' not in own or own['out'].shape[0] < B or own['out'].shape[1] < stride:
                own['out'] = torch.empty((B, stride), dtype=torch.uint8, device=self.device)
            out = own['out'][:B]
        if any(t is None for _, t in meta):
            if 'meta' not in own or own['meta'].shape[1] < B:
                own['meta'] = torch.empty((len(meta), B), dtype=torch.int32, device=self.device)
            meta = [(what, own['meta'][i, :B] if t is None else t) for i, (what, t) in enumerate(meta)]
        if not (out.is_cuda and out.dtype == torch.uint8 and out.dim() == 2 and out.shape[0] == B and out.stride(1) == 1):
            raise SpalignError('%s: out must be a (B,stride) uint8 CUDA tensor with contiguous rows' % name)
        if out.shape[1] < bound:
            raise SpalignError('%s: a row of out holds %d bytes, %s is %d' % (name, out.shape[1], bound_name, bound))
        for what, t in meta:
            if tuple(_req(t, torch.int32, what).shape) != (B,):
                raise SpalignError('%s: %s must be (%d,) int32' % (name, what, B))
        # (a one-row tensor's stride(0) need not be its row length, and nothing steps over it)
        return out, [t for _, t in meta], int(out.stride(0)) if B > 1 else int(out.shape[1])

    # ---- JPEG frames (jpeg.py)
    def jpeg_encode(self, rgb, Ri=None, out=None, nbytes=None, coef=None):
        """rgb (B,H,W,3) uint8, H and W multiples of 16 -> (out (B,stride) uint8, nbytes (B) int32) on the device: row
        b of out begins with the entropy-coded scan of frame b's JPEG in restart intervals of Ri MCUs (nbytes[b]
        bytes; nothing at or past them is written); jpeg.assemble makes the file.  out / nbytes / coef: the caller's
        buffers (stride >= spa_jpeg_scan_bound(H, W, Ri); coef at least B * H * W * 3 / 2 int16, the workspace of the
        quantised coefficients); without them the engine's own, which the next call without them overwrites."""
        from . import jpeg
        rgb = _req(rgb, torch.uint8, 'rgb')
        if rgb.dim() != 4 or rgb.shape[3] != 3:
            raise SpalignError('jpeg_encode: rgb must be (B,H,W,3) uint8, got %s' % (tuple(rgb.shape),))
        B, H, W = (int(v) for v in rgb.shape[:3])
        Ri = jpeg.DEFAULT_RI if Ri is None else int(Ri)
        bound = int(self._lib.spa_jpeg_scan_bound(H, W, Ri))
        if B <= 0 or bound <= 0:
            raise SpalignError('jpeg_encode: %d frames of %d x %d (multiples of 16) with a restart interval of %d MCUs'
                               % (B, H, W, Ri))
        out, (nbytes,), stride = self._stream_out('jpeg_encode', B, bound, 'spa_jpeg_scan_bound(%d, %d, %d)' % (H, W, Ri),
                                                  out, (('nbytes', nbytes),))
        n_coef = B * H * W * 3 // 2
        if coef is None:
            own = getattr(self, '_jpeg_coef', None)
            if own is None or own.numel() < n_coef:
                own = self._jpeg_coef = torch.empty((n_coef,), dtype=torch.int16, device=self.device)
            coef = own
        if _req(coef, torch.int16, 'coef').numel() < n_coef:
            raise SpalignError('jpeg_encode: coef must hold %d int16' % n_coef)
        check(self._lib.spa_jpeg_encode_rgb8(self._ctx, _ptr(rgb), B, H, W, Ri, _ptr(coef), _ptr(out), stride,
                                             _ptr(nbytes), self._s()))
        return out, nbytes

    # ---- overview figures (figure.py)
    def figure_compose(self, frames, planes, luts, modes, layout, decimate=4, gap=16, out=None):
        """The overview figures of a batch (spa_figure_compose_u8) -> the canvas (B,Hc,Wc,3) uint8 on the device.
        frames (B,H,W,3) uint8 or None; planes: 1..4 index planes (B,H,W) uint8 (they may be one tensor several times);
        luts: per panel a (256,3) uint8 colour table on the device; modes: per panel 0 (the table's colour) or 1 (that
        colour at 0.4 over frames); layout (rows, columns).  figure.compose_host restates the bytes and
        figure.canvas_shape the canvas.  out: the caller's canvas; without it the engine's own, which the next call
        without it overwrites."""
        planes, luts, modes = list(planes), list(luts), [int(m) for m in modes]
        P = len(planes)
        if not (1 <= P <= 4 and len(luts) == P and len(modes) == P):
            raise SpalignError('figure_compose: 1..4 panels, each a plane, a table and a mode (got %d, %d, %d)'
                               % (P, len(luts), len(modes)))
        shape = tuple(_req(planes[0], torch.uint8, 'planes[0]').shape)
        if len(shape) != 3 or min(shape) <= 0:
            raise SpalignError('figure_compose: a plane must be (B,H,W) uint8, got %s' % (shape,))
        for p in range(P):
            if tuple(_req(planes[p], torch.uint8, 'planes[%d]' % p).shape) != shape:
                raise SpalignError('figure_compose: planes[%d] is %s, planes[0] %s' % (p, tuple(planes[p].shape), shape))
            if tuple(_req(luts[p], torch.uint8, 'luts[%d]' % p).shape) != (256, 3):
                raise SpalignError('figure_compose: luts[%d] must be (256,3) uint8' % p)
            if modes[p] not in (0, 1):
                raise SpalignError('figure_compose: modes[%d] must be 0 or 1, got %d' % (p, modes[p]))
        B, H, W = shape
        if frames is not None and tuple(_req(frames, torch.uint8, 'frames').shape) != (B, H, W, 3):
            raise SpalignError('figure_compose: frames must be %s uint8, got %s' % ((B, H, W, 3), tuple(frames.shape)))
        if frames is None and any(modes):
            raise SpalignError('figure_compose: a blended panel needs frames')
        R, C = (int(v) for v in layout)
        d, g = int(decimate), int(gap)
        hc, wc = ctypes.c_int32(0), ctypes.c_int32(0)
        if R < 1 or C < 1 or R * C < P or self._lib.spa_figure_canvas_shape(H, W, R, C, d, g, ctypes.byref(hc),
                                                                            ctypes.byref(wc)) != _lib.SPA_OK:
            raise SpalignError('figure_compose: %d panels in a %d x %d layout, decimation %d (1..16), gap %d (0..64)'
                               % (P, R, C, d, g))
        Hc, Wc = hc.value, wc.value
        if out is None:
            own = getattr(self, '_figure_out', None)
            if own is None or own.numel() < B * Hc * Wc * 3:
                own = self._figure_out = torch.empty((B * Hc * Wc * 3,), dtype=torch.uint8, device=self.device)
            out = own[:B * Hc * Wc * 3].view(B, Hc, Wc, 3)
        if tuple(_req(out, torch.uint8, 'out').shape) != (B, Hc, Wc, 3):
            raise SpalignError('figure_compose: out must be %s uint8, got %s' % ((B, Hc, Wc, 3), tuple(out.shape)))
        check(self._lib.spa_figure_compose_u8(self._ctx, _ptr(frames), B, H, W, P,
                                              (ctypes.c_void_p * P)(*[t.data_ptr() for t in planes]),
                                              (ctypes.c_void_p * P)(*[t.data_ptr() for t in luts]),
                                              (ctypes.c_int32 * P)(*modes), R, C, d, g, _ptr(out), Hc, Wc, self._s()))
        return out


_DEFAULT = None


def default_engine():
    """Process-wide Engine (one spa_ctx per process/GPU)."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Engine()
    return _DEFAULT


class PyRandom(object):
    """CPython `random` stream (random.seed(1111); random.shuffle), host side."""

    def __init__(self, seed=1111):
        self._lib = _lib.lib()
        h = ctypes.c_void_p()
        check(self._lib.spa_pyrandom_create(seed, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        try:
            self._lib.spa_pyrandom_destroy(self._h)
        except Exception:
            pass

    def shuffle_select(self, counts, n_anchors):
        """counts: int32 numpy (N,) -> ranks (N, n_anchors) int32, n_valid (N,) int32."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        N = counts.size
        ranks = np.zeros((N, n_anchors), np.int32)
        n_valid = np.zeros((N,), np.int32)
        check(self._lib.spa_pyrandom_shuffle_select_host(
            self._h, counts.ctypes.data_as(ctypes.c_void_p), N, n_anchors,
            ranks.ctypes.data_as(ctypes.c_void_p), n_valid.ctypes.data_as(ctypes.c_void_p)))
        return ranks, n_valid


class NpRandom(object):
    """numpy legacy global RandomState stream (np.random.seed(1111); np.random.shuffle)."""

    def __init__(self, seed=1111):
        self._lib = _lib.lib()
        h = ctypes.c_void_p()
        check(self._lib.spa_nprandom_create(seed, ctypes.byref(h)))
        self._h = h

    def __del__(self):
        try:
            self._lib.spa_nprandom_destroy(self._h)
        except Exception:
            pass

    def shuffle(self, a):
        assert a.dtype == np.int64 and a.flags.c_contiguous
        check(self._lib.spa_nprandom_shuffle_host(self._h, a.ctypes.data_as(ctypes.c_void_p), a.size))
        return a

    def state(self):
        """numpy's rk_state as it stands: (628,) uint32 = 624 state words, the position in the current block, padding —
        what Engine.np_kmeans_init keeps in device memory."""
        out = np.zeros(628, np.uint32)
        check(self._lib.spa_nprandom_state(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def set_state(self, state628):
        """continue from a state taken with state() (or downloaded from the device copy np_kmeans_init advances)"""
        a = np.ascontiguousarray(state628, dtype=np.uint32)
        assert a.size == 628
        check(self._lib.spa_nprandom_set_state(self._h, a.ctypes.data_as(ctypes.c_void_p)))
