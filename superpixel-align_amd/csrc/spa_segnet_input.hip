// Input stage of SegNet-Basic training on the GPU (train_segnet.py --loader_procs): what
// segnet_train.ZippedEstimatedCityscapesDataset.get_example computes on the host from a decoded frame, same bits.
//
//   image   uint8 (B,H,W,3) interleaved (a decoded PNG) -> float32 (B,3,h,w) planar, 0..255:
//             widen, resize each channel as a FLOAT image (Pillow's mode 'F' BICUBIC, or OpenCV's float INTER_CUBIC as
//             segnet_train.resize_bicubic_float restates it), add the per-image lighting shift, flip.
//   label   uint8 (B,C,H,W) masks -> int32, or float32 (B,C,H,W) scores -> float32, (B,C,h,w): nearest resize through
//             index tables, flip.
//
// Pillow (src/libImaging/Resample.c, ImagingResampleHorizontal_32bpc / Vertical_32bpc): per output sample a double
// that starts at 0 accumulates (double)pixel * k[x] in tap order and is stored as float32; the horizontal pass runs
// first and the vertical pass reads its float32 results; a pass whose size does not change is not run.  The taps are
// the normalised float64 coefficients of precompute_coeffs, built on the host (segnet_train.pil_bicubic_coeffs) and
// handed in as device tables: bounds (n_out, 2) {first tap, tap count}, k (n_out, ksize) doubles.  __dmul_rn and
// __dadd_rn keep the product and the sum two roundings (no fma), as spa_segnet_score does for BILINEAR.
//
// The OpenCV form: four float32 taps per axis at clamped indices (segnet_train._cv_cubic_float_taps), a float32 sum
// from 0 in tap order of float32 products, horizontal pass first, both passes always run.
//
// The lighting shift is numpy's `float32 array += float64 array`: (float)((double)v + shift), one rounding.
// One thread owns one output pixel of one pass (its three channels); no atomics, no host synchronisation.
#include "spa_common.h"

// the sample (b, c, y, x) of the pass's source: the decoded bytes, or the float32 planes of the pass before
template <bool U8> struct InSrc;
template <> struct InSrc<true> {
    const uint8_t *p; int H, W;
    __device__ __forceinline__ float at(int b, int c, int y, int x) const
    { return (float)p[(((long long)b * H + y) * W + x) * 3 + c]; }
};
template <> struct InSrc<false> {
    const float *p; int H, W;
    __device__ __forceinline__ float at(int b, int c, int y, int x) const
    { return p[(((long long)b * 3 + c) * H + y) * W + x]; }
};

// the last pass's store: shift (B,3) doubles or NULL, flip (B) bytes or NULL; out (B,3,h,w)
__device__ __forceinline__ void in_store(float v, int b, int c, int y, int x, int h, int w, const double *shift,
                                         const uint8_t *flip, float *out)
{
    if (shift) v = (float)__dadd_rn((double)v, shift[b * 3 + c]);
    if (flip && flip[b]) x = w - 1 - x;
    out[(((long long)b * 3 + c) * h + y) * w + x] = v;
}

// One pass along X (AXIS 0) or Y (AXIS 1): src (.., H, W) -> (.., oh, ow) with oh == H (AXIS 0) or ow == W (AXIS 1).
// CV false: bounds (n_out, 2), taps (n_out, ksize) double.  CV true: bounds (n_out, 4) clamped indices, taps (n_out, 4)
// float.  LAST: the store applies shift and flip; otherwise plain planar float32.
template <int AXIS, bool U8, bool CV, bool LAST>
__global__ __launch_bounds__(256) void k_in_pass(InSrc<U8> src, int oh, int ow, const int32_t *__restrict__ bounds,
                                                 const void *__restrict__ taps, int ksize,
                                                 const double *__restrict__ shift, const uint8_t *__restrict__ flip,
                                                 float *__restrict__ out)
{
    const int b = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= ow) return;
    const int o = AXIS == 0 ? x : y;
    float r[3];
    if (CV) {
        const int32_t *idx = bounds + o * 4;
        const float *k = (const float *)taps + o * 4;
        float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sy = AXIS == 0 ? y : idx[t], sx = AXIS == 0 ? idx[t] : x;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(src.at(b, c, sy, sx), k[t]));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = acc[c];
    } else {
        const int first = bounds[o * 2], n = bounds[o * 2 + 1];
        const double *k = (const double *)taps + (long long)o * ksize;
        double acc[3] = {0.0, 0.0, 0.0};
        for (int t = 0; t < n; ++t) {
            const int sy = AXIS == 0 ? y : first + t, sx = AXIS == 0 ? first + t : x;
            const double kt = k[t];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __dadd_rn(acc[c], __dmul_rn((double)src.at(b, c, sy, sx), kt));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = (float)acc[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (LAST) in_store(r[c], b, c, y, x, oh, ow, shift, flip, out);
        else out[(((long long)b * 3 + c) * oh + y) * ow + x] = r[c];
    }
}

// equal sizes: the image is widened only (then shifted and flipped)
__global__ __launch_bounds__(256) void k_in_widen(InSrc<true> src, const double *__restrict__ shift,
                                                  const uint8_t *__restrict__ flip, float *__restrict__ out)
{
    const int b = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= src.W) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) in_store(src.at(b, c, y, x), b, c, y, x, src.H, src.W, shift, flip, out);
}

template <int AXIS, bool U8, bool CV, bool LAST>
static void in_launch(hipStream_t s, InSrc<U8> src, int B, int oh, int ow, const int32_t *bounds, const void *taps,
                      int ksize, const double *shift, const uint8_t *flip, float *out)
{
    hipLaunchKernelGGL((k_in_pass<AXIS, U8, CV, LAST>), dim3((ow + 255) / 256, oh, B), dim3(256), 0, s, src, oh, ow,
                       bounds, taps, ksize, shift, flip, out);
}

extern "C" int spa_segnet_train_input(spa_ctx *ctx, const uint8_t *src, int32_t B, int32_t H, int32_t W, int32_t h,
                                      int32_t w, int32_t backend, const int32_t *xb, const void *xk, int32_t ksx,
                                      const int32_t *yb, const void *yk, int32_t ksy, const double *shift,
                                      const uint8_t *flip, float *tmp, float *out, void *stream)
{
    SPA_ARG(ctx && src && out && B > 0 && H > 0 && W > 0 && h > 0 && w > 0);
    SPA_ARG(B < 65536 && H < 65536 && h < 65536);
    SPA_ARG(backend == 0 || backend == 1);
    hipStream_t s = spa_stream(stream);
    const InSrc<true> in{src, H, W};
    if (H == h && W == w) {
        hipLaunchKernelGGL(k_in_widen, dim3((W + 255) / 256, H, B), dim3(256), 0, s, in, shift, flip, out);
        SPA_LAUNCH_CHECK();
        return SPA_OK;
    }
    const bool cv = backend == 1;
    const bool do_x = cv || W != w, do_y = cv || H != h;
    SPA_ARG(!do_x || (xb && xk && (cv || ksx > 0)));
    SPA_ARG(!do_y || (yb && yk && (cv || ksy > 0)));
    SPA_ARG(!(do_x && do_y) || tmp);
    if (do_x && do_y) {
        const InSrc<false> mid{tmp, H, w};
        if (cv) {
            in_launch<0, true, true, false>(s, in, B, H, w, xb, xk, 4, nullptr, nullptr, tmp);
            in_launch<1, false, true, true>(s, mid, B, h, w, yb, yk, 4, shift, flip, out);
        } else {
            in_launch<0, true, false, false>(s, in, B, H, w, xb, xk, ksx, nullptr, nullptr, tmp);
            in_launch<1, false, false, true>(s, mid, B, h, w, yb, yk, ksy, shift, flip, out);
        }
    } else if (do_x) {
        in_launch<0, true, false, true>(s, in, B, h, w, xb, xk, ksx, shift, flip, out);
    } else {
        in_launch<1, true, false, true>(s, in, B, h, w, yb, yk, ksy, shift, flip, out);
    }
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

// labels: out[b, c, y, x'] = (To)src[b, c, yi[y], xi[x]], x' = x or w - 1 - x.  Planes = B * C.
template <typename Ti, typename To>
__global__ __launch_bounds__(256) void k_in_label(const Ti *__restrict__ src, int C, int H, int W, int h, int w,
                                                  const int32_t *__restrict__ yi, const int32_t *__restrict__ xi,
                                                  const uint8_t *__restrict__ flip, To *__restrict__ out)
{
    const int p = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const Ti v = src[((long long)p * H + yi[y]) * W + xi[x]];
    const int xo = (flip && flip[p / C]) ? w - 1 - x : x;
    out[((long long)p * h + y) * w + xo] = (To)v;
}

extern "C" int spa_segnet_train_label(spa_ctx *ctx, const void *src, int32_t is_float, int32_t B, int32_t C, int32_t H,
                                      int32_t W, int32_t h, int32_t w, const int32_t *yi, const int32_t *xi,
                                      const uint8_t *flip, void *out, void *stream)
{
    SPA_ARG(ctx && src && out && yi && xi && B > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0);
    SPA_ARG((long long)B * C < 65536 && h < 65536);
    hipStream_t s = spa_stream(stream);
    const dim3 grid((w + 255) / 256, h, B * C);
    if (is_float)
        hipLaunchKernelGGL((k_in_label<float, float>), grid, dim3(256), 0, s, (const float *)src, C, H, W, h, w, yi, xi,
                           flip, (float *)out);
    else
        hipLaunchKernelGGL((k_in_label<uint8_t, int32_t>), grid, dim3(256), 0, s, (const uint8_t *)src, C, H, W, h, w, yi,
                           xi, flip, (int32_t *)out);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
