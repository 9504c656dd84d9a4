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

// the sample (b, c, y, x) of the pass's source: the float32 planes of the pass before (IN_F32), the decoded bytes of
// one contiguous batch (IN_U8), or the decoded bytes of B frames wherever they lie (IN_U8_PTRS: a device table of B
// addresses, the _ptrs entry points).  The accessor is all that differs between the entry points.
enum { IN_F32 = 0, IN_U8 = 1, IN_U8_PTRS = 2 };
template <int KIND> struct InSrc;
template <> struct InSrc<IN_U8> {
    const uint8_t *p; int H, W;
    __device__ __forceinline__ float at(int b, int c, int y, int x) const
    { return (float)p[(((long long)b * H + y) * W + x) * 3 + c]; }
};
template <> struct InSrc<IN_U8_PTRS> {
    const uint8_t *const *p; int H, W;
    __device__ __forceinline__ float at(int b, int c, int y, int x) const
    { return (float)p[b][((long long)y * W + x) * 3 + c]; }
};
template <> struct InSrc<IN_F32> {
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
template <int AXIS, int KIND, bool CV, bool LAST>
__global__ __launch_bounds__(256) void k_in_pass(InSrc<KIND> src, int oh, int ow, const int32_t *__restrict__ bounds,
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
template <int KIND>
__global__ __launch_bounds__(256) void k_in_widen(InSrc<KIND> src, const double *__restrict__ shift,
                                                  const uint8_t *__restrict__ flip, float *__restrict__ out)
{
    const int b = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= src.W) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) in_store(src.at(b, c, y, x), b, c, y, x, src.H, src.W, shift, flip, out);
}

template <int AXIS, int KIND, bool CV, bool LAST>
static void in_launch(hipStream_t s, InSrc<KIND> src, int B, int oh, int ow, const int32_t *bounds, const void *taps,
                      int ksize, const double *shift, const uint8_t *flip, float *out)
{
    hipLaunchKernelGGL((k_in_pass<AXIS, KIND, CV, LAST>), dim3((ow + 255) / 256, oh, B), dim3(256), 0, s, src, oh, ow,
                       bounds, taps, ksize, shift, flip, out);
}

// the passes of both image entry points; KIND: how the decoded bytes are found (IN_U8 or IN_U8_PTRS)
template <int KIND>
static int in_image(spa_ctx *ctx, InSrc<KIND> in, int32_t B, int32_t h, int32_t w, int32_t backend, const int32_t *xb,
                    const void *xk, int32_t ksx, const int32_t *yb, const void *yk, int32_t ksy, const double *shift,
                    const uint8_t *flip, float *tmp, float *out, void *stream)
{
    const int H = in.H, W = in.W;
    SPA_ARG(ctx && in.p && out && B > 0 && H > 0 && W > 0 && h > 0 && w > 0);
    SPA_ARG(B < 65536 && H < 65536 && h < 65536);
    SPA_ARG(backend == 0 || backend == 1);
    hipStream_t s = spa_stream(stream);
    if (H == h && W == w) {
        hipLaunchKernelGGL(k_in_widen<KIND>, dim3((W + 255) / 256, H, B), dim3(256), 0, s, in, shift, flip, out);
        SPA_LAUNCH_CHECK();
        return SPA_OK;
    }
    const bool cv = backend == 1;
    const bool do_x = cv || W != w, do_y = cv || H != h;
    SPA_ARG(!do_x || (xb && xk && (cv || ksx > 0)));
    SPA_ARG(!do_y || (yb && yk && (cv || ksy > 0)));
    SPA_ARG(!(do_x && do_y) || tmp);
    if (do_x && do_y) {
        const InSrc<IN_F32> mid{tmp, H, w};
        if (cv) {
            in_launch<0, KIND, true, false>(s, in, B, H, w, xb, xk, 4, nullptr, nullptr, tmp);
            in_launch<1, IN_F32, true, true>(s, mid, B, h, w, yb, yk, 4, shift, flip, out);
        } else {
            in_launch<0, KIND, false, false>(s, in, B, H, w, xb, xk, ksx, nullptr, nullptr, tmp);
            in_launch<1, IN_F32, false, true>(s, mid, B, h, w, yb, yk, ksy, shift, flip, out);
        }
    } else if (do_x) {
        in_launch<0, KIND, false, true>(s, in, B, h, w, xb, xk, ksx, shift, flip, out);
    } else {
        in_launch<1, KIND, false, true>(s, in, B, h, w, yb, yk, ksy, shift, flip, out);
    }
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_input(spa_ctx *ctx, const uint8_t *src, int32_t B, int32_t H, int32_t W, int32_t h,
                                      int32_t w, int32_t backend, const int32_t *xb, const void *xk, int32_t ksx,
                                      const int32_t *yb, const void *yk, int32_t ksy, const double *shift,
                                      const uint8_t *flip, float *tmp, float *out, void *stream)
{
    return in_image(ctx, InSrc<IN_U8>{src, H, W}, B, h, w, backend, xb, xk, ksx, yb, yk, ksy, shift, flip, tmp, out,
                    stream);
}

extern "C" int spa_segnet_train_input_ptrs(spa_ctx *ctx, const uint8_t *const *srcs, int32_t B, int32_t H, int32_t W,
                                           int32_t h, int32_t w, int32_t backend, const int32_t *xb, const void *xk,
                                           int32_t ksx, const int32_t *yb, const void *yk, int32_t ksy,
                                           const double *shift, const uint8_t *flip, float *tmp, float *out,
                                           void *stream)
{
    return in_image(ctx, InSrc<IN_U8_PTRS>{srcs, H, W}, B, h, w, backend, xb, xk, ksx, yb, yk, ksy, shift, flip, tmp,
                    out, stream);
}

// labels: out[b, c, y, x'] = (To)src[b, c, yi[y], xi[x]], x' = x or w - 1 - x.  Planes = B * C.
// The plane p of the source: in one contiguous batch, or in the example p / C of a device table of B addresses (the
// _ptrs entry point), which need not be aligned for Ti: the value is read byte-wise there.
template <typename Ti, bool PTRS> struct LabSrc;
template <typename Ti> struct LabSrc<Ti, false> {
    const Ti *p;
    __device__ __forceinline__ Ti at(int plane, int C, long long plane_size, long long i) const
    { return p[plane * plane_size + i]; }
};
template <typename Ti> struct LabSrc<Ti, true> {
    const uint8_t *const *p;
    __device__ __forceinline__ Ti at(int plane, int C, long long plane_size, long long i) const
    {
        Ti v;
        __builtin_memcpy(&v, p[plane / C] + ((plane % C) * plane_size + i) * (long long)sizeof(Ti), sizeof(Ti));
        return v;
    }
};

template <typename Ti, typename To, bool PTRS>
__global__ __launch_bounds__(256) void k_in_label(LabSrc<Ti, PTRS> src, int C, int H, int W, int h, int w,
                                                  const int32_t *__restrict__ yi, const int32_t *__restrict__ xi,
                                                  const uint8_t *__restrict__ flip, To *__restrict__ out)
{
    const int p = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= w) return;
    const Ti v = src.at(p, C, (long long)H * W, (long long)yi[y] * W + xi[x]);
    const int xo = (flip && flip[p / C]) ? w - 1 - x : x;
    out[((long long)p * h + y) * w + xo] = (To)v;
}

template <bool PTRS>
static int in_label(spa_ctx *ctx, const void *src, int32_t is_float, int32_t B, int32_t C, int32_t H, int32_t W,
                    int32_t h, int32_t w, const int32_t *yi, const int32_t *xi, const uint8_t *flip, void *out,
                    void *stream)
{
    SPA_ARG(ctx && src && out && yi && xi && B > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0);
    SPA_ARG((long long)B * C < 65536 && h < 65536);
    hipStream_t s = spa_stream(stream);
    const dim3 grid((w + 255) / 256, h, B * C);
    typedef decltype(LabSrc<float, PTRS>::p) Pf;
    typedef decltype(LabSrc<uint8_t, PTRS>::p) Pb;
    if (is_float)
        hipLaunchKernelGGL((k_in_label<float, float, PTRS>), grid, dim3(256), 0, s, LabSrc<float, PTRS>{(Pf)src}, C, H,
                           W, h, w, yi, xi, flip, (float *)out);
    else
        hipLaunchKernelGGL((k_in_label<uint8_t, int32_t, PTRS>), grid, dim3(256), 0, s, LabSrc<uint8_t, PTRS>{(Pb)src},
                           C, H, W, h, w, yi, xi, flip, (int32_t *)out);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_label(spa_ctx *ctx, const void *src, int32_t is_float, int32_t B, int32_t C, int32_t H,
                                      int32_t W, int32_t h, int32_t w, const int32_t *yi, const int32_t *xi,
                                      const uint8_t *flip, void *out, void *stream)
{
    return in_label<false>(ctx, src, is_float, B, C, H, W, h, w, yi, xi, flip, out, stream);
}

extern "C" int spa_segnet_train_label_ptrs(spa_ctx *ctx, const void *const *srcs, int32_t is_float, int32_t B,
                                           int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, const int32_t *yi,
                                           const int32_t *xi, const uint8_t *flip, void *out, void *stream)
{
    return in_label<true>(ctx, (const void *)srcs, is_float, B, C, H, W, h, w, yi, xi, flip, out, stream);
}
