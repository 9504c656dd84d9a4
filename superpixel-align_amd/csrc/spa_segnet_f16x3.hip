// SegNet-Basic inference at float32 accuracy on the f16 matrix cores (labels_from_segnet.py --split_planes): the four
// layer forms of spa_segnet.hip with every float32 operand carried as two half-precision planes and three products per
// float32 product (the split of spa_segnet_dev.h).
//
// Numeric contract.  The folded weights get one scale exponent, the activations ONE PER IMAGE -- of conv1's operand as
// k_segnet_conv computes it, of the map, or of a decoder's pooled map (its unpooled values are a subset of it).  A
// per-batch scale would make an image's planes depend on its neighbours; with a per-image one an image's outputs have
// the same bits whatever the batch size and its position in the batch.  The two cross terms of a product are issued
// first and kept in accumulators of their own (sg_mma3), added to the h_a h_b accumulators after the K loop; the sum is
// multiplied by 2^-(k_x + k_w) (v_ldexp, exact) BEFORE the bias is added, and everything after that is the float32
// inference epilogue.  Maps, indices and probabilities keep the float32 path's types, shapes and layouts, so
// spa_segnet_score follows unchanged.
//
// The exponents are computed on the device inside each call: per-workgroup maxima of |v| in one launch -- blockIdx.x =
// image, the last one the weights -- then one workgroup per exponent reduces them.  No atomics are used and the host
// never waits.  The weights are split once per call into a packed f16 plane pair in the context workspace,
// stream-ordered.
//
// The split staging and K loop (shared with spa_segnet_train_f16x3.hip) are spa_segnet_split_main.inc;
// this file owns the per-image maxima, the kernel's LDS and launches, the workspaces and the entry points.
#include "spa_segnet_dev.h"

// part[blockIdx.x * SG_NAMAX + blockIdx.y] = the bit pattern of max |v| over this workgroup's share of operand
// blockIdx.x: for blockIdx.x < B image blockIdx.x's activations -- n4 float4 of the 64-channel map x, or with CONV1
// the standardised, LRN-normalised (3,H,W) image as the kernels stage it -- and for blockIdx.x == B the nw4 float4 of
// the weights wt.  Grid (B + 1, SG_NAMAX); x and wt 16-byte aligned.
template <bool CONV1>
__global__ __launch_bounds__(256) void k_sgx_amax(const float *__restrict__ x, long long n4, int B, int H, int W,
                                                  SgStd st, const float *__restrict__ wt, long long nw4,
                                                  unsigned *__restrict__ part)
{
    __shared__ unsigned red[256];
    const int t = threadIdx.x, j = blockIdx.x, g = blockIdx.y;
    unsigned m = 0u;
    if (CONV1 && j < B) {
        const long long plane = (long long)H * W;
        const float *xb = x + (long long)j * 3 * plane;
        for (long long i = (long long)g * 256 + t; i < plane; i += (long long)SG_NAMAX * 256) {
            const sg_f32x4 v = sg_conv1_val(xb, plane, (int)(i / W), (int)(i % W), H, W, st);
            m = max(m, max(max(sg_absbits(v.x), sg_absbits(v.y)), sg_absbits(v.z)));
        }
    } else {
        const sg_f32x4 *a = j < B ? (const sg_f32x4 *)x + (long long)j * n4 : (const sg_f32x4 *)wt;
        const long long n = j < B ? n4 : nw4;
        for (long long i = (long long)g * 256 + t; i < n; i += (long long)SG_NAMAX * 256) {
            const sg_f32x4 v = a[i];
            m = max(max(m, max(sg_absbits(v.x), sg_absbits(v.y))), max(sg_absbits(v.z), sg_absbits(v.w)));
        }
    }
    red[t] = m;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) red[t] = max(red[t], red[t + d]);
        __syncthreads();
    }
    if (t == 0) part[(long long)j * SG_NAMAX + g] = red[0];
}

// MODE SG_CONV1: X (B,3,H,W) float32 planar 0..255.  SG_ENC: X (B,H,W,64).  Both write Y (B,H/2,W/2,64) pooled and
// Yi (B,H/2,W/2,64) uint8 argmax (ky * 2 + kx, first maximum).  SG_DEC / SG_DEC1: X, I (B,H/2,W/2,64) = the pooled
// map and indices of the matching encoder; Y (B,H,W,64), or for SG_DEC1 (B,2,H,W) planar softmax probabilities
// (wc (2,64), bc (2) the classifier).  bias (64) float32.  Wp: the h plane, then the l plane, each (49,64,64) =
// (tap, n, c) for the 64-channel forms or (7,64,32) = (K step, n, k) for conv1 (k = 4 (tap - 8 step) + c, zero past
// tap 48).  ex[b] = image b's scale exponent, ex[gridDim.z] = the weights'.
template <int MODE>
__global__ __launch_bounds__(SG_THREADS, 2) void k_segnet_conv_f16x3(const float *__restrict__ X,
                                                                     const uint8_t *__restrict__ I,
                                                                     const unsigned short *__restrict__ Wp,
                                                                     const float *__restrict__ bias,
                                                                     const float *__restrict__ wc,
                                                                     const float *__restrict__ bc,
                                                                     float *__restrict__ Y, uint8_t *__restrict__ Yi,
                                                                     const int *__restrict__ ex, int H, int W,
                                                                     SgStd st)
{
    constexpr int IN = sg_input_form_of(MODE);                            // the input form
    __shared__ __attribute__((aligned(16))) unsigned short xs[SG_HPIX * sg_ps_split(IN)];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SG_TH, tx0 = blockIdx.x * SG_TW;
    const int kin = ex[b], kw = ex[gridDim.z];
    const float sc = sg_pow2(kin);
    const auto [fi, fq, frow, fcol] = sg_geom(lane, w);

    sg_f32x4 acc[4][4], accx[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = accx[m][nt] = (sg_f32x4){0.f, 0.f, 0.f, 0.f};

#include "spa_segnet_split_main.inc"

    // ---- the float32 sums: cross terms added, then unscaled exactly
    const int unscale = -(kin + kw);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[m][nt][r] = ldexpf(acc[m][nt][r] + accx[m][nt][r], unscale);

#include "spa_segnet_infer_epilogue.inc"
}

// ---------------------------------------------------------------------------------------------------- C ABI
// The exponents of the B images' activations (ex[0 .. B - 1]) and of the weights (ex[B]), and the split weights, on
// stream s without a host synchronisation.  n4: float4 per image of a 64-channel operand (Cin == 3: conv1's operand of
// the image x instead).  Workspaces: the weight planes share WS_SEGNET_WF16X3 and the maxima WS_SEGNET_AMAX with the
// split-plane training entry points; every user writes them before it reads them on the stream it was given, so
// calls ordered on one stream (the contract of every workspace here) cannot see each other's contents.
static int sgx_prepare(spa_ctx *ctx, hipStream_t s, const float *x, long long n4, int Cin, int B, int H, int W,
                       const SgStd &st, const float *wt, unsigned short **wp, int **ex)
{
    int rc = spa_ws_reserve(ctx, WS_SEGNET_WF16X3, 2 * SG_W64 * sizeof(unsigned short), (void **)wp);
    if (rc != SPA_OK) return rc;
    unsigned *part = nullptr;
    const size_t nop = (size_t)B + 1;
    rc = spa_ws_reserve(ctx, WS_SEGNET_AMAX, nop * SG_NAMAX * sizeof(unsigned) + nop * sizeof(int), (void **)&part);
    if (rc != SPA_OK) return rc;
    *ex = (int *)(part + nop * SG_NAMAX);
    dim3 grid(B + 1, SG_NAMAX);
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgx_amax<true>, grid, dim3(256), 0, s, x, 0ll, B, H, W, st, wt, 49ll * 64 * 4 / 4, part);
    else
        hipLaunchKernelGGL(k_sgx_amax<false>, grid, dim3(256), 0, s, x, n4, B, H, W, st, wt, (long long)SG_W64 / 4,
                           part);
    SPA_LAUNCH_CHECK();
    sg_launch_scale(s, B + 1, part, *ex);
    SPA_LAUNCH_CHECK();
    if (Cin == 3)
        sg_launch_split_wpack1(s, wt, *ex + B, *wp);
    else
        sg_launch_split_wpack64(s, wt, 0, *ex + B, *wp);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_encode_f16x3(spa_ctx *ctx, const float *x, int32_t x_layout, int32_t B, int32_t H, int32_t W,
                                       int32_t Cin, const float *wt, const float *bias, const float *mean_host,
                                       const float *std_host, float *pooled, uint8_t *idx, void *stream)
{
    SgStd st = {};
    int rc = sg_check_encode("spa_segnet_encode_f16x3", ctx, x, x_layout, B, H, W, Cin, wt, bias, mean_host, std_host,
                             pooled, idx, &st);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    unsigned short *wp = nullptr;
    int *ex = nullptr;
    rc = sgx_prepare(ctx, s, x, (long long)H * W * 16, Cin, B, H, W, st, wt, &wp, &ex);
    if (rc != SPA_OK) return rc;
    const dim3 grid = sg_conv_grid(B, H, W);
    if (Cin == 3)
        hipLaunchKernelGGL(k_segnet_conv_f16x3<SG_CONV1>, grid, dim3(SG_THREADS), 0, s, x, nullptr, wp, bias, nullptr,
                           nullptr, pooled, idx, ex, H, W, st);
    else
        hipLaunchKernelGGL(k_segnet_conv_f16x3<SG_ENC>, grid, dim3(SG_THREADS), 0, s, x, nullptr, wp, bias, nullptr,
                           nullptr, pooled, idx, ex, H, W, st);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode_f16x3(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                       int32_t Hh, int32_t Wh, const float *wt, const float *bias, const float *wc,
                                       const float *bc, float *y, void *stream)
{
    int rc = sg_check_decode("spa_segnet_decode_f16x3", ctx, x, idx, x_layout, B, Hh, Wh, wt, bias, wc, bc, y);
    if (rc != SPA_OK) return rc;
    const int H = 2 * Hh, W = 2 * Wh;
    hipStream_t s = spa_stream(stream);
    unsigned short *wp = nullptr;
    int *ex = nullptr;
    rc = sgx_prepare(ctx, s, x, (long long)Hh * Wh * 16, 64, B, H, W, SgStd{}, wt, &wp, &ex);
    if (rc != SPA_OK) return rc;
    const dim3 grid = sg_conv_grid(B, H, W);
    if (wc)
        hipLaunchKernelGGL(k_segnet_conv_f16x3<SG_DEC1>, grid, dim3(SG_THREADS), 0, s, x, idx, wp, bias, wc, bc, y,
                           nullptr, ex, H, W, SgStd{});
    else
        hipLaunchKernelGGL(k_segnet_conv_f16x3<SG_DEC>, grid, dim3(SG_THREADS), 0, s, x, idx, wp, bias, nullptr,
                           nullptr, y, nullptr, ex, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode_logits_f16x3(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout,
                                              int32_t B, int32_t Hh, int32_t Wh, const float *wt, const float *bias,
                                              const float *wc, const float *bc, float *y, void *stream)
{
    int rc = sg_check_decode("spa_segnet_decode_logits_f16x3", ctx, x, idx, x_layout, B, Hh, Wh, wt, bias, wc, bc, y,
                             true);
    if (rc != SPA_OK) return rc;
    const int H = 2 * Hh, W = 2 * Wh;
    hipStream_t s = spa_stream(stream);
    unsigned short *wp = nullptr;
    int *ex = nullptr;
    rc = sgx_prepare(ctx, s, x, (long long)Hh * Wh * 16, 64, B, H, W, SgStd{}, wt, &wp, &ex);
    if (rc != SPA_OK) return rc;
    hipLaunchKernelGGL(k_segnet_conv_f16x3<SG_DEC1L>, sg_conv_grid(B, H, W), dim3(SG_THREADS), 0, s, x, idx, wp, bias,
                       wc, bc, y, nullptr, ex, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
