// SegNet-Basic inference (labels_from_segnet.py --dtype bf16) on the bf16 matrix cores: the four layer forms of
// spa_segnet.hip with bf16 operands and float32 accumulation.
//
// Numeric contract.  Every product operand is the round-to-nearest-even bf16 of the float32 value k_segnet_conv
// multiplies at that point (the input forms of spa_segnet_dev.h, rounded while staged) and of the folded float32 weight
// (rounded once per call into a packed bf16 copy in the context workspace, stream-ordered, as the bf16 training entry
// points do).  The products are v_mfma_f32_16x16x32_bf16 accumulating in float32; the epilogue is the float32 one.
// Maps, indices and probabilities stay float32 / uint8 in memory with the float32 path's shapes and layouts, so
// spa_segnet_score follows unchanged.
//
// The bf16 staging and K loop (shared with spa_segnet_train_bf16.hip) are sg_conv_main_bf16 of spa_segnet_dev.h; this
// file owns the kernel's LDS and launches, the weight workspace and the entry points.  Like that file it is compiled with
// -fno-slp-vectorize (Makefile: conv1's LRN must not be packed into v_pk_*_f32 instructions).
#include "spa_segnet_dev.h"

// MODE SG_CONV1: X (B,3,H,W) float32 planar 0..255, Wb (7,64,32) bf16 = (K step, n, k), k = 4 (tap - 8 step) + c,
// zero past tap 48.  SG_ENC: X (B,H,W,64), Wb (49,64,64) bf16 = (tap, n, c).  Both write Y (B,H/2,W/2,64) pooled and
// Yi (B,H/2,W/2,64) uint8 argmax (ky * 2 + kx, first maximum).  SG_DEC / SG_DEC1: X, I (B,H/2,W/2,64) = the pooled
// map and indices of the matching encoder; Y (B,H,W,64), or for SG_DEC1 (B,2,H,W) planar softmax probabilities
// (wc (2,64), bc (2) the classifier).  bias (64) float32.
template <int MODE>
__global__ __launch_bounds__(SG_THREADS) void k_segnet_conv_bf16(const float *__restrict__ X,
                                                                 const uint8_t *__restrict__ I,
                                                                 const unsigned short *__restrict__ Wb,
                                                                 const float *__restrict__ bias,
                                                                 const float *__restrict__ wc,
                                                                 const float *__restrict__ bc, float *__restrict__ Y,
                                                                 uint8_t *__restrict__ Yi, int H, int W, SgStd st)
{
    constexpr int IN = sg_input_form_of(MODE);                            // the input form
    __shared__ __attribute__((aligned(16))) unsigned short xs[SG_HPIX * sg_ps_bf16(IN)];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SG_TH, tx0 = blockIdx.x * SG_TW;
    const SgGeom g = sg_geom(lane, w);
    const int fi = g.fi, fq = g.fq;

    sg_f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = (sg_f32x4){0.f, 0.f, 0.f, 0.f};

    sg_conv_main_bf16<IN>(acc, xs, X, I, Wb, b, ty0, tx0, g, H, W, st);

    sg_infer_epilogue<MODE>(acc, bias, wc, bc, Y, Yi, b, ty0, tx0, w, fi, fq, H, W);
}

// ---------------------------------------------------------------------------------------------------- C ABI
extern "C" int spa_segnet_encode_bf16(spa_ctx *ctx, const float *x, int32_t x_layout, int32_t B, int32_t H, int32_t W,
                                      int32_t Cin, const float *wt, const float *bias, const float *mean_host,
                                      const float *std_host, float *pooled, uint8_t *idx, void *stream)
{
    SgStd st = {};
    int rc = sg_check_encode("spa_segnet_encode_bf16", ctx, x, x_layout, B, H, W, Cin, wt, bias, mean_host, std_host,
                             pooled, idx, &st);
    if (rc != SPA_OK) return rc;
    unsigned short *wb = nullptr;
    rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, SG_W64 * sizeof(unsigned short), (void **)&wb);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    if (Cin == 3)
        sg_launch_bf16_wpack1(s, wt, wb);
    else
        sg_launch_bf16_wpack64(s, wt, 0, wb);
    SPA_LAUNCH_CHECK();
    const dim3 grid = sg_conv_grid(B, H, W);
    if (Cin == 3)
        hipLaunchKernelGGL(k_segnet_conv_bf16<SG_CONV1>, grid, dim3(SG_THREADS), 0, s, x, nullptr, wb, bias, nullptr,
                           nullptr, pooled, idx, H, W, st);
    else
        hipLaunchKernelGGL(k_segnet_conv_bf16<SG_ENC>, grid, dim3(SG_THREADS), 0, s, x, nullptr, wb, bias, nullptr,
                           nullptr, pooled, idx, H, W, st);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode_bf16(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                      int32_t Hh, int32_t Wh, const float *wt, const float *bias, const float *wc,
                                      const float *bc, float *y, void *stream)
{
    int rc = sg_check_decode("spa_segnet_decode_bf16", ctx, x, idx, x_layout, B, Hh, Wh, wt, bias, wc, bc, y);
    if (rc != SPA_OK) return rc;
    const int H = 2 * Hh, W = 2 * Wh;
    unsigned short *wb = nullptr;
    rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, SG_W64 * sizeof(unsigned short), (void **)&wb);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    sg_launch_bf16_wpack64(s, wt, 0, wb);
    SPA_LAUNCH_CHECK();
    const dim3 grid = sg_conv_grid(B, H, W);
    if (wc)
        hipLaunchKernelGGL(k_segnet_conv_bf16<SG_DEC1>, grid, dim3(SG_THREADS), 0, s, x, idx, wb, bias, wc, bc, y,
                           nullptr, H, W, SgStd{});
    else
        hipLaunchKernelGGL(k_segnet_conv_bf16<SG_DEC>, grid, dim3(SG_THREADS), 0, s, x, idx, wb, bias, nullptr,
                           nullptr, y, nullptr, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode_logits_bf16(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout,
                                             int32_t B, int32_t Hh, int32_t Wh, const float *wt, const float *bias,
                                             const float *wc, const float *bc, float *y, void *stream)
{
    int rc = sg_check_decode("spa_segnet_decode_logits_bf16", ctx, x, idx, x_layout, B, Hh, Wh, wt, bias, wc, bc, y,
                             true);
    if (rc != SPA_OK) return rc;
    const int H = 2 * Hh, W = 2 * Wh;
    unsigned short *wb = nullptr;
    rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, SG_W64 * sizeof(unsigned short), (void **)&wb);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    sg_launch_bf16_wpack64(s, wt, 0, wb);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_segnet_conv_bf16<SG_DEC1L>, sg_conv_grid(B, H, W), dim3(SG_THREADS), 0, s, x, idx, wb, bias, wc,
                       bc, y, nullptr, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
