// SegNet-Basic inference (models/segnet_basic.py, the network labels_from_segnet.py evaluates) on the float32 matrix
// cores: every 7x7 convolution is an implicit GEMM on v_mfma_f32_16x16x4_f32 (float32 in, float32 accumulate: an exact
// fmaf chain per output), M = output pixels, N = the 64 output channels, K = 49 taps x Cin.
//
//   encoder (conv1 .. conv4):  pooled, idx = maxpool2x2_argmax(relu(conv7x7(x) + bias))      (BatchNorm folded)
//   decoder (decode4 .. 2):    y = conv7x7(unpool(x, idx)) + bias
//   decode1:                   p = softmax(conv1x1(conv7x7(unpool(x, idx)) + bias; wc) + bc)
//   score:                     mask = argmax(Pillow BILINEAR resize of p to the evaluation shape)
//   decode1, raw scores:       z = conv1x1(...; wc) + bc, no softmax (utils/create_demovideo.py: predict() without scores)
//   overlay:                   score's mask of z, and utils/create_movie.py's blend of the road colour into the frames
//
// Tiling, input forms, the float32 K loop (shared with spa_segnet_train.hip) and the epilogues: spa_segnet_dev.h.  This
// file owns the kernel's LDS and launches, the entry points and the score kernel.
#include "spa_segnet_dev.h"

// MODE SG_CONV1: X (B,3,H,W) float32 planar 0..255, Wt (49,64,4).  SG_ENC: X (B,H,W,64), Wt (49,64,64).  Both write
// Y (B,H/2,W/2,64) pooled and Yi (B,H/2,W/2,64) uint8 argmax (ky * 2 + kx, first maximum).
// SG_DEC / SG_DEC1: X, I (B,H/2,W/2,64) = the pooled map and indices of the matching encoder; Y (B,H,W,64), or for
// SG_DEC1 (B,2,H,W) planar softmax probabilities (wc (2,64), bc (2) the classifier), for SG_DEC1L the classifier's two
// sums before the softmax, in the same place (here and in the bf16 and split-plane kernels).
template <int MODE>
__global__ __launch_bounds__(SG_THREADS) void k_segnet_conv(const float *__restrict__ X, const uint8_t *__restrict__ I,
                                                            const float *__restrict__ Wt, const float *__restrict__ bias,
                                                            const float *__restrict__ wc, const float *__restrict__ bc,
                                                            float *__restrict__ Y, uint8_t *__restrict__ Yi, int H, int W,
                                                            SgStd st)
{
    constexpr int IN = sg_input_form_of(MODE);              // the input form
    __shared__ __attribute__((aligned(16))) float xs[SG_HPIX * sg_ps_f32(IN)];

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

    sg_conv_main_f32<IN>(acc, xs, X, I, Wt, b, ty0, tx0, g, H, W, st);

    sg_infer_epilogue<MODE>(acc, bias, wc, bc, Y, Yi, b, ty0, tx0, w, fi, fq, H, W);
}

// Pillow's Image.resize(BILINEAR) of a mode 'F' image (chainercv.transforms.resize of the float32 score, PIL backend),
// upscales: per axis the coefficients of Resample.c precompute_coeffs in double (support 1, window bounds rounded by
// truncation and clipped, weights normalised by their sum), a horizontal pass accumulated in double and stored as
// float32, then the vertical pass over those float32 rows.  Each thread recomputes the (at most 3) horizontal values it
// needs with the same operations in the same order, so the result is Pillow's, bit for bit.
__device__ __forceinline__ int sg_pil_coeffs(int o, int in_size, double scale, double *k)
{
    const double center = (o + 0.5) * scale;
    int lo = (int)(center - 1.0 + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + 1.0 + 0.5);
    if (hi > in_size) hi = in_size;
    const int n = hi - lo;
    double ww = 0.0;
    for (int j = 0; j < 3; ++j) {
        double t = 0.0;
        if (j < n) {
            double x = ((double)(j + lo) - center + 0.5) * 1.0;
            if (x < 0.0) x = -x;
            t = x < 1.0 ? 1.0 - x : 0.0;
        }
        k[j] = t;
        ww += t;
    }
    for (int j = 0; j < 3; ++j)
        if (ww != 0.0) k[j] /= ww;
    return lo | (n << 24);
}

__global__ __launch_bounds__(256) void k_segnet_score(const float *__restrict__ P, int h, int w, int H, int W,
                                                      uint8_t *__restrict__ mask, float *__restrict__ S)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W) return;
    double kx[3], ky[3];
    const int bx = sg_pil_coeffs(x, w, (double)w / (double)W, kx);
    const int by = sg_pil_coeffs(y, h, (double)h / (double)H, ky);
    const int x0 = bx & 0xffffff, nx = bx >> 24, y0 = by & 0xffffff, ny = by >> 24;
    float out[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *pc = P + ((long long)b * 2 + c) * h * w;
        double sv = 0.0;
        for (int j = 0; j < ny; ++j) {
            const float *row = pc + (long long)(y0 + j) * w + x0;
            double sh = 0.0;
            for (int i = 0; i < nx; ++i) sh += (double)row[i] * kx[i];
            sv += (double)(float)sh * ky[j];
        }
        out[c] = (float)sv;
    }
    const long long o = ((long long)b * H + y) * W + x;
    mask[o] = out[1] > out[0] ? 1 : 0;                // argmax, ties to class 0
    if (S) {
        S[((long long)b * 2) * H * W + (long long)y * W + x] = out[0];
        S[((long long)b * 2 + 1) * H * W + (long long)y * W + x] = out[1];
    }
}

// k_segnet_score, the class map of segnet.label_mask on the raw labelIds bytes and k_confusion in one pass.  A block
// is 64 x 4 threads over a tile of 256 columns x SG_LE_ROWS rows: a thread owns four adjacent columns, keeps their
// horizontal coefficients and walks rows ty, ty + 4, ...  Every sample is formed by k_segnet_score's operations in its
// order, so mask and scores have its bits.  VEC (W a multiple of 4, bases aligned): one 4-byte label load, one 4-byte
// mask store and two 16-byte score stores per thread and row; otherwise bytes and dwords.  The counts are integers:
// registers, wave shuffles, LDS across the four waves, one 64-bit atomicAdd per block and class.
#define SG_LE_ROWS 16

template <bool VEC>
__global__ __launch_bounds__(256) void k_segnet_label_eval(const float *__restrict__ P, int h, int w, int H, int W,
                                                           const uint8_t *__restrict__ ids, uint8_t *__restrict__ mask,
                                                           float *__restrict__ S, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned sc[4][4];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, b = blockIdx.z;
    const int xb = (blockIdx.x * 64 + tx) * 4;
    const int yb = blockIdx.y * SG_LE_ROWS;
    double kx[4][3];
    int x0[4], nx[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x = xb + p < W ? xb + p : W - 1;     // columns past the edge: a valid column, never stored
        const int bx = sg_pil_coeffs(x, w, (double)w / (double)W, kx[p]);
        x0[p] = bx & 0xffffff;
        nx[p] = bx >> 24;
    }
    unsigned c[4] = {0, 0, 0, 0};
    const long long plane = (long long)H * W;
    if (xb < W) {
        for (int r = ty; r < SG_LE_ROWS; r += 4) {
            const int y = yb + r;
            if (y >= H) break;
            double ky[3];
            const int by = sg_pil_coeffs(y, h, (double)h / (double)H, ky);
            const int y0 = by & 0xffffff, ny = by >> 24;
            float out[2][4];
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const float *pc = P + ((long long)b * 2 + ch) * h * w;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    double sv = 0.0;
                    for (int j = 0; j < ny; ++j) {
                        const float *row = pc + (long long)(y0 + j) * w + x0[p];
                        double sh = 0.0;
                        for (int i = 0; i < nx[p]; ++i) sh += (double)row[i] * kx[p][i];
                        sv += (double)(float)sh * ky[j];
                    }
                    out[ch][p] = (float)sv;
                }
            }
            const long long o = ((long long)b * H + y) * W + xb;
            uint8_t m[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) m[p] = out[1][p] > out[0][p] ? 1 : 0;      // argmax, ties to class 0
            uint8_t g[4] = {0, 0, 0, 0};
            if (VEC) {
                *(uint32_t *)(mask + o) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) |
                                          ((uint32_t)m[3] << 24);
                if (S) {
                    float *s0 = S + (long long)b * 2 * plane + (long long)y * W + xb;
                    *(float4 *)s0 = make_float4(out[0][0], out[0][1], out[0][2], out[0][3]);
                    *(float4 *)(s0 + plane) = make_float4(out[1][0], out[1][1], out[1][2], out[1][3]);
                }
                if (ids) {
                    const uint32_t v = *(const uint32_t *)(ids + o);
#pragma unroll
                    for (int p = 0; p < 4; ++p) g[p] = (uint8_t)(v >> (8 * p));
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (xb + p >= W) break;
                    mask[o + p] = m[p];
                    if (S) {
                        float *s0 = S + (long long)b * 2 * plane + (long long)y * W + xb + p;
                        s0[0] = out[0][p];
                        s0[plane] = out[1][p];
                    }
                    if (ids) g[p] = ids[o + p];
                }
            }
            if (ids) {
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    if (xb + p < W && g[p] > 6) c[(g[p] == 7 ? 2 : 0) + m[p]] += 1;   // ids 0..6 are ignored
            }
        }
    }
    if (!counts) return;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        for (int o = 32; o > 0; o >>= 1) c[j] += __shfl_down(c[j], o);
    if (tx == 0)
        for (int j = 0; j < 4; ++j) sc[ty][j] = c[j];
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned t = sc[0][threadIdx.x] + sc[1][threadIdx.x] + sc[2][threadIdx.x] + sc[3][threadIdx.x];
        if (t) atomicAdd(counts + (long long)b * 4 + threadIdx.x, (unsigned long long)t);
    }
}

extern "C" int spa_segnet_label_eval(spa_ctx *ctx, const float *prob, int32_t B, int32_t h, int32_t w, int32_t H,
                                     int32_t W, const uint8_t *label_ids, uint8_t *mask, float *scores, int64_t *counts,
                                     void *stream)
{
    SPA_ARG(ctx && prob && mask && B > 0 && B < 65536 && h > 0 && w > 0 && H > 0 && W > 0);
    SPA_ARG(H < 65536 && W < (1 << 24) && h < (1 << 24) && w < (1 << 24));
    if ((label_ids == nullptr) != (counts == nullptr)) {
        spa_set_error("spa_segnet_label_eval: label_ids and counts must be given together or both be NULL");
        return SPA_ERR_ARG;
    }
    if (H < h || W < w) {
        spa_set_error("spa_segnet_label_eval: (%d, %d) -> (%d, %d) is a downscale; only upscales are supported", h, w, H,
                      W);
        return SPA_ERR_ARG;
    }
    hipStream_t s = spa_stream(stream);
    if (counts) SPA_HIP(hipMemsetAsync(counts, 0, (size_t)B * 4 * sizeof(int64_t), s));
    const bool vec = W % 4 == 0 && (((uintptr_t)mask | (uintptr_t)label_ids) & 3) == 0 && ((uintptr_t)scores & 15) == 0;
    const dim3 grid((W + 255) / 256, (H + SG_LE_ROWS - 1) / SG_LE_ROWS, B);
    if (vec)
        hipLaunchKernelGGL(k_segnet_label_eval<true>, grid, dim3(256), 0, s, prob, h, w, H, W, label_ids, mask, scores,
                           (unsigned long long *)counts);
    else
        hipLaunchKernelGGL(k_segnet_label_eval<false>, grid, dim3(256), 0, s, prob, h, w, H, W, label_ids, mask, scores,
                           (unsigned long long *)counts);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

// k_segnet_score's mask and utils/create_movie.py's blend of the road colour into the frames in one pass, with
// k_segnet_label_eval's layout (64 x 4 threads over 256 columns x SG_LE_ROWS rows, a thread owns four adjacent columns
// and walks rows) and its sample arithmetic, so the mask has k_segnet_score's bits.  Where the mask is 1 a channel is
// (uint8)(alpha * color + (1 - alpha) * v) in double, each product and the sum rounded on its own (no FMA) and the cast
// truncating: numpy's img[pred == 1] = alpha * pred_color[pred == 1] + (1 - alpha) * img[pred == 1].  ac[c] = alpha *
// color[c] (one rounding, made on the host), om = 1 - alpha.  VEC (W a multiple of 4, bases 4-byte aligned): three
// dword frame loads, three dword stores and one dword mask store per thread and row; otherwise bytes.  No LDS: every
// sample is read by the lane that needs it, and nothing is reduced.
struct SgBlend {
    double ac[3], om;
};

__device__ __forceinline__ uint32_t sg_blend_byte(uint32_t v, double ac, double om)
{
    return (uint32_t)(uint8_t)__dadd_rn(ac, __dmul_rn(om, (double)v));
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_segnet_overlay(const float *__restrict__ P, int h, int w, int H, int W,
                                                        const uint8_t *__restrict__ frames, SgBlend bl,
                                                        uint8_t *__restrict__ mask, uint8_t *__restrict__ blended)
{
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, b = blockIdx.z;
    const int xb = (blockIdx.x * 64 + tx) * 4;
    const int yb = blockIdx.y * SG_LE_ROWS;
    if (xb >= W) return;
    double kx[4][3];
    int x0[4], nx[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int x = xb + p < W ? xb + p : W - 1;     // columns past the edge: a valid column, never stored
        const int bx = sg_pil_coeffs(x, w, (double)w / (double)W, kx[p]);
        x0[p] = bx & 0xffffff;
        nx[p] = bx >> 24;
    }
    for (int r = ty; r < SG_LE_ROWS; r += 4) {
        const int y = yb + r;
        if (y >= H) break;
        double ky[3];
        const int by = sg_pil_coeffs(y, h, (double)h / (double)H, ky);
        const int y0 = by & 0xffffff, ny = by >> 24;
        float out[2][4];
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const float *pc = P + ((long long)b * 2 + ch) * h * w;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                double sv = 0.0;
                for (int j = 0; j < ny; ++j) {
                    const float *row = pc + (long long)(y0 + j) * w + x0[p];
                    double sh = 0.0;
                    for (int i = 0; i < nx[p]; ++i) sh += (double)row[i] * kx[p][i];
                    sv += (double)(float)sh * ky[j];
                }
                out[ch][p] = (float)sv;
            }
        }
        const long long o = ((long long)b * H + y) * W + xb;
        uint32_t m[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) m[p] = out[1][p] > out[0][p] ? 1u : 0u;      // argmax, ties to class 0
        if (VEC) {
            *(uint32_t *)(mask + o) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
            const uint32_t *src = (const uint32_t *)(frames + o * 3);
            uint32_t *dst = (uint32_t *)(blended + o * 3);
            uint32_t v[3] = {src[0], src[1], src[2]};
#pragma unroll
            for (int k = 0; k < 12; ++k) {             // byte k of the 12: pixel k / 3, channel k % 3
                if (!m[k / 3]) continue;
                const uint32_t sh = 8 * (k & 3);
                const uint32_t q = sg_blend_byte((v[k >> 2] >> sh) & 0xffu, bl.ac[k % 3], bl.om);
                v[k >> 2] = (v[k >> 2] & ~(0xffu << sh)) | (q << sh);
            }
            dst[0] = v[0];
            dst[1] = v[1];
            dst[2] = v[2];
        } else {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (xb + p >= W) break;
                mask[o + p] = (uint8_t)m[p];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t v = frames[(o + p) * 3 + c];
                    blended[(o + p) * 3 + c] = (uint8_t)(m[p] ? sg_blend_byte(v, bl.ac[c], bl.om) : v);
                }
            }
        }
    }
}

extern "C" int spa_segnet_overlay(spa_ctx *ctx, const float *score, int32_t B, int32_t h, int32_t w, int32_t H,
                                  int32_t W, const uint8_t *frames, const uint8_t *color_host, double alpha,
                                  uint8_t *mask, uint8_t *blended, void *stream)
{
    SPA_ARG(ctx && score && frames && color_host && mask && blended);
    SPA_ARG(B > 0 && B < 65536 && h > 0 && w > 0 && H > 0 && W > 0);
    SPA_ARG(H < 65536 && W < (1 << 24) && h < (1 << 24) && w < (1 << 24));
    if (H < h || W < w) {
        spa_set_error("spa_segnet_overlay: (%d, %d) -> (%d, %d) is a downscale; only upscales are supported", h, w, H, W);
        return SPA_ERR_ARG;
    }
    if (!(alpha >= 0.0 && alpha <= 1.0)) {             // NaN included
        spa_set_error("spa_segnet_overlay: alpha must lie in [0, 1], got %g", alpha);
        return SPA_ERR_ARG;
    }
    const size_t nb = (size_t)B * H * W * 3;
    if ((uintptr_t)blended < (uintptr_t)frames + nb && (uintptr_t)frames < (uintptr_t)blended + nb) {
        spa_set_error("spa_segnet_overlay: blended overlaps frames");
        return SPA_ERR_ARG;
    }
    SgBlend bl;
    for (int c = 0; c < 3; ++c) bl.ac[c] = alpha * (double)color_host[c];
    bl.om = 1.0 - alpha;
    hipStream_t s = spa_stream(stream);
    const bool vec = W % 4 == 0 && (((uintptr_t)mask | (uintptr_t)frames | (uintptr_t)blended) & 3) == 0;
    const dim3 grid((W + 255) / 256, (H + SG_LE_ROWS - 1) / SG_LE_ROWS, B);
    if (vec)
        hipLaunchKernelGGL(k_segnet_overlay<true>, grid, dim3(256), 0, s, score, h, w, H, W, frames, bl, mask, blended);
    else
        hipLaunchKernelGGL(k_segnet_overlay<false>, grid, dim3(256), 0, s, score, h, w, H, W, frames, bl, mask, blended);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_encode(spa_ctx *ctx, const float *x, int32_t x_layout, int32_t B, int32_t H, int32_t W,
                                 int32_t Cin, const float *wt, const float *bias, const float *mean_host,
                                 const float *std_host, float *pooled, uint8_t *idx, void *stream)
{
    SgStd st = {};
    int rc = sg_check_encode("spa_segnet_encode", ctx, x, x_layout, B, H, W, Cin, wt, bias, mean_host, std_host, pooled,
                             idx, &st);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    const dim3 grid = sg_conv_grid(B, H, W);
    if (Cin == 3)
        hipLaunchKernelGGL(k_segnet_conv<SG_CONV1>, grid, dim3(SG_THREADS), 0, s, x, nullptr, wt, bias, nullptr, nullptr,
                           pooled, idx, H, W, st);
    else
        hipLaunchKernelGGL(k_segnet_conv<SG_ENC>, grid, dim3(SG_THREADS), 0, s, x, nullptr, wt, bias, nullptr, nullptr,
                           pooled, idx, H, W, st);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                 int32_t Hh, int32_t Wh, const float *wt, const float *bias, const float *wc,
                                 const float *bc, float *y, void *stream)
{
    int rc = sg_check_decode("spa_segnet_decode", ctx, x, idx, x_layout, B, Hh, Wh, wt, bias, wc, bc, y);
    if (rc != SPA_OK) return rc;
    const int H = 2 * Hh, W = 2 * Wh;
    hipStream_t s = spa_stream(stream);
    const dim3 grid = sg_conv_grid(B, H, W);
    if (wc)
        hipLaunchKernelGGL(k_segnet_conv<SG_DEC1>, grid, dim3(SG_THREADS), 0, s, x, idx, wt, bias, wc, bc, y, nullptr, H,
                           W, SgStd{});
    else
        hipLaunchKernelGGL(k_segnet_conv<SG_DEC>, grid, dim3(SG_THREADS), 0, s, x, idx, wt, bias, nullptr, nullptr, y,
                           nullptr, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode_logits(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                        int32_t Hh, int32_t Wh, const float *wt, const float *bias, const float *wc,
                                        const float *bc, float *y, void *stream)
{
    int rc = sg_check_decode("spa_segnet_decode_logits", ctx, x, idx, x_layout, B, Hh, Wh, wt, bias, wc, bc, y, true);
    if (rc != SPA_OK) return rc;
    const int H = 2 * Hh, W = 2 * Wh;
    hipStream_t s = spa_stream(stream);
    hipLaunchKernelGGL(k_segnet_conv<SG_DEC1L>, sg_conv_grid(B, H, W), dim3(SG_THREADS), 0, s, x, idx, wt, bias, wc, bc,
                       y, nullptr, H, W, SgStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_score(spa_ctx *ctx, const float *prob, int32_t B, int32_t h, int32_t w, int32_t H, int32_t W,
                                uint8_t *mask, float *scores, void *stream)
{
    SPA_ARG(ctx && prob && mask && B > 0 && B < 65536 && h > 0 && w > 0 && H > 0 && W > 0);
    SPA_ARG(H < 65536 && W < (1 << 24) && h < (1 << 24) && w < (1 << 24));
    if (H < h || W < w) {
        spa_set_error("spa_segnet_score: (%d, %d) -> (%d, %d) is a downscale; only upscales are supported", h, w, H, W);
        return SPA_ERR_ARG;
    }
    hipStream_t s = spa_stream(stream);
    hipLaunchKernelGGL(k_segnet_score, dim3((W + 255) / 256, H, B), dim3(256), 0, s, prob, h, w, H, W, mask, scores);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
