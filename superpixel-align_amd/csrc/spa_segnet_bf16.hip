// SegNet-Basic inference (labels_from_segnet.py --dtype bf16) on the bf16 matrix cores: the four layer forms of
// spa_segnet.hip -- conv1 (the planar image, standardised and LRN-normalised in the load), conv2-4 (a 64-channel map),
// decode4-2 (the pooled map unpooled through its index map in the load) and decode1 (the same, plus the 1x1
// classifier and the softmax) -- with bf16 operands and float32 accumulation.
//
// Numeric contract.  Every product operand is the round-to-nearest-even bf16 of the float32 value k_segnet_conv
// multiplies at that point: the standardised, LRN-normalised conv1 input (the float32 operations of sg_lrn3), the map
// value or the unpooled value (zero where the index does not select the position), and the folded float32 weight
// (rounded once per call into a packed bf16 copy in the context workspace, stream-ordered, as the bf16 training entry
// points do).  The products are v_mfma_f32_16x16x32_bf16 accumulating in float32.  The epilogue is k_segnet_conv's,
// in float32: bias, ReLU, 2x2 max-pool with the first maximum's index in window order, and decode1's classifier fmaf
// chain, 16-lane butterfly and softmax.  Maps, indices and probabilities stay float32 / uint8 in memory with the float32
// path's shapes and layouts, so spa_segnet_score follows unchanged.  No atomics: an image's outputs have the same bits
// whatever the batch size and its position in the batch.
//
// Tiling: k_sgb_conv's (spa_segnet_train_bf16.hip), which is k_segnet_conv's.  One workgroup = 8 x 32 output pixels x
// 64 channels, 4 waves, wave w owns output rows 2w, 2w + 1; a 16-row MFMA tile = four 2x2 pooling blocks, so the C/D
// layout (row = 4 (lane >> 4) + reg, the same as the float32 instruction's) puts one pooling window in the four
// accumulator registers of one lane.  The A operand is 16 pixels x 32 input channels: a lane reads 8 consecutive
// channels of one pixel (16 bytes) from a channels-last bf16 halo in LDS (14 x 38 pixels x 40 bf16 = 42 560 bytes),
// staged in two 32-channel chunks.  conv1's K is (tap, channel) with the 3 channels padded to 4: a 32-wide K step packs
// 8 taps, the 49 taps fill 7 steps with the last 7 zero.
#include "spa_common.h"

typedef float sgi_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 sgi_bf16x8 __attribute__((ext_vector_type(8)));

#define SGI_TH 8                       // output tile rows
#define SGI_TW 32                      // output tile columns
#define SGI_HH (SGI_TH + 6)            // halo rows
#define SGI_HW (SGI_TW + 6)            // halo columns
#define SGI_HPIX (SGI_HH * SGI_HW)     // 532 halo pixels
#define SGI_THREADS 256
#define SGI_PS 40                      // LDS bf16 per staged pixel of a 32-channel chunk (64 bytes + 16 of padding)

enum { SGI_CONV1 = 0, SGI_ENC = 1, SGI_DEC = 2, SGI_DEC1 = 3 };

struct SgiStd {
    float mean[3], std[3];
};

__device__ __forceinline__ unsigned sgi_bits(float f)
{
    const __bf16 h = (__bf16)f;                    // round to nearest even; subnormals kept, NaN stays NaN
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}

__device__ __forceinline__ unsigned sgi_pack2(float a, float b) { return sgi_bits(a) | (sgi_bits(b) << 16); }

__device__ __forceinline__ uint4 sgi_pack8(sgi_f32x4 lo, sgi_f32x4 hi)
{
    return make_uint4(sgi_pack2(lo.x, lo.y), sgi_pack2(lo.z, lo.w), sgi_pack2(hi.x, hi.y), sgi_pack2(hi.z, hi.w));
}

// Chainer's local_response_normalization with three channels: the float32 operations of sg_lrn3 (spa_segnet.hip)
__device__ __forceinline__ void sgi_lrn3(float &a, float &b, float &c)
{
    const float a2 = a * a, b2 = b * b, c2 = c * c;
    const float s0 = (a2 + b2) + c2;
    const float s1 = (b2 + a2) + c2;
    const float s2 = (c2 + b2) + a2;
    const float alpha = 1e-4f / 5.f;
    a = a * powf(1.f + alpha * s0, -0.75f);
    b = b * powf(1.f + alpha * s1, -0.75f);
    c = c * powf(1.f + alpha * s2, -0.75f);
}

// the standardised, LRN-normalised conv1 input at (gy, gx) as k_segnet_conv<SG_CONV1> stages it, rounded to bf16
// (4 values, channel 3 zero); zero outside the image
__device__ __forceinline__ uint2 sgi_conv1_px(const float *xb, long long plane, int gy, int gx, int H, int W,
                                              const SgiStd &st)
{
    float r = 0.f, g = 0.f, bl = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const long long o = (long long)gy * W + gx;
        r = xb[o];
        g = xb[plane + o];
        bl = xb[2 * plane + o];
        r = (r - st.mean[0]) / st.std[0];          // img -= mean; img /= std (two roundings)
        g = (g - st.mean[1]) / st.std[1];
        bl = (bl - st.mean[2]) / st.std[2];
        sgi_lrn3(r, g, bl);
    }
    return make_uint2(sgi_pack2(r, g), sgi_pack2(bl, 0.f));
}

// channels [c, c + 8) of the 64-channel input at full-resolution (gy, gx) as bf16: ENC reads the map, DEC / DEC1 the
// pooled map at (gy/2, gx/2) where its index selects (gy & 1, gx & 1), zero elsewhere; zero outside the image
template <int MODE>
__device__ __forceinline__ uint4 sgi_px8(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H, int W)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        if (MODE == SGI_ENC) {
            const float *p = X + (((long long)b * H + gy) * W + gx) * 64 + c;
            v = sgi_pack8(*(const sgi_f32x4 *)p, *(const sgi_f32x4 *)(p + 4));
        } else {
            const int Hh = H >> 1, Wh = W >> 1;
            const long long o = (((long long)b * Hh + (gy >> 1)) * Wh + (gx >> 1)) * 64 + c;
            sgi_f32x4 lo = *(const sgi_f32x4 *)(X + o), hi = *(const sgi_f32x4 *)(X + o + 4);
            const unsigned i0 = *(const unsigned *)(I + o), i1 = *(const unsigned *)(I + o + 4);
            const unsigned sel = (unsigned)(((gy & 1) << 1) | (gx & 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (((i0 >> (8 * j)) & 0xffu) != sel) lo[j] = 0.f;
                if (((i1 >> (8 * j)) & 0xffu) != sel) hi[j] = 0.f;
            }
            v = sgi_pack8(lo, hi);
        }
    }
    return v;
}

// MODE SGI_CONV1: X (B,3,H,W) float32 planar 0..255, Wb (7,64,32) bf16 = (K step, n, k), k = 4 (tap - 8 step) + c,
// zero past tap 48.  SGI_ENC: X (B,H,W,64), Wb (49,64,64) bf16 = (tap, n, c).  Both write Y (B,H/2,W/2,64) pooled and
// Yi (B,H/2,W/2,64) uint8 argmax (ky * 2 + kx, first maximum).  SGI_DEC / SGI_DEC1: X, I (B,H/2,W/2,64) = the pooled
// map and indices of the matching encoder; Y (B,H,W,64), or for SGI_DEC1 (B,2,H,W) planar softmax probabilities
// (wc (2,64), bc (2) the classifier).  bias (64) float32.
template <int MODE>
__global__ __launch_bounds__(SGI_THREADS) void k_segnet_conv_bf16(const float *__restrict__ X,
                                                                  const uint8_t *__restrict__ I,
                                                                  const unsigned short *__restrict__ Wb,
                                                                  const float *__restrict__ bias,
                                                                  const float *__restrict__ wc,
                                                                  const float *__restrict__ bc, float *__restrict__ Y,
                                                                  uint8_t *__restrict__ Yi, int H, int W, SgiStd st)
{
    constexpr int PS = MODE == SGI_CONV1 ? 4 : SGI_PS;
    constexpr int NCH = MODE == SGI_CONV1 ? 1 : 2;                       // 32-channel chunks
    __shared__ __attribute__((aligned(16))) unsigned short xs[SGI_HPIX * PS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SGI_TH, tx0 = blockIdx.x * SGI_TW;
    const int Hh = H >> 1, Wh = W >> 1;

    // this lane's fragment pixel: tile row i = lane & 15 is pixel (i & 3) of 2x2 block i >> 2
    const int fi = lane & 15, fq = lane >> 4;
    const int frow = 2 * w + ((fi & 3) >> 1), fcol = 2 * (fi >> 2) + (fi & 1);

    sgi_f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = (sgi_f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < NCH; ++ch) {
        if (ch) __syncthreads();
        // ---- stage the bf16 halo of channels [32 ch, 32 ch + 32) (conv1: its 3 channels and a zero)
        if (MODE == SGI_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGI_HPIX; p += SGI_THREADS)
                *(uint2 *)&xs[p * PS] = sgi_conv1_px(xb, plane, ty0 - 3 + p / SGI_HW, tx0 - 3 + p % SGI_HW, H, W, st);
        } else {
            constexpr int IN = MODE == SGI_ENC ? SGI_ENC : SGI_DEC;
            for (int e = tid; e < SGI_HPIX * 4; e += SGI_THREADS) {
                const int p = e >> 2, q = e & 3;
                *(uint4 *)&xs[p * PS + 8 * q] =
                    sgi_px8<IN>(X, I, b, ty0 - 3 + p / SGI_HW, tx0 - 3 + p % SGI_HW, 32 * ch + 8 * q, H, W);
            }
        }
        __syncthreads();

        if (MODE == SGI_CONV1) {
            // lane quarter fq holds taps t0 = 8 s + 2 fq and t0 + 1 of K step s, 4 channels each
            const unsigned short *xr = &xs[(frow * SGI_HW + fcol) * PS];
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int t0 = 8 * s + 2 * fq, t1 = t0 + 1;
                const int o0 = ((t0 / 7) * SGI_HW + t0 % 7) * PS, o1 = ((t1 / 7) * SGI_HW + t1 % 7) * PS;
                sgi_bf16x8 bw[4], a[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    bw[nt] = *(const sgi_bf16x8 *)(Wb + ((long long)s * 64 + 16 * nt + fi) * 32 + 8 * fq);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint2 lo = t0 < 49 ? *(const uint2 *)&xr[o0 + 8 * m * PS] : make_uint2(0u, 0u);
                    const uint2 hi = t1 < 49 ? *(const uint2 *)&xr[o1 + 8 * m * PS] : make_uint2(0u, 0u);
                    a[m] = __builtin_bit_cast(sgi_bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bw[nt], acc[m][nt], 0, 0, 0);
            }
        } else {
            // K order inside a chunk: lane quarter fq holds channels 32 ch + 8 fq .. + 7 of both operands
            const unsigned short *wl = Wb + (long long)fi * 64 + 32 * ch + 8 * fq;
            for (int ky = 0; ky < 7; ++ky) {
                const unsigned short *xr = &xs[((frow + ky) * SGI_HW + fcol) * PS + 8 * fq];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const unsigned short *wt = wl + (long long)(ky * 7 + kx) * 64 * 64;
                    sgi_bf16x8 bw[4], a[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bw[nt] = *(const sgi_bf16x8 *)(wt + nt * 16 * 64);
#pragma unroll
                    for (int m = 0; m < 4; ++m) a[m] = *(const sgi_bf16x8 *)&xr[(kx + 8 * m) * PS];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
                            acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bw[nt], acc[m][nt], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue (k_segnet_conv's).  Lane: channel n = 16 nt + (lane & 15); register r = pixel r (ky * 2 + kx) of
    // block (lane >> 4) of MFMA tile m, i.e. output rows ty0 + 2w + (r >> 1), columns tx0 + 8m + 2 (lane >> 4) + (r & 1).
    const int oy = ty0 + 2 * w, ox = tx0 + 2 * fq;
    if (MODE == SGI_CONV1 || MODE == SGI_ENC) {
        const int py = oy >> 1;
        if (py >= Hh) return;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int px = (ox >> 1) + 4 * m;
            if (px >= Wh) continue;
            const long long o = (((long long)b * Hh + py) * Wh + px) * 64;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
                const float bn = bias[n];
                float best = 0.f;
                int arg = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = acc[m][nt][r] + bn;
                    v = v > 0.f ? v : 0.f;                            // relu
                    if (r == 0 || best < v) { best = v; arg = r; }     // first maximum in window order
                }
                Y[o + n] = best;
                Yi[o + n] = (uint8_t)arg;
            }
        }
    } else if (MODE == SGI_DEC) {
        if (oy >= H) return;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int x = ox + 8 * m;
            if (x >= W) continue;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
                const float bn = bias[n];
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Y[(((long long)b * H + oy + (r >> 1)) * W + x + (r & 1)) * 64 + n] = acc[m][nt][r] + bn;
            }
        }
    } else {
        // decode1: classifier over the 64 channels = this lane's four channels, then a butterfly over the 16 lanes of
        // the block (commutative pairwise sums: every lane of the group ends with the same bits), then the softmax
        float w0[4], w1[4], bn[4];
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            bn[nt] = bias[16 * nt + fi];
            w0[nt] = wc[16 * nt + fi];
            w1[nt] = wc[64 + 16 * nt + fi];
        }
        const float b0 = bc[0], b1 = bc[1];
        const long long plane = (long long)H * W;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            float z0[4], z1[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s0 = 0.f, s1 = 0.f;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const float h = acc[m][nt][r] + bn[nt];
                    s0 = fmaf(h, w0[nt], s0);
                    s1 = fmaf(h, w1[nt], s1);
                }
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) {
                    s0 += __shfl_xor(s0, d, 64);
                    s1 += __shfl_xor(s1, d, 64);
                }
                z0[r] = s0 + b0;
                z1[r] = s1 + b1;
            }
            const int x = ox + 8 * m;
            if (oy >= H || x >= W || fi >= 4) continue;
            float za = z0[0], zb = z1[0];
#pragma unroll
            for (int r = 1; r < 4; ++r)
                if (fi == r) { za = z0[r]; zb = z1[r]; }
            const float mx = za > zb ? za : zb;
            const float e0 = expf(za - mx), e1 = expf(zb - mx);
            const float sum = e0 + e1;
            const long long o = (long long)b * 2 * plane + (long long)(oy + (fi >> 1)) * W + x + (fi & 1);
            Y[o] = e0 / sum;
            Y[o + plane] = e1 / sum;
        }
    }
}

// the bf16 weights of a 64-channel layer: Wb[t][o][i] = bf16(Wt[t][o][i])
__global__ __launch_bounds__(256) void k_segnet_wpack64_bf16(const float *__restrict__ Wt,
                                                             unsigned short *__restrict__ Wb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 49 * 64 * 64) return;
    Wb[i] = (unsigned short)sgi_bits(Wt[i]);
}

// conv1's bf16 weights in K steps of 8 taps: Wb[s][n][k] = bf16(Wt[8 s + k / 4][n][k % 4]), zero past tap 48
__global__ __launch_bounds__(256) void k_segnet_wpack1_bf16(const float *__restrict__ Wt,
                                                            unsigned short *__restrict__ Wb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 7 * 64 * 32) return;
    const int s = i >> 11, n = (i >> 5) & 63, k = i & 31, t = 8 * s + (k >> 2);
    Wb[i] = t < 49 ? (unsigned short)sgi_bits(Wt[(t * 64 + n) * 4 + (k & 3)]) : (unsigned short)0;
}

// ---------------------------------------------------------------------------------------------------- C ABI
// The argument checks are spa_segnet_encode's / spa_segnet_decode's, in their order: the same shapes, layouts and
// alignments are taken and refused, and a refused call launches nothing.
static bool sgi_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

extern "C" int spa_segnet_encode_bf16(spa_ctx *ctx, const float *x, int32_t x_layout, int32_t B, int32_t H, int32_t W,
                                      int32_t Cin, const float *wt, const float *bias, const float *mean_host,
                                      const float *std_host, float *pooled, uint8_t *idx, void *stream)
{
    SPA_ARG(ctx && x && wt && bias && pooled && idx && B > 0 && B < 65536 && H > 0 && W > 0);
    SPA_ARG(Cin == 3 || Cin == 64);
    SPA_ARG(Cin == 3 ? (H % 16 == 0 && W % 16 == 0) : (H % 2 == 0 && W % 2 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SGI_TH < 65536);
    SPA_ARG(sgi_al16(x) && sgi_al16(wt));
    if (Cin == 3) {
        SPA_ARG(mean_host && std_host);
        if (x_layout != SPA_LAYOUT_NCHW) {
            spa_set_error("spa_segnet_encode_bf16: the conv1 input is the planar (B,3,H,W) image");
            return SPA_ERR_LAYOUT;
        }
    } else if (x_layout != SPA_LAYOUT_NHWC) {
        spa_set_error("spa_segnet_encode_bf16: 64-channel inputs must be channels-last (B,H,W,64)");
        return SPA_ERR_LAYOUT;
    }
    SgiStd st = {};
    if (Cin == 3)
        for (int c = 0; c < 3; ++c) { st.mean[c] = mean_host[c]; st.std[c] = std_host[c]; }
    unsigned short *wb = nullptr;
    int rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, 49 * 64 * 64 * sizeof(unsigned short), (void **)&wb);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    if (Cin == 3)
        hipLaunchKernelGGL(k_segnet_wpack1_bf16, dim3(7 * 64 * 32 / 256), dim3(256), 0, s, wt, wb);
    else
        hipLaunchKernelGGL(k_segnet_wpack64_bf16, dim3(49 * 64 * 64 / 256), dim3(256), 0, s, wt, wb);
    SPA_LAUNCH_CHECK();
    dim3 grid((W + SGI_TW - 1) / SGI_TW, (H + SGI_TH - 1) / SGI_TH, B);
    if (Cin == 3)
        hipLaunchKernelGGL(k_segnet_conv_bf16<SGI_CONV1>, grid, dim3(SGI_THREADS), 0, s, x, nullptr, wb, bias, nullptr,
                           nullptr, pooled, idx, H, W, st);
    else
        hipLaunchKernelGGL(k_segnet_conv_bf16<SGI_ENC>, grid, dim3(SGI_THREADS), 0, s, x, nullptr, wb, bias, nullptr,
                           nullptr, pooled, idx, H, W, st);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode_bf16(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                      int32_t Hh, int32_t Wh, const float *wt, const float *bias, const float *wc,
                                      const float *bc, float *y, void *stream)
{
    SPA_ARG(ctx && x && idx && wt && bias && y && B > 0 && B < 65536 && Hh > 0 && Wh > 0);
    SPA_ARG((wc == nullptr) == (bc == nullptr));
    const int H = 2 * Hh, W = 2 * Wh;
    SPA_ARG(!wc || (H % 16 == 0 && W % 16 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SGI_TH < 65536);
    SPA_ARG(sgi_al16(x) && sgi_al16(wt) && ((uintptr_t)idx & 3) == 0);
    if (x_layout != SPA_LAYOUT_NHWC) {
        spa_set_error("spa_segnet_decode_bf16: the pooled map and its indices must be channels-last (B,H/2,W/2,64)");
        return SPA_ERR_LAYOUT;
    }
    unsigned short *wb = nullptr;
    int rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, 49 * 64 * 64 * sizeof(unsigned short), (void **)&wb);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    hipLaunchKernelGGL(k_segnet_wpack64_bf16, dim3(49 * 64 * 64 / 256), dim3(256), 0, s, wt, wb);
    SPA_LAUNCH_CHECK();
    dim3 grid((W + SGI_TW - 1) / SGI_TW, (H + SGI_TH - 1) / SGI_TH, B);
    if (wc)
        hipLaunchKernelGGL(k_segnet_conv_bf16<SGI_DEC1>, grid, dim3(SGI_THREADS), 0, s, x, idx, wb, bias, wc, bc, y,
                           nullptr, H, W, SgiStd{});
    else
        hipLaunchKernelGGL(k_segnet_conv_bf16<SGI_DEC>, grid, dim3(SGI_THREADS), 0, s, x, idx, wb, bias, nullptr,
                           nullptr, y, nullptr, H, W, SgiStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
