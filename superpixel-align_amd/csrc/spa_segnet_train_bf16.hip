// SegNet-Basic training (train_segnet.py --dtype bf16) on the bf16 matrix cores: the eight pass forms of
// spa_segnet_train.hip -- forward (conv1's image, a 64-channel map, the decoder's unpooled map), dgrad (plain and the
// decoder's pooled-gradient gather) and wgrad (conv1, encoder, decoder) -- with bf16 operands and float32 accumulation.
//
// Operands and outputs stay float32 in memory.  Every product operand is the round-to-nearest-even bf16 of the float32
// value the float32 kernels use at that point, rounded while it is staged: the standardised, LRN-normalised conv1
// input (computed in float32 exactly as sgt_conv1_px computes it), the map values and the unpooled value, dy, and the
// weights (rounded once per call into a packed bf16 copy in the context workspace).  The products are
// v_mfma_f32_16x16x32_bf16 accumulating in float32; y, dx, the BN partial sums (float32 per workgroup, reduced in
// float64 in block order) and dW (split-K, the chunks summed in chunk order in float64) are float32 as before.  No
// atomics; the work split depends on the shape only, so the bits do not depend on the run or the device.
//
// Forward and dgrad keep the float32 kernel's tiling (one workgroup = 8 x 32 output pixels x 64 channels, wave w owns
// rows 2w, 2w + 1, a 16-row MFMA tile = four 2x2 blocks).  The A operand is 16 pixels x 32 input channels: a lane
// reads 8 consecutive channels of one pixel (16 bytes) from a channels-last bf16 halo in LDS, staged in two 32-channel
// chunks.  conv1's K is (tap, channel) with the 3 channels padded to 4: a 32-wide K step packs 8 taps, the 49 taps
// fill 7 steps with the last 7 zero.
//
// wgrad sums over pixels: K = 32 consecutive pixels of one row.  The gradient tile and the shifted input rows are
// staged channels-last in LDS and read with ds_read_b64_tr_b16, which turns 4 pixels x 16 channels into each lane's
// 4 pixels of one channel: two reads make a K step's fragment for either operand, at any pixel shift kx.
#include "spa_common.h"

typedef float sgb_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 sgb_bf16x8 __attribute__((ext_vector_type(8)));
typedef short sgb_s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) sgb_s16x4 sgb_lds_s16x4;

#define SGB_TH 8
#define SGB_TW 32
#define SGB_HH (SGB_TH + 6)
#define SGB_HW (SGB_TW + 6)
#define SGB_HPIX (SGB_HH * SGB_HW)
#define SGB_THREADS 256
#define SGB_PS 40                    // LDS bf16 per staged pixel of a 32-channel chunk (64 bytes + 16 of padding)

enum { SGB_CONV1 = 0, SGB_ENC = 1, SGB_DEC = 2 };
enum { SGB_FULL = 0, SGB_POOLED = 1 };

struct SgbStd {
    float mean[3], std[3];
};

__device__ __forceinline__ unsigned sgb_bits(float f)
{
    const __bf16 h = (__bf16)f;                    // round to nearest even; subnormals kept, NaN stays NaN
    return (unsigned)__builtin_bit_cast(unsigned short, h);
}

__device__ __forceinline__ unsigned sgb_pack2(float a, float b) { return sgb_bits(a) | (sgb_bits(b) << 16); }

__device__ __forceinline__ uint4 sgb_pack8(sgb_f32x4 lo, sgb_f32x4 hi)
{
    return make_uint4(sgb_pack2(lo.x, lo.y), sgb_pack2(lo.z, lo.w), sgb_pack2(hi.x, hi.y), sgb_pack2(hi.z, hi.w));
}

// Chainer's local_response_normalization with three channels: the float32 operations of sgt_lrn3
__device__ __forceinline__ void sgb_lrn3(float &a, float &b, float &c)
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

// the standardised, LRN-normalised conv1 input at (gy, gx) as sgt_conv1_px computes it, rounded to bf16 (4 values,
// channel 3 zero); zero outside the image
__device__ __forceinline__ uint2 sgb_conv1_px(const float *xb, long long plane, int gy, int gx, int H, int W,
                                              const SgbStd &st)
{
    float r = 0.f, g = 0.f, bl = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        const long long o = (long long)gy * W + gx;
        r = xb[o];
        g = xb[plane + o];
        bl = xb[2 * plane + o];
        r = (r - st.mean[0]) / st.std[0];
        g = (g - st.mean[1]) / st.std[1];
        bl = (bl - st.mean[2]) / st.std[2];
        sgb_lrn3(r, g, bl);
    }
    return make_uint2(sgb_pack2(r, g), sgb_pack2(bl, 0.f));
}

// channels [c, c + 8) of the 64-channel input at full-resolution (gy, gx) as bf16: ENC reads the map, DEC the pooled
// map at (gy/2, gx/2) where its index selects (gy & 1, gx & 1), zero elsewhere; zero outside the image
template <int MODE>
__device__ __forceinline__ uint4 sgb_px8(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H, int W)
{
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        if (MODE == SGB_ENC) {
            const float *p = X + (((long long)b * H + gy) * W + gx) * 64 + c;
            v = sgb_pack8(*(const sgb_f32x4 *)p, *(const sgb_f32x4 *)(p + 4));
        } else {
            const int Hh = H >> 1, Wh = W >> 1;
            const long long o = (((long long)b * Hh + (gy >> 1)) * Wh + (gx >> 1)) * 64 + c;
            sgb_f32x4 lo = *(const sgb_f32x4 *)(X + o), hi = *(const sgb_f32x4 *)(X + o + 4);
            const unsigned i0 = *(const unsigned *)(I + o), i1 = *(const unsigned *)(I + o + 4);
            const unsigned sel = (unsigned)(((gy & 1) << 1) | (gx & 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (((i0 >> (8 * j)) & 0xffu) != sel) lo[j] = 0.f;
                if (((i1 >> (8 * j)) & 0xffu) != sel) hi[j] = 0.f;
            }
            v = sgb_pack8(lo, hi);
        }
    }
    return v;
}

// Y = conv7x7(input form MODE of X (, I); Wb) at output resolution (H, W).  Wb bf16: (49,64,64) = (tap, n, c) for the
// 64-channel forms, (7,64,32) = (K step, n, k) for conv1 (k = 4 (tap - 8 step) + c, zero past tap 48).
// EPI SGB_FULL: Y (B,H,W,64); with part != NULL also part[blk][0..63] = sum y, part[blk][64..127] = sum y^2 over the
// workgroup's in-image pixels (blk = (b * gridDim.y + tile row) * gridDim.x + tile column).
// EPI SGB_POOLED: Y (B,H/2,W/2,64) = the value at the position Io (B,H/2,W/2,64) selects in each 2x2 block.
template <int MODE, int EPI>
__global__ __launch_bounds__(SGB_THREADS) void k_sgb_conv(const float *__restrict__ X, const uint8_t *__restrict__ I,
                                                          const unsigned short *__restrict__ Wb,
                                                          const uint8_t *__restrict__ Io, float *__restrict__ Y,
                                                          float *__restrict__ part, int H, int W, SgbStd st)
{
    constexpr int PS = MODE == SGB_CONV1 ? 4 : SGB_PS;
    constexpr int NCH = MODE == SGB_CONV1 ? 1 : 2;                       // 32-channel chunks
    constexpr int NB = SGB_HPIX * PS * 2 > 8192 ? SGB_HPIX * PS * 2 : 8192;  // the halo, or the BN reduction
    __shared__ __attribute__((aligned(16))) unsigned short xs[NB / 2];
    float *red = (float *)xs;

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SGB_TH, tx0 = blockIdx.x * SGB_TW;

    const int fi = lane & 15, fq = lane >> 4;
    const int frow = 2 * w + ((fi & 3) >> 1), fcol = 2 * (fi >> 2) + (fi & 1);

    sgb_f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = (sgb_f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < NCH; ++ch) {
        if (ch) __syncthreads();
        if (MODE == SGB_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGB_HPIX; p += SGB_THREADS)
                *(uint2 *)&xs[p * PS] = sgb_conv1_px(xb, plane, ty0 - 3 + p / SGB_HW, tx0 - 3 + p % SGB_HW, H, W, st);
        } else {
            for (int e = tid; e < SGB_HPIX * 4; e += SGB_THREADS) {
                const int p = e >> 2, q = e & 3;
                *(uint4 *)&xs[p * PS + 8 * q] =
                    sgb_px8<MODE>(X, I, b, ty0 - 3 + p / SGB_HW, tx0 - 3 + p % SGB_HW, 32 * ch + 8 * q, H, W);
            }
        }
        __syncthreads();

        if (MODE == SGB_CONV1) {
            // lane quarter fq holds taps t0 = 8 s + 2 fq and t0 + 1 of K step s, 4 channels each
            const unsigned short *xr = &xs[(frow * SGB_HW + fcol) * PS];
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int t0 = 8 * s + 2 * fq, t1 = t0 + 1;
                const int o0 = ((t0 / 7) * SGB_HW + t0 % 7) * PS, o1 = ((t1 / 7) * SGB_HW + t1 % 7) * PS;
                sgb_bf16x8 bw[4], a[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    bw[nt] = *(const sgb_bf16x8 *)(Wb + ((long long)s * 64 + 16 * nt + fi) * 32 + 8 * fq);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint2 lo = t0 < 49 ? *(const uint2 *)&xr[o0 + 8 * m * PS] : make_uint2(0u, 0u);
                    const uint2 hi = t1 < 49 ? *(const uint2 *)&xr[o1 + 8 * m * PS] : make_uint2(0u, 0u);
                    a[m] = __builtin_bit_cast(sgb_bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bw[nt], acc[m][nt], 0, 0, 0);
            }
        } else {
            const unsigned short *wl = Wb + (long long)fi * 64 + 32 * ch + 8 * fq;
            for (int ky = 0; ky < 7; ++ky) {
                const unsigned short *xr = &xs[((frow + ky) * SGB_HW + fcol) * PS + 8 * fq];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const unsigned short *wt = wl + (long long)(ky * 7 + kx) * 64 * 64;
                    sgb_bf16x8 bw[4], a[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) bw[nt] = *(const sgb_bf16x8 *)(wt + nt * 16 * 64);
#pragma unroll
                    for (int m = 0; m < 4; ++m) a[m] = *(const sgb_bf16x8 *)&xr[(kx + 8 * m) * PS];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
                            acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], bw[nt], acc[m][nt], 0, 0, 0);
                }
            }
        }
    }

    // epilogue (the float32 kernel's): lane holds channel n = 16 nt + fi, register r = pixel (r >> 1, r & 1) of the
    // 2x2 block at output rows oy, oy + 1 and columns x, x + 1 with x = ox + 8 m.  H and W are even.
    const int oy = ty0 + 2 * w, ox = tx0 + 2 * fq;
    const bool row_in = oy < H;
    if (EPI == SGB_FULL) {
        float s[4] = {0.f, 0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int x = ox + 8 * m;
            if (x >= W || !row_in) continue;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[m][nt][r];
                    Y[(((long long)b * H + oy + (r >> 1)) * W + x + (r & 1)) * 64 + n] = v;
                    s[nt] += v;
                    q[nt] = fmaf(v, v, q[nt]);
                }
            }
        }
        if (part) {
            // fixed order: lanes' sums -> LDS [wave][fq][channel], then 128 threads add the 16 entries of a channel
            __syncthreads();                                           // xs is free once every wave left the K loop
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
                red[((w * 4 + fq) * 64 + n) * 2] = s[nt];
                red[((w * 4 + fq) * 64 + n) * 2 + 1] = q[nt];
            }
            __syncthreads();
            if (tid < 128) {
                const int n = tid & 63, k = tid >> 6;
                float t = 0.f;
                for (int j = 0; j < 16; ++j) t += red[(j * 64 + n) * 2 + k];
                const long long blk = ((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
                part[blk * 128 + k * 64 + n] = t;
            }
        }
    } else {
        const int Hh = H >> 1, Wh = W >> 1;
        const int py = oy >> 1;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int px = (ox >> 1) + 4 * m;
            if (px >= Wh || py >= Hh) continue;
            const long long o = (((long long)b * Hh + py) * Wh + px) * 64;
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = 16 * nt + fi;
                const int r = Io[o + n];
                const sgb_f32x4 a = acc[m][nt];
                Y[o + n] = r == 0 ? a[0] : r == 1 ? a[1] : r == 2 ? a[2] : a[3];
            }
        }
    }
}

// stats[k * 64 + n] = sum over the nblk partials of part[blk][k * 64 + n], in block order, in double: the reduction
// of k_sgt_bnstat (one workgroup per (k, n); thread t takes blocks t, t + 256, ...; then a fixed tree)
__global__ __launch_bounds__(256) void k_sgb_bnstat(const float *__restrict__ part, long long nblk,
                                                    double *__restrict__ stats)
{
    __shared__ double red[256];
    const int j = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (long long i = t; i < nblk; i += 256) s += (double)part[i * 128 + j];
    red[t] = s;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) red[t] += red[t + d];
        __syncthreads();
    }
    if (t == 0) stats[j] = red[0];
}

// the bf16 weights of a 64-channel layer: Wb[t][o][i] = bf16(Wt[t][o][i]), or with rot (dgrad) bf16(Wt[48 - t][i][o])
__global__ __launch_bounds__(256) void k_sgb_wpack64(const float *__restrict__ Wt, int rot,
                                                     unsigned short *__restrict__ Wb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 49 * 64 * 64) return;
    const int t = i / 4096, o = (i >> 6) & 63, c = i & 63;
    Wb[i] = (unsigned short)sgb_bits(rot ? Wt[((48 - t) * 64 + c) * 64 + o] : Wt[i]);
}

// conv1's bf16 weights in K steps of 8 taps: Wb[s][n][k] = bf16(Wt[8 s + k / 4][n][k % 4]), zero past tap 48
__global__ __launch_bounds__(256) void k_sgb_wpack1(const float *__restrict__ Wt, unsigned short *__restrict__ Wb)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 7 * 64 * 32) return;
    const int s = i >> 11, n = (i >> 5) & 63, k = i & 31, t = 8 * s + (k >> 2);
    Wb[i] = t < 49 ? (unsigned short)sgb_bits(Wt[(t * 64 + n) * 4 + (k & 3)]) : (unsigned short)0;
}

// ---------------------------------------------------------------------------------------------------- wgrad
#define SGBW_TR 2                    // tile rows: one K step each
#define SGBW_TW 32                   // tile columns = the K step's 32 pixels
#define SGBW_GS 72                   // LDS bf16 per staged 64-channel pixel (128 bytes + 16 of padding)
#define SGBW_MAXCH 96                // chunks of K at most

static inline int sgb_wgrad_chunks(long long tiles) { return (int)(tiles < SGBW_MAXCH ? tiles : SGBW_MAXCH); }

// one K step's bf16 operand fragment from two transposed LDS reads: p0 the lane's address for pixels k .. k + 3, p1
// for k + 4 .. k + 7 (ds_read_b64_tr_b16: lane 4q + p of each 16-lane group names row q, columns 4p .. 4p + 3 of a
// 4 x 16 block; lane i receives column i of the 4 rows).  Every lane of the wave must take part.
__device__ __forceinline__ sgb_bf16x8 sgb_tr8(const unsigned short *p0, const unsigned short *p1)
{
    const sgb_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((sgb_lds_s16x4 *)p0);
    const sgb_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((sgb_lds_s16x4 *)p1);
    return __builtin_bit_cast(sgb_bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// part[(chunk * 49 + ky * 7 + kx) * 64 * CP + n * CP + c] = the chunk's sum of G[p][n] * X[p + (ky - 3, kx - 3)][c].
// G (B,H,W,64) channels-last.  Grid (chunks, 7): blockIdx.y = ky.  K step s of a tile = its row s, k = column.
// MFMA A = G (rows n, lane 16-group fq holds pixels 8 fq .. 8 fq + 7), B = X shifted by the tap (columns c).
// 64-channel forms: wave w owns channels c = 16 w .. 16 w + 15 of all seven taps of the row and all 64 n.
// conv1 (CP 4): the 16 MFMA columns are (kx, c) = (4 ct + (j >> 2), j & 3) for column tiles ct 0, 1 (kx 7 is
// discarded); wave w owns column tile w >> 1 and the row tiles nt = 2 (w & 1), 2 (w & 1) + 1.
template <int MODE>
__global__ __launch_bounds__(SGB_THREADS) void k_sgb_wgrad(const float *__restrict__ G, const float *__restrict__ X,
                                                           const uint8_t *__restrict__ I, float *__restrict__ part,
                                                           int B, int H, int W, int nch, SgbStd st)
{
    constexpr int CP = MODE == SGB_CONV1 ? 4 : 64;
    constexpr int XW = MODE == SGB_CONV1 ? SGBW_TW + 8 : SGBW_TW + 6;     // staged input columns (conv1: kx 7 too)
    constexpr int XS = MODE == SGB_CONV1 ? 4 : SGBW_GS;                    // LDS bf16 per staged input pixel
    __shared__ __attribute__((aligned(16))) unsigned short gs[SGBW_TR * SGBW_TW * SGBW_GS];
    __shared__ __attribute__((aligned(16))) unsigned short xs[SGBW_TR * XW * XS];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fi = lane & 15, fq = lane >> 4;
    const int ky = blockIdx.y, chunk = blockIdx.x;
    const int txn = (W + SGBW_TW - 1) / SGBW_TW, tyn = H / SGBW_TR;
    const long long tiles = (long long)B * tyn * txn;
    const long long t0 = tiles * chunk / nch, t1 = tiles * (chunk + 1) / nch;
    const long long plane = (long long)H * W;

    constexpr int NA = MODE == SGB_CONV1 ? 2 : 7;
    constexpr int NT = MODE == SGB_CONV1 ? 2 : 4;
    const int nt0 = MODE == SGB_CONV1 ? 2 * (w & 1) : 0;
    sgb_f32x4 acc[NA][NT];
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[a][nt] = (sgb_f32x4){0.f, 0.f, 0.f, 0.f};

    // the lane's transposed-read addresses (pixel row (fi >> 2) of the 4-pixel block, column group fi & 3)
    const int kp = 8 * fq + (fi >> 2);
    const unsigned short *ga = &gs[kp * SGBW_GS + 4 * (fi & 3)];
    const unsigned short *xa = MODE == SGB_CONV1 ? &xs[(kp + 4 * (w >> 1) + (fi & 3)) * XS]
                                                 : &xs[kp * XS + 16 * w + 4 * (fi & 3)];

    for (long long t = t0; t < t1; ++t) {
        const int tx = (int)(t % txn);
        const long long r2 = t / txn;
        const int ty = (int)(r2 % tyn), b = (int)(r2 / tyn);
        const int y0 = ty * SGBW_TR, x0 = tx * SGBW_TW;
        if (t != t0) __syncthreads();
        // stage G (zero past the right edge: those pixels contribute nothing) and the input rows y0 + ky - 3 + r
        for (int e = tid; e < SGBW_TR * SGBW_TW * 8; e += SGB_THREADS) {
            const int p = e >> 3, q = e & 7;
            const int gy = y0 + p / SGBW_TW, gx = x0 + p % SGBW_TW;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (gx < W) {
                const float *g = G + (((long long)b * H + gy) * W + gx) * 64 + 8 * q;
                v = sgb_pack8(*(const sgb_f32x4 *)g, *(const sgb_f32x4 *)(g + 4));
            }
            *(uint4 *)&gs[p * SGBW_GS + 8 * q] = v;
        }
        if (MODE == SGB_CONV1) {
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGBW_TR * XW; p += SGB_THREADS)
                *(uint2 *)&xs[p * XS] = sgb_conv1_px(xb, plane, y0 + ky - 3 + p / XW, x0 - 3 + p % XW, H, W, st);
        } else {
            for (int e = tid; e < SGBW_TR * XW * 8; e += SGB_THREADS) {
                const int p = e >> 3, q = e & 7;
                *(uint4 *)&xs[p * XS + 8 * q] =
                    sgb_px8<MODE>(X, I, b, y0 + ky - 3 + p / XW, x0 - 3 + p % XW, 8 * q, H, W);
            }
        }
        __syncthreads();

#pragma unroll
        for (int s = 0; s < SGBW_TR; ++s) {
            sgb_bf16x8 a[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const unsigned short *p0 = ga + s * SGBW_TW * SGBW_GS + 16 * (nt0 + nt);
                a[nt] = sgb_tr8(p0, p0 + 4 * SGBW_GS);
            }
            if (MODE == SGB_CONV1) {
                const unsigned short *p0 = xa + s * XW * XS;
                const sgb_bf16x8 bx = sgb_tr8(p0, p0 + 4 * XS);
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt], bx, acc[0][nt], 0, 0, 0);
            } else {
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const unsigned short *p0 = xa + (s * XW + kx) * XS;
                    const sgb_bf16x8 bx = sgb_tr8(p0, p0 + 4 * XS);
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[kx][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[nt], bx, acc[kx][nt], 0, 0, 0);
                }
            }
        }
    }

    // D layout: column (c or (kx, c)) = lane & 15, row n = 16 nt + 4 (lane >> 4) + r
    float *pb = part + ((long long)chunk * 49 + ky * 7) * 64 * CP;
    if (MODE == SGB_CONV1) {
        const int kx = 4 * (w >> 1) + (fi >> 2), c = fi & 3;
        if (kx < 7) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    pb[((long long)kx * 64 + 16 * (nt0 + nt) + 4 * fq + r) * CP + c] = acc[0][nt][r];
        }
    } else {
        const int c = 16 * w + fi;
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) pb[((long long)kx * 64 + 16 * nt + 4 * fq + r) * CP + c] = acc[kx][nt][r];
    }
}

// dw[i] = sum over chunks j = 0 .. nch - 1 of part[j * n + i], in chunk order, in double, rounded once (k_sgt_wsum)
__global__ __launch_bounds__(256) void k_sgb_wsum(const float *__restrict__ part, int nch, int n, float *__restrict__ dw)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int j = 0; j < nch; ++j) s += (double)part[(long long)j * n + i];
    dw[i] = (float)s;
}

// ---------------------------------------------------------------------------------------------------- C ABI
// The argument checks are the float32 entry points' (spa_segnet_train.hip): the same shapes, layouts and alignments
// are taken and refused, and a refused call launches nothing.
static bool sgb_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

static int sgb_check_shape(int B, int H, int W, int Cin)
{
    SPA_ARG(B > 0 && B < 65536 && H > 0 && W > 0);
    SPA_ARG(Cin == 3 ? (H % 16 == 0 && W % 16 == 0) : (H % 2 == 0 && W % 2 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SGB_TH < 65536);
    return SPA_OK;
}

static int sgb_input_form(const char *fn, int32_t Cin, int32_t x_layout, const float *mean_host, const float *std_host,
                          const uint8_t *idx, SgbStd *st)
{
    SPA_ARG(Cin == 3 || Cin == 64);
    if (Cin == 3) {
        SPA_ARG(mean_host && std_host && !idx);
        if (x_layout != SPA_LAYOUT_NCHW) {
            spa_set_error("%s: the conv1 input is the planar (B,3,H,W) image", fn);
            return SPA_ERR_LAYOUT;
        }
        for (int c = 0; c < 3; ++c) { st->mean[c] = mean_host[c]; st->std[c] = std_host[c]; }
    } else {
        SPA_ARG(((uintptr_t)idx & 3) == 0);
        if (x_layout != SPA_LAYOUT_NHWC) {
            spa_set_error("%s: 64-channel inputs (and index maps) must be channels-last", fn);
            return SPA_ERR_LAYOUT;
        }
    }
    return SPA_OK;
}

extern "C" int spa_segnet_train_forward_bf16(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout,
                                             int32_t B, int32_t H, int32_t W, int32_t Cin, const float *wt,
                                             const float *mean_host, const float *std_host, float *y, double *stats,
                                             void *stream)
{
    SPA_ARG(ctx && x && wt && y);
    int rc = sgb_check_shape(B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgb_al16(x) && sgb_al16(wt));
    SgbStd st = {};
    rc = sgb_input_form("spa_segnet_train_forward_bf16", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    hipStream_t s = spa_stream(stream);
    dim3 grid((W + SGB_TW - 1) / SGB_TW, (H + SGB_TH - 1) / SGB_TH, B);
    const long long nblk = (long long)grid.x * grid.y * grid.z;
    unsigned short *wb = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, 49 * 64 * 64 * sizeof(unsigned short), (void **)&wb)) != SPA_OK)
        return rc;
    float *part = nullptr;
    if (stats) {
        if ((rc = spa_ws_reserve(ctx, WS_SEGNET_BNPART, (size_t)nblk * 128 * sizeof(float), (void **)&part)) != SPA_OK)
            return rc;
    }
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgb_wpack1, dim3(7 * 64 * 32 / 256), dim3(256), 0, s, wt, wb);
    else
        hipLaunchKernelGGL(k_sgb_wpack64, dim3(49 * 64 * 64 / 256), dim3(256), 0, s, wt, 0, wb);
    SPA_LAUNCH_CHECK();
    if (Cin == 3)
        hipLaunchKernelGGL((k_sgb_conv<SGB_CONV1, SGB_FULL>), grid, dim3(SGB_THREADS), 0, s, x, nullptr, wb, nullptr,
                           y, part, H, W, st);
    else if (!idx)
        hipLaunchKernelGGL((k_sgb_conv<SGB_ENC, SGB_FULL>), grid, dim3(SGB_THREADS), 0, s, x, nullptr, wb, nullptr, y,
                           part, H, W, st);
    else
        hipLaunchKernelGGL((k_sgb_conv<SGB_DEC, SGB_FULL>), grid, dim3(SGB_THREADS), 0, s, x, idx, wb, nullptr, y,
                           part, H, W, st);
    SPA_LAUNCH_CHECK();
    if (stats) {
        hipLaunchKernelGGL(k_sgb_bnstat, dim3(128), dim3(256), 0, s, part, nblk, stats);
        SPA_LAUNCH_CHECK();
    }
    return SPA_OK;
}

extern "C" int spa_segnet_train_dgrad_bf16(spa_ctx *ctx, const float *dy, const float *wt, const uint8_t *idx,
                                           int32_t B, int32_t H, int32_t W, float *dx, void *stream)
{
    SPA_ARG(ctx && dy && wt && dx);
    int rc = sgb_check_shape(B, H, W, 64);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgb_al16(dy) && sgb_al16(wt) && ((uintptr_t)idx & 3) == 0);
    unsigned short *wb = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WBF16, 49 * 64 * 64 * sizeof(unsigned short), (void **)&wb)) != SPA_OK)
        return rc;
    hipStream_t s = spa_stream(stream);
    hipLaunchKernelGGL(k_sgb_wpack64, dim3(49 * 64 * 64 / 256), dim3(256), 0, s, wt, 1, wb);
    SPA_LAUNCH_CHECK();
    dim3 grid((W + SGB_TW - 1) / SGB_TW, (H + SGB_TH - 1) / SGB_TH, B);
    if (idx)
        hipLaunchKernelGGL((k_sgb_conv<SGB_ENC, SGB_POOLED>), grid, dim3(SGB_THREADS), 0, s, dy, nullptr, wb, idx, dx,
                           nullptr, H, W, SgbStd{});
    else
        hipLaunchKernelGGL((k_sgb_conv<SGB_ENC, SGB_FULL>), grid, dim3(SGB_THREADS), 0, s, dy, nullptr, wb, nullptr,
                           dx, nullptr, H, W, SgbStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_train_wgrad_bf16(spa_ctx *ctx, const float *dy, const float *x, const uint8_t *idx,
                                           int32_t x_layout, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                           const float *mean_host, const float *std_host, float *dw, void *stream)
{
    SPA_ARG(ctx && dy && x && dw);
    int rc = sgb_check_shape(B, H, W, Cin);
    if (rc != SPA_OK) return rc;
    SPA_ARG(sgb_al16(dy) && sgb_al16(x));
    SgbStd st = {};
    rc = sgb_input_form("spa_segnet_train_wgrad_bf16", Cin, x_layout, mean_host, std_host, idx, &st);
    if (rc != SPA_OK) return rc;
    const int CP = Cin == 3 ? 4 : 64;
    const long long tiles = (long long)B * (H / SGBW_TR) * ((W + SGBW_TW - 1) / SGBW_TW);
    const int nch = sgb_wgrad_chunks(tiles);
    const int n = 49 * 64 * CP;
    float *part = nullptr;
    if ((rc = spa_ws_reserve(ctx, WS_SEGNET_WGRAD, (size_t)nch * n * sizeof(float), (void **)&part)) != SPA_OK)
        return rc;
    hipStream_t s = spa_stream(stream);
    dim3 grid(nch, 7);
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgb_wgrad<SGB_CONV1>, grid, dim3(SGB_THREADS), 0, s, dy, x, nullptr, part, B, H, W, nch,
                           st);
    else if (!idx)
        hipLaunchKernelGGL(k_sgb_wgrad<SGB_ENC>, grid, dim3(SGB_THREADS), 0, s, dy, x, nullptr, part, B, H, W, nch, st);
    else
        hipLaunchKernelGGL(k_sgb_wgrad<SGB_DEC>, grid, dim3(SGB_THREADS), 0, s, dy, x, idx, part, B, H, W, nch, st);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sgb_wsum, dim3((n + 255) / 256), dim3(256), 0, s, part, nch, n, dw);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
