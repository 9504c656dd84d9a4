// SegNet-Basic inference at float32 accuracy on the f16 matrix cores (labels_from_segnet.py --split_planes): the four
// layer forms of spa_segnet.hip -- conv1 (the planar image, standardised and LRN-normalised in the load), conv2-4 (a
// 64-channel map), decode4-2 (the pooled map unpooled through its index map in the load) and decode1 (the same, plus
// the 1x1 classifier and the softmax) -- with every float32 operand carried as two half-precision planes and three
// products per float32 product.  The main loop is k_sgh_conv's (spa_segnet_train_f16x3.hip), the epilogues are
// k_segnet_conv's as k_segnet_conv_bf16 restates them for the 16x16x32 C/D layout.
//
// Numeric contract.  Each operand gets one power of two t = 2^k that brings its largest magnitude into [2^14, 2^15)
// (k = 0 for an all-zero operand): the folded weights get one exponent, the activations ONE PER IMAGE -- conv1's
// operand as k_segnet_conv computes it (the float32 operations of sg_lrn3), the map, or a decoder's pooled map (its
// unpooled values are a subset of it).  A per-batch scale would make an image's planes depend on its neighbours; with
// a per-image one an image's outputs have the same bits whatever the batch size and its position in the batch.  A
// value v becomes h = f16_rn(t v), l = f16_rn(t v - h); a product a b is h_a h_b + h_a l_b + l_a h_b: three
// v_mfma_f32_16x16x32_f16 accumulating in float32, the two cross terms issued first and kept in accumulators of their
// own, added to the h_a h_b accumulators in the epilogue (l_a l_b, 2^-22 of the product, is dropped).  The epilogue
// multiplies by 2^-(k_x + k_w) (v_ldexp, exact) BEFORE the bias is added; everything after that is the float32
// inference epilogue, operation for operation: bias, ReLU, 2x2 max-pool with the first maximum's index in window order,
// and decode1's classifier fmaf chain, 16-lane butterfly and softmax.  Maps, indices and probabilities keep the float32
// path's types, shapes and layouts, so spa_segnet_score follows unchanged.
//
// The exponents are computed on the device inside each call: per-workgroup maxima of |v| (bit patterns: non-negative
// floats order as unsigned integers) in one launch -- blockIdx.x = image, the last one the weights -- then one
// workgroup per exponent reduces them.  A max is exact in any order, no atomics are used and the host never waits.
// The weights are split once per call into a packed f16 plane pair in the context workspace, stream-ordered.
//
// Tiling: one workgroup = 8 x 32 output pixels x 64 channels, 4 waves, wave w owns output rows 2w, 2w + 1; a 16-row
// MFMA tile = four 2x2 pooling blocks, so the C/D layout (row = 4 (lane >> 4) + reg) puts one pooling window in the four
// accumulator registers of one lane.  The halo holds a pixel's 32-channel chunk as [32 h | 32 l] (144 bytes with
// padding: 14 x 38 pixels = 74.8 KiB, two workgroups per CU, conflict-free ds_read_b128), staged in two chunks.
// conv1's K is (tap, channel) with the 3 channels padded to 4: a 32-wide K step packs 8 taps, the 49 taps fill 7 steps
// with the last 7 zero.
#include "spa_common.h"

typedef float sgx_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 sgx_f16x8 __attribute__((ext_vector_type(8)));

#define SGX_TH 8                       // output tile rows
#define SGX_TW 32                      // output tile columns
#define SGX_HH (SGX_TH + 6)            // halo rows
#define SGX_HW (SGX_TW + 6)            // halo columns
#define SGX_HPIX (SGX_HH * SGX_HW)     // 532 halo pixels
#define SGX_THREADS 256
#define SGX_PS 72                      // LDS f16 per staged pixel of a 32-channel chunk: 32 h, 32 l, 16 bytes of padding
#define SGX_NAMAX 256                  // workgroups of one operand's max reduction
#define SGX_W64 (49 * 64 * 64)         // f16 per plane of a 64-channel layer's weights
#define SGX_W1 (7 * 64 * 32)           // f16 per plane of conv1's weights

enum { SGX_CONV1 = 0, SGX_ENC = 1, SGX_DEC = 2, SGX_DEC1 = 3 };

struct SgxStd {
    float mean[3], std[3];
};

// 2^k as a float (k in [-113, 126], as k_sgx_scale produces)
__device__ __forceinline__ float sgx_pow2(int k) { return __uint_as_float((unsigned)(127 + k) << 23); }

// h = f16_rn(v sc), l = f16_rn(v sc - h) as bit patterns (sc a power of two: v sc and the difference are exact)
__device__ __forceinline__ void sgx_split(float v, float sc, unsigned short &h, unsigned short &l)
{
    const float s = v * sc;
    const _Float16 hh = (_Float16)s;
    const _Float16 ll = (_Float16)(s - (float)hh);
    h = __builtin_bit_cast(unsigned short, hh);
    l = __builtin_bit_cast(unsigned short, ll);
}

// eight float32 values -> their h plane (returned) and l plane (through l), packed in channel order
__device__ __forceinline__ uint4 sgx_split8(sgx_f32x4 lo, sgx_f32x4 hi, float sc, uint4 &l)
{
    uint4 h;
    h.x = spa_split16_pair(lo.x, lo.y, sc, l.x);
    h.y = spa_split16_pair(lo.z, lo.w, sc, l.y);
    h.z = spa_split16_pair(hi.x, hi.y, sc, l.z);
    h.w = spa_split16_pair(hi.z, hi.w, sc, l.w);
    return h;
}

// Chainer's local_response_normalization with three channels: the float32 operations of sg_lrn3 (spa_segnet.hip)
__device__ __forceinline__ void sgx_lrn3(float &a, float &b, float &c)
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

// the standardised, LRN-normalised conv1 input at (gy, gx) as k_segnet_conv<SG_CONV1> stages it; zero outside the image
__device__ __forceinline__ sgx_f32x4 sgx_conv1_val(const float *xb, long long plane, int gy, int gx, int H, int W,
                                                   const SgxStd &st)
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
        sgx_lrn3(r, g, bl);
    }
    return (sgx_f32x4){r, g, bl, 0.f};
}

// that value split: the h plane's 4 values (channel 3 zero) returned, the l plane's through l
__device__ __forceinline__ uint2 sgx_conv1_px(const float *xb, long long plane, int gy, int gx, int H, int W,
                                              const SgxStd &st, float sc, uint2 &l)
{
    const sgx_f32x4 v = sgx_conv1_val(xb, plane, gy, gx, H, W, st);
    uint2 h;
    h.x = spa_split16_pair(v.x, v.y, sc, l.x);
    h.y = spa_split16_pair(v.z, 0.f, sc, l.y);
    return h;
}

// channels [c, c + 8) of the 64-channel input at full-resolution (gy, gx), split: ENC reads the map, DEC / DEC1 the
// pooled map at (gy/2, gx/2) where its index selects (gy & 1, gx & 1), zero elsewhere; zero outside the image
template <int MODE>
__device__ __forceinline__ uint4 sgx_px8(const float *X, const uint8_t *I, int b, int gy, int gx, int c, int H, int W,
                                         float sc, uint4 &l)
{
    uint4 h = make_uint4(0u, 0u, 0u, 0u);
    l = h;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        if (MODE == SGX_ENC) {
            const float *p = X + (((long long)b * H + gy) * W + gx) * 64 + c;
            h = sgx_split8(*(const sgx_f32x4 *)p, *(const sgx_f32x4 *)(p + 4), sc, l);
        } else {
            const int Hh = H >> 1, Wh = W >> 1;
            const long long o = (((long long)b * Hh + (gy >> 1)) * Wh + (gx >> 1)) * 64 + c;
            sgx_f32x4 lo = *(const sgx_f32x4 *)(X + o), hi = *(const sgx_f32x4 *)(X + o + 4);
            const unsigned i0 = *(const unsigned *)(I + o), i1 = *(const unsigned *)(I + o + 4);
            const unsigned sel = (unsigned)(((gy & 1) << 1) | (gx & 1));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (((i0 >> (8 * j)) & 0xffu) != sel) lo[j] = 0.f;
                if (((i1 >> (8 * j)) & 0xffu) != sel) hi[j] = 0.f;
            }
            h = sgx_split8(lo, hi, sc, l);
        }
    }
    return h;
}

__device__ __forceinline__ sgx_f16x8 sgx_frag(uint4 v) { return __builtin_bit_cast(sgx_f16x8, v); }

// one K step's products a b = h_a h_b + h_a l_b + l_a h_b, small terms first: the two cross terms (2^-11 of h_a h_b)
// into their own accumulator x, h_a h_b into acc; the epilogue adds the two (sgh_mma3 records why)
__device__ __forceinline__ void sgx_mma3(sgx_f32x4 &acc, sgx_f32x4 &x, sgx_f16x8 ah, sgx_f16x8 al, sgx_f16x8 bh,
                                         sgx_f16x8 bl)
{
    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, x, 0, 0, 0);
    x = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, x, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------- scales
__device__ __forceinline__ unsigned sgx_absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// part[blockIdx.x * SGX_NAMAX + blockIdx.y] = the bit pattern of max |v| over this workgroup's share of operand
// blockIdx.x: for blockIdx.x < B image blockIdx.x's activations -- n4 float4 of the 64-channel map x, or with CONV1
// the standardised, LRN-normalised (3,H,W) image as the kernels stage it -- and for blockIdx.x == B the nw4 float4 of
// the weights wt.  Grid (B + 1, SGX_NAMAX); x and wt 16-byte aligned.
template <bool CONV1>
__global__ __launch_bounds__(256) void k_sgx_amax(const float *__restrict__ x, long long n4, int B, int H, int W,
                                                  SgxStd st, const float *__restrict__ wt, long long nw4,
                                                  unsigned *__restrict__ part)
{
    __shared__ unsigned red[256];
    const int t = threadIdx.x, j = blockIdx.x, g = blockIdx.y;
    unsigned m = 0u;
    if (CONV1 && j < B) {
        const long long plane = (long long)H * W;
        const float *xb = x + (long long)j * 3 * plane;
        for (long long i = (long long)g * 256 + t; i < plane; i += (long long)SGX_NAMAX * 256) {
            const sgx_f32x4 v = sgx_conv1_val(xb, plane, (int)(i / W), (int)(i % W), H, W, st);
            m = max(m, max(max(sgx_absbits(v.x), sgx_absbits(v.y)), sgx_absbits(v.z)));
        }
    } else {
        const sgx_f32x4 *a = j < B ? (const sgx_f32x4 *)x + (long long)j * n4 : (const sgx_f32x4 *)wt;
        const long long n = j < B ? n4 : nw4;
        for (long long i = (long long)g * 256 + t; i < n; i += (long long)SGX_NAMAX * 256) {
            const sgx_f32x4 v = a[i];
            m = max(max(m, max(sgx_absbits(v.x), sgx_absbits(v.y))), max(sgx_absbits(v.z), sgx_absbits(v.w)));
        }
    }
    red[t] = m;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) red[t] = max(red[t], red[t + d]);
        __syncthreads();
    }
    if (t == 0) part[(long long)j * SGX_NAMAX + g] = red[0];
}

// ex[j] = k with 2^k max|v| in [2^14, 2^15) for operand j = blockIdx.x (maxima part[j * SGX_NAMAX ..]); k = 0 for an
// all-zero operand.  The exponent is clamped to [-112, 127] so that 2^k is a normal float: a maximum below 2^-112
// (subnormal inputs) lands lower, a NaN or infinite one at 2^-113.
__global__ __launch_bounds__(256) void k_sgx_scale(const unsigned *__restrict__ part, int *__restrict__ ex)
{
    __shared__ unsigned red[256];
    const int t = threadIdx.x;
    unsigned m = 0u;
    for (int i = t; i < SGX_NAMAX; i += 256) m = max(m, part[(long long)blockIdx.x * SGX_NAMAX + i]);
    red[t] = m;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (t < d) red[t] = max(red[t], red[t + d]);
        __syncthreads();
    }
    if (t == 0) {
        const unsigned bits = red[0];
        int e = (int)(bits >> 23) - 127;
        e = e < -112 ? -112 : (e > 127 ? 127 : e);
        ex[blockIdx.x] = bits == 0u ? 0 : 14 - e;
    }
}

// the split planes of a 64-channel layer's weights with scale 2^ex[0]: Wp[0][t][o][i] = h, Wp[1][t][o][i] = l of
// Wt[t][o][i]
__global__ __launch_bounds__(256) void k_sgx_wpack64(const float *__restrict__ Wt, const int *__restrict__ ex,
                                                     unsigned short *__restrict__ Wp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SGX_W64) return;
    sgx_split(Wt[i], sgx_pow2(ex[0]), Wp[i], Wp[SGX_W64 + i]);
}

// conv1's split weights in K steps of 8 taps: plane j, Wp[j][s][n][k] of Wt[8 s + k / 4][n][k % 4], zero past tap 48
__global__ __launch_bounds__(256) void k_sgx_wpack1(const float *__restrict__ Wt, const int *__restrict__ ex,
                                                    unsigned short *__restrict__ Wp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= SGX_W1) return;
    const int s = i >> 11, n = (i >> 5) & 63, k = i & 31, t = 8 * s + (k >> 2);
    sgx_split(t < 49 ? Wt[(t * 64 + n) * 4 + (k & 3)] : 0.f, sgx_pow2(ex[0]), Wp[i], Wp[SGX_W1 + i]);
}

// ---------------------------------------------------------------------------------------------------- layers
// MODE SGX_CONV1: X (B,3,H,W) float32 planar 0..255.  SGX_ENC: X (B,H,W,64).  Both write Y (B,H/2,W/2,64) pooled and
// Yi (B,H/2,W/2,64) uint8 argmax (ky * 2 + kx, first maximum).  SGX_DEC / SGX_DEC1: X, I (B,H/2,W/2,64) = the pooled
// map and indices of the matching encoder; Y (B,H,W,64), or for SGX_DEC1 (B,2,H,W) planar softmax probabilities
// (wc (2,64), bc (2) the classifier).  bias (64) float32.  Wp: the h plane, then the l plane, each (49,64,64) =
// (tap, n, c) for the 64-channel forms or (7,64,32) = (K step, n, k) for conv1 (k = 4 (tap - 8 step) + c, zero past
// tap 48).  ex[b] = image b's scale exponent, ex[gridDim.z] = the weights'.
template <int MODE>
__global__ __launch_bounds__(SGX_THREADS, 2) void k_segnet_conv_f16x3(const float *__restrict__ X,
                                                                      const uint8_t *__restrict__ I,
                                                                      const unsigned short *__restrict__ Wp,
                                                                      const float *__restrict__ bias,
                                                                      const float *__restrict__ wc,
                                                                      const float *__restrict__ bc,
                                                                      float *__restrict__ Y, uint8_t *__restrict__ Yi,
                                                                      const int *__restrict__ ex, int H, int W,
                                                                      SgxStd st)
{
    constexpr int PS = MODE == SGX_CONV1 ? 8 : SGX_PS;                   // conv1: [4 h | 4 l] per pixel
    constexpr int NCH = MODE == SGX_CONV1 ? 1 : 2;                       // 32-channel chunks
    constexpr int WPL = MODE == SGX_CONV1 ? SGX_W1 : SGX_W64;            // f16 per weight plane
    __shared__ __attribute__((aligned(16))) unsigned short xs[SGX_HPIX * PS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = blockIdx.y * SGX_TH, tx0 = blockIdx.x * SGX_TW;
    const int Hh = H >> 1, Wh = W >> 1;
    const int kin = ex[b], kw = ex[gridDim.z];
    const float sc = sgx_pow2(kin);

    // this lane's fragment pixel: tile row i = lane & 15 is pixel (i & 3) of 2x2 block i >> 2
    const int fi = lane & 15, fq = lane >> 4;
    const int frow = 2 * w + ((fi & 3) >> 1), fcol = 2 * (fi >> 2) + (fi & 1);

    sgx_f32x4 acc[4][4], accx[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[m][nt] = accx[m][nt] = (sgx_f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < NCH; ++ch) {
        if (ch) __syncthreads();
        // ---- stage the split halo of channels [32 ch, 32 ch + 32) (conv1: its 3 channels and a zero)
        if (MODE == SGX_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SGX_HPIX; p += SGX_THREADS) {
                uint2 l;
                const uint2 h = sgx_conv1_px(xb, plane, ty0 - 3 + p / SGX_HW, tx0 - 3 + p % SGX_HW, H, W, st, sc, l);
                *(uint4 *)&xs[p * PS] = make_uint4(h.x, h.y, l.x, l.y);
            }
        } else {
            constexpr int IN = MODE == SGX_ENC ? SGX_ENC : SGX_DEC;
            for (int e = tid; e < SGX_HPIX * 4; e += SGX_THREADS) {
                const int p = e >> 2, q = e & 3;
                uint4 l;
                const uint4 h =
                    sgx_px8<IN>(X, I, b, ty0 - 3 + p / SGX_HW, tx0 - 3 + p % SGX_HW, 32 * ch + 8 * q, H, W, sc, l);
                *(uint4 *)&xs[p * PS + 8 * q] = h;
                *(uint4 *)&xs[p * PS + 32 + 8 * q] = l;
            }
        }
        __syncthreads();

        if (MODE == SGX_CONV1) {
            // lane quarter fq holds taps t0 = 8 s + 2 fq and t0 + 1 of K step s, 4 channels each
            const unsigned short *xr = &xs[(frow * SGX_HW + fcol) * PS];
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int t0 = 8 * s + 2 * fq, t1 = t0 + 1;
                const int o0 = ((t0 / 7) * SGX_HW + t0 % 7) * PS, o1 = ((t1 / 7) * SGX_HW + t1 % 7) * PS;
                sgx_f16x8 bh[4], bl[4], ah[4], al[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const unsigned short *wq = Wp + ((long long)s * 64 + 16 * nt + fi) * 32 + 8 * fq;
                    bh[nt] = *(const sgx_f16x8 *)wq;
                    bl[nt] = *(const sgx_f16x8 *)(wq + WPL);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint4 lo = t0 < 49 ? *(const uint4 *)&xr[o0 + 8 * m * PS] : make_uint4(0u, 0u, 0u, 0u);
                    const uint4 hi = t1 < 49 ? *(const uint4 *)&xr[o1 + 8 * m * PS] : make_uint4(0u, 0u, 0u, 0u);
                    ah[m] = sgx_frag(make_uint4(lo.x, lo.y, hi.x, hi.y));
                    al[m] = sgx_frag(make_uint4(lo.z, lo.w, hi.z, hi.w));
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) sgx_mma3(acc[m][nt], accx[m][nt], ah[m], al[m], bh[nt], bl[nt]);
            }
        } else {
            // K order inside a chunk: lane quarter fq holds channels 32 ch + 8 fq .. + 7 of both operands
            const unsigned short *wl = Wp + (long long)fi * 64 + 32 * ch + 8 * fq;
            for (int ky = 0; ky < 7; ++ky) {
                const unsigned short *xr = &xs[((frow + ky) * SGX_HW + fcol) * PS + 8 * fq];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const unsigned short *wt = wl + (long long)(ky * 7 + kx) * 64 * 64;
                    sgx_f16x8 bh[4], bl[4], ah[4], al[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        bh[nt] = *(const sgx_f16x8 *)(wt + nt * 16 * 64);
                        bl[nt] = *(const sgx_f16x8 *)(wt + WPL + nt * 16 * 64);
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        ah[m] = *(const sgx_f16x8 *)&xr[(kx + 8 * m) * PS];
                        al[m] = *(const sgx_f16x8 *)&xr[(kx + 8 * m) * PS + 32];
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) sgx_mma3(acc[m][nt], accx[m][nt], ah[m], al[m], bh[nt], bl[nt]);
                }
            }
        }
    }

    // ---- the float32 sums: cross terms added, then unscaled exactly
    const int unscale = -(kin + kw);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[m][nt][r] = ldexpf(acc[m][nt][r] + accx[m][nt][r], unscale);

    // ---- epilogue (k_segnet_conv's).  Lane: channel n = 16 nt + (lane & 15); register r = pixel r (ky * 2 + kx) of
    // block (lane >> 4) of MFMA tile m, i.e. output rows ty0 + 2w + (r >> 1), columns tx0 + 8m + 2 (lane >> 4) + (r & 1).
    const int oy = ty0 + 2 * w, ox = tx0 + 2 * fq;
    if (MODE == SGX_CONV1 || MODE == SGX_ENC) {
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
    } else if (MODE == SGX_DEC) {
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

// ---------------------------------------------------------------------------------------------------- C ABI
// The argument checks are spa_segnet_encode's / spa_segnet_decode's, in their order: the same shapes, layouts and
// alignments are taken and refused, and a refused call launches nothing.
static bool sgx_al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The exponents of the B images' activations (ex[0 .. B - 1]) and of the weights (ex[B]), and the split weights, on
// stream s without a host synchronisation.  n4: float4 per image of a 64-channel operand (Cin == 3: conv1's operand of
// the image x instead).  Workspaces: the weight planes share WS_SEGNET_WF16X3 and the maxima WS_SEGNET_AMAX with the
// split-plane training entry points; every user writes them before it reads them on the stream it was given, so
// calls ordered on one stream (the contract of every workspace here) cannot see each other's contents.
static int sgx_prepare(spa_ctx *ctx, hipStream_t s, const float *x, long long n4, int Cin, int B, int H, int W,
                       const SgxStd &st, const float *wt, unsigned short **wp, int **ex)
{
    int rc = spa_ws_reserve(ctx, WS_SEGNET_WF16X3, 2 * SGX_W64 * sizeof(unsigned short), (void **)wp);
    if (rc != SPA_OK) return rc;
    unsigned *part = nullptr;
    const size_t nop = (size_t)B + 1;
    rc = spa_ws_reserve(ctx, WS_SEGNET_AMAX, nop * SGX_NAMAX * sizeof(unsigned) + nop * sizeof(int), (void **)&part);
    if (rc != SPA_OK) return rc;
    *ex = (int *)(part + nop * SGX_NAMAX);
    dim3 grid(B + 1, SGX_NAMAX);
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgx_amax<true>, grid, dim3(256), 0, s, x, 0ll, B, H, W, st, wt, 49ll * 64 * 4 / 4, part);
    else
        hipLaunchKernelGGL(k_sgx_amax<false>, grid, dim3(256), 0, s, x, n4, B, H, W, st, wt, (long long)SGX_W64 / 4,
                           part);
    SPA_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_sgx_scale, dim3(B + 1), dim3(256), 0, s, part, *ex);
    SPA_LAUNCH_CHECK();
    if (Cin == 3)
        hipLaunchKernelGGL(k_sgx_wpack1, dim3(SGX_W1 / 256), dim3(256), 0, s, wt, *ex + B, *wp);
    else
        hipLaunchKernelGGL(k_sgx_wpack64, dim3(SGX_W64 / 256), dim3(256), 0, s, wt, *ex + B, *wp);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_encode_f16x3(spa_ctx *ctx, const float *x, int32_t x_layout, int32_t B, int32_t H, int32_t W,
                                       int32_t Cin, const float *wt, const float *bias, const float *mean_host,
                                       const float *std_host, float *pooled, uint8_t *idx, void *stream)
{
    SPA_ARG(ctx && x && wt && bias && pooled && idx && B > 0 && B < 65536 && H > 0 && W > 0);
    SPA_ARG(Cin == 3 || Cin == 64);
    SPA_ARG(Cin == 3 ? (H % 16 == 0 && W % 16 == 0) : (H % 2 == 0 && W % 2 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SGX_TH < 65536);
    SPA_ARG(sgx_al16(x) && sgx_al16(wt));
    if (Cin == 3) {
        SPA_ARG(mean_host && std_host);
        if (x_layout != SPA_LAYOUT_NCHW) {
            spa_set_error("spa_segnet_encode_f16x3: the conv1 input is the planar (B,3,H,W) image");
            return SPA_ERR_LAYOUT;
        }
    } else if (x_layout != SPA_LAYOUT_NHWC) {
        spa_set_error("spa_segnet_encode_f16x3: 64-channel inputs must be channels-last (B,H,W,64)");
        return SPA_ERR_LAYOUT;
    }
    SgxStd st = {};
    if (Cin == 3)
        for (int c = 0; c < 3; ++c) { st.mean[c] = mean_host[c]; st.std[c] = std_host[c]; }
    hipStream_t s = spa_stream(stream);
    unsigned short *wp = nullptr;
    int *ex = nullptr;
    int rc = sgx_prepare(ctx, s, x, (long long)H * W * 16, Cin, B, H, W, st, wt, &wp, &ex);
    if (rc != SPA_OK) return rc;
    dim3 grid((W + SGX_TW - 1) / SGX_TW, (H + SGX_TH - 1) / SGX_TH, B);
    if (Cin == 3)
        hipLaunchKernelGGL(k_segnet_conv_f16x3<SGX_CONV1>, grid, dim3(SGX_THREADS), 0, s, x, nullptr, wp, bias, nullptr,
                           nullptr, pooled, idx, ex, H, W, st);
    else
        hipLaunchKernelGGL(k_segnet_conv_f16x3<SGX_ENC>, grid, dim3(SGX_THREADS), 0, s, x, nullptr, wp, bias, nullptr,
                           nullptr, pooled, idx, ex, H, W, st);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

extern "C" int spa_segnet_decode_f16x3(spa_ctx *ctx, const float *x, const uint8_t *idx, int32_t x_layout, int32_t B,
                                       int32_t Hh, int32_t Wh, const float *wt, const float *bias, const float *wc,
                                       const float *bc, float *y, void *stream)
{
    SPA_ARG(ctx && x && idx && wt && bias && y && B > 0 && B < 65536 && Hh > 0 && Wh > 0);
    SPA_ARG((wc == nullptr) == (bc == nullptr));
    const int H = 2 * Hh, W = 2 * Wh;
    SPA_ARG(!wc || (H % 16 == 0 && W % 16 == 0));
    SPA_ARG((long long)H * W * 64 < (1ll << 31) && H / SGX_TH < 65536);
    SPA_ARG(sgx_al16(x) && sgx_al16(wt) && ((uintptr_t)idx & 3) == 0);
    if (x_layout != SPA_LAYOUT_NHWC) {
        spa_set_error("spa_segnet_decode_f16x3: the pooled map and its indices must be channels-last (B,H/2,W/2,64)");
        return SPA_ERR_LAYOUT;
    }
    hipStream_t s = spa_stream(stream);
    unsigned short *wp = nullptr;
    int *ex = nullptr;
    int rc = sgx_prepare(ctx, s, x, (long long)Hh * Wh * 16, 64, B, H, W, SgxStd{}, wt, &wp, &ex);
    if (rc != SPA_OK) return rc;
    dim3 grid((W + SGX_TW - 1) / SGX_TW, (H + SGX_TH - 1) / SGX_TH, B);
    if (wc)
        hipLaunchKernelGGL(k_segnet_conv_f16x3<SGX_DEC1>, grid, dim3(SGX_THREADS), 0, s, x, idx, wp, bias, wc, bc, y,
                           nullptr, ex, H, W, SgxStd{});
    else
        hipLaunchKernelGGL(k_segnet_conv_f16x3<SGX_DEC>, grid, dim3(SGX_THREADS), 0, s, x, idx, wp, bias, nullptr,
                           nullptr, y, nullptr, ex, H, W, SgxStd{});
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
