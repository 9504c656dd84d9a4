// Winograd F(2x2, 3x3) for the heavy 3x3 (dilated) stride-1 layers of the float32 DRN (models/drn.py:230-285:
// layers 5-8, 256/512 channels at 1/8 resolution).  The float32 matrix pipe is the wall of the float32 network
// (spa_conv3x3_f32 and MIOpen both sit at 0.88 of its peak), so the only way past it is fewer multiplications:
// the minimal filtering algorithm computes a 2x2 output tile from a 4x4 input tile with 16 instead of 36
// multiplications per (input channel, output channel) — 2.25x less matrix work — at the price of two streaming
// transforms.  float32 throughout; measured against a float64 convolution the result is as close as the direct
// float32 one (5e-7 vs 3e-7 of the map's scale: the transforms of F(2x2,3x3) only add and halve).
//
//   Y = A^T [ sum_c (G g G^T) .* (B^T d B) ] A        per 2x2 output tile, d = its 4x4 input tile
//
// A dilated convolution is d*d independent ordinary convolutions on the sub-grids (y mod d, x mod d); tiles are
// cut on the sub-grids, so dilation only changes addresses.
//
//   k_wino_in    X (B,H,W,C) -> V [16][T][C]   (T tiles; position-major, so every GEMM reads one dense matrix)
//   GEMM         M[p] (T x K) = V[p] (T x C) . U[p]^T,  U[p] = (G g G^T)[p] as (K, C): the float32 MFMA kernel of
//                spa_conv32.hip in its 1x1 form (V[p] seen as an image of 256-"pixel" rows), all 16 in one
//                launch of persistent workgroups
//   k_wino_out   M [16][T][K] -> Y (B,H,W,K) with bias, residual and ReLU
//
// HBM traffic per layer: X once, V written and read (4x X), M written and read (4x Y), Y once — 38 GB per 30
// images of a 512 -> 512 layer, ~5 ms of streaming next to a GEMM of 16 ms, against 33 ms of direct convolution.
#include "spa_common.h"
#include "spa_wino_dev.h"

int conv1x1_f32_raw(spa_ctx *ctx, const float *x, long long rows, int32_t Cin, const float *wt, int32_t Cout,
                    float *y, void *stream, int zcount);          // spa_conv32.hip

// the tile decode on the host, for the numbering test: out = (b, sy, sx, ty, tx) of tile t of the F(4x4) tiling
extern "C" int spa_wino4_tile_decode(int32_t B, int32_t H, int32_t W, int32_t dilation, int32_t interleaved, int64_t t, int32_t *out)
{
    SPA_ARG(out && B > 0 && H > 0 && W > 0 && dilation >= 1);
    WinoGeom g;
    wino4_geom(B, H, W, dilation, &g);
    SPA_ARG(t >= 0 && t < g.T);
    g.interleaved = interleaved != 0;
    wino_tile(g, t, out[0], out[1], out[2], out[3], out[4]);
    return SPA_OK;
}


__device__ __forceinline__ float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 f4sub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// workgroup ids go round-robin over the 8 XCDs; give every XCD (= every L2) a contiguous range of tiles, so that the
// rows two vertically adjacent tiles share are fetched into one L2, not eight (PMC: k_wino_in read 2.2x its input)
__device__ __forceinline__ long long wino_block()
{
    const long long nb = gridDim.x, id = blockIdx.x;
    const long long q = nb / 8, rem = nb % 8, xcd = id % 8, idx = id / 8;
    return (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + idx;
}


// one thread = one tile x 4 channels: 16 float4 loads, B^T d B, 16 float4 stores
__global__ __launch_bounds__(256) void k_wino_in(const float *__restrict__ X, float *__restrict__ V, WinoGeom g, int C,
                                                 long long Tpad)
{
    const int c4 = C >> 2;
    const long long id = wino_block() * 256 + threadIdx.x;
    if (id >= g.T * c4) return;
    const long long t = id / c4;
    const int c = (int)(id - t * c4) << 2;
    int b, sy, sx, ty, tx;
    wino_tile(g, t, b, sy, sx, ty, tx);
    float4 dv[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = sy + (2 * ty - 1 + i) * g.d;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = sx + (2 * tx - 1 + j) * g.d;
            const bool ok = y >= 0 && y < g.H && x >= 0 && x < g.W;
            dv[i][j] = ok ? *(const float4 *)(X + (((long long)b * g.H + y) * g.W + x) * C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    // rows: B^T d
    float4 r[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r[0][j] = f4sub(dv[0][j], dv[2][j]);
        r[1][j] = f4add(dv[1][j], dv[2][j]);
        r[2][j] = f4sub(dv[2][j], dv[1][j]);
        r[3][j] = f4sub(dv[1][j], dv[3][j]);
    }
    // columns: (B^T d) B
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v0 = f4sub(r[i][0], r[i][2]), v1 = f4add(r[i][1], r[i][2]);
        const float4 v2 = f4sub(r[i][2], r[i][1]), v3 = f4sub(r[i][1], r[i][3]);
        float *o = V + ((long long)(i * 4) * Tpad + t) * C + c;
        *(float4 *)(o) = v0;
        *(float4 *)(o + Tpad * C) = v1;
        *(float4 *)(o + 2 * Tpad * C) = v2;
        *(float4 *)(o + 3 * Tpad * C) = v3;
    }
}

// one thread = one tile x 4 output channels: 16 float4 loads, A^T m A, epilogue, up to 4 float4 stores
template <int HAS_RES>
__global__ __launch_bounds__(256) void k_wino_out(const float *__restrict__ M, float *__restrict__ Y,
                                                  const float *__restrict__ bias, const float *__restrict__ R,
                                                  WinoGeom g, int K, long long Tpad, int relu)
{
    const int k4 = K >> 2;
    const long long id = wino_block() * 256 + threadIdx.x;
    if (id >= g.T * k4) return;
    const long long t = id / k4;
    const int k = (int)(id - t * k4) << 2;
    int b, sy, sx, ty, tx;
    wino_tile(g, t, b, sy, sx, ty, tx);
    float4 m[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) m[i][j] = *(const float4 *)(M + ((long long)(i * 4 + j) * Tpad + t) * K + k);
    // rows: A^T m  (2 x 4)
    float4 s[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[0][j] = f4add(f4add(m[0][j], m[1][j]), m[2][j]);
        s[1][j] = f4sub(f4sub(m[1][j], m[2][j]), m[3][j]);
    }
    const float4 bv = *(const float4 *)(bias + k);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int y = sy + (2 * ty + i) * g.d;
        if (y >= g.H) continue;
        const float4 o0 = f4add(f4add(s[i][0], s[i][1]), s[i][2]);
        const float4 o1 = f4sub(f4sub(s[i][1], s[i][2]), s[i][3]);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = sx + (2 * tx + j) * g.d;
            if (x >= g.W) continue;
            float4 v = f4add(j == 0 ? o0 : o1, bv);
            const long long off = (((long long)b * g.H + y) * g.W + x) * K + k;
            if (HAS_RES) v = f4add(v, *(const float4 *)(R + off));
            if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            *(float4 *)(Y + off) = v;
        }
    }
}

static void wino_geom(int B, int H, int W, int d, WinoGeom *g)
{
    g->B = B; g->H = H; g->W = W; g->d = d; g->interleaved = wino_interleave(d);
    const int hs = (H + d - 1) / d, ws = (W + d - 1) / d;         // the largest sub-grid
    g->th = (hs + 1) / 2; g->tw = (ws + 1) / 2;
    g->T = (long long)B * d * d * g->th * g->tw;
}

// rows of V / M per position, padded to whole 256-row GEMM tiles
extern "C" int64_t spa_wino_tiles(int32_t B, int32_t H, int32_t W, int32_t dilation)
{
    WinoGeom g;
    wino_geom(B, H, W, dilation, &g);
    return (g.T + 255) / 256 * 256;
}

// x (B,H,W,Cin) float32 channels-last; u (16,Cout,Cin) float32 = (G g G^T)[4i+j] per (output, input) channel;
// v_scratch 16 * spa_wino_tiles * Cin floats, m_scratch 16 * spa_wino_tiles * Cout floats (caller-owned: calls on
// different streams do not share them); otherwise as spa_conv3x3_f32
extern "C" int spa_conv3x3_wino_f32(spa_ctx *ctx, const float *x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                    const float *u, int32_t Cout, const float *bias, const float *residual,
                                    int32_t relu, int32_t dilation, float *v_scratch, float *m_scratch, float *y,
                                    void *stream)
{
    SPA_ARG(ctx && x && u && bias && y && v_scratch && m_scratch && B > 0 && H > 0 && W > 0 && dilation >= 1);
    SPA_ARG(Cin % 32 == 0 && Cout % 64 == 0);
    SPA_ARG((((uintptr_t)x | (uintptr_t)u | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)v_scratch |
              (uintptr_t)m_scratch) % 16) == 0);
    hipStream_t s = spa_stream(stream);
    WinoGeom g;
    wino_geom(B, H, W, dilation, &g);
    g.interleaved = ctx->wino_operands >= 1 && wino_interleave(dilation);
    const long long Tpad = (g.T + 255) / 256 * 256;
    SPA_ARG(g.T * (Cin > Cout ? Cin : Cout) / 4 < (1ll << 31) * 256);
    {
        SpaProfScope prof_(ctx, PROF_WINO_IN, s);
        const long long n = g.T * (Cin / 4);
        hipLaunchKernelGGL(k_wino_in, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, v_scratch, g, Cin, Tpad);
    }
    // (rows T .. Tpad of V are never written: their products land in rows of M nothing reads)
    {
        // the 16 GEMMs as ONE launch of persistent workgroups
        int rc = conv1x1_f32_raw(ctx, v_scratch, Tpad, Cin, u, Cout, m_scratch, stream, 16);
        if (rc != SPA_OK) return rc;
    }
    {
        SpaProfScope prof_(ctx, PROF_WINO_OUT, s);
        const long long n = g.T * (Cout / 4);
        if (residual)
            hipLaunchKernelGGL(k_wino_out<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)m_scratch, y,
                               bias, residual, g, Cout, Tpad, relu);
        else
            hipLaunchKernelGGL(k_wino_out<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)m_scratch, y,
                               bias, residual, g, Cout, Tpad, relu);
    }
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

// =========================================================================================================
// F(4x4, 3x3): a 4x4 output tile from a 6x6 input tile with 36 instead of 144 multiplications per channel pair —
// 4x less matrix work than the direct form, V and M 2.25x the activations instead of 4x.  Interpolation points
// 0, 1, -1, 1/2, -2, infinity (NOT the textbook 0, +-1, +-2: measured in float32 on a 256 -> 256 layer the textbook set
// is 1.0e-5 of the map's scale from a float64 convolution, this set 4.7e-6; through the whole DRN-D-22 the final map is
// 1.1e-6 from the float64 network against 2.4e-6 for direct float32 convolutions and 0.8e-6 for F(2x2,3x3), tools/wino_points.py).
//
//   B^T = | 2 -3 -4  3  2  0 |     A^T = | 1  1  1   1    1  0 |     G = | 1/2    0     0   |
//         | 0 -2  1  5  2  0 |           | 0  1 -1  1/2  -2  0 |         | 1/6   1/6   1/6  |
//         | 0 -2  5 -1 -2  0 |           | 0  1  1  1/4   4  0 |         | 1/6  -1/6   1/6  |
//         | 0  2  1 -2 -1  0 |           | 0  1 -1  1/8  -8  1 |         | 16/15 8/15  4/15 |
//         | 0  1 -2 -1  2  0 |                                           | 1/30 -1/15  2/15 |
//         | 0  2 -3 -4  3  2 |                                           |  0     0    1/2  |
// (row 3 of B^T is the generated row / 16 and row 3 of G x 16: powers of two, no rounding.)
// A thread owns one tile x 4 channels (float4): 36 values in flight.
// =========================================================================================================

// (numbering the F(4x4) tiles in blocks of 4 x 4 tiles, so that consecutive workgroups transform tiles whose 6 x 6
// input patches overlap in both directions, was measured: no change — the overlap is served by L2 / MALL anyway —
// and it padded small sub-grids to multiples of 4 tiles: 4x the work on a 7 x 7 sub-grid.  Row-major it is.)

// PLANES (float4 only; the operand of k_gemm_f16x3_stag<..., PLANES>): every value is scaled by its position's exact power of
// two 2^(14 - e - p_i - p_j), e from *amax, and written as the two half-precision planes the GEMM multiplies — the 32 bytes of
// an 8-channel chunk become [8 x h][8 x l].  Same bytes per element and the same row pitch as the float32 form; the split is
// the GEMM's own (wino_split_h / wino_split_l), done once per element.  (A thread's 4 channels are half of each plane of a
// chunk: written as two 8-byte stores the kernel was 0.05-0.08 ms slower per 30 images of a 512-channel layer than the float32
// form, with the halves exchanged between neighbouring lanes and ONE 16-byte store per lane it runs at the float32 form's time.)
template <typename V, bool PLANES = false>
__global__ __launch_bounds__(256) void k_wino4_in(const float *__restrict__ X, float *__restrict__ Vout, WinoGeom g, int C,
                                                  long long Tpad, const unsigned *__restrict__ amax = nullptr)
{
    constexpr int VN = sizeof(V) / 4;
    const int c2 = C / VN;
    const long long id = wino_block() * 256 + threadIdx.x;
    if (id >= g.T * c2) return;
    const long long t = id / c2;
    const int c = (int)(id - t * c2) * VN;
    int b, sy, sx, ty, tx;
    wino_tile(g, t, b, sy, sx, ty, tx);
    // columns first: r[a][:] = (row a of d) . B  (6 values), then rows: out[i][j] = sum_a Bt[i][a] r[a][j]
    V r[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        const int y = sy + (4 * ty - 1 + a) * g.d;
        V dv[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const int x = sx + (4 * tx - 1 + j) * g.d;
            const bool ok = y >= 0 && y < g.H && x >= 0 && x < g.W;
            dv[j] = ok ? *(const V *)(X + (((long long)b * g.H + y) * g.W + x) * C + c) : wino_zero<V>();
        }
        wino4_bt(dv, r[a]);
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const V col[6] = {r[0][j], r[1][j], r[2][j], r[3][j], r[4][j], r[5][j]};
        V o[6];
        wino4_bt(col, o);
#pragma unroll
        // (non-temporal stores of V were measured: 1.60 instead of 1.31 ms per 30 images of a 512-channel layer)
        for (int i = 0; i < 6; ++i) {
            if constexpr (PLANES) {
                static_assert(sizeof(V) == 16, "a thread owns half an 8-channel chunk");
                const float sc = wino_pow2(14 - wino_amax_exp(*amax) - wino4_psum(i * 6 + j));
                const unsigned h0 = wino_split_h(o[i].x, o[i].y, sc), h1 = wino_split_h(o[i].z, o[i].w, sc);
                const unsigned l0 = wino_split_l(o[i].x, o[i].y, sc, h0), l1 = wino_split_l(o[i].z, o[i].w, sc, h1);
                // chunk c / 8 of the row belongs to a pair of neighbouring lanes (C / 4 is even: same tile, both active): the even
                // lane (channels c .. c + 3) takes the odd lane's h and stores the 16 bytes of h, the odd lane takes the even
                // lane's l and stores the 16 bytes of l — one 16-byte store per lane, as in the float32 form
                const bool odd = (c >> 2) & 1;
                const unsigned r0 = wino_lane_swap(odd ? h0 : l0), r1 = wino_lane_swap(odd ? h1 : l1);
                float *chunk = Vout + ((long long)(i * 6 + j) * Tpad + t) * C + (c & ~7);
                *((uint4 *)chunk + (odd ? 1 : 0)) = odd ? make_uint4(r0, r1, l0, l1) : make_uint4(h0, h1, r0, r1);
            } else {
                *(V *)(Vout + ((long long)(i * 6 + j) * Tpad + t) * C + c) = o[i];
            }
        }
    }
}

template <int HAS_RES, typename V>
__global__ __launch_bounds__(256) void k_wino4_out(const float *__restrict__ M, float *__restrict__ Y,
                                                   const float *__restrict__ bias, const float *__restrict__ R,
                                                   WinoGeom g, int K, long long Tpad, int relu)
{
    constexpr int VN = sizeof(V) / 4;
    const int k2 = K / VN;
    const long long id = wino_block() * 256 + threadIdx.x;
    if (id >= g.T * k2) return;
    const long long t = id / k2;
    const int k = (int)(id - t * k2) * VN;
    int b, sy, sx, ty, tx;
    wino_tile(g, t, b, sy, sx, ty, tx);
    // rows: s[:][j] = A^T m[:][j] (4 x 6), then columns
    V s[4][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        V col[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) col[i] = *(const V *)(M + ((long long)(i * 6 + j) * Tpad + t) * K + k);
        V o[4];
        wino4_at(col, o);
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i][j] = o[i];
    }
    const V bv = *(const V *)(bias + k);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int y = sy + (4 * ty + i) * g.d;
        V o[4];
        wino4_at(s[i], o);
        if (y >= g.H) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int x = sx + (4 * tx + j) * g.d;
            if (x >= g.W) continue;
            V v = o[j] + bv;
            const long long off = (((long long)b * g.H + y) * g.W + x) * K + k;
            if (HAS_RES) v = v + *(const V *)(R + off);
            if (relu) v = wino_relu(v);
            *(V *)(Y + off) = v;
        }
    }
}

// =========================================================================================================
// F(4x4, 3x3) with the GEMMs on the 16-bit matrix cores at float32 accuracy (spa_gemm16.hip): the GEMM kernel splits V
// (float32, written by k_wino4_in as for the float32 GEMMs) into two half-precision planes of an exactly (power-of-two)
// scaled value while it feeds the matrix cores.
//   scale of position (i, j):  2^(14 - e - p_i - p_j),  e = exponent of amax >= max |x| over the layer input,
//   p = ceil(log2(row sums of |B^T|)) = 4 4 4 3 3 4  ->  |V_ij| <= 2^(p_i + p_j) amax, scaled magnitude < 2^15:
//   half precision cannot overflow, and what it loses at the small end is 2^-25 of that bound in absolute terms
//   (2^-40 of the layer's largest activation) — its 40 binades are enough for float32-class accuracy of the sums.
// amax comes from the producer of x (k_wino4_out tracks the maximum of what it stores; k_amax for other producers);
// the weights' planes carry a static per-position scale t_ij, and k_wino4_out undoes both (cs[i][j] = 2^(p_i+p_j) / t_ij
// from the host, 2^(e - 14) from amax) while it reads M.
// =========================================================================================================

// amax[0] = bits of max |x| (as unsigned: non-negative floats order like their bit patterns)
__global__ __launch_bounds__(256) void k_amax(const float4 *__restrict__ x, long long n4, unsigned *__restrict__ amax)
{
    __shared__ unsigned red[4];
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = x[i];
        m = max(max(m, __float_as_uint(v.x) & 0x7fffffffu), max(__float_as_uint(v.y) & 0x7fffffffu,
                max(__float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu)));
    }
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        if (m > *(volatile unsigned *)amax) atomicMax(amax, m);
    }
}

// k_wino4_out for the scaled GEMMs: M[i][j] * cs[i][j] * 2^(e - 14); optionally the maximum of what it stores
template <int HAS_RES, typename V = float4>
__global__ __launch_bounds__(256, 2) void k_wino4_out_s(const float *__restrict__ M, float *__restrict__ Y,
                                                     const float *__restrict__ bias, const float *__restrict__ R,
                                                     WinoGeom g, int K, long long Tpad, int relu, WinoScale cs,
                                                     const unsigned *__restrict__ amax_in, unsigned *__restrict__ amax_out)
{
    constexpr int VN = sizeof(V) / 4;       // channels per thread
    const int k2 = K / VN;
    const long long id = wino_block() * 256 + threadIdx.x;
    unsigned mx = 0;
    if (id < g.T * k2) {
        const long long t = id / k2;
        const int k = (int)(id - t * k2) * VN;
        int b, sy, sx, ty, tx;
        wino_tile(g, t, b, sy, sx, ty, tx);
        const float inv = wino_pow2(wino_amax_exp(*amax_in) - 14);
        V s[4][6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            V col[6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
                // M is read exactly once: non-temporal (1.66 instead of 1.70 ms per 30 images of a 512-channel layer)
                col[i] = (cs.c[i * 6 + j] * inv) * wino_nt_load((const V *)(M + ((long long)(i * 6 + j) * Tpad + t) * K + k));
            V o[4];
            wino4_at(col, o);
#pragma unroll
            for (int i = 0; i < 4; ++i) s[i][j] = o[i];
        }
        const V bv = *(const V *)(bias + k);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int y = sy + (4 * ty + i) * g.d;
            V o[4];
            wino4_at(s[i], o);
            if (y >= g.H) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int x = sx + (4 * tx + j) * g.d;
                if (x >= g.W) continue;
                V v = o[j] + bv;
                const long long off = (((long long)b * g.H + y) * g.W + x) * K + k;
                if (HAS_RES) v = v + *(const V *)(R + off);
                if (relu) v = wino_relu(v);
                *(V *)(Y + off) = v;
                mx = max(mx, wino_absmax_bits(v));
            }
        }
    }
    if (amax_out) {
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
        if ((threadIdx.x & 63) == 0 && mx > *(volatile unsigned *)amax_out) atomicMax(amax_out, mx);
    }
}

extern "C" int64_t spa_wino4_tiles(int32_t B, int32_t H, int32_t W, int32_t dilation)
{
    WinoGeom g;
    wino4_geom(B, H, W, dilation, &g);
    return (g.T + 255) / 256 * 256;
}

// as spa_conv3x3_wino_f32 with u (36,Cout,Cin) = (G g G^T)[6i+j] of the matrices above and scratch of
// 36 * spa_wino4_tiles rows
extern "C" int spa_conv3x3_wino4_f32(spa_ctx *ctx, const float *x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                     const float *u, int32_t Cout, const float *bias, const float *residual,
                                     int32_t relu, int32_t dilation, float *v_scratch, float *m_scratch, float *y,
                                     void *stream)
{
    SPA_ARG(ctx && x && u && bias && y && v_scratch && m_scratch && B > 0 && H > 0 && W > 0 && dilation >= 1);
    SPA_ARG(Cin % 32 == 0 && Cout % 64 == 0);
    SPA_ARG((((uintptr_t)x | (uintptr_t)u | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)v_scratch |
              (uintptr_t)m_scratch) % 16) == 0);
    hipStream_t s = spa_stream(stream);
    WinoGeom g;
    wino4_geom(B, H, W, dilation, &g);
    g.interleaved = ctx->wino_operands >= 1 && wino_interleave(dilation);
    const long long Tpad = (g.T + 255) / 256 * 256;
    SPA_ARG(g.T * (Cin > Cout ? Cin : Cout) / 2 < (1ll << 31) * 256);
    {
        SpaProfScope prof_(ctx, PROF_WINO_IN, s);
        const long long n = g.T * (Cin / 4);
        hipLaunchKernelGGL((k_wino4_in<float4, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, v_scratch, g, Cin, Tpad,
                           (const unsigned *)nullptr);
    }
    {
        int rc = conv1x1_f32_raw(ctx, v_scratch, Tpad, Cin, u, Cout, m_scratch, stream, 36);
        if (rc != SPA_OK) return rc;
    }
    {
        SpaProfScope prof_(ctx, PROF_WINO_OUT, s);
        const long long n = g.T * (Cout / 4);
        if (residual)
            hipLaunchKernelGGL((k_wino4_out<1, float4>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)m_scratch, y,
                               bias, residual, g, Cout, Tpad, relu);
        else
            hipLaunchKernelGGL((k_wino4_out<0, float4>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)m_scratch, y,
                               bias, residual, g, Cout, Tpad, relu);
    }
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

int gemm_f16x3_raw(spa_ctx *ctx, const float *x, long long rows, int32_t Cin, const void *wt, int32_t Cout, float *y,
                   void *stream, int zcount, const void *amax, int planes);          // spa_gemm16.hip
int gemm_f16x3_tile(int32_t Cout);

// amax[0] = bit pattern of max |x| over n floats (n a multiple of 4): the scale input of spa_conv3x3_wino4_f16s for a
// tensor whose producer did not track it
extern "C" int spa_amax_f32(spa_ctx *ctx, const float *x, int64_t n, void *amax, void *stream)
{
    SPA_ARG(ctx && x && amax && n > 0 && n % 4 == 0 && ((uintptr_t)x % 16) == 0);
    hipStream_t s = spa_stream(stream);
    spa_zero_word(amax, s);
    long long blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_amax, dim3((unsigned)blocks), dim3(256), 0, s, (const float4 *)x, (long long)(n / 4), (unsigned *)amax);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

// F(4x4,3x3) with the 36 GEMMs on the 16-bit matrix cores at float32 accuracy.  u2: the two-plane form of the scaled
// (G g G^T)[6i+j] (36, Cout, Cin/32, 2, 32) half precision; cs: 36 floats 2^(p_i + p_j) / t_ij (host); amax_in: device
// word holding the bit pattern of a bound on max |x| (spa_amax_f32, or the amax_out of the call that produced x);
// amax_out: device word that receives the bound for y, or NULL.  The rest as spa_conv3x3_wino4_f32.
extern "C" int spa_conv3x3_wino4_f16s(spa_ctx *ctx, const float *x, int32_t B, int32_t H, int32_t W, int32_t Cin,
                                      const void *u2, const float *cs, int32_t Cout, const float *bias,
                                      const float *residual, int32_t relu, int32_t dilation, const void *amax_in,
                                      void *amax_out, void *v_scratch, float *m_scratch, float *y, void *stream)
{
    SPA_ARG(ctx && x && u2 && cs && bias && y && v_scratch && m_scratch && amax_in && B > 0 && H > 0 && W > 0 && dilation >= 1);
    SPA_ARG(Cin % 32 == 0 && Cout % 128 == 0);
    SPA_ARG((((uintptr_t)x | (uintptr_t)u2 | (uintptr_t)y | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)v_scratch |
              (uintptr_t)m_scratch) % 16) == 0);
    hipStream_t s = spa_stream(stream);
    WinoGeom g;
    wino4_geom(B, H, W, dilation, &g);
    g.interleaved = ctx->wino_operands >= 1 && wino_interleave(dilation);
    // V as the GEMM's planes: the 256 x 256 tile's kernel takes them (spa_gemm16.hip), and they pay from two channel tiles on —
    // the GEMM splits an element once per channel tile, and with ONE tile (256 -> 256, 30 images) taking the split out of it
    // measured 0.01 ms of 0.96, inside the spread, next to +0.015 ms in the transform; with two tiles 0.06 (256 -> 512) and
    // 0.16-0.18 ms (512 -> 512) for nothing in the transform (profiles/r8_wino_operands_ab.txt)
    const int planes = ctx->wino_operands >= 2 && gemm_f16x3_tile(Cout) == 256 && Cout >= 512;
    const long long Tpad = (g.T + 255) / 256 * 256;
    SPA_ARG(g.T * (Cin > Cout ? Cin : Cout) / 4 < (1ll << 31) * 256);
    WinoScale sc;
    for (int i = 0; i < 36; ++i) sc.c[i] = cs[i];
    if (amax_out) spa_zero_word(amax_out, s);
    {
        SpaProfScope prof_(ctx, PROF_WINO_IN, s);
        const long long n = g.T * (Cin / 4);
        if (planes)
            hipLaunchKernelGGL((k_wino4_in<float4, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, (float *)v_scratch, g, Cin, Tpad,
                               (const unsigned *)amax_in);
        else
            hipLaunchKernelGGL((k_wino4_in<float4, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, (float *)v_scratch, g, Cin, Tpad,
                               (const unsigned *)nullptr);
    }
    {
        int rc = gemm_f16x3_raw(ctx, (const float *)v_scratch, Tpad, Cin, u2, Cout, m_scratch, stream, 36, amax_in, planes);
        if (rc != SPA_OK) return rc;
    }
    {
        SpaProfScope prof_(ctx, PROF_WINO_OUT, s);
        const long long n = g.T * (Cout / 4);
        if (residual)
            hipLaunchKernelGGL((k_wino4_out_s<1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)m_scratch, y,
                               bias, residual, g, Cout, Tpad, relu, sc, (const unsigned *)amax_in, (unsigned *)amax_out);
        else
            hipLaunchKernelGGL((k_wino4_out_s<0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float *)m_scratch, y,
                               bias, residual, g, Cout, Tpad, relu, sc, (const unsigned *)amax_in, (unsigned *)amax_out);
    }
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
