// The stride-2 3x3 opening convolution of DRN layers 3 and 4 (models/drn.py:204-206) with the block's 1x1 stride-2 projection, on
// the 16-bit matrix cores at float32 accuracy: the shape-specific kernel behind spa_conv3x3_s2_f16s (spa_conv32.hip), built like
// layer 2 (k_drn_layer2_f16x3, spa_stem.hip).  The generic kernel it replaces for these shapes (k_conv3x3_f32<0, BM, 9, 128, true, 2>)
// carries the projection as output rows whose weights are zero at eight taps (nine matrix instructions per needed one), splits
// every pixel fragment in registers at every tap, and stages three input rows per output row.  Here
//   - a workgroup owns a 2-D tile of TH x 32 output pixels; the (2 TH + 1) x 65 input pixels it touches go to LDS ONCE, as the two
//     half-precision planes of the scaled value (h = rn16(x 2^(14-e)), l = rn16(x 2^(14-e) - h), e from *amax_in as in the generic
//     kernel), pixel pitch 4 Cin + 16 bytes: two pixels (the stride) are 32 bytes mod 256 apart, so each 16-lane group of a
//     ds_read_b128 fragment read (rows {0-3, 12-15} at one 16-byte chunk, rows {4-11} at the next) falls on 16 different slots;
//   - a wave keeps the weight fragments of ITS 16 convolution channels (all nine taps) and 16 projection channels (centre tap) in
//     registers for the whole launch — the weights never pass through LDS — and walks the tile's rows, two 16-pixel fragments at
//     a time: per K block two plane reads per fragment feed three matrix instructions per accumulator;
//   - the projection is computed from the centre tap only, into its own accumulators;
//   - workgroups are persistent (one per CU: the patch is 84 / 88 KB); the next tile's patch is requested right after this tile's
//     planes are complete and travels under its matrix work — into registers with 32 input channels (as in layer 2); with 64,
//     where a wave's weights alone are 160 registers, into a float32 staging area behind the planes by 16-byte LDS-DMA loads.
// Measured on the way (30 images, 64 -> 128+128, alone): four waves holding two channel groups each (512 registers a wave, half the
// fragment reads) 0.72 ms against 0.65 with eight waves of one group; re-issuing each staging load inside the conversion loop as soon as its slot
// is free (loads in flight in every phase) 0.79 ms: the LDS-DMA instructions cost more between the conversion's vector
// instructions than in one burst.  The generic kernel takes 1.00 ms; 32 -> 64+64: 0.83 against 1.78 ms.
// Same bits as the generic kernel: K blocks in its (dy, 32-channel block, dx) order, the three products of a block in its order
// (wl.xh, wh.xl, wh.xh), the same k -> lane assignment (lane group g holds channels 8 g .. 8 g + 7 of the block in both operands),
// float32 accumulation from zero, the same epilogue arithmetic.  The eight taps the generic kernel also accumulates for the
// projection multiply by zero weights: they add exact zeros.
#include "spa_common.h"

typedef float s2_f4 __attribute__((ext_vector_type(4)));
typedef _Float16 s2_h8 __attribute__((ext_vector_type(8)));

#define S2_TW 32
#define S2_PW (2 * S2_TW + 1)

// orders LDS traffic only (__syncthreads() would also wait for the previous tile's output stores)
__device__ __forceinline__ void s2_lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int CIN> struct S2Geom {
    static constexpr int TH = CIN == 32 ? 4 : 2;              // output rows per tile: the patch is 84 / 88 KB
    static constexpr int PH = 2 * TH + 1;
    static constexpr int PITCH = 4 * CIN + 16;                // bytes per staged pixel: CIN h | CIN l | 16 pad
    static constexpr int PATCH = PH * S2_PW * PITCH;
    // 64 input channels: the next tile's patch waits in LDS behind the planes, brought there by 16-byte LDS-DMA loads (1 KB per
    // wave and load) — NS of a lane's NU float4, as many as the CU's LDS holds; the others, and all of them with 32 channels, wait
    // in registers
    static constexpr int NW = 8;                              // waves
    static constexpr int NE = PH * S2_PW * (CIN / 4), NU = (NE + NW * 64 - 1) / (NW * 64);     // float4 elements of a patch, per lane
    static constexpr int NS = CIN == 32 ? 0 : (NU < 9 ? NU : 9);
    static constexpr int LDS = PATCH + NS * NW * 1024;
    static_assert(LDS <= 160 * 1024 && PATCH % 16 == 0, "LDS of a CU");
};

// x (B,Hi,Wi,CIN) float32; wt2 (Cout, 9, CIN/32, 2, 32) half precision, Cout = 16 NG (+ 16 NG projection rows when PROJ);
// y (B,Ho,Wo,16 NG), y2 (B,Ho,Wo,16 NG).  NG = 16-channel groups of the convolution: 4 (two waves per group, each half of the
// tile's rows) or 8 (one wave per group).
template <int CIN, int NG, bool PROJ>
__global__ __launch_bounds__(S2Geom<CIN>::NW * 64) void k_conv3x3_s2_tile(const float *__restrict__ x, int B, int Hi, int Wi, int Ho, int Wo,
                                                                const unsigned short *__restrict__ wt2, const float *__restrict__ bias,
                                                                float inv_t, int relu, const unsigned *__restrict__ amax_in,
                                                                unsigned *__restrict__ amax_out, float *__restrict__ y,
                                                                float *__restrict__ y2)
{
    typedef S2Geom<CIN> G;
    constexpr int TH = G::TH, PITCH = G::PITCH, KC = CIN / 32, CS = 16 * NG;
    constexpr int NW = G::NW, S2_THREADS = NW * 64, NE = G::NE, NU = G::NU, NS = G::NS;
    constexpr bool LIGHT = CIN == 64;                         // registers are short: bias and projection weights come from the cache per tile row
    constexpr int NPH = NW / NG, ITER = TH / NPH;             // waves per channel group, tile rows per wave
    static_assert(TH % NPH == 0 && NPH * NG == NW, "rows per wave");
    extern __shared__ __attribute__((aligned(16))) char s2_patch[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int frow = lane & 15, fk = lane >> 4;
    const int cg = wave % NG, ph = wave / NG;                 // the wave's channel group and its share of the tile's rows
    const int tiles_x = (Wo + S2_TW - 1) / S2_TW, tiles_y = (Ho + TH - 1) / TH;
    const int n_tiles = tiles_x * tiles_y * B;

    // this wave's weight fragments: channel cg * 16 + frow, halfs 8 fk .. 8 fk + 7 of each plane of each (tap, 32-channel block)
    s2_h8 wh[9][KC], wl[9][KC], qh[KC], ql[KC];
    float4 bias_c, bias_p;
    {
        const unsigned short *wr = wt2 + (size_t)(cg * 16 + frow) * (9 * KC * 64) + 8 * fk;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                wh[tap][kc] = *(const s2_h8 *)(wr + (tap * KC + kc) * 64);
                wl[tap][kc] = *(const s2_h8 *)(wr + (tap * KC + kc) * 64 + 32);
            }
        bias_c = bias_p = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!LIGHT) bias_c = *(const float4 *)(bias + cg * 16 + 4 * fk);
        if (PROJ && !LIGHT) {
            const unsigned short *pr = wt2 + (size_t)(CS + cg * 16 + frow) * (9 * KC * 64) + 8 * fk;
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                qh[kc] = *(const s2_h8 *)(pr + (4 * KC + kc) * 64);
                ql[kc] = *(const s2_h8 *)(pr + (4 * KC + kc) * 64 + 32);
            }
            bias_p = *(const float4 *)(bias + CS + cg * 16 + 4 * fk);
        }
    }
    float sc, unscale;
    {
        const unsigned bits = *amax_in;
        int e = (int)(bits >> 23) - 127;
        e = bits == 0u ? 0 : (e < -100 ? -100 : (e > 100 ? 100 : e));
        sc = __uint_as_float((unsigned)(127 + 14 - e) << 23);
        unscale = __uint_as_float((unsigned)(127 - 14 + e) << 23) * inv_t;
    }

    constexpr int Q = CIN / 4;                                // float4 elements per pixel
    float4 raw[NU - NS > 0 ? NU - NS : 1];
    char *const stage = s2_patch + G::PATCH + wave * 1024;    // float4 u of this wave's lanes: stage + u * NW * 1024 + 16 lane
    auto patch_load = [&](int tile) {
        const int b = tile / (tiles_x * tiles_y), tr = tile - b * (tiles_x * tiles_y);
        const int ty0 = (tr / tiles_x) * TH, tx0 = (tr % tiles_x) * S2_TW;
        const float *src = x + (long long)b * Hi * Wi * CIN;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            int e = tid + u * S2_THREADS;
            e = e < NE ? e : NE - 1;
            const int pix = e / Q, q = e % Q;
            const int iy = pix / S2_PW, ix = pix - iy * S2_PW;
            const int gy = 2 * ty0 - 1 + iy, gx = 2 * tx0 - 1 + ix;
            const int cy = min(max(gy, 0), Hi - 1), cx = min(max(gx, 0), Wi - 1);   // (a clamped pixel is replaced by zeros below)
            const float *g = src + ((long long)cy * Wi + cx) * CIN + 4 * q;
            if (u < NS)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                                 (__attribute__((address_space(3))) void *)(stage + u * (NW * 1024)), 16, 0, 0);
            else raw[u - NS] = *(const float4 *)g;
        }
    };
    unsigned amx = 0;
    if ((int)blockIdx.x < n_tiles) patch_load(blockIdx.x);
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int b = tile / (tiles_x * tiles_y), tr = tile - b * (tiles_x * tiles_y);
        const int ty0 = (tr / tiles_x) * TH, tx0 = (tr % tiles_x) * S2_TW;
        // ---- the patch as two half-precision planes, built once
        if (NS > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the LDS-DMA loads of this tile's patch have landed
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int e = tid + u * S2_THREADS;
            if (e >= NE) continue;
            const int pix = e / Q, q = e % Q;
            const int iy = pix / S2_PW, ix = pix - iy * S2_PW;
            const int gy = 2 * ty0 - 1 + iy, gx = 2 * tx0 - 1 + ix;
            const bool in = (unsigned)gy < (unsigned)Hi && (unsigned)gx < (unsigned)Wi;
            const float4 rv = u < NS ? *(const float4 *)(stage + u * (NW * 1024) + 16 * lane) : raw[u < NS ? 0 : u - NS];
            const float v0 = in ? rv.x : 0.f, v1 = in ? rv.y : 0.f, v2 = in ? rv.z : 0.f, v3 = in ? rv.w : 0.f;
            unsigned l01, l23;
            const unsigned h01 = spa_split16_pair(v0, v1, sc, l01);
            const unsigned h23 = spa_split16_pair(v2, v3, sc, l23);
            char *o = s2_patch + pix * PITCH + q * 8;
            *(uint2 *)o = make_uint2(h01, h23);
            *(uint2 *)(o + 2 * CIN) = make_uint2(l01, l23);
        }
        s2_lds_barrier();
        if (tile + (int)gridDim.x < n_tiles) patch_load(tile + (int)gridDim.x);     // the next tile's input travels under the matrix work
        // ---- tile row r: output pixels (r, frow) and (r, 16 + frow); tap (dy, dx) of output (r, c) is patch pixel (2 r + dy, 2 c + dx)
#pragma unroll 1
        for (int it = 0; it < ITER; ++it) {
            const int r = ph * ITER + it;
            const char *pb = s2_patch + ((2 * r) * S2_PW + 2 * frow) * PITCH + 16 * fk;
            s2_f4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f}, p0 = {0.f, 0.f, 0.f, 0.f}, p1 = {0.f, 0.f, 0.f, 0.f};
            if (PROJ && LIGHT) {
                size_t off = (size_t)(CS + frow) * (9 * KC * 64) + 8 * fk + 4 * KC * 64;
                asm volatile("" : "+v"(off));               // (not loop invariant for the compiler: it would keep them in registers)
#pragma unroll
                for (int kc = 0; kc < KC; ++kc) {
                    const unsigned short *pr = wt2 + off + (size_t)(cg * 16) * (9 * KC * 64) + kc * 64;
                    qh[kc] = *(const s2_h8 *)pr;
                    ql[kc] = *(const s2_h8 *)(pr + 32);
                }
            }
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int kc = 0; kc < KC; ++kc)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int tap = dy * 3 + dx;
                        const char *f = pb + (dy * S2_PW + dx) * PITCH + kc * 64;
                        const s2_h8 fh0 = *(const s2_h8 *)f, fl0 = *(const s2_h8 *)(f + 2 * CIN);
                        const s2_h8 fh1 = *(const s2_h8 *)(f + 32 * PITCH), fl1 = *(const s2_h8 *)(f + 32 * PITCH + 2 * CIN);
                        c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[tap][kc], fh0, c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[tap][kc], fh1, c1, 0, 0, 0);
                        if (PROJ && tap == 4) {
                            p0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ql[kc], fh0, p0, 0, 0, 0);
                            p1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(ql[kc], fh1, p1, 0, 0, 0);
                        }
                        c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[tap][kc], fl0, c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[tap][kc], fl1, c1, 0, 0, 0);
                        if (PROJ && tap == 4) {
                            p0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(qh[kc], fl0, p0, 0, 0, 0);
                            p1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(qh[kc], fl1, p1, 0, 0, 0);
                        }
                        c0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[tap][kc], fh0, c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[tap][kc], fh1, c1, 0, 0, 0);
                        if (PROJ && tap == 4) {
                            p0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(qh[kc], fh0, p0, 0, 0, 0);
                            p1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(qh[kc], fh1, p1, 0, 0, 0);
                        }
                    }
            // ---- epilogue: the lane holds channels cg * 16 + 4 fk .. + 3 of pixels frow (c0, p0) and 16 + frow (c1, p1)
            const int gy = ty0 + r;
            if (gy < Ho) {
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int gx = tx0 + hf * 16 + frow;
                    if (gx >= Wo) continue;
                    const long long pix = ((long long)b * Ho + gy) * Wo + gx;
                    const s2_f4 a = hf ? c1 : c0;
                    if (LIGHT) {
                        bias_c = *(const float4 *)(bias + cg * 16 + 4 * fk);
                        if (PROJ) bias_p = *(const float4 *)(bias + CS + cg * 16 + 4 * fk);
                    }
                    float v0 = a[0] * unscale + bias_c.x, v1 = a[1] * unscale + bias_c.y, v2 = a[2] * unscale + bias_c.z, v3 = a[3] * unscale + bias_c.w;
                    if (relu) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
                    *(float4 *)(y + pix * CS + cg * 16 + 4 * fk) = make_float4(v0, v1, v2, v3);
                    amx = max(max(amx, __float_as_uint(v0) & 0x7fffffffu), max(__float_as_uint(v1) & 0x7fffffffu,
                              max(__float_as_uint(v2) & 0x7fffffffu, __float_as_uint(v3) & 0x7fffffffu)));
                    if (PROJ) {
                        const s2_f4 p = hf ? p1 : p0;
                        *(float4 *)(y2 + pix * CS + cg * 16 + 4 * fk) = make_float4(p[0] * unscale + bias_p.x, p[1] * unscale + bias_p.y,
                                                                                    p[2] * unscale + bias_p.z, p[3] * unscale + bias_p.w);
                    }
                }
            }
        }
        s2_lds_barrier();                   // every wave is done with the patch: the next tile's planes overwrite it
    }
    if (amax_out) {
        for (int o = 32; o > 0; o >>= 1) amx = max(amx, (unsigned)__shfl_xor((int)amx, o));
        if (lane == 0 && amx > *(volatile unsigned *)amax_out) atomicMax(amax_out, amx);
    }
}

template <int CIN, int NG, bool PROJ>
static int s2_tile_launch(spa_ctx *ctx, int bit, const float *x, int B, int Hi, int Wi, const void *wt2, float inv_t, const float *bias,
                          int relu, const void *amax_in, void *amax_out, float *y, float *y2, hipStream_t s)
{
    typedef S2Geom<CIN> G;
    constexpr int NW = G::NW;
    if (!(ctx->convs2_attr_done & bit)) {
        SPA_HIP(hipFuncSetAttribute((const void *)k_conv3x3_s2_tile<CIN, NG, PROJ>, hipFuncAttributeMaxDynamicSharedMemorySize, G::LDS));
        ctx->convs2_attr_done |= bit;
    }
    const int Ho = (Hi + 1) / 2, Wo = (Wi + 1) / 2;
    const long long n_tiles = (long long)((Wo + S2_TW - 1) / S2_TW) * ((Ho + G::TH - 1) / G::TH) * B;
    SPA_ARG(n_tiles < (1ll << 31));
    long long grid = ctx->n_cu;             // one workgroup per CU (LDS), persistent
    if (grid > n_tiles) grid = n_tiles;
    hipLaunchKernelGGL((k_conv3x3_s2_tile<CIN, NG, PROJ>), dim3((unsigned)grid), dim3(NW * 64), G::LDS, s, x, B, Hi, Wi, Ho, Wo,
                       (const unsigned short *)wt2, bias, inv_t, relu, (const unsigned *)amax_in, (unsigned *)amax_out, y, y2);
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}

// the shapes this file takes: Cin 32 / 64, csplit 64 / 128 with a projection of the same width, or 128 channels and no projection
bool conv3x3_s2_tile_takes(int32_t Cin, int32_t Cout, int32_t csplit, const float *y2)
{
    if (Cin != 32 && Cin != 64) return false;
    if (y2) return (csplit == 64 || csplit == 128) && Cout == 2 * csplit;
    return csplit == 128 && Cout == 128;
}

// called by spa_conv3x3_s2_f16s (arguments checked, *amax_out zeroed, timing scope open)
int conv3x3_s2_tile_launch(spa_ctx *ctx, const float *x, int32_t B, int32_t Hi, int32_t Wi, int32_t Cin, const void *wt2, float inv_t,
                           int32_t csplit, const float *bias, int32_t relu, const void *amax_in, void *amax_out, float *y, float *y2,
                           hipStream_t s)
{
#define S2_GO(C, N, P, BIT) return s2_tile_launch<C, N, P>(ctx, BIT, x, B, Hi, Wi, wt2, inv_t, bias, relu, amax_in, amax_out, y, y2, s)
    if (y2) {
        if (Cin == 32 && csplit == 64) S2_GO(32, 4, true, 1);
        if (Cin == 32 && csplit == 128) S2_GO(32, 8, true, 2);
        if (Cin == 64 && csplit == 64) S2_GO(64, 4, true, 4);
        if (Cin == 64 && csplit == 128) S2_GO(64, 8, true, 8);
    } else {
        if (Cin == 32 && csplit == 128) S2_GO(32, 8, false, 16);
        if (Cin == 64 && csplit == 128) S2_GO(64, 8, false, 32);
    }
#undef S2_GO
    SPA_ARG(!"conv3x3_s2_tile_launch: shape not taken");
    return SPA_OK;
}
