// The drivers' overview figures, composed where their sources are (cli.save_figure's 2x2 panels, labels_from_segnet's
// 1x3).  The format is fixed in include/spalign.h (spa_figure_compose_u8) and restated on the host in figure.py
// (compose_host): every panel is a d-fold decimated view of one index plane, coloured through a 256-entry table and, in
// SPA_FIGURE_BLEND, laid over the frame at 0.4; a canvas byte is the round-half-up mean of its window, in integers.
//
//   k_figure<D>   one launch, two kinds of workgroup:
//     panel workgroups   D > 0: a lane per 16 source columns of one panel row: per source row one 16-byte load of the
//                        plane and three of the frame, 16 / D canvas pixels.  D = 0: a lane per panel pixel, byte loads,
//                        any d, pitch and address.
//     fill workgroups    a lane per canvas pixel: 255 where no panel is.
//
// A canvas byte belongs to a panel or to the fill, never to both, and a panel pixel to one lane: every byte has one
// writer, so there are no atomics, nothing is zeroed, and a call leaves the same bits whatever the canvas held.
#include "spa_common.h"

#define FIG_THREADS 256

struct FigArgs {
    const uint8_t *frames;
    const uint8_t *planes[SPA_FIGURE_MAX_PANELS];
    const uint8_t *luts[SPA_FIGURE_MAX_PANELS];
    int modes[SPA_FIGURE_MAX_PANELS];
    int B, H, W, P, R, C, d, g;
    int Hp, Wp, Hc, Wc;
    int nseg;                            // lanes per panel row
    long long panel_items;               // B * P * Hp * nseg
    long long canvas_pixels;             // B * Hc * Wc
    unsigned panel_blocks;
};

// the canvas pixel (oy, ox) lies in one of the P panels
__device__ __forceinline__ bool fig_in_panel(const FigArgs &a, int oy, int ox)
{
    const int py = oy - a.g, px = ox - a.g;
    if (py < 0 || px < 0) return false;
    const int cr = py / (a.Hp + a.g), cc = px / (a.Wp + a.g);
    const int wy = py - cr * (a.Hp + a.g), wx = px - cc * (a.Wp + a.g);
    return cr < a.R && cc < a.C && wy < a.Hp && wx < a.Wp && cr * a.C + cc < a.P;
}

__device__ __forceinline__ uint32_t fig_round(uint32_t S, uint32_t n)
{
    return (2u * S + 5u * n) / (10u * n);
}

template <int D>
__global__ __launch_bounds__(FIG_THREADS) void k_figure(const FigArgs a, uint8_t *__restrict__ out)
{
    if (blockIdx.x >= a.panel_blocks) {
        const long long i = (long long)(blockIdx.x - a.panel_blocks) * FIG_THREADS + threadIdx.x;
        if (i >= a.canvas_pixels) return;
        const int ox = (int)(i % a.Wc), oy = (int)((i / a.Wc) % a.Hc);
        if (fig_in_panel(a, oy, ox)) return;
        uint8_t *o = out + i * 3;
        o[0] = 255; o[1] = 255; o[2] = 255;
        return;
    }

    // table entry = R | G << 8 | B << 16
    __shared__ uint32_t lut[SPA_FIGURE_MAX_PANELS][256];
    for (int i = threadIdx.x; i < a.P * 256; i += FIG_THREADS) {
        const uint8_t *e = a.luts[i >> 8] + 3 * (i & 255);
        lut[i >> 8][i & 255] = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
    }
    __syncthreads();

    const long long i = (long long)blockIdx.x * FIG_THREADS + threadIdx.x;
    if (i >= a.panel_items) return;
    const int seg = (int)(i % a.nseg);
    const long long q = i / a.nseg;
    const int y = (int)(q % a.Hp);
    const int p = (int)((q / a.Hp) % a.P), b = (int)(q / ((long long)a.Hp * a.P));
    const uint8_t *__restrict__ plane = a.planes[p];
    const uint8_t *__restrict__ frames = a.frames;
    const uint32_t *tab = lut[p];
    const bool blend = a.modes[p] == SPA_FIGURE_BLEND;
    const int d = D > 0 ? D : a.d;
    const int r0 = y * d, r1 = r0 + d < a.H ? r0 + d : a.H;
    const int oy = a.g + (p / a.C) * (a.Hp + a.g) + y, ox0 = a.g + (p % a.C) * (a.Wp + a.g);
    uint8_t *orow = out + (((long long)b * a.Hc + oy) * a.Wc + ox0) * 3;

    if (D > 0) {
        constexpr int DD = D > 0 ? D : 1, PPT = 16 / DD;
        uint32_t S[PPT][3];
#pragma unroll
        for (int j = 0; j < PPT; ++j) S[j][0] = S[j][1] = S[j][2] = 0u;
        for (int r = r0; r < r1; ++r) {
            const long long pix = ((long long)b * a.H + r) * a.W + 16 * seg;
            const uint4 pl = *(const uint4 *)(plane + pix);
            const uint32_t pw[4] = {pl.x, pl.y, pl.z, pl.w};
            if (blend) {
                const uint4 *f = (const uint4 *)(frames + pix * 3);
                const uint4 f0 = f[0], f1 = f[1], f2 = f[2];
                const uint32_t fw[12] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, f2.x, f2.y, f2.z, f2.w};
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const uint32_t e = tab[(pw[c >> 2] >> (8 * (c & 3))) & 255u];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const uint32_t v = (fw[(3 * c + k) >> 2] >> (8 * ((3 * c + k) & 3))) & 255u;
                        S[c / DD][k] += 3u * v + 2u * ((e >> (8 * k)) & 255u);
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const uint32_t e = tab[(pw[c >> 2] >> (8 * (c & 3))) & 255u];
#pragma unroll
                    for (int k = 0; k < 3; ++k) S[c / DD][k] += 5u * ((e >> (8 * k)) & 255u);
                }
            }
        }
        // W % 16 == 0 and D divides 16: every window is D columns wide and all PPT pixels are inside the panel
        const uint32_t n = (uint32_t)(r1 - r0) * DD;
        uint8_t *o = orow + (long long)seg * PPT * 3;
#pragma unroll
        for (int j = 0; j < PPT; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) o[3 * j + k] = (uint8_t)fig_round(S[j][k], n);
    } else {
        const int c0 = seg * d, c1 = c0 + d < a.W ? c0 + d : a.W;
        uint32_t S0 = 0u, S1 = 0u, S2 = 0u;
        for (int r = r0; r < r1; ++r) {
            const long long row = ((long long)b * a.H + r) * a.W;
            for (int c = c0; c < c1; ++c) {
                const uint32_t e = tab[plane[row + c]];
                if (blend) {
                    const uint8_t *v = frames + (row + c) * 3;
                    S0 += 3u * v[0] + 2u * (e & 255u);
                    S1 += 3u * v[1] + 2u * ((e >> 8) & 255u);
                    S2 += 3u * v[2] + 2u * ((e >> 16) & 255u);
                } else {
                    S0 += 5u * (e & 255u);
                    S1 += 5u * ((e >> 8) & 255u);
                    S2 += 5u * ((e >> 16) & 255u);
                }
            }
        }
        const uint32_t n = (uint32_t)(r1 - r0) * (uint32_t)(c1 - c0);
        uint8_t *o = orow + (long long)seg * 3;
        o[0] = (uint8_t)fig_round(S0, n);
        o[1] = (uint8_t)fig_round(S1, n);
        o[2] = (uint8_t)fig_round(S2, n);
    }
}

extern "C" int spa_figure_canvas_shape(int32_t H, int32_t W, int32_t R, int32_t C, int32_t d, int32_t g, int32_t *Hc,
                                       int32_t *Wc)
{
    if (!Hc || !Wc || H <= 0 || W <= 0 || R < 1 || C < 1 || d < 1 || d > SPA_FIGURE_MAX_DECIMATE || g < 0 ||
        g > SPA_FIGURE_MAX_GAP)
        return SPA_ERR_ARG;
    const int64_t Hp = ((int64_t)H + d - 1) / d, Wp = ((int64_t)W + d - 1) / d;
    const int64_t h = (R * Hp + ((int64_t)R + 1) * g + 15) / 16 * 16, w = (C * Wp + ((int64_t)C + 1) * g + 15) / 16 * 16;
    if (h > 0x7fffffffLL || w > 0x7fffffffLL) return SPA_ERR_ARG;
    *Hc = (int32_t)h;
    *Wc = (int32_t)w;
    return SPA_OK;
}

extern "C" int spa_figure_compose_u8(spa_ctx *ctx, const uint8_t *frames, int32_t B, int32_t H, int32_t W, int32_t P,
                                     const uint8_t *const *planes, const uint8_t *const *luts, const int32_t *modes,
                                     int32_t R, int32_t C, int32_t d, int32_t g, uint8_t *out, int32_t Hc, int32_t Wc,
                                     void *stream)
{
    SPA_ARG(ctx && planes && luts && modes && out);
    SPA_ARG(B > 0 && H > 0 && W > 0);
    SPA_ARG(P >= 1 && P <= SPA_FIGURE_MAX_PANELS);
    SPA_ARG(R >= 1 && C >= 1 && (int64_t)R * C >= P);
    SPA_ARG(d >= 1 && d <= SPA_FIGURE_MAX_DECIMATE && g >= 0 && g <= SPA_FIGURE_MAX_GAP);
    int32_t hc = 0, wc = 0;
    SPA_ARG(spa_figure_canvas_shape(H, W, R, C, d, g, &hc, &wc) == SPA_OK);
    if (Hc != hc || Wc != wc) {
        spa_set_error("spa_figure_compose_u8: the canvas is %d x %d, spa_figure_canvas_shape gives %d x %d", Hc, Wc, hc,
                      wc);
        return SPA_ERR_ARG;
    }
    FigArgs a;
    bool any_blend = false;
    for (int p = 0; p < SPA_FIGURE_MAX_PANELS; ++p) {
        a.planes[p] = a.luts[p] = nullptr;
        a.modes[p] = SPA_FIGURE_TABLE;
    }
    for (int p = 0; p < P; ++p) {
        SPA_ARG(planes[p] && luts[p]);
        SPA_ARG(modes[p] == SPA_FIGURE_TABLE || modes[p] == SPA_FIGURE_BLEND);
        SPA_ARG(modes[p] == SPA_FIGURE_TABLE || frames);
        any_blend = any_blend || modes[p] == SPA_FIGURE_BLEND;
        a.planes[p] = planes[p];
        a.luts[p] = luts[p];
        a.modes[p] = modes[p];
    }
    a.frames = any_blend ? frames : nullptr;
    a.B = B; a.H = H; a.W = W; a.P = P; a.R = R; a.C = C; a.d = d; a.g = g;
    a.Hp = (H + d - 1) / d; a.Wp = (W + d - 1) / d; a.Hc = Hc; a.Wc = Wc;

    bool vec = (16 % d) == 0 && (W & 15) == 0 && ((uintptr_t)a.frames & 15) == 0;
    for (int p = 0; p < P; ++p) vec = vec && ((uintptr_t)planes[p] & 15) == 0;
    a.nseg = vec ? W / 16 : a.Wp;
    a.panel_items = (long long)B * P * a.Hp * a.nseg;
    a.canvas_pixels = (long long)B * Hc * Wc;
    const long long pb = (a.panel_items + FIG_THREADS - 1) / FIG_THREADS;
    const long long fb = (a.canvas_pixels + FIG_THREADS - 1) / FIG_THREADS;
    SPA_ARG(pb + fb <= 0x7fffffffLL);
    a.panel_blocks = (unsigned)pb;
    const dim3 grid((unsigned)(pb + fb)), block(FIG_THREADS);
    hipStream_t s = spa_stream(stream);
    switch (vec ? d : 0) {
    case 1: hipLaunchKernelGGL(k_figure<1>, grid, block, 0, s, a, out); break;
    case 2: hipLaunchKernelGGL(k_figure<2>, grid, block, 0, s, a, out); break;
    case 4: hipLaunchKernelGGL(k_figure<4>, grid, block, 0, s, a, out); break;
    case 8: hipLaunchKernelGGL(k_figure<8>, grid, block, 0, s, a, out); break;
    case 16: hipLaunchKernelGGL(k_figure<16>, grid, block, 0, s, a, out); break;
    default: hipLaunchKernelGGL(k_figure<0>, grid, block, 0, s, a, out); break;
    }
    SPA_LAUNCH_CHECK();
    return SPA_OK;
}
