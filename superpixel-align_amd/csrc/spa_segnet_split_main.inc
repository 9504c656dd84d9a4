// The staging and K loop of a split-plane forward / dgrad convolution (three v_mfma_f32_16x16x32_f16 per K step,
// sg_mma3), included as TEXT in the body of k_segnet_conv_f16x3 and k_sgh_conv -- the one copy both kernels compile.
// Not a function like sg_conv_main_f32 / sg_conv_main_bf16: these kernels sit at the 256-VGPR limit, and as a call the
// same code moved their spills and made the compiler pack k_sgh_conv's BN partial sums (v_pk_add_f32 / v_pk_fma_f32);
// as text every instruction count stays as verified (profiles/segnet_refactor_isa.md).
//
// A block with no return in it: code may follow the include.
// Expects in scope: MODE (CONV1 test), IN (input form), X, I, Wp (the h plane, then the l plane, each in the bf16
// layouts), sc = 2^k of this workgroup's input, b, ty0, tx0, tid, fi, fq, frow, fcol, H, W, st, the LDS halo xs
// (SG_HPIX pixels of sg_ps_split(IN) f16) and the accumulators acc (h_a h_b) and accx (the cross terms).
// The halo holds a pixel's 32-channel chunk as [32 h | 32 l] (144 bytes with padding: 14 x 38 pixels = 74.8 KiB, two
// workgroups per CU, conflict-free ds_read_b128), staged in two chunks; conv1's K is (tap, channel) with the 3 channels
// padded to 4: a 32-wide K step packs 8 taps, the 49 taps fill 7 steps with the last 7 zero.
{
    constexpr int PS = sg_ps_split(IN);
    constexpr int NCH = MODE == SG_CONV1 ? 1 : 2;                        // 32-channel chunks
    constexpr int WPL = MODE == SG_CONV1 ? SG_W1 : SG_W64;               // f16 per weight plane
    for (int ch = 0; ch < NCH; ++ch) {
        if (ch) __syncthreads();
        // ---- stage the split halo of channels [32 ch, 32 ch + 32) (conv1: its 3 channels and a zero)
        if (MODE == SG_CONV1) {
            const long long plane = (long long)H * W;
            const float *xb = X + (long long)b * 3 * plane;
            for (int p = tid; p < SG_HPIX; p += SG_THREADS) {
                uint2 l;
                const uint2 h = sg_split_conv1_px(xb, plane, ty0 - 3 + p / SG_HW, tx0 - 3 + p % SG_HW, H, W, st, sc, l);
                *(uint4 *)&xs[p * PS] = make_uint4(h.x, h.y, l.x, l.y);
            }
        } else {
            for (int e = tid; e < SG_HPIX * 4; e += SG_THREADS) {
                const int p = e >> 2, q = e & 3;
                uint4 l;
                const uint4 h =
                    sg_split_px8<IN>(X, I, b, ty0 - 3 + p / SG_HW, tx0 - 3 + p % SG_HW, 32 * ch + 8 * q, H, W, sc, l);
                *(uint4 *)&xs[p * PS + 8 * q] = h;
                *(uint4 *)&xs[p * PS + 32 + 8 * q] = l;
            }
        }
        __syncthreads();

        if (MODE == SG_CONV1) {
            // lane quarter fq holds taps t0 = 8 s + 2 fq and t0 + 1 of K step s, 4 channels each
            const unsigned short *xr = &xs[(frow * SG_HW + fcol) * PS];
#pragma unroll
            for (int s = 0; s < 7; ++s) {
                const int t0 = 8 * s + 2 * fq, t1 = t0 + 1;
                const int o0 = ((t0 / 7) * SG_HW + t0 % 7) * PS, o1 = ((t1 / 7) * SG_HW + t1 % 7) * PS;
                sg_f16x8 bh[4], bl[4], ah[4], al[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const unsigned short *wq = Wp + ((long long)s * 64 + 16 * nt + fi) * 32 + 8 * fq;
                    bh[nt] = *(const sg_f16x8 *)wq;
                    bl[nt] = *(const sg_f16x8 *)(wq + WPL);
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint4 lo = t0 < 49 ? *(const uint4 *)&xr[o0 + 8 * m * PS] : make_uint4(0u, 0u, 0u, 0u);
                    const uint4 hi = t1 < 49 ? *(const uint4 *)&xr[o1 + 8 * m * PS] : make_uint4(0u, 0u, 0u, 0u);
                    ah[m] = sg_f16_frag(make_uint4(lo.x, lo.y, hi.x, hi.y));
                    al[m] = sg_f16_frag(make_uint4(lo.z, lo.w, hi.z, hi.w));
                }
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) sg_mma3(acc[m][nt], accx[m][nt], ah[m], al[m], bh[nt], bl[nt]);
            }
        } else {
            // K order inside a chunk: lane quarter fq holds channels 32 ch + 8 fq .. + 7 of both operands
            const unsigned short *wl = Wp + (long long)fi * 64 + 32 * ch + 8 * fq;
            for (int ky = 0; ky < 7; ++ky) {
                const unsigned short *xr = &xs[((frow + ky) * SG_HW + fcol) * PS + 8 * fq];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const unsigned short *wt = wl + (long long)(ky * 7 + kx) * 64 * 64;
                    sg_f16x8 bh[4], bl[4], ah[4], al[4];
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) {
                        bh[nt] = *(const sg_f16x8 *)(wt + nt * 16 * 64);
                        bl[nt] = *(const sg_f16x8 *)(wt + WPL + nt * 16 * 64);
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        ah[m] = *(const sg_f16x8 *)&xr[(kx + 8 * m) * PS];
                        al[m] = *(const sg_f16x8 *)&xr[(kx + 8 * m) * PS + 32];
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) sg_mma3(acc[m][nt], accx[m][nt], ah[m], al[m], bh[nt], bl[nt]);
                }
            }
        }
    }
}
