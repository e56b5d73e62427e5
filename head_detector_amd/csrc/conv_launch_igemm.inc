// Host-side launchers of conv_igemm_kernel (included inside an anonymous namespace by conv_igemm.hip and conv_rings.hip, after conv_kernels.inc and conv_cfg_list.h).
template <int BP, int BC, int WP, int WC, int KBS, int NST>
VGH_TILE_LAUNCHER(launch_cfg) {
    static PerDevice opted_in;
    if (lds > 64 * 1024) (void)opt_in_dynamic_lds(opted_in, lds, conv_igemm_kernel<BP, BC, WP, WC, KBS, 0, NST>, conv_igemm_kernel<BP, BC, WP, WC, KBS, 1, NST>);
    const dim3 grid(g.chunk * 8), block((BP / WP) * (BC / WC) * 64);
    constexpr int nw = (BP / WP) * (BC / WC);
    constexpr int loop_lds = NST * KBS * (BP + BC) * 64 + (NST > 2 ? nw * 1024 : 0), epi_lds = nw * 32 * (WC + 4) * 4;
    if (NST == 2 && (a.nkb + KBS - 1) / KBS == 1) {  // the whole K fits one stage: no second buffer -> more blocks per CU
        const int one = KBS * (BP + BC) * 64, epi = (BP / WP) * (BC / WC) * 32 * (WC + 4) * 4;
        lds = one > epi ? one : epi;
    }
    // r06: tiles whose LDS-transposed epilogue strips outweigh their stage buffers (the 96-cout wave tiles) take the REGISTER epilogue (EPI = 3, no LDS) for plain bf16
    // convs: the block's LDS drops to its stages and more blocks share a CU
#ifdef VGH_EXPERIMENTS  // measured r06 (profiles/r06_ab_regepi.txt): single-stream sum -0.9 % (L) / -1.5 % (M), the two-lane forward unchanged, stage1.conv3 33 us slower: not adopted
    static const int regepi = getenv("VGH_REGEPI") ? atoi(getenv("VGH_REGEPI")) : 0;
    if constexpr (epi_lds > loop_lds && loop_lds <= 64 * 1024) {
        if (regepi && a.fast_epi && !a.out_f32 && !a.res && !a.shuffle && a.act != VGH_ACT_SILU) {
            const int l3 = (NST == 2 && (a.nkb + KBS - 1) / KBS == 1) ? KBS * (BP + BC) * 64 : loop_lds;
            hipLaunchKernelGGL((conv_igemm_kernel<BP, BC, WP, WC, KBS, 3, NST>), grid, block, l3, st, a, g.ntc, g.total, g.chunk);
            return VGH_OK;
        }
    }
#endif
    if (a.fast_epi)
        hipLaunchKernelGGL((conv_igemm_kernel<BP, BC, WP, WC, KBS, 1, NST>), grid, block, lds, st, a, g.ntc, g.total, g.chunk);
    else
        hipLaunchKernelGGL((conv_igemm_kernel<BP, BC, WP, WC, KBS, 0, NST>), grid, block, lds, st, a, g.ntc, g.total, g.chunk);
    return VGH_OK;
}

// loader-wave tiles (conv_igemm_kernel<..., LF>): LF x the waves, the same LDS
template <int BP, int BC, int WP, int WC, int KBS, int NST, int LF>
VGH_TILE_LAUNCHER(launch_cfg_lf) {
    static PerDevice opted_in;
    if (lds > 64 * 1024) (void)opt_in_dynamic_lds(opted_in, lds, conv_igemm_kernel<BP, BC, WP, WC, KBS, 0, NST, 0, 0, LF>, conv_igemm_kernel<BP, BC, WP, WC, KBS, 1, NST, 0, 0, LF>);
    const dim3 grid(g.chunk * 8), block((BP / WP) * (BC / WC) * 64 * LF);
    if (a.fast_epi)
        hipLaunchKernelGGL((conv_igemm_kernel<BP, BC, WP, WC, KBS, 1, NST, 0, 0, LF>), grid, block, lds, st, a, g.ntc, g.total, g.chunk);
    else
        hipLaunchKernelGGL((conv_igemm_kernel<BP, BC, WP, WC, KBS, 0, NST, 0, 0, LF>), grid, block, lds, st, a, g.ntc, g.total, g.chunk);
    return VGH_OK;
}

