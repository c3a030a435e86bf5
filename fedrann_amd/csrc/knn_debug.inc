// Part of libfedrann_hip.so (included by fedrann_hip.hip ahead of the k-NN launchers): what a development build reads
// back from the kernels after a pass -- read, print, clear.  The release library compiles none of it.

// FDR_DEBUG_COUNTERS builds with bit 1 of the debug knob set: the counters the `pass` kernels of plan p have added up,
// behind everything `st` has queued, printed under `names` and cleared.  Every other build: nothing.
static int dump_debug_counters(hipStream_t st, const char *pass, const KnnPlan &p, const char *names) {
#ifdef FDR_DEBUG_COUNTERS
    if (!(dev_knobs().debug & 2)) return FDR_OK;
    unsigned long long c[8];
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpyFromSymbol(c, HIP_SYMBOL(g_dbg_counters), sizeof(c)));
    fprintf(stderr, "[fdr debug] %s grid %d x %d  %s: %llu, %llu, %llu, %llu, %llu, %llu\n", pass, p.nqb, p.nseg, names, c[0],
            c[1], c[2], c[3], c[4], c[5]);
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_counters), z, sizeof(z)));
#endif
    return FDR_OK;
}

#ifdef FDR_STAMPS
static int dump_stamps(hipStream_t st, int waves) {
    unsigned long long s[16][8];
    HIP_TRY(hipStreamSynchronize(st));  // (the other queues' launches too: `st` has joined them)
    HIP_TRY(hipMemcpyFromSymbol(s, HIP_SYMBOL(g_stamps), sizeof(s)));
    for (int w = 0; w < waves; ++w) {
        const double st_n = (double)std::max<unsigned long long>(1, s[w][5]);
        // (knn_prefilter_kernel: 0 dma-issue, 1 mfma+score, 2 share, 3 vmcnt(0), 4 barrier; knn_prefilter_pp_kernel: 0 pipe
        // turn, 1 dma-issue, 2 scoring, 3 / 4 barrier after the pipe / the other turn, 6 long other turns)
        fprintf(stderr, "[fdr stamps] wave %d: stages %llu  per stage (s_memtime ticks): ph0 %.0f  ph1 %.0f  ph2 %.0f  ph3 %.0f  "
                        "ph4 %.0f  long turns %llu\n", w, s[w][5], s[w][0] / st_n, s[w][1] / st_n, s[w][2] / st_n,
                s[w][3] / st_n, s[w][4] / st_n, s[w][6]);
    }
    unsigned long long z[16][8] = {};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), z, sizeof(z)));
    return FDR_OK;
}
#endif
