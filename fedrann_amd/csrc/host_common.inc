// Part of libfedrann_hip.so (included by fedrann_hip.hip) and of the host-only sanitizer build
// (tests/host_san/host_san.cpp): plain C++, no HIP.
#define FDR_EXPORT extern "C" __attribute__((visibility("default")))
// a helper that the kernels and the host share (the host-only sanitizer build has no HIP attributes)
#ifdef __HIPCC__
#define FDR_HOST_DEVICE __host__ __device__
#else
#define FDR_HOST_DEVICE
#endif
typedef unsigned long long u64;

// Development knobs: ONE table, read in ONE place.  The release library compiles the defaults in -- no getenv, no
// knob names in the binary (tests/test_abi.py scans it); a -DFDR_DEV build (devtools/build_dev.sh) reads
// FDR_KNN_<NAME> from the environment every time a plan is made.  The release library reads one variable, once:
// FDR_KNN_MODE in fdr_create (the initial k-NN mode of the context).
#ifndef FDR_W8_DEFAULT
#define FDR_W8_DEFAULT 1  // (a release-mode A/B of the knob's default: -DFDR_W8_DEFAULT=2 = round 3's two-unit stages)
#endif
struct DevKnobs {
    int extra = 0;         // EXTRA: candidates kept beyond k in the prefilter pass (0: the rule of prefilter_extra)
    int w8 = FDR_W8_DEFAULT;  // W8: eight-wave prefilter shape: 0 never, 1 when it fills a round, 3 always, 2 round 3's two-unit stages
    int d256 = 3;          // D256: 0 the 168-VGPR d <= 256 shape always, 1 / 2 / 3 the 256-VGPR variants (see prefilter_shape)
    int shape = -1;        // SHAPE: index into kShapes for the exact kernel (-1: knn_choose_shape's rule)
    int slots = 0;         // SLOTS: workgroups per CU of the dispatch model (0: the model's own count)
    double ov = 0.0;       // OV: fixed cost of a work item in tiles (0: 96 fp16 / 16 fp32)
    int nseg = 0;          // NSEG: that many equal target segments (0: the plan search)
    int streams = -1;      // STREAMS: queues of the synchronised rounds (-1: two where the shape allows)
    int cohort_slots = 0;  // COHORT_SLOTS: workgroups per launch of the rounds (0: the resident slots)
    int cohort = 1;        // COHORT: 0 no synchronised rounds, 1 when the query blocks exceed a round, 2 also below
    int cohort_ns = 0;     // COHORT_NS: segments of the rounds (0: the cost model's choice)
    int range8 = -1;       // RANGE8: eight-wave range pass at d <= 128: -1 from 65536 plateau queries, 0 never, 1 always
    int xrounds = 0;       // XROUNDS: the exact kernel in synchronised rounds: 0 one launch, 1 one queue, 2 two queues
    int ordered = 0;       // ORDERED: 1 the ordered scan without synchronised rounds too
    int rangepp = -1;      // RANGEPP: the range pass on the ping-pong skeleton: -1 from 4096 plateau queries, 0 never, 1 always
    int pp = -1;           // PP: the ping-pong candidate pass: -1 where prefilter_shape's rules choose it, 0 never, 1 always
    int debug = 0;         // DEBUG: bit 0 skip the top-k slow path (WRONG RESULTS, timing only), 1 event counters, 3 print
                           //        the plan, 4 the real test with a threshold nothing passes
};
#ifdef FDR_DEV
static DevKnobs dev_knobs() {
    DevKnobs k;
    auto geti = [](const char *name, int &v) { if (const char *e = getenv(name)) v = atoi(e); };
    geti("FDR_KNN_EXTRA", k.extra);
    geti("FDR_KNN_W8", k.w8);
    geti("FDR_KNN_D256", k.d256);
    geti("FDR_KNN_SHAPE", k.shape);
    geti("FDR_KNN_SLOTS", k.slots);
    if (const char *e = getenv("FDR_KNN_OV")) k.ov = atof(e);
    geti("FDR_KNN_NSEG", k.nseg);
    geti("FDR_KNN_STREAMS", k.streams);
    geti("FDR_KNN_COHORT_SLOTS", k.cohort_slots);
    geti("FDR_KNN_COHORT", k.cohort);
    geti("FDR_KNN_COHORT_NS", k.cohort_ns);
    geti("FDR_KNN_RANGE8", k.range8);
    geti("FDR_KNN_XROUNDS", k.xrounds);
    geti("FDR_KNN_ORDERED", k.ordered);
    geti("FDR_KNN_PP", k.pp);
    geti("FDR_KNN_RANGEPP", k.rangepp);
    geti("FDR_KNN_DEBUG", k.debug);
    return k;
}
#else
static constexpr DevKnobs dev_knobs() { return DevKnobs(); }
#endif

// host threads this process may really use: the affinity mask (hardware_concurrency) capped by the cgroup's CPU quota
static int host_cpu_budget() {
    int n = (int)std::thread::hardware_concurrency();
    if (n < 1) n = 1;
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32];
        long long period = 0;
        if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0) {
            const long long quota = atoll(q);
            if (quota > 0) n = (int)std::max<long long>(1, std::min<long long>(n, quota / period));
        }
        fclose(f);
    }
    return n;
}

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
