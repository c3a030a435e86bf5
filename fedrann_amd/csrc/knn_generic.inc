// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit), not compiled on its own.
// ------------------------------------------------------------------------------------------
// Exact cosine k-NN for sizes outside the MFMA kernels' shapes: d > 1024, or k > 64 / d > 512 below 8192 targets
// (knn_route).
//
// The reference accepts any -n / --nndescent-n-neighbors (fedrann/__main__.py:128-146); its defaults (500, 50)
// and BASELINE.json's configurations run on the MFMA kernels (knn_exact.inc, knn_prefilter.inc).  This kernel
// keeps the rest of the flags' range usable, with the same canonical arithmetic (the fp32 fma chain over the
// components in ascending order, clamp(1 - c, 0, 1), the zero-row rules, (distance, index) order) on the vector
// ALU: GEN_QPB query rows per workgroup stay in LDS, every thread walks one target row per chunk of 256 and
// keeps one chain per query, and a query's K best keys live in a 512-key LDS array that is re-sorted (bitonic,
// the list's 256 slots + the chunk's 256 keys) only when the chunk holds a key below the current K-th.
// Any DP that is a multiple of 8, K <= GEN_LIST.  It reads every target row once per GEN_QPB queries from L2 /
// HBM: a fallback, two orders of magnitude below the MFMA kernels.
// ------------------------------------------------------------------------------------------
#define GEN_QPB 4
#define GEN_LIST 256

__global__ __launch_bounds__(256) void knn_generic_kernel(const float *__restrict__ Qhat,
                                                          const unsigned char *__restrict__ qzero, int nq,
                                                          const float *__restrict__ That,
                                                          const unsigned char *__restrict__ tzero, int nt, int t_base,
                                                          int DP, int K, int *__restrict__ idx_out,
                                                          float *__restrict__ dist_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gen_smem[];
    f32x4 *qs = reinterpret_cast<f32x4 *>(gen_smem);  // [GEN_QPB][DP / 4] query rows in the kernel layout
    __shared__ u64 keys[GEN_QPB][2 * GEN_LIST];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * GEN_QPB;
    const int groups = DP / 8;  // 8 components = two f32x4: even components k0 k2 k4 k6 | odd components k1 k3 k5 k7
    for (int i = tid; i < GEN_QPB * (DP / 4); i += 256) {
        const int q = i / (DP / 4), c = i - q * (DP / 4);
        const int row = min(q0 + q, nq - 1);
        qs[i] = reinterpret_cast<const f32x4 *>(Qhat + (size_t)row * DP)[c];
    }
    bool qz[GEN_QPB];
    u64 kth[GEN_QPB];
#pragma unroll
    for (int q = 0; q < GEN_QPB; ++q) {
        qz[q] = qzero[min(q0 + q, nq - 1)] != 0;
        kth[q] = KEY_INF;  // (no key is admitted above it; KEY_INF itself marks an empty slot)
        keys[q][tid] = KEY_INF;
        keys[q][GEN_LIST + tid] = KEY_INF;
    }
    __syncthreads();
    for (int chunk = 0; chunk < nt; chunk += 256) {
        const int t = chunk + tid;
        const bool valid = t < nt;
        const f32x4 *tp = reinterpret_cast<const f32x4 *>(That + (size_t)(valid ? t : nt - 1) * DP);
        float c[GEN_QPB];
#pragma unroll
        for (int q = 0; q < GEN_QPB; ++q) c[q] = 0.0f;
        for (int g = 0; g < groups; ++g) {
            const f32x4 te = tp[2 * g], to = tp[2 * g + 1];
#pragma unroll
            for (int q = 0; q < GEN_QPB; ++q) {  // canonical chain: components 8g .. 8g + 7 in ascending order
                const f32x4 qe = qs[q * (DP / 4) + 2 * g], qo = qs[q * (DP / 4) + 2 * g + 1];
                c[q] = __builtin_fmaf(qe.x, te.x, c[q]);
                c[q] = __builtin_fmaf(qo.x, to.x, c[q]);
                c[q] = __builtin_fmaf(qe.y, te.y, c[q]);
                c[q] = __builtin_fmaf(qo.y, to.y, c[q]);
                c[q] = __builtin_fmaf(qe.z, te.z, c[q]);
                c[q] = __builtin_fmaf(qo.z, to.z, c[q]);
                c[q] = __builtin_fmaf(qe.w, te.w, c[q]);
                c[q] = __builtin_fmaf(qo.w, to.w, c[q]);
            }
        }
        const bool tz = valid && tzero[t] != 0;
#pragma unroll
        for (int q = 0; q < GEN_QPB; ++q) {
            // two all-zero rows are at distance 0, a zero row and a non-zero row at 1 (their chain is exactly 0)
            const float dist = (qz[q] && tz) ? 0.0f : dist_from_sim(c[q]);
            const u64 key = valid ? (((u64)__float_as_uint(dist) << 32) | (unsigned)(t_base + t)) : KEY_INF;
            if (!__syncthreads_or(key < kth[q])) continue;  // (workgroup-uniform)
            keys[q][GEN_LIST + tid] = key;
            __syncthreads();
            // ascending bitonic sort of the 512 keys: 256 threads, elements tid and tid + 256
            for (int k2 = 2; k2 <= 2 * GEN_LIST; k2 <<= 1)
                for (int j = k2 >> 1; j > 0; j >>= 1) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int i = tid + e * 256, ixj = i ^ j;
                        if (ixj > i) {
                            const u64 a = keys[q][i], b = keys[q][ixj];
                            const bool up = (i & k2) == 0;
                            if ((a > b) == up) {
                                keys[q][i] = b;
                                keys[q][ixj] = a;
                            }
                        }
                    }
                    __syncthreads();
                }
            kth[q] = keys[q][K - 1];
            __syncthreads();
            keys[q][GEN_LIST + tid] = KEY_INF;  // (the upper half is the next chunk's)
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < GEN_QPB; ++q)
        if (q0 + q < nq && tid < K) {
            const u64 key = keys[q][tid];
            idx_out[(size_t)(q0 + q) * K + tid] = (int)(unsigned)(key & 0xffffffffull);
            dist_out[(size_t)(q0 + q) * K + tid] = __uint_as_float((unsigned)(key >> 32));
        }
}
