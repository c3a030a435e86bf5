// fedrann_hip.hip -- gfx950 (MI355X / CDNA4) kernels + C-ABI for FEDRANN's hot path.
//
//   K1 embed_csr_kernel      E = A . P          (feature_extraction.py:167-213 in the reference)
//   K2 normalize_rows_kernel E -> Ehat          (done inside pynndescent in the reference)
//   K3 knn_tile_kernel       exact cosine top-k (nearest_neighbors.py:39-55 -> pynndescent)
//   K4 knn_merge_kernel      merge of per-segment top-k lists
//   S1-S4 (knn_sparse.inc)   exact cosine (S1j, S3j: Jaccard; S1w, S3w: weighted Jaccard) top-k on the sparse feature
//                            rows themselves (no projection)
//
// Written for wave64 / MFMA / 160 KB LDS directly; there is no other backend.
// ABI: include/fedrann_hip.h.  Design notes and rooflines: DESIGN.md.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/fedrann_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#include "host_common.inc"  // error plumbing, FDR_EXPORT, the development knobs (plain C++: shared with the sanitizer build)

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? FDR_E_NOMEM : FDR_E_HIP, "%s failed: %s",  \
                        #expr, hipGetErrorString(e_));                                         \
    } while (0)

// ------------------------------------------------------------------------------------------
// K1  E = A . P   -- CSR-row-parallel, one wave per read row.
//
// P (F x d) is "very sparse": >= 90 % of its feature rows are empty (density 1/sqrt(F)), so the
// projection is stored as
//   ftab[w]    = { bits: which of features 32w..32w+31 have a non-empty P row,
//                  prefix: number of non-empty rows among features < 32w }          (8 B / 32 features)
//   rowinfo[r] = { start, count, first column, first value bits } of the r-th non-empty row  (16 B)
//   ent[q]     = { column, fp32 bits }   (entries beyond a row's first)
// A wave streams a row's column ids in coalesced 64-id chunks, tests the bitmap words (L2 resident) and
// fetches rowinfo for the hits; several rows' (short rows: eight, one chunk each) or chunks' (long rows: two
// rows, four chunks each) dependent id -> bitmap -> rowinfo chains are in flight at once.  Hits are then
// applied in ascending feature order by the whole wave (lane l owns columns l, l+64, ...), which reproduces
// scipy's sequential fp32 sums bit for bit.
// ------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(256) void embed_csr_kernel(
    long long n_rows, const long long *__restrict__ a_indptr, const int *__restrict__ a_indices,
    long long n_features, const uint2 *__restrict__ ftab, const uint4 *__restrict__ rowinfo,
    const uint2 *__restrict__ ent, int d, float *__restrict__ E) {
    constexpr int NACC = DP / 64;
    static_assert(DP <= 512, "d > 512: embed_csr_wide_kernel");
    constexpr int GR = 8;   // rows a wave takes per turn
    constexpr int NB = 4;   // long rows: 64-id chunks in flight per row
    constexpr int RPW = 2;  // long rows: rows in flight
    // The id -> bitmap -> rowinfo chain is three dependent loads (~2 us a row) and the rows in flight are all that hides
    // it (stubbed lookups: the kernel's time does not depend on where rowinfo comes from, and the ordered application below
    // is 18 % of it).  SHORT rows -- every row of a turn within 64 ids: a compacted CSR's ~17 live ids -- run eight chains
    // side by side with one chunk each; LONG rows (a raw CSR's ~170 ids) two chains with four chunks each.
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
    // hits in ascending lane = ascending feature order, applied by the whole wave (lane l owns columns l, l + 64, ...)
    auto apply = [&](float (&acc)[NACC], const uint4 &inf, const bool h) __attribute__((always_inline)) {
        u64 m = __ballot(h);
        while (m) {  // wave-uniform
            const int src = __builtin_ctzll(m);
            m &= m - 1;
            int q = __builtin_amdgcn_readlane((int)inf.x, src);
            const int ee = q + __builtin_amdgcn_readlane((int)inf.y, src);
            unsigned c = (unsigned)__builtin_amdgcn_readlane((int)inf.z, src);
            float v = __int_as_float(__builtin_amdgcn_readlane((int)inf.w, src));
            while (true) {
#pragma unroll
                for (int i = 0; i < NACC; ++i)
                    if (c == (unsigned)(lane + 64 * i)) acc[i] += v;
                if (++q >= ee) break;
                const uint2 en = ent[q];  // same address in every lane
                c = en.x;
                v = __uint_as_float(en.y);
            }
        }
    };
    auto store_row = [&](const long long row, const float (&acc)[NACC]) __attribute__((always_inline)) {
        float *out = E + row * (long long)d;
#pragma unroll
        for (int i = 0; i < NACC; ++i)
            if (lane + 64 * i < d) out[lane + 64 * i] = acc[i];
    };
    for (long long row0 = wave0 * GR; row0 < n_rows; row0 += nwaves * GR) {
        long long beg[GR], len_max = 0;
        int len[GR];
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            const long long row = row0 + r < n_rows ? row0 + r : n_rows - 1;
            beg[r] = a_indptr[row];
            const long long l = row0 + r < n_rows ? a_indptr[row + 1] - beg[r] : 0;
            len[r] = (int)(l < 64 ? l : 64);
            len_max = l > len_max ? l : len_max;
        }
        if (len_max <= 64) {  // (wave-uniform)
            int f[GR];
            uint2 w[GR];
            uint4 info[GR];
            bool hit[GR];
#pragma unroll
            for (int r = 0; r < GR; ++r) f[r] = lane < len[r] ? a_indices[beg[r] + lane] : -1;
#pragma unroll
            for (int r = 0; r < GR; ++r) {
                w[r] = make_uint2(0u, 0u);
                if (f[r] >= 0 && (long long)f[r] < n_features) w[r] = ftab[f[r] >> 5];
            }
#pragma unroll
            for (int r = 0; r < GR; ++r) {
                const unsigned bit = 1u << (f[r] & 31);
                hit[r] = (w[r].x & bit) != 0u;
                info[r] = make_uint4(0u, 0u, 0u, 0u);
                if (hit[r]) info[r] = rowinfo[w[r].y + __popc(w[r].x & (bit - 1u))];
            }
#pragma unroll
            for (int r = 0; r < GR; ++r) {
                if (row0 + r >= n_rows) continue;  // (wave-uniform)
                float acc[NACC];
#pragma unroll
                for (int i = 0; i < NACC; ++i) acc[i] = 0.0f;
                apply(acc, info[r], hit[r]);
                store_row(row0 + r, acc);
            }
            continue;
        }
        for (int p0 = 0; p0 < GR && row0 + p0 < n_rows; p0 += RPW) {  // long rows, pair by pair
            const long long prow0 = row0 + p0;
            long long pbeg[RPW], pend[RPW];
            int f[RPW][NB];
            uint2 w[RPW][NB];
            uint4 info[RPW][NB];
            bool hit[RPW][NB];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const long long row = prow0 + r < n_rows ? prow0 + r : n_rows - 1;
                pbeg[r] = a_indptr[row];
                pend[r] = prow0 + r < n_rows ? a_indptr[row + 1] : pbeg[r];
            }
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const long long pos = pbeg[r] + 64 * u + lane;
                    f[r][u] = pos < pend[r] ? a_indices[pos] : -1;
                }
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    w[r][u] = make_uint2(0u, 0u);
                    if (f[r][u] >= 0 && (long long)f[r][u] < n_features) w[r][u] = ftab[f[r][u] >> 5];
                }
#pragma unroll
            for (int r = 0; r < RPW; ++r)
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const unsigned bit = 1u << (f[r][u] & 31);
                    hit[r][u] = (w[r][u].x & bit) != 0u;
                    info[r][u] = make_uint4(0u, 0u, 0u, 0u);
                    if (hit[r][u]) info[r][u] = rowinfo[w[r][u].y + __popc(w[r][u].x & (bit - 1u))];
                }
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                if (prow0 + r >= n_rows) continue;  // (wave-uniform)
                float acc[NACC];
#pragma unroll
                for (int i = 0; i < NACC; ++i) acc[i] = 0.0f;
#pragma unroll
                for (int u = 0; u < NB; ++u) apply(acc, info[r][u], hit[r][u]);
                // rows longer than the 256 ids in flight (the full CSR of a long read): the rest, chunk by chunk
                for (long long base = pbeg[r] + 64 * NB; base < pend[r]; base += 64 * NB) {
                    int f2[NB];
                    uint2 w2[NB];
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const long long pos = base + 64 * u + lane;
                        f2[u] = pos < pend[r] ? a_indices[pos] : -1;
                    }
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        w2[u] = make_uint2(0u, 0u);
                        if (f2[u] >= 0 && (long long)f2[u] < n_features) w2[u] = ftab[f2[u] >> 5];
                    }
#pragma unroll
                    for (int u = 0; u < NB; ++u) {
                        const unsigned bit = 1u << (f2[u] & 31);
                        const bool h2 = (w2[u].x & bit) != 0u;
                        uint4 i2 = make_uint4(0u, 0u, 0u, 0u);
                        if (h2) i2 = rowinfo[w2[u].y + __popc(w2[u].x & (bit - 1u))];
                        apply(acc, i2, h2);
                    }
                }
                store_row(prow0 + r, acc);
            }
        }
    }
}

// d > 512 (16+ accumulators per lane and row): two rows per wave and turn, four chunks each -- round 3's kernel; with the
// eight-row turns above hipcc no longer unrolls its loops at DP = 2048 (a stack array, 144 B of scratch).
template <int DP>
__global__ __launch_bounds__(256) void embed_csr_wide_kernel(
    long long n_rows, const long long *__restrict__ a_indptr, const int *__restrict__ a_indices,
    long long n_features, const uint2 *__restrict__ ftab, const uint4 *__restrict__ rowinfo,
    const uint2 *__restrict__ ent, int d, float *__restrict__ E) {
    constexpr int NACC = DP / 64;
    constexpr int NB = 4;   // 64-id chunks in flight per wave and row
    constexpr int RPW = 2;  // rows a wave has in flight: the id -> bitmap -> rowinfo chain is three dependent loads (~2 us a
                            // row), and the occupancy that hides it is all there is -- two rows' chains side by side
    const int lane = threadIdx.x & 63;
    const long long wave0 = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * (blockDim.x >> 6);
    for (long long row0 = wave0 * RPW; row0 < n_rows; row0 += nwaves * RPW) {
        long long beg[RPW], end[RPW];
        int f[RPW][NB];
        uint2 w[RPW][NB];
        uint4 info[RPW][NB];
        bool hit[RPW][NB];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const long long row = row0 + r < n_rows ? row0 + r : n_rows - 1;
            beg[r] = a_indptr[row];
            end[r] = row0 + r < n_rows ? a_indptr[row + 1] : beg[r];
        }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const long long pos = beg[r] + 64 * u + lane;
                f[r][u] = pos < end[r] ? a_indices[pos] : -1;
            }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                w[r][u] = make_uint2(0u, 0u);
                if (f[r][u] >= 0 && (long long)f[r][u] < n_features) w[r][u] = ftab[f[r][u] >> 5];
            }
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const unsigned bit = 1u << (f[r][u] & 31);
                hit[r][u] = (w[r][u].x & bit) != 0u;
                info[r][u] = make_uint4(0u, 0u, 0u, 0u);
                if (hit[r][u]) info[r][u] = rowinfo[w[r][u].y + __popc(w[r][u].x & (bit - 1u))];
            }
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            if (row0 + r >= n_rows) break;  // (wave-uniform)
            float acc[NACC];
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] = 0.0f;
            // hits in ascending lane = ascending feature order, applied by the whole wave (lane l owns columns l, l + 64, ...)
            auto apply = [&](const uint4 &inf, const bool h) {
                u64 m = __ballot(h);
                while (m) {  // wave-uniform
                    const int src = __builtin_ctzll(m);
                    m &= m - 1;
                    int q = __builtin_amdgcn_readlane((int)inf.x, src);
                    const int ee = q + __builtin_amdgcn_readlane((int)inf.y, src);
                    unsigned c = (unsigned)__builtin_amdgcn_readlane((int)inf.z, src);
                    float v = __int_as_float(__builtin_amdgcn_readlane((int)inf.w, src));
                    while (true) {
#pragma unroll
                        for (int i = 0; i < NACC; ++i)
                            if (c == (unsigned)(lane + 64 * i)) acc[i] += v;
                        if (++q >= ee) break;
                        const uint2 en = ent[q];  // same address in every lane
                        c = en.x;
                        v = __uint_as_float(en.y);
                    }
                }
            };
#pragma unroll
            for (int u = 0; u < NB; ++u) apply(info[r][u], hit[r][u]);
            // rows longer than the 256 ids in flight (the full CSR of a long read): the rest, chunk by chunk
            for (long long base = beg[r] + 64 * NB; base < end[r]; base += 64 * NB) {
                int f2[NB];
                uint2 w2[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const long long pos = base + 64 * u + lane;
                    f2[u] = pos < end[r] ? a_indices[pos] : -1;
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    w2[u] = make_uint2(0u, 0u);
                    if (f2[u] >= 0 && (long long)f2[u] < n_features) w2[u] = ftab[f2[u] >> 5];
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const unsigned bit = 1u << (f2[u] & 31);
                    const bool h2 = (w2[u].x & bit) != 0u;
                    uint4 i2 = make_uint4(0u, 0u, 0u, 0u);
                    if (h2) i2 = rowinfo[w2[u].y + __popc(w2[u].x & (bit - 1u))];
                    apply(i2, h2);
                }
            }
            float *out = E + (row0 + r) * (long long)d;
#pragma unroll
            for (int i = 0; i < NACC; ++i)
                if (lane + 64 * i < d) out[lane + 64 * i] = acc[i];
        }
    }
}

// ------------------------------------------------------------------------------------------
// K2  row normalisation into the k-NN kernel's layout.
//
// One lane per row runs the canonical chain n = fma(x_k, x_k, n), k ascending (the same order
// the MFMA uses along K), rinv = (float)(1/sqrt((double)n)), xhat_k = x_k * rinv.  A 64-row tile is
// staged through LDS so that both the global read and the global write are coalesced.
// Output row: DP floats, zero padded; inside each group of 8 components the order is
// [k0 k2 k4 k6 | k1 k3 k5 k7] so that lane-half h of the MFMA reads its four K-steps
// (components 8g + 2s + h, s = 0..3) as ONE 16-byte access.
// ------------------------------------------------------------------------------------------
template <int DP, int RB, bool VEC>
__global__ __launch_bounds__(256) void normalize_rows_kernel(const float *__restrict__ E,
                                                             long long n_rows, int d,
                                                             float *__restrict__ Ehat,
                                                             unsigned char *__restrict__ zero) {
    // 256 threads move the RB rows in and out (VEC: 16 bytes per lane and access -- d a multiple of 4, both bases 16-byte
    // aligned: 32 instead of 128 dependent-latency round trips per row block, four waves of them instead of one), the first
    // RB threads run the rows' chains.
    __shared__ float tile[RB][DP + 1];  // +1: the per-lane row walk below is bank-conflict free
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * RB;
    const int nr = (int)min((long long)RB, n_rows - row0);
    const float *src = E + row0 * (long long)d;
    if (d < DP || nr < RB) {
        for (int i = tid; i < RB * DP; i += 256) tile[i / DP][i % DP] = 0.0f;
        __syncthreads();
    }
    const int total = nr * d;
    if constexpr (VEC) {
        const f32x4 *src4 = reinterpret_cast<const f32x4 *>(src);
        for (int i4 = tid; i4 < total / 4; i4 += 256) {
            const f32x4 v = src4[i4];
            const int i = 4 * i4, r = i / d, c = i - r * d;  // (d % 4 == 0: the four stay in one row)
            tile[r][c] = v[0];
            tile[r][c + 1] = v[1];
            tile[r][c + 2] = v[2];
            tile[r][c + 3] = v[3];
        }
    } else {
        for (int i = tid; i < total; i += 256) tile[i / d][i % d] = src[i];
    }
    __syncthreads();
    if (tid < RB) {
        float n = 0.0f;
#pragma unroll 8
        for (int k = 0; k < DP; ++k) {
            const float x = tile[tid][k];
            n = __builtin_fmaf(x, x, n);
        }
        float ri = 0.0f;
        if (n > 0.0f) ri = (float)(1.0 / sqrt((double)n));
#pragma unroll 8
        for (int k = 0; k < DP; ++k) tile[tid][k] = tile[tid][k] * ri;
        if (tid < nr) zero[row0 + tid] = n > 0.0f ? 0 : 1;
    }
    __syncthreads();
    float *dst = Ehat + row0 * (long long)DP;
    if constexpr (VEC) {
        f32x4 *dst4 = reinterpret_cast<f32x4 *>(dst);
        for (int i4 = tid; i4 < nr * DP / 4; i4 += 256) {
            const int i = 4 * i4, r = i / DP, p = i % DP;  // (p % 4 == 0: s = 0 .. 3 below)
            const int g = p >> 3, hh = (p >> 2) & 1;
            const float *t = &tile[r][8 * g + hh];
            dst4[i4] = f32x4{t[0], t[2], t[4], t[6]};
        }
    } else {
        for (int i = tid; i < nr * DP; i += 256) {
            const int r = i / DP, p = i % DP;
            const int g = p >> 3, hh = (p >> 2) & 1, s = p & 3;
            dst[i] = tile[r][8 * g + 2 * s + hh];
        }
    }
}

#include "knn_plan.inc"           // shapes, LDS budgets, target segments (plain C++)
#include "knn_workspace.inc"      // the workspace of a k-NN call: its regions, once (plain C++)
#include "projection_tables.inc"  // the embed kernel's lookup tables (plain C++)
#include "csr_compact.inc"        // dead-feature filter (plain C++)
#include "host_upload.inc"        // host CSR -> device in chunks, raw over PCIe and compacted on the host at once: the scheduler (plain C++)
#include "knn_exact.inc"      // K3 / K4: fp32 MFMA tile kernel with LDS top-k lists, merge
#include "knn_exact_wide.inc"  // K3s: K3 for 512 < d <= 1024, the components split over two waves
#include "knn_prefilter.inc"  // P1 / P2: fp16 MFMA candidate pass, merges, certificate + re-rank, range pass; fragment_addresses, RangeHits
#include "knn_prefilter_pp.inc"  // P1 and the range pass for the 256-register shapes: the two waves of a SIMD take turns at the matrix pipe
#include "knn_order.inc"      // P1: scan order by chunk mask (sort keys, ordered fp16 copy)
#include "knn_prefilter_live.inc"  // P1 at d <= 128: only the query block's non-empty chunks (block masks, blocked copy)
#include "dedup_classes.inc"  // duplicate-row classes: hash, tables, gathers, expansion
#include "knn_generic.inc"    // d > 1024, or k > 64 / d > 512 below 8192 targets: every pair on the vector ALU

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// The one idea of a buffer that the context has: an array of T that only grows, in device memory (DevArray<T>) or
// in pinned host memory (PinnedArray<T>).  reserve() counts elements, frees before it allocates and holds at least
// one byte once it has allocated; ptr() is the one statement of the element type.  Non-copyable.
template <class T, bool Pinned>
class GrowArray {
    void *p = nullptr;
    size_t cap = 0;  // bytes

public:
    int reserve(size_t count) {
        const size_t bytes = count * sizeof(T), ask = bytes ? bytes : 1;
        if (bytes <= cap) return FDR_OK;
        release();
        const hipError_t e = Pinned ? hipHostMalloc(&p, ask, hipHostMallocDefault) : hipMalloc(&p, ask);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(FDR_E_NOMEM, "%s(%zu bytes) failed: %s", Pinned ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
        }
        cap = bytes;
        return FDR_OK;
    }
    T *ptr() const { return static_cast<T *>(p); }
    void release() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    size_t bytes() const { return cap; }  // the capacity
    GrowArray() = default;
    GrowArray(const GrowArray &) = delete;
    GrowArray &operator=(const GrowArray &) = delete;
    ~GrowArray() { release(); }  // (fdr_destroy has made the context's device current)
};
template <class T>
using DevArray = GrowArray<T, false>;
template <class T>
using PinnedArray = GrowArray<T, true>;
template <class... A>
static void release_all(A &...arrays) {
    (arrays.release(), ...);
}

// `count` elements between the host and a device array: one hipMemcpyAsync, whose size and types the array states.
// Neither reserves nor synchronises.
template <class T>
static hipError_t upload(const DevArray<T> &to, const T *src, size_t count, hipStream_t st) {
    return hipMemcpyAsync(to.ptr(), src, count * sizeof(T), hipMemcpyHostToDevice, st);
}
template <class T>
static hipError_t download(T *dst, const DevArray<T> &from, size_t count, hipStream_t st) {
    return hipMemcpyAsync(dst, from.ptr(), count * sizeof(T), hipMemcpyDeviceToHost, st);
}

// A rocprim algorithm on temporary storage that the context owns.  `call(tmp, bytes)` makes the rocprim call with these
// two as its first arguments, so the algorithm's other arguments are written once: rocprim_reserve asks it for its
// size (tmp = null) and grows the storage, rocprim_run does the same and then runs it.  At least one byte is held, so
// the run never passes the null pointer that rocprim takes for another size query.  A sequence of several algorithms
// calls rocprim_reserve with all of them first: then no run of the sequence regrows the storage (a regrow would be
// safe, hipFree waits for the device, but it stalls the queue).
template <class... F>
static int rocprim_reserve(DevArray<char> &tmp, const F &...calls) {
    size_t need = 1;
    hipError_t e = hipSuccess;
    auto ask = [&](const auto &call) {
        size_t bytes = 0;
        if (e == hipSuccess) e = call(nullptr, bytes);
        need = std::max(need, bytes);
    };
    (ask(calls), ...);
    if (e != hipSuccess) return fail(FDR_E_HIP, "rocprim temporary storage size query failed: %s", hipGetErrorString(e));
    return tmp.reserve(need);
}
template <class F>
static int rocprim_run(DevArray<char> &tmp, const char *what, const F &call) {
    if (int rc = rocprim_reserve(tmp, call)) return rc;
    size_t bytes = tmp.bytes();
    const hipError_t e = call(tmp.ptr(), bytes);
    if (e != hipSuccess)  // (HIP_TRY's message)
        return fail(e == hipErrorOutOfMemory ? FDR_E_NOMEM : FDR_E_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return FDR_OK;
}

// What the last k-NN call did, for the fdr_last_* getters.
struct KnnCallRecord {
    struct {
        int flagged = 0;               // queries that took the exact path (exact mode certifies nothing: 0)
        int launches = 0, queues = 0;  // of the candidate pass
    } pass;
    int unique_targets = 0, unique_queries = 0;  // duplicate-row classes
    // fdr_last_query_paths: per-query path codes (in that call's workspace), or one code for all rows
    struct {
        const uint8_t *dev = nullptr;
        int64_t n = 0;  // 0: nothing recorded
        uint8_t all = FDR_PATH_NONE;
        hipStream_t stream = nullptr;
    } paths;
    fdr_knn_trace trace = {};  // fdr_last_knn_trace: the kernels the call ran
};

// The arguments of a k-NN call: nq query rows against nt target rows numbered from t_base, k neighbours each.
struct KnnArgs {
    const float *Qhat;  // queries, normalised (normalize_rows_kernel's layout), and their all-zero flags
    const uint8_t *qzero;
    int64_t nq;
    const float *That;  // targets, likewise
    const uint8_t *tzero;
    int64_t nt, t_base;
    int d, k;
    int32_t *idx;  // [nq, k] results
    float *dist;
    void *ws;
    size_t ws_bytes;
    hipStream_t st;
};

// Every stage owns its device scratch and the state that describes it, in one struct of the context: release() frees
// the one and resets the other in the same place, so neither outlives the other.

// fdr_kmer_search / fdr_kmer_search_indices (kmer_search.inc)
struct KmerSearchScratch {
    DevArray<unsigned char> seq;           // the reads' characters, concatenated (+ 64 bytes of padding)
    DevArray<long long> off;               // [n_reads + 1] their offsets
    DevArray<u64> lib_codes;               // the library's codes
    DevArray<u64> keys;                    // the table: code + 1 (0: a free slot) ...
    DevArray<unsigned> vals;               // ... and its library index
    DevArray<u64> bloom;                   // the filter's words
    DevArray<unsigned long long> counter;  // hits found (counts past the hit buffer's capacity)
    DevArray<u64> pairs, sorted;           // the hits (read << 32 | index) as found; sorted
    DevArray<int> flag, scan;              // 1 where a sorted hit differs from its predecessor; the inclusive scan
    DevArray<int> indices, rows;           // the unique hits' index and read parts
    DevArray<long long> indptr;            // [n_reads + 1] the rows' first unique hits
    DevArray<char> tmp;                    // rocprim's temporary storage
    long long nnz = 0;                     // unique hits of the last search, until fdr_kmer_search_indices fetches them
    void release() {
        release_all(seq, off, lib_codes, keys, vals, bloom, counter, pairs, sorted, flag, scan, indices, rows, indptr, tmp);
        nnz = 0;
    }
};

// fdr_kmer_count_* (kmer_search.inc): counting in blocks, the export, the W-way merge, the fetch
struct KmerCountScratch {
    // a block of reads (kc_block_runs)
    DevArray<unsigned char> seq;  // the block's characters (+ 64 bytes of padding)
    DevArray<long long> off;      // its reads' offsets
    DevArray<u64> codes;          // one canonical code per position; once they are sorted, the block's run codes
    DevArray<u64> sorted;         // the block's sorted codes; after the last block, the KEPT codes that the fetch copies
    DevArray<unsigned> run_len;   // the runs' lengths ...
    DevArray<unsigned> n_runs;    // ... and their number
    DevArray<u64> run_counts;     // the lengths as 64-bit counts
    // the table accumulated over the blocks: [acc] is current and holds na entries, the other one takes the next merge
    // (fdr_kmer_count_merge, which replaces the table anyway, puts the host's runs into [0])
    DevArray<u64> acc_codes[2], acc_counts[2];
    DevArray<u64> merged_codes, merged_counts;  // table and block merged, equal codes not yet summed; in the W-way merge
                                                // the owners' codes and totals at their merged places
    DevArray<unsigned long long> n_table;       // entries after the sum
    // the threshold (fdr_kmer_count_finish, km_merge)
    DevArray<int> keep, keep_scan;  // 1 per entry that stays; the inclusive scan
    DevArray<u64> kept_counts;      // the kept entries' counts (their codes: `sorted`)
    // the small tables of the W-way merge and of the export
    DevArray<long long> run_off, samp_pre;  // [n_runs + 1] each: the runs' offsets, the prefix of their sample counts
    DevArray<u64> samples, bounds;          // every KM_STRIDE-th code of every run; sorted: the tile boundaries
    DevArray<long long> slices;             // [tiles + 1, n_runs] a tile's first element in each run
    DevArray<long long> part_off;           // [n_parts + 1] fdr_kmer_count_export_dev
    DevArray<char> tmp;                     // rocprim's temporary storage
    int k = 0;         // incremental counting: k (0: not begun, finished, or released)
    int acc = 0;       // ... which of the two tables is current
    long long na = 0;  // ... its entries
    long long n = 0;   // kept entries of the last finish / merge, until fdr_kmer_count_fetch fetches them
    // These two survive release(): the setting of fdr_set_kmer_count_block, and the blocks of the last count, which
    // fdr_last_kmer_count_blocks reports after the fetch as well (fdr_kmer_count_begin resets it).
    int64_t block_chars = 0;
    int blocks = 0;
    void release() {
        release_all(seq, off, codes, sorted, run_len, n_runs, run_counts, acc_codes[0], acc_codes[1], acc_counts[0],
                    acc_counts[1], merged_codes, merged_counts, n_table, keep, keep_scan, kept_counts, run_off, samp_pre,
                    samples, bounds, slices, part_off, tmp);
        k = acc = 0;
        na = n = 0;
    }
};

// The context's one sparse index (knn_sparse.inc): what fdr_sparse_index_build leaves for the searches, and the
// build's scratch, which is kept with it
struct SparseIndex {
    DevArray<long long> indptr;      // [n + 1] the rows
    DevArray<int> indices;           // the stored entries' features ...
    DevArray<float> values;          // ... their values, as given (absent: every entry 1) ...
    DevArray<float> xhat;            // ... normalised (cosine); as the postings take them (weighted Jaccard)
    DevArray<int> asize;             // [n] the rows' set sizes (Jaccard)
    DevArray<float> mass;            // [n] the rows' fp32 sums of values (weighted Jaccard)
    DevArray<unsigned char> zero;    // [n] zero (Jaccard: empty) rows
    DevArray<u64> keys, sorted_keys; // S1's posting keys (feature << 32 | row); sorted.  `keys`: see run_flags()
    DevArray<unsigned> pos, sorted_pos;  // each key's stored entry, the sort's values; sorted.  `pos`: see posting_rows()
    DevArray<int> efeat;             // each stored entry's run (-1: no posting)
    DevArray<float> pval;            // the postings' values (cosine, weighted Jaccard)
    DevArray<long long> runptr;      // [runs + 1] the runs' first postings
    DevArray<int> runfeat;           // [runs] the runs' features, ascending: how a query row outside the index finds a run
    DevArray<int> heavy;             // [n] a search's queries for S3r
    DevArray<u64> cnt;               // SP_CNT_* counters in [0, 8) (SP_CNT_RUNS: the number of runs); behind them zidx() and zdist()
    DevArray<char> tmp;              // rocprim's temporary storage
    struct Built {  // the index these hold; none after a refused or failed build
        bool valid = false;
        int metric = 0;
        long long n = 0, kept = 0, nzero = 0;  // rows, postings, zero (Jaccard: empty) rows
        long long n_features = 0;              // the columns: the ids a query row may hold
    } built;
    // The sort has read the unsorted keys, and nothing reads them again: their 8 bytes per stored entry hold two int32
    // per posting (kept <= stored entries), the run-start flags in [0, kept) and the inclusive run numbers behind them.
    int *run_flags() const { return reinterpret_cast<int *>(keys.ptr()); }
    int *run_numbers(long long kept) const { return run_flags() + kept; }
    // Likewise S2 reads the sorted positions only, so it writes the posting rows (int32, one per posting, in posting
    // order) over the unsorted ones; that is where the searches read them.
    int *posting_rows() const { return reinterpret_cast<int *>(pos.ptr()); }
    // S4's closed-form row of a zero query lies behind the eight counters: FDR_MAX_K indices, then FDR_MAX_K distances
    // (written per search, read by S3 in the same search).
    static constexpr size_t cnt_words = 8 + FDR_MAX_K;
    int *zidx() const { return reinterpret_cast<int *>(cnt.ptr() + 8); }
    float *zdist() const { return reinterpret_cast<float *>(zidx() + FDR_MAX_K); }
    template <class F>
    auto each(F f) {
        return f(indptr, indices, values, xhat, asize, mass, zero, keys, sorted_keys, pos, sorted_pos, efeat, pval, runptr,
                 runfeat, heavy, cnt, tmp);
    }
    size_t bytes() {  // fdr_sparse_index_info: everything held, the build's scratch included
        return each([](auto &...a) { return (a.bytes() + ...); });
    }
    void release() {
        each([](auto &...a) { release_all(a...); });
        built = {};
    }
};

// The query rows of fdr_sparse_index_query (knn_sparse.inc): a CSR of rows that need not be in the index, uploaded per
// call, and what S1q makes of them, the query side of that call's search.  Grows as needed; released with the index.
struct SparseQuerySet {
    DevArray<long long> indptr;    // [nq + 1] the query rows
    DevArray<int> indices;         // the stored entries' features ...
    DevArray<float> values;        // ... their values, as given (absent: every entry 1) ...
    DevArray<float> xhat;          // ... normalised (cosine); raw (weighted Jaccard)
    DevArray<int> efeat;           // each stored entry's run in the INDEX (-1: none)
    DevArray<int> asize;           // [nq] the set sizes (Jaccard)
    DevArray<float> mass;          // [nq] the masses (weighted Jaccard)
    DevArray<unsigned char> zero;  // [nq] zero (empty, zero-mass) queries
    DevArray<int> heavy;           // [nq] the call's queries for S3r
    template <class F>
    auto each(F f) {
        return f(indptr, indices, values, xhat, efeat, asize, mass, zero, heavy);
    }
    size_t bytes() {
        return each([](auto &...a) { return (a.bytes() + ...); });
    }
    void release() {
        each([](auto &...a) { release_all(a...); });
    }
};

// What a radius search counts, emits and holds (knn_radius_common.inc: the protocol; each index owns one): the
// per-query counts and their scan, the counted entries as keys (dist_bits << 32 | row) and the held result of the last
// call, which the owner's *_radius_fetch copies out.  Grows as needed; released with its owner.
#define RR_FLAG_MISMATCH 0  // queries whose emitted count differs from the counted one (or that hold a row out of range)
#define RR_FLAG_ZLIST 1     // the zero rows that zlist took
#define RR_FLAG_ZEROQ 2     // the dense search's: zero rows among the call's queries ...
#define RR_FLAG_NZERO 3     // ... and the index's zero rows (a build's count)
#define RR_FLAGS 4
struct RadiusResult {
    DevArray<long long> count, off;  // [nq + 1] the queries' counts (a 0 behind them); their exclusive scan
    DevArray<u64> keys, sorted;      // [counted] the keys as the emit pass leaves them, then the result (see idx());
                                     // every query's keys in (distance bits, index) order
    DevArray<int> zlist;             // [zero rows of the index] in index order: the row of a zero query
    DevArray<u64> flags;             // RR_FLAG_*
    long long counted = 0;           // the total of the last call's counts: the entries of keys and sorted
    long long held = -1;             // hits of the last radius call, until the owner's next call (-1: none)
    // The unsorted keys are dead once the sort has read them: their 8 bytes per entry take the result, `held`
    // indices (int32) and behind them `held` distances (held <= counted).
    int *idx() const { return reinterpret_cast<int *>(keys.ptr()); }
    float *dist() const { return reinterpret_cast<float *>(idx() + held); }
    void drop() { held = -1; }
    template <class F>
    auto each(F f) { return f(count, off, keys, sorted, zlist, flags); }
    size_t bytes() { return each([](auto &...a) { return (a.bytes() + ...); }); }
    void release() {
        each([](auto &...a) { release_all(a...); });
        counted = 0;
        held = -1;
    }
};

// The radius searches of the sparse index (knn_sparse_radius.inc): what they hold beside their RadiusResult, in which
// `keys` takes the heavy queries' hits as found.  Released with the index.
struct SparseRadius {
    RadiusResult rr;
    DevArray<long long> seg_lo, seg_hi;  // [heavy queries] their segments of the keys, for the segmented sort
    DevArray<unsigned char> handed;  // [nq] queries the count pass handed to its range form: the emit pass skips them
    size_t bytes() { return rr.bytes() + seg_lo.bytes() + seg_hi.bytes() + handed.bytes(); }
    void release() {
        rr.release();
        release_all(seg_lo, seg_hi, handed);
    }
};

// The context's one dense index (knn_dense_radius.inc): what fdr_dense_index_build / _embed leave for the radius
// searches, and those searches' buffers.  Independent of the sparse index; grows as needed; kept until
// fdr_dense_index_free.
struct DenseIndex {
    DevArray<float> ehat;          // [n, dp] the normalised rows (normalize_rows_kernel's layout)
    DevArray<_Float16> half;       // ... their fp16 copy, which the range pass streams
    DevArray<unsigned char> zero;  // [n] zero rows
    DevArray<float> qhat;          // fdr_dense_index_radius_query: the call's query rows, likewise
    DevArray<_Float16> qhalf;
    DevArray<unsigned char> qzero;
    DevArray<float> theta;         // [nq] the queries' thresholds (a zero query: -inf)
    RadiusResult rr;               // count: the candidates, then the hits, per query; off: the candidates' segments;
                                   // keys: D-R3's; sorted: D-R2's rows in the first half, then the sorted keys
    DevArray<long long> ind;       // [nq + 1] the hits' exclusive scan (the result's indptr)
    DevArray<int> fill;            // [nq] rows the emit pass wrote, or would have written, per query
    DevArray<char> tmp;            // rocprim's temporary storage
    bool valid = false;
    long long n = 0, nzero = 0;
    int d = 0, dp = 0;
    long long last_candidates = 0, last_hits = 0;  // fdr_dense_index_info: the last radius call
    int last_query_blocks = 0, last_segments = 0;
    template <class F>
    auto each(F f) {
        return f(ehat, half, zero, qhat, qhalf, qzero, theta, ind, fill, tmp);
    }
    size_t bytes() { return rr.bytes() + each([](auto &...a) { return (a.bytes() + ...); }); }
    void release() {
        each([](auto &...a) { release_all(a...); });
        rr.release();
        valid = false;
        n = nzero = 0;
        d = dp = 0;
        last_candidates = last_hits = 0;
        last_query_blocks = last_segments = 0;
    }
};

// fdr_topk_merge (topk_merge.inc): the parts as uploaded, the merged rows before they are copied out, and the record
// of a refused call.  Grows as needed; freed with the context.
struct TopkMergeScratch {
    DevArray<int> idx_parts;     // [n_parts, nq, kp] the candidates' indices ...
    DevArray<float> dist_parts;  // ... and distances, part-major
    DevArray<int> idx_out;       // [nq, k] the merged rows
    DevArray<float> dist_out;
    DevArray<u64> refusal;       // [1] the smallest (query, part, rule) the check found; all ones: none
    void release() { release_all(idx_parts, dist_parts, idx_out, dist_out, refusal); }
};

// fdr_radius_merge (radius_merge.inc): the ragged parts as uploaded, where their rows start, the merged rows before
// they are copied out, and the record of a refused call.  Grows as needed; freed with the context.
struct RadiusMergeScratch {
    DevArray<int> starts;             // [n_parts, nq + 1] row (p, q)'s first entry in idx_parts / dist_parts
    DevArray<int> indptr_out;         // [nq + 1] the merged rows' first entries
    DevArray<int2> items;             // the kernel's work items: (query, chunk of 64 of its entries)
    DevArray<int> idx_parts;          // the parts' entries, concatenated in part order: the indices ...
    DevArray<float> dist_parts;       // ... and the distances
    DevArray<int> idx_out;            // the merged rows
    DevArray<float> dist_out;
    DevArray<u64> refusal;            // [1] the smallest (query, part, rule) the check found; all ones: none
    std::vector<int> h_starts, h_indptr_out;  // the host's side of starts and indptr_out (built from the checked indptrs)
    std::vector<int2> h_items;                // ... and of items
    void release() { release_all(starts, indptr_out, items, idx_parts, dist_parts, idx_out, dist_out, refusal); }
};

// fdr_graph_symmetrize (graph_symmetrize.inc): the graph as uploaded, its rows ordered by index, what the count pass
// found per entry, and the result, counted and held in a RadiusResult of its own (count / off: the result's rows; keys:
// as the emit pass leaves them, then the held result; sorted: the rows in key order).  Grows as needed; freed by
// fdr_graph_free and with the context.
struct GraphSymScratch {
    RadiusResult rr;
    DevArray<long long> indptr;    // [n + 1] the input's row pointer
    DevArray<int> idx;             // the input's entries as uploaded: the indices ...
    DevArray<float> dist;          // ... and the distances
    DevArray<int> row;             // per entry: its row
    DevArray<u64> packed, byidx;   // per entry: index << 32 | distance bits, as uploaded; every row ordered by index
    DevArray<unsigned> partner;    // per entry of byidx (q -> t): the bits of (t -> q), GS_NO_PARTNER where t does not list q
    DevArray<unsigned> fill;       // [n] entries the emit pass placed through a row's cursor
    DevArray<u64> refusal;         // [1] the smallest (row, rule) the checks found; all ones: none
    DevArray<char> tmp;            // rocprim's temporary storage
    std::vector<long long> h_off;  // the result's row pointer on its way to indptr_out
    template <class F>
    auto each(F f) {
        return f(indptr, idx, dist, row, packed, byidx, partner, fill, refusal, tmp);
    }
    size_t bytes() { return rr.bytes() + each([](auto &...a) { return (a.bytes() + ...); }); }
    void release() {
        each([](auto &...a) { release_all(a...); });
        rr.release();
    }
};

// fdr_graph_components (graph_components.inc): the union-find over the rows and what its labelling passes make of it.
// The graph itself goes through GraphSymScratch's input arrays.  Grows as needed; freed by fdr_graph_free and with the
// context.
struct GraphCompScratch {
    DevArray<int> parent;        // [n] the union-find: parent[x] <= x, a root is its own parent
    DevArray<int> root;          // [n] every row's root once the links are in: its component's smallest row
    DevArray<unsigned> count;    // [n] rows per root (0 at every other row)
    DevArray<int> flag, rank;    // [n + 1] root[r] == r (a 0 behind them); their exclusive scan, whose last element is C
    DevArray<int> label;         // [n] rank[root[r]]
    DevArray<long long> size;    // [n] the first C: count[] of the roots, in label order
    template <class F>
    auto each(F f) { return f(parent, root, count, flag, rank, label, size); }
    size_t bytes() { return each([](auto &...a) { return (a.bytes() + ...); }); }
    void release() { each([](auto &...a) { release_all(a...); }); }
};

// fdr_graph_expand (graph_expand.inc): the distinct rows within two hops of a block of rows.  The graph itself goes
// through GraphSymScratch's input arrays, as fdr_graph_components' does.  The held result is `out` with its row pointer
// on the device (`off`) and on the host (h_off: fdr_rescore_rows_refine lists its work items from it), kept until the
// next fdr_graph_expand or fdr_graph_free, whatever fdr_graph_symmetrize and fdr_graph_components do in between.
struct GraphExpandScratch {
    DevArray<long long> bound, boff;  // [nq + 1] the rows' upper bounds (a 0 behind them); their exclusive scan
    DevArray<unsigned> cand;          // [bound entries + 1] the one- and two-hop indices as gathered; then the run heads
    DevArray<unsigned> sorted;        // [bound entries] every segment ascending
    DevArray<unsigned> pos;           // [bound entries + 1] the run heads' exclusive scan: an entry's place in `out`
    DevArray<long long> off;          // [nq + 1] HELD: the result's row pointer
    DevArray<int> out;                // [held] HELD: the result's indices
    DevArray<u64> flags;              // [1] stores that fell outside their segment (an internal error)
    std::vector<long long> h_off;     // [nq + 1] HELD: `off` on the host
    long long held = -1;              // the held result's entries (-1: none)
    long long n = 0, q_lo = 0, nq = 0;  // the held result's graph and rows
    template <class F>
    auto each(F f) { return f(bound, boff, cand, sorted, pos, off, out, flags); }
    size_t bytes() { return each([](auto &...a) { return (a.bytes() + ...); }); }
    void drop() { held = -1; }
    void release() {
        each([](auto &...a) { release_all(a...); });
        std::vector<long long>().swap(h_off);
        held = -1;
        n = q_lo = nq = 0;
    }
};

// The re-score calls (sparse_rescore.inc).  RsCsr: a CSR as uploaded and what the row pass X1 makes of its rows.
// RsLists: rectangular candidate lists, the re-scored rows before they are copied out, and the record of a refused
// call.  fdr_sparse_rescore owns one of each (SparseRescoreScratch), valid within one call, freed with the context;
// the held row set of fdr_rescore_rows_* (RescoreRowSet) owns another of each, so neither call sees the other's.
#define RS_CNT_ERR 0      // or of SP_ERR_* bits of the rows
#define RS_CNT_REFUSAL 1  // the smallest candidate outside [0, n): X2 (query row of the call << 8 | slot), X3 (query
                          // row of the call << 32 | position in its row); all ones: none
#define RS_CNT_WORDS 2
struct RsCsr {
    DevArray<long long> indptr;      // [n + 1] the rows
    DevArray<int> indices;           // the stored entries' features ...
    DevArray<float> values;          // ... their values, as given (absent: every entry 1) ...
    DevArray<float> x;               // ... normalised (cosine); raw (weighted Jaccard)
    DevArray<unsigned char> present; // ... 1 where the value is not +-0 (Jaccard with values)
    DevArray<int> asize;             // [n] the set sizes (Jaccard)
    DevArray<float> mass;            // [n] the masses (weighted Jaccard)
    DevArray<unsigned char> zero;    // [n] zero (empty, zero-mass) rows
    template <class F>
    auto each(F f) { return f(indptr, indices, values, x, present, asize, mass, zero); }
    size_t bytes() { return each([](auto &...a) { return (a.bytes() + ...); }); }
    void release() { each([](auto &...a) { release_all(a...); }); }
};
struct RsLists {
    DevArray<int> cand;              // [nq, k_in] the candidates
    DevArray<int> idx_out;           // [nq, k_out] the re-scored rows
    DevArray<float> dist_out;
    DevArray<u64> cnt;               // RS_CNT_*
    size_t bytes() { return cand.bytes() + idx_out.bytes() + dist_out.bytes() + cnt.bytes(); }
    void release() { release_all(cand, idx_out, dist_out, cnt); }
};
struct SparseRescoreScratch {
    RsCsr csr;
    RsLists lists;
    void release() {
        csr.release();
        lists.release();
    }
};

// The context's one re-score row set (fdr_rescore_rows_*, sparse_rescore.inc): the rows as fdr_rescore_rows_build's X1
// left them, for any number of _knn (X2) and _radius (X3) calls, and those calls' buffers.  Independent of the sparse
// index, the dense index and fdr_sparse_rescore's scratch; grows as needed; kept until fdr_rescore_rows_free.
struct RescoreRowSet {
    RsCsr csr;                        // (values: dead behind X1, released by the build)
    RsLists lists;                    // _knn's lists and results; cand and cnt serve _radius too
    DevArray<long long> cand_indptr;  // [nq + 1] _radius: the candidates' segments
    DevArray<int2> items;             // ... its work items: (query row of the call, batch of FDR_MAX_K of its candidates)
    std::vector<int2> h_items;        // ... as the host lists them while it checks cand_indptr
    RadiusResult rr;                  // count: the hits per query; off: their scan; keys: X3's, in the candidates'
                                      // places, then the result; sorted: the candidate segments, sorted
    DevArray<char> tmp;               // rocprim's temporary storage
    bool valid = false, has_values = false;
    int metric = 0;
    long long n = 0, stored = 0;
    size_t bytes() {
        return csr.bytes() + lists.bytes() + cand_indptr.bytes() + items.bytes() + rr.bytes() + tmp.bytes();
    }
    void release() {
        csr.release();
        lists.release();
        release_all(cand_indptr, items, tmp);
        std::vector<int2>().swap(h_items);
        rr.release();
        valid = has_values = false;
        metric = 0;
        n = stored = 0;
    }
};

// The projection that fdr_projection_load left for launch_embed (K1's tables, see embed_csr_kernel), fdr_csr_compact
// and the upload scheduler (the bitmap's host copy).
struct Projection {
    DevArray<uint2> ftab;          // [ceil(n_features / 32)] bitmap word, prefix
    DevArray<uint4> crow;          // [p_rows] the non-empty rows' records (the kernel's rowinfo)
    DevArray<uint2> ent;           // the entries beyond a row's first
    std::vector<uint32_t> h_bits;  // host copy of ftab's bitmap words
    long long n_features = 0;
    int d = 0;
    long long p_nnz = 0, p_rows = 0;
    bool loaded() const { return n_features > 0; }
    // The host builds the tables as plain C++ records (projection_tables.inc, shared with the sanitizer build); the
    // kernel reads the same bytes as uint2 / uint4.
    static const uint2 *as_dev(const PU2 *t) { return reinterpret_cast<const uint2 *>(t); }
    static const uint4 *as_dev(const PU4 *t) { return reinterpret_cast<const uint4 *>(t); }
    static_assert(sizeof(PU2) == sizeof(uint2) && sizeof(PU4) == sizeof(uint4), "table records = the kernel's uint2 / uint4");
    void release() {
        release_all(ftab, crow, ent);
        h_bits.clear();
        n_features = p_nnz = p_rows = 0;
        d = 0;
    }
};

// A host CSR on its way to the device (upload_csr, upload_embed_pipelined and its UploadLink): valid within one call.
struct CsrUpload {
    DevArray<int64_t> a_indptr, c_indptr;    // the caller's rows as they are; the chunks the host compacted
    DevArray<int32_t> a_indices, c_indices;
    PinnedArray<int32_t> stage_ids;          // the compacted chunks' pinned staging, which the helpers fill
    PinnedArray<int64_t> stage_ptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // the two raw runs in flight; [2] behind the last copy out of the staging
    hup::WorkerPool pool;                    // the helpers
    // Before a pipelined upload reserves or fills anything: the events exist, and the staging is not touched (grown,
    // or written by this call's helpers) under a copy the last call left in flight.
    int begin() {
        for (hipEvent_t &e : ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_TRY(hipEventSynchronize(ev[2]));
        return FDR_OK;
    }
    void release() {  // (the caller has synchronised the stream and stopped the pool)
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        release_all(a_indptr, c_indptr, a_indices, c_indices, stage_ids, stage_ptr);
    }
};

// The scratch of the calls that take host pointers (fdr_embed, fdr_knn, fdr_embed_knn; fdr_dense_index_build / _embed /
// _radius_query for E).  Grows as needed, freed with the context; the contents are valid only inside the call that
// wrote them, so nothing that outlives a call (an index, a held result) may live here.
struct CallScratch {
    DevArray<float> E;      // [n, d] the call's rows as uploaded or embedded
    DevArray<float> Ehat;   // [n, dp] ... normalised (normalize_rows_kernel's layout)
    DevArray<uint8_t> zero; // [n] ... their all-zero flags
    DevArray<char> ws;      // the k-NN workspace: bytes, which knn_workspace.inc carves by offset (KnnArgs::ws)
    void release() { release_all(E, Ehat, zero, ws); }
};
// Where a search's [nq, k] results wait for their copy to the host: the dense host-pointer calls (knn_from_device_E)
// and the sparse index's searches (sp_search_tail) both stage here, each for the length of one call.
struct ResultStaging {
    DevArray<int32_t> idx;
    DevArray<float> dist;
    void release() { release_all(idx, dist); }
};

// fdr_set_knn_capture / fdr_last_candidates / fdr_last_range_sets / fdr_last_live_stage_lists (test support): the
// context's copies of the prefilter pass's intermediate results, taken out of the call's workspace.
struct KnnCapture {
    int what = 0;                                  // FDR_CAPTURE_* of fdr_set_knn_capture; survives the calls
    bool cand_valid = false, range_valid = false;
    int64_t nq = 0, n_range = 0;
    int kp = 0, qbits = 0;
    DevArray<u64> cand;                            // [nq, kp] the merged candidate keys
    DevArray<int> rq, rcnt, rrows;                 // per range query: id, count, [RANGE_CAP] rows ...
    DevArray<float> rtheta;                        // ... and threshold
    hipStream_t stream = nullptr;                  // of the call that wrote these
    DevArray<uint16_t> lists;                      // the live-chunk pass's stage lists (FDR_CAPTURE_LIVE_LISTS) ...
    struct {                                       // ... and their geometry
        int nseg = 0;  // 0: nothing recorded
        int nt = 0;
        SegBounds segs;
        hipStream_t stream = nullptr;
    } skip;
    // `count` elements of a call's workspace, device to device, behind the first `at` of one of the arrays
    template <class T>
    static hipError_t keep(const DevArray<T> &to, size_t at, const T *from, size_t count, hipStream_t st) {
        return hipMemcpyAsync(to.ptr() + at, from, count * sizeof(T), hipMemcpyDeviceToDevice, st);
    }
    void invalidate() {  // every k-NN entry point, and a prefilter call that failed: the getters refuse
        cand_valid = range_valid = false;
        nq = n_range = 0;
        skip.nseg = 0;
    }
    void release() {
        release_all(cand, rq, rcnt, rrows, rtheta, lists);
        invalidate();
    }
};

struct fdr_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    hipStream_t aux_stream[3] = {nullptr, nullptr, nullptr};  // further queues for the prefilter pass's launches
    hipEvent_t aux_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // [0] fork, [1..3] joins
    hipDeviceProp_t prop;
    Projection proj;       // fdr_projection_load's tables
    CsrUpload up;          // the host-pointer calls: a CSR on its way to the device ...
    CallScratch call;      // ... their rows and workspace ...
    ResultStaging res;     // ... and results, which the sparse searches stage here too
    KmerSearchScratch ks;  // k-mer search, k-mer count / merge (kmer_search.inc): both released at every fetch
    KmerCountScratch kc;
    SparseIndex sp;        // sparse k-NN (knn_sparse.inc): kept until fdr_sparse_index_free
    SparseQuerySet spq;    // ... and the query rows of fdr_sparse_index_query, released with it
    SparseRadius spr;      // ... and the radius searches' counts and hits (knn_sparse_radius.inc), released with it
    DenseIndex di;         // the dense index and its radius searches (knn_dense_radius.inc): kept until fdr_dense_index_free
    TopkMergeScratch tm;   // the merge of the ranks' candidate lists (topk_merge.inc): kept until fdr_destroy
    RadiusMergeScratch rm; // the merge of the ranks' ragged radius rows (radius_merge.inc): kept until fdr_destroy
    SparseRescoreScratch rs;  // the exact re-score of candidate lists (sparse_rescore.inc): kept until fdr_destroy
    RescoreRowSet rrs;     // the held re-score rows and their calls (sparse_rescore.inc): kept until fdr_rescore_rows_free
    GraphSymScratch gs;    // a graph's symmetrised rows and their call (graph_symmetrize.inc): kept until fdr_graph_free
    GraphCompScratch gc;   // a graph's union-find and labels (graph_components.inc): kept until fdr_graph_free
    GraphExpandScratch ge; // a block of rows' two-hop candidates and their call (graph_expand.inc): kept until fdr_graph_free
    // timing: when enabled, every launch of kernel kind i gets its own hipEvent pair on the launch
    // stream; fdr_timing_read() sums the elapsed times of all launches since the last read
    int knn_mode = FDR_MODE_AUTO;
    int dedup_mode = FDR_DEDUP_AUTO;
    int live_mode = FDR_LIVE_AUTO;  // fdr_set_live_chunks
    std::vector<unsigned> live_host;  // the live-chunk plan's read-back: the query blocks' masks
    int skip_mode = FDR_SKIP_AUTO;    // fdr_set_live_skip
    int tail_mode = FDR_TAIL_AUTO;    // fdr_set_pass_tail
    std::vector<hipEvent_t> tail_ev;  // "this queue has been given group g's last launch" (launch_rounds), made on demand
    std::vector<int> skip_host;       // ... and the lengths of the stage lists, [segment][mask value]
    int compact_mode = FDR_COMPACT_AUTO;  // fdr_set_rerank_compact
    KnnCallRecord last;  // what the fdr_last_* getters report
    KnnCapture cap;      // the prefilter pass's intermediate results, where fdr_set_knn_capture asked for them
    // duplicate-row classes built by fdr_knn_classes_dev for the calls that follow it (fdr_knn_unique_dev /
    // fdr_knn_expand_dev): the tables live in the caller's workspace
    struct {
        bool valid = false;
        const float *That = nullptr;
        const uint8_t *tzero = nullptr;
        int64_t nt = 0, nq_max = 0;
        int d = 0, k = 0, nu = 0;
        void *ws = nullptr;
        size_t ws_bytes = 0;
    } cls;
    bool timing = false;
    std::vector<hipEvent_t> ev_pool[FDR_NUM_KERNELS];  // start, stop, start, stop, ...
    size_t ev_used[FDR_NUM_KERNELS] = {};
};

// Every k-NN entry point starts here, before its argument checks: no earlier call's trace, path codes or capture
// survive it.  `pass` and the unique counts do: fdr_last_uncertified / fdr_last_prefilter_launches / fdr_last_unique
// report the last SEARCH, also after an fdr_knn_expand_dev or a call that failed its checks.
static void knn_call_begin(fdr_ctx *ctx) {
    ctx->last.trace = fdr_knn_trace{};
    ctx->last.paths = {};
    ctx->cap.invalidate();
}

// the trace's header: a call of `kind` on (dp, k, nq, nt)
static void knn_call_header(fdr_ctx *ctx, int kind, int dp, int k, int64_t nq, int64_t nt) {
    ctx->last.trace.kind = kind;
    ctx->last.trace.dp = dp;
    ctx->last.trace.k = k;
    ctx->last.trace.queries = nq;
    ctx->last.trace.targets = nt;
}
// "this whole call took `path`": one code for all nq rows, no candidate pass, nothing left uncertified
static void knn_call_whole(fdr_ctx *ctx, uint8_t path, int kind, int dp, int k, int64_t nq, int64_t nt) {
    knn_call_header(ctx, kind, dp, k, nq, nt);
    ctx->last.paths = {nullptr, nq, path, nullptr};
    ctx->last.pass = {};
}

static int timing_begin(fdr_ctx *ctx, int kind, hipStream_t st) {
    if (!ctx->timing) return FDR_OK;
    std::vector<hipEvent_t> &pool = ctx->ev_pool[kind];
    if (ctx->ev_used[kind] + 2 > pool.size()) {
        hipEvent_t a, b;
        HIP_TRY(hipEventCreate(&a));
        HIP_TRY(hipEventCreate(&b));
        pool.push_back(a);
        pool.push_back(b);
    }
    HIP_TRY(hipEventRecord(pool[ctx->ev_used[kind]], st));
    return FDR_OK;
}

static int timing_end(fdr_ctx *ctx, int kind, hipStream_t st) {
    if (!ctx->timing) return FDR_OK;
    HIP_TRY(hipEventRecord(ctx->ev_pool[kind][ctx->ev_used[kind] + 1], st));
    ctx->ev_used[kind] += 2;
    return FDR_OK;
}

static int use_device(fdr_ctx *ctx) {
    if (!ctx) return fail(FDR_E_ARG, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    return FDR_OK;
}

FDR_EXPORT const char *fdr_last_error(void) { return g_err; }

FDR_EXPORT int fdr_padded_dim(int d) { return padded_dim(d); }

FDR_EXPORT int fdr_create(int device_id, fdr_ctx **out) {
    if (!out) return fail(FDR_E_ARG, "fdr_create: out is null");
    *out = nullptr;
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (n <= 0) return fail(FDR_E_HIP, "no HIP device visible: the MI355X path cannot run");
    if (device_id < 0 || device_id >= n)
        return fail(FDR_E_ARG, "device %d out of range (have %d)", device_id, n);
    fdr_ctx *c = new (std::nothrow) fdr_ctx();
    if (!c) return fail(FDR_E_NOMEM, "out of host memory");
    c->device = device_id;
    hipError_t e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipGetDeviceProperties(&c->prop, device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(FDR_E_HIP, "fdr_create: device %d: %s", device_id, hipGetErrorString(e));
    }
    c->num_cus = c->prop.multiProcessorCount > 0 ? c->prop.multiProcessorCount : 256;
    // the one environment variable of the release library, read once: the context's initial k-NN mode
    if (const char *m = getenv("FDR_KNN_MODE")) {
        if (strcmp(m, "exact") == 0) c->knn_mode = FDR_MODE_EXACT;
        else if (strcmp(m, "prefilter") == 0) c->knn_mode = FDR_MODE_PREFILTER;
    }
    *out = c;
    return FDR_OK;
}

FDR_EXPORT int fdr_destroy(fdr_ctx *ctx) {
    if (!ctx) return FDR_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->up.pool.stop();
    ctx->up.release();
    for (int i = 0; i < FDR_NUM_KERNELS; ++i)
        for (hipEvent_t e : ctx->ev_pool[i]) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(ctx->stream);
    for (hipStream_t a : ctx->aux_stream)
        if (a) {
            (void)hipStreamSynchronize(a);
            (void)hipStreamDestroy(a);
        }
    for (hipEvent_t e : ctx->aux_ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->tail_ev) (void)hipEventDestroy(e);
    delete ctx;
    return FDR_OK;
}

FDR_EXPORT int fdr_device_info(fdr_ctx *ctx, char *buf, int buflen) {
    if (!ctx || !buf || buflen <= 0) return fail(FDR_E_ARG, "fdr_device_info: bad argument");
    snprintf(buf, (size_t)buflen, "%s|%s|%d|%zu", ctx->prop.name, ctx->prop.gcnArchName,
             ctx->prop.multiProcessorCount, (size_t)ctx->prop.totalGlobalMem);
    return FDR_OK;
}

FDR_EXPORT int fdr_last_uncertified(fdr_ctx *ctx) { return ctx ? ctx->last.pass.flagged : 0; }

FDR_EXPORT int fdr_last_query_paths(fdr_ctx *ctx, uint8_t *paths, int64_t n_queries) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (!paths || n_queries <= 0) return fail(FDR_E_ARG, "last_query_paths: bad argument");
    const auto &rec = ctx->last.paths;
    if (rec.n != n_queries)
        return fail(FDR_E_STATE, "last_query_paths: the last k-NN call recorded codes for %lld query rows, not %lld",
                    (long long)rec.n, (long long)n_queries);
    if (!rec.dev) {
        memset(paths, rec.all, (size_t)n_queries);
        return FDR_OK;
    }
    HIP_TRY(hipMemcpyAsync(paths, rec.dev, (size_t)n_queries, hipMemcpyDeviceToHost, rec.stream));
    HIP_TRY(hipStreamSynchronize(rec.stream));
    return FDR_OK;
}

FDR_EXPORT int fdr_last_unique(fdr_ctx *ctx, int *unique_targets, int *unique_queries) {
    if (!ctx || !unique_targets || !unique_queries) return fail(FDR_E_ARG, "bad argument");
    *unique_targets = ctx->last.unique_targets;
    *unique_queries = ctx->last.unique_queries;
    return FDR_OK;
}

FDR_EXPORT int fdr_last_prefilter_launches(fdr_ctx *ctx, int *launches, int *queues) {
    if (!ctx || !launches || !queues) return fail(FDR_E_ARG, "bad argument");
    *launches = ctx->last.pass.launches;
    *queues = ctx->last.pass.queues;
    return FDR_OK;
}

FDR_EXPORT int fdr_last_knn_trace(fdr_ctx *ctx, fdr_knn_trace *out) {
    if (!ctx || !out) return fail(FDR_E_ARG, "bad argument");
    *out = ctx->last.trace;
    return FDR_OK;
}

FDR_EXPORT int fdr_set_knn_capture(fdr_ctx *ctx, int what) {
    if (!ctx || what < 0 || what > (FDR_CAPTURE_CANDIDATES | FDR_CAPTURE_RANGE | FDR_CAPTURE_LIVE_LISTS)) return fail(FDR_E_ARG, "bad capture flags");
    ctx->cap.what = what;
    return FDR_OK;
}

FDR_EXPORT int fdr_last_candidates(fdr_ctx *ctx, uint64_t *keys, int64_t n_queries, int32_t kp, int32_t *qbits_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (!keys || n_queries <= 0 || kp <= 0) return fail(FDR_E_ARG, "last_candidates: bad argument");
    if (!ctx->cap.cand_valid) return fail(FDR_E_STATE, "last_candidates: the last k-NN call captured no candidates");
    if (ctx->cap.nq != n_queries || ctx->cap.kp != kp)
        return fail(FDR_E_STATE, "last_candidates: the last k-NN call captured %lld x %d keys, not %lld x %d",
                    (long long)ctx->cap.nq, ctx->cap.kp, (long long)n_queries, kp);
    static_assert(sizeof(u64) == sizeof(uint64_t), "the ABI's keys are the kernels'");
    HIP_TRY(download(reinterpret_cast<u64 *>(keys), ctx->cap.cand, (size_t)n_queries * kp, ctx->cap.stream));
    HIP_TRY(hipStreamSynchronize(ctx->cap.stream));
    if (qbits_out) *qbits_out = ctx->cap.qbits;
    return FDR_OK;
}

FDR_EXPORT int fdr_last_range_sets(fdr_ctx *ctx, int64_t n_range, int32_t *queries, float *theta, int32_t *counts,
                                   int32_t *rows) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (!queries || !theta || !counts || !rows || n_range <= 0) return fail(FDR_E_ARG, "last_range_sets: bad argument");
    if (!ctx->cap.range_valid) return fail(FDR_E_STATE, "last_range_sets: the last k-NN call captured no range pass");
    if (ctx->cap.n_range != n_range)
        return fail(FDR_E_STATE, "last_range_sets: the last k-NN call captured %lld range queries, not %lld",
                    (long long)ctx->cap.n_range, (long long)n_range);
    const hipStream_t st = ctx->cap.stream;
    HIP_TRY(download(queries, ctx->cap.rq, (size_t)n_range, st));
    HIP_TRY(download(theta, ctx->cap.rtheta, (size_t)n_range, st));
    HIP_TRY(download(counts, ctx->cap.rcnt, (size_t)n_range, st));
    HIP_TRY(download(rows, ctx->cap.rrows, (size_t)n_range * RANGE_CAP, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int64_t i = 0; i < n_range; ++i)  // (the slots the pass did not fill hold whatever the workspace held)
        for (int m = std::max(0, std::min(counts[i], RANGE_CAP)); m < RANGE_CAP; ++m) rows[i * RANGE_CAP + m] = -1;
    return FDR_OK;
}

FDR_EXPORT int fdr_set_knn_mode(fdr_ctx *ctx, int mode) {
    if (!ctx || mode < FDR_MODE_AUTO || mode > FDR_MODE_PREFILTER) return fail(FDR_E_ARG, "bad k-NN mode");
    ctx->knn_mode = mode;
    return FDR_OK;
}

FDR_EXPORT int fdr_set_dedup_mode(fdr_ctx *ctx, int mode) {
    if (!ctx || mode < FDR_DEDUP_AUTO || mode > FDR_DEDUP_FORCE) return fail(FDR_E_ARG, "bad duplicate-row mode");
    ctx->dedup_mode = mode;
    return FDR_OK;
}

FDR_EXPORT int fdr_set_live_chunks(fdr_ctx *ctx, int mode) {
    if (!ctx || mode < FDR_LIVE_AUTO || mode > FDR_LIVE_FORCE) return fail(FDR_E_ARG, "bad live-chunk mode");
    ctx->live_mode = mode;
    return FDR_OK;
}

FDR_EXPORT int fdr_set_pass_tail(fdr_ctx *ctx, int mode) {
    if (!ctx || mode < FDR_TAIL_AUTO || mode > FDR_TAIL_EARLY_GROUP) return fail(FDR_E_ARG, "bad pass-tail mode");
    ctx->tail_mode = mode;
    return FDR_OK;
}

FDR_EXPORT int fdr_set_live_skip(fdr_ctx *ctx, int mode) {
    if (!ctx || mode < FDR_SKIP_AUTO || mode > FDR_SKIP_OFF) return fail(FDR_E_ARG, "bad stage-skip mode");
    ctx->skip_mode = mode;
    return FDR_OK;
}

FDR_EXPORT int fdr_set_rerank_compact(fdr_ctx *ctx, int mode) {
    if (!ctx || mode < FDR_COMPACT_AUTO || mode > FDR_COMPACT_FORCE) return fail(FDR_E_ARG, "bad compact re-rank mode");
    ctx->compact_mode = mode;
    return FDR_OK;
}

FDR_EXPORT int fdr_last_live_stage_lists(fdr_ctx *ctx, int32_t segment, int32_t *first_row_out, int32_t *nstages_out,
                                         int32_t *lens, uint16_t *lists) {
    int rc = use_device(ctx);
    if (rc) return rc;
    const auto &rec = ctx->cap.skip;
    if (rec.nseg <= 0)
        return fail(FDR_E_STATE, "last_live_stage_lists: the last k-NN call captured no live-chunk pass's stage lists");
    if (segment < 0 || segment >= rec.nseg || !nstages_out)
        return fail(FDR_E_ARG, "last_live_stage_lists: bad argument (the pass had %d segments)", rec.nseg);
    const int t_begin = rec.segs.b[segment], t_end = std::min(rec.nt, rec.segs.b[segment + 1]);
    const int nstages = t_end > t_begin ? (t_end - t_begin + 127) >> 7 : 0;
    *nstages_out = nstages;
    if (first_row_out) *first_row_out = t_begin;
    if (lens) memcpy(lens, ctx->skip_host.data() + (size_t)segment * 256, 256 * sizeof(int));
    if (!lists || nstages == 0) return FDR_OK;
    const int stride = live_list_stride(nstages);
    const size_t row = (size_t)nstages * sizeof *lists;  // (a list's entries, in bytes)
    HIP_TRY(hipMemcpy2DAsync(lists, row, ctx->cap.lists.ptr() + (size_t)live_stage_row(t_begin, segment) * 256,
                             (size_t)stride * sizeof *lists, row, 256, hipMemcpyDeviceToHost, rec.stream));
    HIP_TRY(hipStreamSynchronize(rec.stream));
    for (int v = 0; v < 256; ++v)  // (the entries behind a list's end hold whatever the workspace held)
        for (int i = std::max(0, std::min(ctx->skip_host[(size_t)segment * 256 + v], nstages)); i < nstages; ++i)
            lists[(size_t)v * nstages + i] = 0xffffu;
    return FDR_OK;
}

FDR_EXPORT int fdr_timing(fdr_ctx *ctx, int enable) {
    if (!ctx) return fail(FDR_E_ARG, "null context");
    ctx->timing = enable != 0;
    for (int i = 0; i < FDR_NUM_KERNELS; ++i) ctx->ev_used[i] = 0;
    return FDR_OK;
}

FDR_EXPORT int fdr_timing_read(fdr_ctx *ctx, int which, int *count_out, float *total_ms_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (which < 0 || which >= FDR_NUM_KERNELS || !count_out || !total_ms_out)
        return fail(FDR_E_ARG, "fdr_timing_read: bad argument");
    float total = 0.f;
    const size_t used = ctx->ev_used[which];
    for (size_t i = 0; i + 1 < used; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventSynchronize(ctx->ev_pool[which][i + 1]));
        HIP_TRY(hipEventElapsedTime(&ms, ctx->ev_pool[which][i], ctx->ev_pool[which][i + 1]));
        total += ms;
    }
    *count_out = (int)(used / 2);
    *total_ms_out = total;
    ctx->ev_used[which] = 0;
    return FDR_OK;
}

// ---- projection ------------------------------------------------------------------------------
FDR_EXPORT int fdr_projection_load(fdr_ctx *ctx, int64_t n_features, int32_t d,
                                   const int64_t *p_indptr, const int32_t *p_cols,
                                   const float *p_vals) {
    int rc = use_device(ctx);
    if (rc) return rc;
    ProjectionTables T;
    if ((rc = build_projection_tables(n_features, d, p_indptr, p_cols, p_vals, T))) return rc;
    const std::vector<PU2> &ftab = T.ftab, &ent = T.ent;
    const std::vector<PU4> &crow = T.rowinfo;
    Projection &P = ctx->proj;
    if ((rc = P.ftab.reserve(ftab.size()))) return rc;
    if ((rc = P.crow.reserve(crow.size()))) return rc;
    if ((rc = P.ent.reserve(ent.size()))) return rc;
    HIP_TRY(upload(P.ftab, P.as_dev(ftab.data()), ftab.size(), ctx->stream));
    HIP_TRY(upload(P.crow, P.as_dev(crow.data()), crow.size(), ctx->stream));
    HIP_TRY(upload(P.ent, P.as_dev(ent.data()), ent.size(), ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    P.n_features = n_features;
    P.d = d;
    P.p_nnz = p_indptr[n_features];
    P.p_rows = T.rows;
    P.h_bits.resize(ftab.size());  // host copy of the bitmap: fdr_csr_compact
    for (size_t w = 0; w < ftab.size(); ++w) P.h_bits[w] = ftab[w].x;
    return FDR_OK;
}

FDR_EXPORT int fdr_csr_compact(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices,
                               int64_t *out_indptr, int32_t *out_indices, int64_t out_capacity, int32_t n_threads) {
    if (!ctx) return fail(FDR_E_ARG, "null context");
    if (!ctx->proj.loaded()) return fail(FDR_E_STATE, "csr_compact: no projection loaded");
    return csrc::compact(ctx->proj.h_bits, ctx->proj.n_features, n_rows, a_indptr, a_indices, out_indptr, out_indices,
                         out_capacity, n_threads);
}

FDR_EXPORT int fdr_host_register(fdr_ctx *ctx, void *ptr, size_t bytes) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (!ptr || bytes == 0) return fail(FDR_E_ARG, "host_register: empty buffer");
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return FDR_OK;
}

FDR_EXPORT int fdr_host_unregister(fdr_ctx *ctx, void *ptr) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (!ptr) return fail(FDR_E_ARG, "host_unregister: null pointer");
    HIP_TRY(hipHostUnregister(ptr));
    return FDR_OK;
}

// ---- launches --------------------------------------------------------------------------------
static int launch_embed(fdr_ctx *ctx, int64_t n_rows, const int64_t *d_indptr,
                        const int32_t *d_indices, float *d_E, hipStream_t st) {
    const Projection &P = ctx->proj;
    if (!P.loaded()) return fail(FDR_E_STATE, "embed: no projection loaded");
    if (n_rows < 0) return fail(FDR_E_ARG, "embed: n_rows < 0");
    if (n_rows == 0) return FDR_OK;
    const int dp = fdr_padded_dim(P.d);
    const long long blocks_needed = (n_rows + 7) / 8;  // (four waves per block, two to eight rows per wave and turn; grid-stride)
    const int grid = (int)std::min<long long>(blocks_needed, (long long)ctx->num_cus * 8 * 4);
    int trc = timing_begin(ctx, FDR_KERNEL_EMBED, st);
    if (trc) return trc;
#define FDR_LAUNCH_EMBED(DP_)                                                                   \
    hipLaunchKernelGGL(FDR_EMBED_KERNEL<DP_>, dim3(grid), dim3(256), 0, st, (long long)n_rows,  \
                       (const long long *)d_indptr, d_indices, P.n_features, P.ftab.ptr(),      \
                       P.crow.ptr(), P.ent.ptr(), P.d, d_E)
#define FDR_EMBED_KERNEL embed_csr_kernel
    if (dp == 128)
        FDR_LAUNCH_EMBED(128);
    else if (dp == 256)
        FDR_LAUNCH_EMBED(256);
    else if (dp == 512)
        FDR_LAUNCH_EMBED(512);
#undef FDR_EMBED_KERNEL
#define FDR_EMBED_KERNEL embed_csr_wide_kernel
    else if (dp == 1024)
        FDR_LAUNCH_EMBED(1024);
    else
        FDR_LAUNCH_EMBED(2048);
#undef FDR_EMBED_KERNEL
#undef FDR_LAUNCH_EMBED
    HIP_TRY(hipGetLastError());
    return timing_end(ctx, FDR_KERNEL_EMBED, st);
}

static int launch_normalize(fdr_ctx *ctx, const float *d_E, int64_t n_rows, int d, float *d_Ehat,
                            uint8_t *d_zero, hipStream_t st) {
    const int dp = fdr_padded_dim(d);
    if (dp < 0) return fail(FDR_E_ARG, "normalize: dimension %d unsupported (1..%d)", d, FDR_MAX_DIM);
    if (n_rows < 0) return fail(FDR_E_ARG, "normalize: n_rows < 0");
    if (n_rows == 0) return FDR_OK;
    const int rb = dp == 128 ? 64 : dp == 256 ? 32 : dp == 512 ? 16 : dp == 1024 ? 8 : 4;
    const long long grid = (n_rows + rb - 1) / rb;
    if (grid > 0x7fffffffll) return fail(FDR_E_ARG, "normalize: too many rows");
    int trc = timing_begin(ctx, FDR_KERNEL_NORMALIZE, st);
    if (trc) return trc;
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(d_E) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_Ehat) & 15) == 0;
#define FDR_LAUNCH_NORM(DP_, RB_)                                                                                  \
    do {                                                                                                            \
        if (vec)                                                                                                    \
            hipLaunchKernelGGL((normalize_rows_kernel<DP_, RB_, true>), dim3((unsigned)grid), dim3(256), 0, st, d_E, \
                               (long long)n_rows, d, d_Ehat, d_zero);                                              \
        else                                                                                                        \
            hipLaunchKernelGGL((normalize_rows_kernel<DP_, RB_, false>), dim3((unsigned)grid), dim3(256), 0, st,    \
                               d_E, (long long)n_rows, d, d_Ehat, d_zero);                                         \
    } while (0)
    if (dp == 128) FDR_LAUNCH_NORM(128, 64);
    else if (dp == 256) FDR_LAUNCH_NORM(256, 32);
    else if (dp == 512) FDR_LAUNCH_NORM(512, 16);
    else if (dp == 1024) FDR_LAUNCH_NORM(1024, 8);
    else FDR_LAUNCH_NORM(2048, 4);
#undef FDR_LAUNCH_NORM
    HIP_TRY(hipGetLastError());
    return timing_end(ctx, FDR_KERNEL_NORMALIZE, st);
}

// ---- k-NN workspaces (knn_workspace.inc): what rocprim asks for, the context's view ---------------------------------
static size_t order_sort_tmp_bytes(size_t rows) {
    size_t t = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t, (u64 *)nullptr, (u64 *)nullptr, (int *)nullptr, (int *)nullptr, rows, 0, 40,
                                    (hipStream_t) nullptr);
    return t;
}
static size_t class_tables_tmp_bytes(size_t rows) {
    size_t t_sort = 0, t_scan = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t_sort, (u64 *)nullptr, (u64 *)nullptr, (int *)nullptr, (int *)nullptr, rows, 0,
                                    64, (hipStream_t) nullptr);
    (void)rocprim::inclusive_scan(nullptr, t_scan, (int *)nullptr, (int *)nullptr, rows, rocprim::plus<int>(),
                                  (hipStream_t) nullptr);
    return std::max(t_sort, t_scan);
}
static WsEnv ws_env(const fdr_ctx *ctx) {
    return {ctx->num_cus, ctx->knn_mode, ctx->dedup_mode, order_sort_tmp_bytes, class_tables_tmp_bytes, ctx->live_mode,
            ctx->compact_mode};
}

FDR_EXPORT size_t fdr_knn_workspace_bytes(fdr_ctx *ctx, int64_t nq, int64_t nt, int32_t d,
                                          int32_t k) {
    if (!ctx || nq <= 0 || nt <= 0 || k <= 0 || k > FDR_MAX_K || fdr_padded_dim(d) < 0) return 0;
    return knn_workspace_bytes(ws_env(ctx), nq, nt, d, k);
}

// ---- the kernels of kShapes (knn_plan.inc) ---------------------------------------------------------------------------
// Built for the entries with `release` set (a development build: every entry); -DFDR_SHAPE_MASK=<bits of KnnShapeId>
// and -DFDR_LH_MASK=<16 | 32 | 48> narrow the candidate pass's kernels further (hipcc takes minutes per kernel).  An
// entry that is not compiled is a null pointer.
#ifndef FDR_SHAPE_MASK
#define FDR_SHAPE_MASK (~0ull)
#endif
#ifndef FDR_LH_MASK
#define FDR_LH_MASK 48
#endif
typedef void (*TileKernel)(const float *, const unsigned char *, int, const float *, const unsigned *, int, int, SegBounds,
                           int, int, u64 *, unsigned *, int, int, int FDR_DBG_PARAM);
typedef void (*PassKernel)(const _Float16 *, int, const _Float16 *, int, int, SegBounds, int, int, u64 *, unsigned *, int,
                           int, int, OrderArgs FDR_DBG_PARAM);
typedef void (*RangeKernel)(const _Float16 *, const float *, int, const _Float16 *, int, int, SegBounds, RangeOut);
static_assert(kShapes[FDR_R128].tps == RANGE_STAGES && kShapes[FDR_R256].tps == RANGE_STAGES &&
              kShapes[FDR_R512].tps == RANGE_STAGES, "the range kernel's ring");

template <int S>
static constexpr bool shape_compiled() {
    constexpr KnnShape e = kShapes[S];
#ifdef FDR_DEV
    constexpr bool built = true;
#else
    constexpr bool built = e.release;
#endif
    constexpr bool pass = e.family == FDR_FAM_PREFILTER || e.family == FDR_FAM_PINGPONG;
    return built && (!pass || (((unsigned long long)(FDR_SHAPE_MASK) >> S) & 1));
}
template <int S>
static constexpr TileKernel tile_kernel() {
    constexpr KnnShape e = kShapes[S];
    if constexpr (e.family == FDR_FAM_TILE && shape_compiled<S>()) return knn_tile_kernel<e.dp, e.nq, e.nw, e.wps>;
    else if constexpr (e.family == FDR_FAM_TILE_SPLIT && shape_compiled<S>()) return knn_tile_split_kernel<e.dp>;
    else return nullptr;
}
template <int S, int LH>
static constexpr PassKernel pass_kernel() {
    constexpr KnnShape e = kShapes[S];
    if constexpr (!shape_compiled<S>() || !(e.lists & LH & FDR_LH_MASK)) return nullptr;
    else if constexpr (e.family == FDR_FAM_PREFILTER)
        return knn_prefilter_kernel<e.dp, e.nq, e.nw, e.wps, e.units(), LH, e.paired && LH == 16>;
    else if constexpr (e.family == FDR_FAM_PINGPONG) return knn_prefilter_pp_kernel<e.dp, e.units(), LH>;
    else return nullptr;
}
template <int S>
static constexpr RangeKernel range_kernel() {
    constexpr KnnShape e = kShapes[S];
    if constexpr (!shape_compiled<S>()) return nullptr;
    else if constexpr (e.family == FDR_FAM_RANGE) return knn_range_kernel<e.dp, e.nw, e.dp == 128 ? e.wps : 2>;  // (kShapes: R256)
    else if constexpr (e.family == FDR_FAM_RANGE_PP) return knn_range_pp_kernel<e.dp, e.units()>;
    else return nullptr;
}
template <size_t... S>
struct KnnKernelTable {
    static constexpr TileKernel tile[] = {tile_kernel<S>()...};
    static constexpr PassKernel pass[][2] = {{pass_kernel<S, 16>(), pass_kernel<S, 32>()}...};  // [shape][K' > 32]
    static constexpr RangeKernel range[] = {range_kernel<S>()...};
};
template <size_t... S>
static KnnKernelTable<S...> knn_kernel_table(std::index_sequence<S...>);
typedef decltype(knn_kernel_table(std::make_index_sequence<FDR_NUM_SHAPES>())) KnnKernels;

static int no_kernel(int shape) {
    return fail(FDR_E_STATE, "this development build was compiled without the kernel shape this call needs (kShapes[%d])",
                shape);
}

#include "knn_debug.inc"  // development builds: the kernels' counters and stamps after a pass

// Launches a pass's work items -- `items` per group; a plain pass is one group of p.nqb * p.nseg -- group by group: each
// in one launch, or (p.cohort > 0: knn_plan_compute) in synchronised rounds of p.cohort workgroups dealt round-robin to
// at most max_queues queues -- the caller's stream and ctx->aux_stream[] -- so that the workgroups of a later launch
// take the slots the stragglers of an earlier one have freed (one queue: every launch ends with its slowest workgroup
// while the rest of the chip idles).  The launches are round_schedule's (knn_plan.inc); a single one stays on the
// caller's stream.  launch(stream, workgroups, first item, group) queues one.  Timed as one `kind` span over all launches
// when they overlap on several queues (their own spans would count the same time twice), else a span per launch
// (span_each) or one around them all.
//
// Work of a group alone (`trigger` != FDR_TAIL_TRIGGER_NONE; the live-chunk pass's merge and re-rank): early(stream,
// group) queues it on ONE further stream, ctx->aux_stream[2], at the group's ready point (round_ready_points) -- behind
// an event on every queue, i.e. behind that queue's last launch of the group -- and r.early[group] says so; the caller
// runs what is left behind the join.  The span of the pass ends at the join of the pass's queues; the further stream
// joins behind it.  Only with at most two queues for the pass: three streams in all.
struct Rounds {
    int launches = 0, queues = 0;
    std::vector<char> early;  // [group]: its own work was queued in front of the join
};
template <class Launch, class Early>
static int launch_rounds(fdr_ctx *ctx, const KnnPlan &p, const std::vector<long long> &items, int max_queues, int kind,
                         bool span_each, hipStream_t st, Rounds &r, Launch launch, int trigger, Early early) {
    const int dealt = p.cohort > 0 ? std::max(1, std::min(p.queues, max_queues)) : 1;
    const std::vector<RoundLaunch> sched = round_schedule(items, p.cohort > 0 ? p.cohort : 0, dealt);
    const int nqueues = sched.size() > 1 ? dealt : 1;
    const std::vector<int> ready = round_ready_points(sched, items.size(), nqueues, nqueues <= 2 ? trigger : FDR_TAIL_TRIGGER_NONE);
    const bool tail = std::any_of(ready.begin(), ready.end(), [](int at) { return at >= 0; });
    r.early.assign(items.size(), 0);
    hipStream_t qs[4] = {st, st, st, st};
    if (nqueues > 1 || tail) {
        if (!ctx->aux_ev[0]) {
            for (hipStream_t &a : ctx->aux_stream) HIP_TRY(hipStreamCreateWithFlags(&a, hipStreamNonBlocking));
            for (hipEvent_t &e : ctx->aux_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        for (int q = 1; q < nqueues; ++q) qs[q] = ctx->aux_stream[q - 1];
    }
    const hipStream_t ts = ctx->aux_stream[2];  // (the pass's own queues: the caller's and aux_stream[0])
    const bool one_span = nqueues > 1 || !span_each;
    int trc;
    if (one_span && (trc = timing_begin(ctx, kind, st))) return trc;
    if (nqueues > 1) {  // what `st` has queued so far is visible to the other queues' launches
        HIP_TRY(hipEventRecord(ctx->aux_ev[0], st));
        for (int q = 1; q < nqueues; ++q) HIP_TRY(hipStreamWaitEvent(qs[q], ctx->aux_ev[0], 0));
    }
    size_t ev_used = 0;
    for (size_t i = 0; i < sched.size(); ++i) {
        const RoundLaunch &l = sched[i];
        bool waited = false;
        for (size_t g = 0; tail && g < ready.size(); ++g) {
            if (ready[g] != (int)i) continue;
            for (int q = 0; q < nqueues && !waited; ++q) {  // behind what every queue has been given so far
                if (ev_used == ctx->tail_ev.size()) {
                    hipEvent_t e;
                    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    ctx->tail_ev.push_back(e);
                }
                HIP_TRY(hipEventRecord(ctx->tail_ev[ev_used], qs[q]));
                HIP_TRY(hipStreamWaitEvent(ts, ctx->tail_ev[ev_used++], 0));
            }
            waited = true;
            if ((trc = early(ts, (int)g))) return trc;
            r.early[g] = 1;
        }
        const hipStream_t ls = qs[l.queue];
        if (!one_span && (trc = timing_begin(ctx, kind, ls))) return trc;
        launch(ls, (unsigned)l.grid, l.base, l.group);
        if (!one_span && (trc = timing_end(ctx, kind, ls))) return trc;
    }
    HIP_TRY(hipGetLastError());
    r.launches = (int)sched.size();
    r.queues = nqueues;
    for (int q = 1; q < nqueues; ++q) {  // `st` waits for everything the other queues have been given
        HIP_TRY(hipEventRecord(ctx->aux_ev[q], qs[q]));
        HIP_TRY(hipStreamWaitEvent(st, ctx->aux_ev[q], 0));
    }
    if (one_span && (trc = timing_end(ctx, kind, st))) return trc;
    if (ev_used > 0) {  // ... and, behind the pass's span, for the groups' early work
        HIP_TRY(hipEventRecord(ctx->aux_ev[3], ts));
        HIP_TRY(hipStreamWaitEvent(st, ctx->aux_ev[3], 0));
    }
    return FDR_OK;
}
template <class Launch>
static int launch_rounds(fdr_ctx *ctx, const KnnPlan &p, const std::vector<long long> &items, int max_queues, int kind,
                         bool span_each, hipStream_t st, Rounds &r, Launch launch) {
    return launch_rounds(ctx, p, items, max_queues, kind, span_each, st, r, launch, FDR_TAIL_TRIGGER_NONE,
                         [](hipStream_t, int) { return FDR_OK; });
}

// The argument checks of a k-NN call, before anything is routed or recorded.  (The workspace's SIZE is checked by the
// path that lays it out.)  Returns FDR_OK for nq == 0 whatever the pointers: the callers launch nothing then.
static int check_knn_args(fdr_ctx *, const KnnArgs &a) {
    const int dp = fdr_padded_dim(a.d);
    if (dp < 0) return fail(FDR_E_ARG, "knn: dimension %d unsupported (1..%d)", a.d, FDR_MAX_DIM);
    if (a.k < 1 || a.k > FDR_MAX_K) return fail(FDR_E_ARG, "knn: k=%d, d=%d outside the MFMA kernels' shapes", a.k, a.d);
    if (a.nq < 0 || a.nt < a.k) return fail(FDR_E_ARG, "knn: need n_targets (%lld) >= k (%d)", (long long)a.nt, a.k);
    if (a.nt + a.t_base > 0x7fffffffll || a.nq > 0x7fffffffll) return fail(FDR_E_ARG, "knn: row numbers exceed int32");
    if (a.nq == 0) return FDR_OK;
    const bool need_ws = knn_route(dp, a.k, a.nt) != FDR_ROUTE_GENERIC;  // (the generic kernel needs no scratch)
    if (!a.Qhat || !a.qzero || !a.That || !a.tzero || !a.idx || !a.dist || (need_ws && !a.ws))
        return fail(FDR_E_ARG, "knn: null device pointer");
    return FDR_OK;
}
static_assert(FDR_MAX_K == FDR_EXACT_MAX_K, "every k the generic kernel takes, the exact MFMA pass takes from 8192 targets");

static int launch_knn_exact(fdr_ctx *ctx, const KnnArgs &a) {
    if (a.nq == 0) return FDR_OK;  // (an empty call is recorded as an exact one and launches nothing)
    const hipStream_t st = a.st;
    const int k = a.k;
    const KnnPlan p = knn_plan(ctx->num_cus, a.nq, a.nt, a.d, k);
    if (a.ws_bytes < p.total_bytes) return fail(FDR_E_ARG, "knn: workspace %zu < required %zu bytes", a.ws_bytes, p.total_bytes);
    const TileKernel kern = KnnKernels::tile[p.shape];
    if (!kern) return no_kernel(p.shape);
    const PlanRegions R = plan_regions(a.ws, p);
    hipLaunchKernelGGL(pack_zero_bits_kernel, dim3((unsigned)((a.nt + 255) / 256)), dim3(256), 0, st,
                       a.tzero, (int)a.nt, R.bits, R.shared, p.nq_pad);
    HIP_TRY(hipGetLastError());
    const KnnShape &sh = kShapes[p.shape];
    const size_t lds = knn_lds_bytes(sh, k);
    if (lds > 160 * 1024) return fail(FDR_E_ARG, "knn: k=%d, d=%d needs %zu B of LDS (> 160 KiB)", k, a.d, lds);
    ctx->last.trace.exact_calls++;
    ctx->last.trace.exact_queries += (int32_t)a.nq;
    ctx->last.trace.exact_waves = sh.nw;
    ctx->last.trace.exact_qsets = sh.nq;
    ctx->last.trace.exact_segments = p.nseg;
    [[maybe_unused]] const int dbg = dev_knobs().debug;  // (development builds only; 0 in the release library)
    const int qcap = knn_qcap(sh, k);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    Rounds r;  // (rounds on at most two queues, like the prefilter pass)
    int trc = launch_rounds(ctx, p, {(long long)p.nqb * p.nseg}, 2, FDR_KERNEL_KNN_TILE, false, st, r,
                            [&](hipStream_t s, unsigned grid, int base, int) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * sh.nw), lds, s, a.Qhat, a.qzero, (int)a.nq, a.That, R.bits, (int)a.nt,
                           (int)a.t_base, p.segs, k, p.nq_pad, R.partial, R.shared, qcap, base, p.nqb FDR_DBG_ARG(dbg));
    });
    if (trc) return trc;
    if ((trc = dump_debug_counters(st, "tile", p, "update calls, rounds, flushes, flush iterations, rescans, -"))) return trc;
    if ((trc = timing_begin(ctx, FDR_KERNEL_KNN_MERGE, st))) return trc;
    hipLaunchKernelGGL(k <= FDR_FAST_MAX_K ? knn_merge_kernel : knn_merge_wide_kernel, dim3((unsigned)((a.nq + 3) / 4)),
                       dim3(256), 0, st, (const u64 *)R.partial, p.nseg, (int)a.nq, p.nq_pad, k, a.idx, a.dist);
    HIP_TRY(hipGetLastError());
    return timing_end(ctx, FDR_KERNEL_KNN_MERGE, st);
}

// ---- prefilter mode: fp16 pass -> certificate + exact re-rank -> exact pass for the rest -------
struct PrefilterCounts { int exact, zero, range; };  // queries left to the exact pass / all-zero / left to the range pass
// What the stages of one call share.
struct PrefilterCall {
    fdr_ctx *ctx;
    KnnArgs a;
    bool self;  // the queries ARE the targets (row i of one is row i of the other): one fp16 copy serves both sides
    int dp;
    PrefilterWs L;
    int shape;  // of the candidate pass (kShapes), its plan, its kernel, the plan's regions in L.knn
    KnnPlan p;
    PassKernel kern;
    PlanRegions R;
    int ib;                      // index bits of the pass's keys
    const _Float16 *p1_q, *p1_t;  // what the candidate pass streams: the fp16 copies, or the ordered ones with
    OrderArgs ord;                // ... their order tables
    const KnnShape &sh() const { return kShapes[shape]; }
    size_t lds() const { return knn_lds_bytes(sh(), L.kp); }
    _Float16 *hq() const { return self ? L.ht : L.hq; }  // the queries' fp16 copy
    // the stages, in the order launch_knn_prefilter runs them (a call takes one of the two passes)
    int setup(), pass_dense(Rounds &r), pass_live(Rounds &r);
    int certify(PrefilterCounts &n), range(PrefilterCounts &n), exact_rest(const PrefilterCounts &n);
    // The queries certify() still has to merge and re-rank behind the join: all of them (one entry, perm == null), or
    // the groups of the live-chunk pass whose work was not queued under the pass (pass_live).
    std::vector<QuerySel> late;
    QuerySel all_queries() const { return QuerySel{nullptr, nullptr, (int)a.nq, (int)a.nq}; }
    int launch_merge(hipStream_t s, const QuerySel &sel), launch_rerank(hipStream_t s, const QuerySel &sel);
};

// What AUTO makes of fdr_set_pass_tail: each part is on only if it cleared the parent's run-to-run range on its own
// (docs/experiments.md A-36).  The descending order did (0.92 ms a step against a range of 0.56); the early merge +
// re-rank gained 0.33 ms more in six of six paired runs, which is inside that range: measured, kept behind
// FDR_TAIL_EARLY, off in AUTO.
#ifndef FDR_TAIL_AUTO_MODE
#define FDR_TAIL_AUTO_MODE FDR_TAIL_ORDER
#endif
static int pass_tail_mode(const fdr_ctx *ctx) { return ctx->tail_mode == FDR_TAIL_AUTO ? FDR_TAIL_AUTO_MODE : ctx->tail_mode; }

// Conversion and set-up, timed as "rerank": fp16 copies, zero bits, ordered and blocked copies, the keys' index bits.
int PrefilterCall::setup() {
    const hipStream_t st = a.st;
    const int64_t nq = a.nq, nt = a.nt;
    int trc = timing_begin(ctx, FDR_KERNEL_KNN_RERANK, st);
    if (trc) return trc;
    HIP_TRY(hipMemsetAsync(L.counter, 0, 64, st));  // certify()'s counters [0 .. 2] and the records' long-row count [8]
    if (L.rc) {  // (d <= 128: the compact records of the re-rank come out of the same pass over the rows)
        hipLaunchKernelGGL(to_half_compact_kernel, dim3((unsigned)((nt * (dp / 8) + 255) / 256)), dim3(256), 0, st, a.That,
                           (long long)nt * (dp / 8), L.ht, L.rc, L.counter + 8);
    } else
        hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)((nt * (dp / 8) + 255) / 256)), dim3(256), 0, st, a.That,
                           (long long)nt * (dp / 8), L.ht);
    if (!self)
        hipLaunchKernelGGL(to_half_kernel, dim3((unsigned)((nq * (dp / 8) + 255) / 256)), dim3(256), 0, st, a.Qhat,
                           (long long)nq * (dp / 8), L.hq);
    hipLaunchKernelGGL(pack_zero_bits_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st,
                       a.tzero, (int)nt, R.bits, R.shared, p.nq_pad);
    HIP_TRY(hipGetLastError());
    ord = {nullptr, nullptr};
    p1_q = hq();
    p1_t = L.ht;
    if (L.ordered) {  // knn_order.inc: rows by chunk mask, fp16 copies in that order
        _Float16 *const ho_t = L.ho_t, *const ho_q = self ? L.ho_t : L.ho_q;
        auto order = [&](const float *X, int64_t n, int *perm, _Float16 *out) -> int {
            hipLaunchKernelGGL(row_chunk_keys_kernel, dim3((unsigned)(((size_t)n * 16 + 255) / 256)), dim3(256), 0, st, X,
                               (int)n, dp, L.okeys, L.ovals);
            size_t tb = L.otmp_bytes;
            HIP_TRY(rocprim::radix_sort_pairs(L.otmp, tb, L.okeys, L.okeys_s, L.ovals, perm, (size_t)n, 0, 40, st));
            const long long groups = (long long)n * (dp / 8);
            hipLaunchKernelGGL(to_half_ordered_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st, X,
                               (const int *)perm, groups, dp / 8, out);
            HIP_TRY(hipGetLastError());
            return FDR_OK;
        };
        int orc;
        if ((orc = order(a.That, nt, L.perm_t, ho_t))) return orc;
        if (L.live) {  // the stages' masks, while the sorted keys are the targets'; the lists a block of each mask value walks
            int max_stages = 1;
            for (int i = 0; i < p.nseg; ++i)
                max_stages = std::max(max_stages, (std::min<int>((int)nt, p.segs.b[i + 1]) - p.segs.b[i] + 127) >> 7);
            hipLaunchKernelGGL(live_stage_masks_kernel, dim3((unsigned)max_stages, (unsigned)p.nseg), dim3(64), 0, st,
                               (const u64 *)L.okeys_s, (int)nt, p.segs, L.live_smask);
            const int all = !(FDR_SKIP_AUTO_ON && ctx->skip_mode == FDR_SKIP_AUTO);
            hipLaunchKernelGGL(live_stage_lists_kernel, dim3(256, (unsigned)p.nseg), dim3(64), 0, st,
                               (const uint8_t *)L.live_smask, (int)nt, p.segs, all, L.live_lists, L.live_lens);
            HIP_TRY(hipGetLastError());
            ctx->last.trace.skip_live = !all;
        }
        if (!self && (orc = order(a.Qhat, nq, L.perm_q, ho_q))) return orc;
        ord.perm_t = L.perm_t;
        p1_t = ho_t;
        ord.perm_q = self ? L.perm_t : L.perm_q;
        p1_q = ho_q;
        if (L.live) {  // the targets once more in blocks of (tile, chunk); the query blocks' masks (the sorted keys are the queries')
            const long long bgroups = (long long)((nt + 31) / 32 + 4) * 32 * 16;
            hipLaunchKernelGGL(to_half_blocked_kernel, dim3((unsigned)((bgroups + 255) / 256)), dim3(256), 0, st, a.That,
                               (const int *)L.perm_t, (int)nt, bgroups, L.hb_t);
            hipLaunchKernelGGL(live_block_masks_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(64), 0, st,
                               (const u64 *)L.okeys_s, (int)nq, L.live_masks);
            HIP_TRY(hipGetLastError());
        }
    }
    int max_seg = 1;
    for (int i = 0; i < p.nseg; ++i) max_seg = std::max(max_seg, p.segs.b[i + 1] - p.segs.b[i]);
    ib = prefilter_index_bits(max_seg);
    if (ib > FDR_PREFILTER_MAX_IB) return fail(FDR_E_ARG, "knn prefilter: segment of %d rows", max_seg);
    if ((trc = timing_end(ctx, FDR_KERNEL_KNN_RERANK, st))) return trc;
    if (lds() > 32768)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds()));
    return FDR_OK;
}

// The dense candidate pass: rounds on up to four queues (one queue: every launch its own timed span).
int PrefilterCall::pass_dense(Rounds &r) {
    late.assign(1, all_queries());
    return launch_rounds(ctx, p, {(long long)p.nqb * p.nseg}, 4, FDR_KERNEL_KNN_PREFILTER, true, a.st, r,
                         [&](hipStream_t s, unsigned grid, int base, int) {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * sh().nw), lds(), s, p1_q, (int)a.nq, p1_t, (int)a.nt, (int)a.t_base,
                           p.segs, L.kp, p.nq_pad, R.partial, R.shared, ib, base, p.nqb, ord FDR_DBG_ARG(dev_knobs().debug));
    });
}

// The live-chunk candidate pass: the blocks' masks come back (nqb words, one synchronisation), live_plan groups the
// blocks by live chunks, and every group runs in synchronised rounds of its own, segment-major -- the NL groups on their
// knn_prefilter_live_kernel<NL>, ascending, then the dense group on kern -- as ONE timed span.  The shipped kernel
// takes a block RANGE and the dense blocks lie scattered over the order (wherever 256 rows straddle two masks), so their
// queries, order-table entries and bound words are gathered side by side first (live_gather_dense_kernel); one launch
// per contiguous run instead cost a whole scan's time per stray block: 147 ms a step at 1 M reads.
int PrefilterCall::pass_live(Rounds &r) {
    const hipStream_t st = a.st;
    const int nqb = p.nqb, kp = L.kp;
    fdr_knn_trace &tr = ctx->last.trace;
    std::vector<unsigned> &masks = ctx->live_host;
    masks.resize((size_t)nqb);
    HIP_TRY(hipMemcpyAsync(masks.data(), L.live_masks, (size_t)nqb * 4, hipMemcpyDeviceToHost, st));
    std::vector<int> &lens = ctx->skip_host;  // (the same synchronisation brings the stage lists' lengths)
    lens.resize((size_t)p.nseg * 256);
    HIP_TRY(hipMemcpyAsync(lens.data(), L.live_lens, (size_t)p.nseg * 256 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (ctx->cap.what & FDR_CAPTURE_LIVE_LISTS) {  // (test support: fdr_last_live_stage_lists)
        const size_t entries = live_stage_rows(a.nt) * 256;
        int crc = ctx->cap.lists.reserve(entries);
        if (crc) return crc;
        HIP_TRY(ctx->cap.keep(ctx->cap.lists, 0, L.live_lists, entries, st));
        ctx->cap.skip = {p.nseg, (int)a.nt, p.segs, st};
    }
    const LivePlan lp = live_plan(masks.data(), nqb, p.nseg, ctx->live_mode == FDR_LIVE_FORCE ? 0 : p.cohort);
    HIP_TRY(hipMemcpyAsync(L.live_ids, lp.ids.data(), (size_t)nqb * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(L.live_order, lp.order.data(), (size_t)nqb * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // (pageable sources that end with this function)
    tr.pass_live = 1;
    // The groups in issue order (fdr_set_pass_tail): the parent's ascending NL, or the dense group first and the
    // cheapest items last; with the early re-rank, every group but the last is merged and re-ranked under the pass.
    const int tail = pass_tail_mode(ctx);
    const std::vector<int> issue = live_issue_order(lp, tail != FDR_TAIL_OFF);
    const int trigger = tail == FDR_TAIL_EARLY ? FDR_TAIL_TRIGGER_LAST : tail == FDR_TAIL_EARLY_GROUP ? FDR_TAIL_TRIGGER_GROUP
                                                                                                    : FDR_TAIL_TRIGGER_NONE;
    int dense_nq = 0;  // queries of the gathered dense group
    std::vector<long long> items;
    std::vector<QuerySel> sels;    // [issued group]: its queries, for the merge and the re-rank
    std::vector<int> sel_queries;  // ... and their number
    for (size_t gi = 0; gi < issue.size(); ++gi) {
        const LiveGroup &g = lp.groups[(size_t)issue[gi]];
        tr.pass_group_order |= g.nl << (4 * (int)gi);
        items.push_back((long long)g.count * p.nseg);
        const int last_block = lp.order[(size_t)(g.first + g.count - 1)];  // (ascending: only the last one can be short)
        sel_queries.push_back((g.count - 1) * 256 + (int)std::min<int64_t>(256, a.nq - (int64_t)last_block * 256));
        if (g.nl != FDR_LIVE_DENSE) {
            sels.push_back(QuerySel{L.live_order + g.first, ord.perm_q, g.count * 256, (int)a.nq});
            tr.pass_live_items[g.nl - FDR_LIVE_MIN_NL] = g.count * p.nseg;
            for (int sg = 0; sg < p.nseg; ++sg) {  // the stages its work items walk, of those the segments hold
                const int len = std::min<int>((int)a.nt, p.segs.b[sg + 1]) - p.segs.b[sg];
                const int64_t nst = len > 0 ? (len + 127) >> 7 : 0;
                int64_t walked = 0;
                for (int i = 0; i < g.count; ++i)
                    walked += std::min<int64_t>(nst, lens[(size_t)sg * 256 + (masks[(size_t)lp.order[(size_t)(g.first + i)]] & 0xffu)]);
                tr.skip_stages_walked += walked;
                tr.skip_stages_skipped += nst * g.count - walked;
            }
            continue;
        }
        tr.pass_live_dense_items = g.count * p.nseg;
        dense_nq = sel_queries.back();
        sels.push_back(QuerySel{nullptr, L.live_perm, dense_nq, dense_nq});
        hipLaunchKernelGGL(live_gather_dense_kernel, dim3((unsigned)g.count), dim3(256), 0, st, p1_q, ord.perm_q,
                           (const unsigned *)R.shared, (int)a.nq, (const int *)(L.live_order + g.first), L.live_hq,
                           L.live_perm, L.live_tau);
    }
    for (int nl = FDR_LIVE_MIN_NL; nl <= FDR_LIVE_MAX_NL; ++nl)
        if (live_lds_bytes(nl) > 32768)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kLiveKernels[nl - FDR_LIVE_MIN_NL]),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)live_lds_bytes(nl)));
    const int rc = launch_rounds(ctx, p, items, 4, FDR_KERNEL_KNN_PREFILTER, false, st, r,
                         [&](hipStream_t s, unsigned grid, int base, int group) {
        const LiveGroup &g = lp.groups[(size_t)issue[(size_t)group]];
        if (g.nl == FDR_LIVE_DENSE)
            hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * sh().nw), lds(), s, (const _Float16 *)L.live_hq, dense_nq, p1_t,
                               (int)a.nt, (int)a.t_base, p.segs, kp, p.nq_pad, R.partial, L.live_tau, ib, base, g.count,
                               OrderArgs{ord.perm_t, (const int *)L.live_perm} FDR_DBG_ARG(dev_knobs().debug));
        else
            hipLaunchKernelGGL(kLiveKernels[g.nl - FDR_LIVE_MIN_NL], dim3(grid), dim3(512), live_lds_bytes(g.nl), s,
                               p1_q, (int)a.nq, (const _Float16 *)L.hb_t, (int)a.nt, (int)a.t_base, p.segs, kp, p.nq_pad,
                               R.partial, R.shared, ib, base, g.count, (const int *)(L.live_order + g.first),
                               (const unsigned *)L.live_ids, ord, (const unsigned *)L.live_masks,
                               reinterpret_cast<const unsigned *>(L.live_lists), (const int *)L.live_lens);
    }, trigger, [&](hipStream_t s, int group) {  // a complete group: its queries' lists are final (a span of its own)
        int erc = timing_begin(ctx, FDR_KERNEL_KNN_RERANK, s);
        if (erc || (erc = launch_merge(s, sels[(size_t)group])) || (erc = launch_rerank(s, sels[(size_t)group]))) return erc;
        tr.rerank_early_queries += sel_queries[(size_t)group];
        return timing_end(ctx, FDR_KERNEL_KNN_RERANK, s);
    });
    if (rc) return rc;
    if (trigger == FDR_TAIL_TRIGGER_NONE) {  // (one merge and one re-rank for everybody, as without the switch)
        late.assign(1, all_queries());
        return FDR_OK;
    }
    late.clear();
    for (size_t i = 0; i < sels.size(); ++i)
        if (!r.early[i]) late.push_back(sels[i]);
    return FDR_OK;
}

// The key merge of the queries `sel` on `s`: their segment lists -> L.cand.
int PrefilterCall::launch_merge(hipStream_t s, const QuerySel &sel) {
    const int64_t mq = p.nseg * L.kp <= 64 ? 4 * MERGE_QPW : 4;  // queries per workgroup of knn_merge_keys_kernel
    hipLaunchKernelGGL(knn_merge_keys_kernel, dim3((unsigned)((sel.n + mq - 1) / mq)), dim3(256), 0, s,
                       (const u64 *)R.partial, p.nseg, sel, p.nq_pad, L.kp, L.cand);
    HIP_TRY(hipGetLastError());
    return FDR_OK;
}

// Certificate + exact re-rank of the queries `sel` on `s`.  Every launch of a call appends to the same exact, zero and
// range lists through the same counters (cleared once, in setup()).
int PrefilterCall::launch_rerank(hipStream_t s, const QuerySel &sel) {
    const float margin = 2.0f * prefilter_eps(ib) + 4.0e-7f;
    // Beside the records the kernel's dense batches are short (the instance of RERANK_ROWS_COMPACT rows).  Whether the
    // records are read is the kernel's own decision, from the long-row count their build left in counter[8] (knn_workspace.inc:
    // RC_LONG_SHARE): no read-back in front of this launch.
    const auto rerank = L.rc ? knn_rerank_kernel<RERANK_ROWS_COMPACT> : knn_rerank_kernel<RERANK_ROWS_DENSE>;
    const int rerank_lds = L.rc ? RERANK_LDS_BYTES(RERANK_ROWS_COMPACT) : RERANK_LDS_BYTES(RERANK_ROWS_DENSE);
    const int long_limit = ctx->compact_mode == FDR_COMPACT_FORCE ? 0x7fffffff : (int)(a.nt / RC_LONG_SHARE);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(rerank), hipFuncAttributeMaxDynamicSharedMemorySize, rerank_lds));
    hipLaunchKernelGGL(rerank, dim3((unsigned)((sel.n + 3) / 4)), dim3(256), rerank_lds, s,
                       (const u64 *)L.cand, L.kp, a.k, a.Qhat, a.qzero, a.That, (int)a.nq, dp, (int)a.t_base, margin,
                       a.idx, a.dist, L.counter, L.flagged, L.rlist, L.theta, L.path, (const unsigned char *)L.rc, long_limit, sel);
    HIP_TRY(hipGetLastError());
    return FDR_OK;
}

// Key merge and capture, certificate + exact re-rank -- of the queries that are still `late` --, zero answers; the
// 12-byte read-back that sizes the passes below.
int PrefilterCall::certify(PrefilterCounts &n) {
    const hipStream_t st = a.st;
    const int kp = L.kp, k = a.k;
    const int64_t nq = a.nq;
    int trc;
    if ((trc = timing_begin(ctx, FDR_KERNEL_KNN_RERANK, st))) return trc;
    for (const QuerySel &sel : late)
        if ((trc = launch_merge(st, sel))) return trc;
    if (ctx->cap.what & FDR_CAPTURE_CANDIDATES) {  // (test support: fdr_last_candidates)
        if ((trc = ctx->cap.cand.reserve((size_t)nq * kp))) return trc;
        HIP_TRY(ctx->cap.keep(ctx->cap.cand, 0, L.cand, (size_t)nq * kp, st));
        ctx->cap.nq = nq;
        ctx->cap.kp = kp;
        ctx->cap.qbits = std::min(20, 32 - ib);
        ctx->cap.stream = st;
        ctx->cap.cand_valid = true;
    }
    for (const QuerySel &sel : late)
        if ((trc = launch_rerank(st, sel))) return trc;
    // all-zero queries share one closed-form answer (their number is only known on the device yet)
    hipLaunchKernelGGL(zero_answer_kernel, dim3(1), dim3(1024), 0, st, (const unsigned *)R.bits, (int)a.nt,
                       (int)a.t_base, k, L.zidx, L.zdist);
    hipLaunchKernelGGL(scatter_zero_answer_kernel, dim3((unsigned)(((int64_t)nq * k + 255) / 256)),
                       dim3(256), 0, st, (const int *)L.zidx, (const float *)L.zdist,
                       (const int *)L.flagged, (int)nq, (const int *)L.counter, k, a.idx, a.dist);
    HIP_TRY(hipGetLastError());
    if ((trc = timing_end(ctx, FDR_KERNEL_KNN_RERANK, st))) return trc;
    int counts[9] = {};  // how many queries could not be certified / are all-zero / need a range pass?  [8]: long rows
    HIP_TRY(hipMemcpyAsync(counts, L.counter, sizeof counts, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    n = {counts[0], counts[1], counts[2]};
    const int long_limit = ctx->compact_mode == FDR_COMPACT_FORCE ? 0x7fffffff : (int)(a.nt / RC_LONG_SHARE);  // (launch_rerank)
    ctx->last.trace.rerank_compact = L.rc && counts[8] <= long_limit;  // (the kernel's own test)
    ctx->last.trace.rerank_compact_entries = L.rc ? RC_ENTRIES : 0;
    ctx->last.trace.rerank_compact_long = counts[8];
    ctx->last.pass.flagged = n.exact + n.range;
    ctx->last.trace.uncertified = n.exact;
    ctx->last.trace.zero_queries = n.zero;
    ctx->last.trace.range_queries = n.range;
    return FDR_OK;
}

// Plateau queries: collect {d~ <= theta} with a second fp16 pass, rank it exactly.  Ranges that overflow are appended
// to the exact list: n.exact becomes its final length.
int PrefilterCall::range(PrefilterCounts &n) {
    const hipStream_t st = a.st;
    const int rcount = n.range;
    fdr_knn_trace &tr = ctx->last.trace;
    int trc;
    if ((trc = timing_begin(ctx, FDR_KERNEL_KNN_RERANK, st))) return trc;
    const bool rcap = ctx->cap.what & FDR_CAPTURE_RANGE;  // (test support: fdr_last_range_sets)
    if (rcap) {
        if ((trc = ctx->cap.rq.reserve((size_t)rcount)) || (trc = ctx->cap.rtheta.reserve((size_t)rcount)) ||
            (trc = ctx->cap.rcnt.reserve((size_t)rcount)) || (trc = ctx->cap.rrows.reserve((size_t)rcount * RANGE_CAP)))
            return trc;
        ctx->cap.stream = st;
    }
    for (int first = 0; first < rcount; first += L.rchunk) {
        const int cq = std::min(L.rchunk, rcount - first);
        hipLaunchKernelGGL(gather_half_queries_kernel, dim3((unsigned)cq), dim3(256), 0, st, (const _Float16 *)hq(),
                           (const float *)L.theta, (const int *)L.rlist, first, cq, dp, L.hqc, L.thetac, L.cnt);
        HIP_TRY(hipGetLastError());
        const int rs = range_shape(dp, cq, rcount);
        const KnnShape &rsh = kShapes[rs];
        const RangeKernel rk = KnnKernels::range[rs];
        if (!rk) return no_kernel(rs);
        const KnnPlan rp = knn_plan(ctx->num_cus, cq, a.nt, a.d, 1, rs);  // (k = 1: ring-only LDS)
        const size_t rlds = knn_lds_bytes(rsh, 1) + (size_t)RANGE_LANE_BUF * 64 * rsh.nw * 4;  // ring + lane buffers
        if (rsh.family == FDR_FAM_RANGE_PP)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(rk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds));
        hipLaunchKernelGGL(rk, dim3((unsigned)rp.nqb, (unsigned)rp.nseg), dim3(64 * rsh.nw), rlds, st, (const _Float16 *)L.hqc,
                           (const float *)L.thetac, cq, (const _Float16 *)L.ht, (int)a.nt, (int)a.t_base, rp.segs, RangeOut{L.cnt, L.rcand});
        HIP_TRY(hipGetLastError());
        tr.range_chunks++;
        tr.range_pp_chunks += rsh.family == FDR_FAM_RANGE_PP;
        tr.range_w8_chunks += rs == FDR_R128_W8;
        if (rcap) {  // this chunk's rows, behind the earlier ones
            const KnnCapture &c = ctx->cap;
            HIP_TRY(c.keep(c.rq, first, L.rlist + first, cq, st));
            HIP_TRY(c.keep(c.rtheta, first, L.thetac, cq, st));
            HIP_TRY(c.keep(c.rcnt, first, L.cnt, cq, st));
            HIP_TRY(c.keep(c.rrows, (size_t)first * RANGE_CAP, L.rcand, (size_t)cq * RANGE_CAP, st));
        }
        hipLaunchKernelGGL(knn_rerank_long_kernel, dim3((unsigned)((cq + 3) / 4)), dim3(256), 0, st,
                           (const int *)(L.rlist + first), cq, (const int *)L.cnt, (const int *)L.rcand, a.k,
                           a.Qhat, a.That, dp, (int)a.t_base, a.idx, a.dist, L.counter, L.flagged, L.path);
        HIP_TRY(hipGetLastError());
    }
    if (rcap) {
        ctx->cap.n_range = rcount;
        ctx->cap.range_valid = true;
    }
    if ((trc = timing_end(ctx, FDR_KERNEL_KNN_RERANK, st))) return trc;
    int count = 0;
    HIP_TRY(hipMemcpyAsync(&count, L.counter, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tr.range_overflow = count - n.exact;
    n.exact = count;
    return FDR_OK;
}

// The exact pass for the exact list's n.exact queries, gathered in chunks -- or for everyone -- in L.knn's regions.
int PrefilterCall::exact_rest(const PrefilterCounts &n) {
    const hipStream_t st = a.st;
    KnnArgs e = a;
    e.ws_bytes = L.knn_bytes;
    if ((int64_t)n.exact * 2 > a.nq - n.zero) {
        ctx->last.trace.exact_fallback = FDR_FALLBACK_WHOLE;
        // every row, the all-zero ones too, is recomputed by the exact kernel: its code, as in exact mode
        // (the trace stays a prefilter trace, and the pass's launches and uncertified count stand)
        ctx->last.paths = {nullptr, a.nq, FDR_PATH_EXACT, nullptr};
        return launch_knn_exact(ctx, e);
    }
    ctx->last.trace.exact_fallback = FDR_FALLBACK_CHUNKED;
    e.Qhat = L.qc;
    e.qzero = L.qzc;
    e.idx = L.idxc;
    e.dist = L.distc;
    for (int first = 0; first < n.exact; first += L.chunk) {
        const int cq = std::min(L.chunk, n.exact - first);
        hipLaunchKernelGGL(gather_queries_kernel, dim3((unsigned)cq), dim3(256), 0, st, a.Qhat, a.qzero,
                           (const int *)L.flagged, first, cq, dp, L.qc, L.qzc);
        HIP_TRY(hipGetLastError());
        e.nq = cq;
        int rc = launch_knn_exact(ctx, e);
        if (rc) return rc;
        hipLaunchKernelGGL(scatter_results_kernel, dim3((unsigned)(((int64_t)cq * a.k + 255) / 256)), dim3(256), 0, st,
                           (const int *)L.idxc, (const float *)L.distc, (const int *)L.flagged, first, cq, a.k, a.idx, a.dist);
        HIP_TRY(hipGetLastError());
    }
    return FDR_OK;
}

static int launch_knn_prefilter(fdr_ctx *ctx, const KnnArgs &a) {
    PrefilterCall c = {ctx, a};
    c.self = a.Qhat == a.That && a.qzero == a.tzero && a.nq == a.nt;
    c.dp = fdr_padded_dim(a.d);
    c.L = prefilter_ws(ws_env(ctx), a.ws, a.nq, a.nt, a.d, a.k);
    if (a.ws_bytes < c.L.total) return fail(FDR_E_ARG, "knn: workspace %zu < required %zu bytes", a.ws_bytes, c.L.total);
    const int kp = c.L.kp;
    knn_call_header(ctx, FDR_TRACE_PREFILTER, c.dp, a.k, a.nq, a.nt);
    ctx->last.paths = {c.L.path, a.nq, FDR_PATH_NONE, a.st};  // (per query: the re-rank kernels write the codes)

    c.shape = prefilter_shape_live(ctx->live_mode, c.dp, kp, a.nq, ctx->num_cus, a.nt);
    c.p = knn_plan(ctx->num_cus, a.nq, a.nt, a.d, kp, c.shape);
    fdr_knn_trace &tr = ctx->last.trace;
    tr.kp = kp;
    tr.pass_waves = c.sh().nw;
    tr.pass_wps = c.sh().wps;
    tr.pass_units = c.sh().tps;
    tr.pass_list_keys = kp <= 32 ? 16 : 32;
    tr.pass_pingpong = c.sh().family == FDR_FAM_PINGPONG;
    tr.pass_segments = c.p.nseg;
    c.kern = KnnKernels::pass[c.shape][kp > 32];
    if (!c.kern) return no_kernel(c.shape);
    c.R = plan_regions(c.L.knn, c.p);
    int rc;
    if ((rc = c.setup())) return rc;
    Rounds r;
    rc = c.L.live ? c.pass_live(r) : c.pass_dense(r);
    ctx->last.pass.launches = r.launches;
    ctx->last.pass.queues = r.queues;
    tr.pass_launches = r.launches;
    tr.pass_queues = r.queues;
    if (rc) return rc;
#ifdef FDR_STAMPS
    if ((rc = dump_stamps(a.st, c.sh().nw))) return rc;
#endif
    if ((rc = dump_debug_counters(a.st, "prefilter", c.p, "wave-tiles, cold, groups, rounds, second rounds, candidates"))) return rc;
    PrefilterCounts n;
    if ((rc = c.certify(n))) return rc;
    if (n.range > 0 && (rc = c.range(n))) return rc;
    if (n.exact <= 0) return FDR_OK;
    return c.exact_rest(n);
}

static int launch_knn_mode(fdr_ctx *ctx, const KnnArgs &a) {
    const int dp = fdr_padded_dim(a.d);
    if (knn_route(dp, a.k, a.nt) == FDR_ROUTE_FAST && a.nq > 0 && knn_prefilter_wanted(ctx->knn_mode, a.nt, a.k)) {
        const int rc = launch_knn_prefilter(ctx, a);
        if (rc) ctx->cap.invalidate();  // (a failed call leaves no capture)
        return rc;
    }
    knn_call_whole(ctx, FDR_PATH_EXACT, FDR_TRACE_EXACT, dp, a.k, a.nq, a.nt);
    return launch_knn_exact(ctx, a);
}

// ---- duplicate-row classes: search unique queries x unique targets, expand --------------------
// Queues the class tables of the n target rows that hash_rows_kernel has hashed into W.hash / W.idx: sort -> class
// starts -> scan -> class tables -> scan -> unique tables.  No synchronise; W.cid[n - 1] is then the number of classes.
// The one builder: the ranks of a row-sharded run (fdr_knn_classes_dev) and a plain call get the same tables from the
// same rows.
static int queue_class_tables(const DedupWs &W, const float *d_That, int n, int dp, hipStream_t st) {
    const unsigned g1 = (unsigned)((n + 255) / 256);
    size_t tb = W.tmp_bytes;
    HIP_TRY(rocprim::radix_sort_pairs(W.tmp, tb, W.hash, W.hash_s, W.idx, W.idx_s, (size_t)n, 0, 64, st));
    hipLaunchKernelGGL(mark_class_starts_kernel, dim3(g1), dim3(256), 0, st, d_That, n, dp, (const u64 *)W.hash_s,
                       (const int *)W.idx_s, W.flag);
    tb = W.tmp_bytes;
    HIP_TRY(rocprim::inclusive_scan(W.tmp, tb, W.flag, W.cid, (size_t)n, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(class_tables_kernel, dim3(g1), dim3(256), 0, st, n, (const int *)W.flag, (const int *)W.cid,
                       (const int *)W.idx_s, W.cls, W.cstart, W.isrep);
    tb = W.tmp_bytes;
    HIP_TRY(rocprim::inclusive_scan(W.tmp, tb, W.isrep, W.upos, (size_t)n, rocprim::plus<int>(), st));
    hipLaunchKernelGGL(unique_tables_kernel, dim3(g1), dim3(256), 0, st, n, (const int *)W.isrep, (const int *)W.upos,
                       (const int *)W.cls, (const int *)W.cstart, W.uofc, W.cofu, W.rep_m);
    HIP_TRY(hipGetLastError());
    return FDR_OK;
}

// expand_classes_kernel: the unique rows' results (idx_u / dist_u, u_stride elements apart; found through uqpos where
// only some unique rows were queries) -> the results of rows [q0, q0 + nq) of the classes in W
static int launch_expand(const DedupWs &W, int64_t q0, int64_t nq, int k, int64_t t_base, const int *uqpos,
                         const int32_t *idx_u, const float *dist_u, int64_t u_stride, int32_t *d_idx, float *d_dist,
                         const uint8_t *upath, uint8_t path_all, uint8_t *rowpath, hipStream_t st) {
    // queries (waves) per workgroup: four while their K * K keys stay within 32 KiB of LDS  (k <= FDR_FAST_MAX_K = 64)
    const int xw = (size_t)4 * k * k * 8 <= 32768 ? 4 : (size_t)2 * k * k * 8 <= 32768 ? 2 : 1;
    const int xq = xw * (64 / k) * EXPAND_UNROLL;
    hipLaunchKernelGGL(expand_classes_kernel, dim3((unsigned)((nq + xq - 1) / xq)), dim3(64 * xw), (size_t)xw * k * k * 8,
                       st, (int)q0, (int)nq, k, 64 / k, (int)t_base, (const int *)W.cls, (const int *)W.uofc, uqpos,
                       (const int *)idx_u, dist_u, (const int *)W.idx_s, (const int4 *)W.rep_m, d_idx, d_dist,
                       (int)u_stride, upath, path_all, rowpath);
    HIP_TRY(hipGetLastError());
    return FDR_OK;
}

static int launch_knn(fdr_ctx *ctx, const KnnArgs &a) {
    int rc = check_knn_args(ctx, a);
    if (rc) return rc;
    const float *const d_Qhat = a.Qhat, *const d_That = a.That;
    const int64_t nq = a.nq, nt = a.nt;
    const int d = a.d, k = a.k;
    const hipStream_t st = a.st;
    const int dp = fdr_padded_dim(d);
    const int route = knn_route(dp, k, nt);
    if (route == FDR_ROUTE_GENERIC) {  // beyond the MFMA kernels' shapes
        if (nq == 0) return FDR_OK;
        ctx->last.unique_targets = (int)nt;
        ctx->last.unique_queries = (int)nq;
        knn_call_whole(ctx, FDR_PATH_GENERIC, FDR_TRACE_GENERIC, dp, k, nq, nt);
        ctx->last.trace.generic = 1;
        int trc = timing_begin(ctx, FDR_KERNEL_KNN_TILE, st);
        if (trc) return trc;
        hipLaunchKernelGGL(knn_generic_kernel, dim3((unsigned)((nq + GEN_QPB - 1) / GEN_QPB)), dim3(256),
                           (size_t)GEN_QPB * dp * 4, st, d_Qhat, a.qzero, (int)nq, d_That, a.tzero, (int)nt, (int)a.t_base, dp, k,
                           a.idx, a.dist);
        HIP_TRY(hipGetLastError());
        return timing_end(ctx, FDR_KERNEL_KNN_TILE, st);
    }
    // the plain search, every row a class of its own, in the first `bytes` of the workspace
    auto plain = [&](size_t bytes) {
        ctx->last.unique_targets = (int)nt;
        ctx->last.unique_queries = (int)nq;
        KnnArgs b = a;
        b.ws_bytes = bytes;
        return launch_knn_mode(ctx, b);
    };
    // the queries must be a block of the target rows (they are in every caller of this library)
    const bool q_in_t = nq > 0 && d_Qhat >= d_That && d_Qhat + (size_t)nq * dp <= d_That + (size_t)nt * dp &&
                        ((d_Qhat - d_That) % dp) == 0;
    // (FDR_ROUTE_WIDE: the exact pass of launch_knn_mode, never the duplicate-row classes)
    if (!(route == FDR_ROUTE_FAST && q_in_t && knn_dedup_wanted(ctx->dedup_mode, nq, nt))) return plain(a.ws_bytes);
    const WsEnv env = ws_env(ctx);
    const DedupWs W = dedup_ws(env, a.ws, nq, nt, d, k);
    if (a.ws_bytes < W.total) return fail(FDR_E_ARG, "knn: workspace %zu < required %zu bytes", a.ws_bytes, W.total);
    const int n = (int)nt;
    const int q0 = (int)((d_Qhat - d_That) / dp);
    const unsigned g16 = (unsigned)(((size_t)n * 16 + 255) / 256), g1 = (unsigned)((n + 255) / 256);

    int trc = timing_begin(ctx, FDR_KERNEL_KNN_DEDUP, st);
    if (trc) return trc;
    hipLaunchKernelGGL(hash_rows_kernel, dim3(g16), dim3(256), 0, st, d_That, n, dp, W.hash, W.idx);
    HIP_TRY(hipGetLastError());
    // From 2^18 targets the sort and the tables (< 1 ms at 1 M rows) are noise next to the search (~ n^2): no probe,
    // no read-back for it; the decision falls on the exact unique counts below.  Below: a hash-table probe (~15 us)
    // tells whether enough rows repeat to pay for the sort and the tables.
    if (ctx->dedup_mode != FDR_DEDUP_FORCE && W.probe_slots) {
        HIP_TRY(hipMemsetAsync(W.probe_table, 0, (size_t)W.probe_slots * 8 + 4, st));
        hipLaunchKernelGGL(dedup_probe_kernel, dim3(g1), dim3(256), 0, st, (const u64 *)W.hash, n, W.probe_table,
                           W.probe_slots - 1, W.probe_count);
        HIP_TRY(hipGetLastError());
        int dups = 0;
        HIP_TRY(hipMemcpyAsync(&dups, W.probe_count, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((double)dups < 0.05 * (double)n) {  // (unique share)^2 > 0.9: not worth it
            if ((trc = timing_end(ctx, FDR_KERNEL_KNN_DEDUP, st))) return trc;
            return plain(W.inner_bytes);
        }
    }
    if ((rc = queue_class_tables(W, d_That, n, dp, st))) return rc;
    HIP_TRY(hipMemsetAsync(W.uqflag, 0, (size_t)n * 4, st));
    hipLaunchKernelGGL(mark_query_classes_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, q0,
                       (int)nq, (const int *)W.cls, (const int *)W.uofc, W.uqflag);
    size_t tb = W.tmp_bytes;
    HIP_TRY(rocprim::inclusive_scan(W.tmp, tb, W.uqflag, W.uqpos, (size_t)n, rocprim::plus<int>(), st));
    HIP_TRY(hipGetLastError());
    int nu = 0, nuq = 0;
    HIP_TRY(hipMemcpyAsync(&nu, W.cid + (n - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&nuq, W.uqpos + (n - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // few duplicates (or, never seen, no room for the inner call): plain search
    if (!dedup_worth(nu, nuq, nt, nq, k, ctx->dedup_mode) || knn_mode_workspace_bytes(env, nuq, nu, d, k) > W.inner_bytes) {
        if ((trc = timing_end(ctx, FDR_KERNEL_KNN_DEDUP, st))) return trc;
        return plain(W.inner_bytes);
    }
    ctx->last.unique_targets = nu;
    ctx->last.unique_queries = nuq;
    hipLaunchKernelGGL(gather_unique_rows_kernel, dim3(g16), dim3(256), 0, st, d_That, a.tzero, n, dp,
                       (const int *)W.isrep, (const int *)W.upos, W.U, W.uzero);
    if (nuq != nu)  // (else the unique queries are the unique rows: no copy, see below)
        hipLaunchKernelGGL(gather_unique_queries_kernel, dim3((unsigned)(((size_t)nu * 16 + 255) / 256)), dim3(256),
                           0, st, (const float *)W.U, (const unsigned char *)W.uzero, nu, dp, (const int *)W.uqflag,
                           (const int *)W.uqpos, W.Uq, W.uqz);
    HIP_TRY(hipGetLastError());
    if ((trc = timing_end(ctx, FDR_KERNEL_KNN_DEDUP, st))) return trc;
    // unique rows are stored in ascending representative order, and the unique queries are a subsequence
    // of them; the inner search numbers targets 0..nu-1
    // (every unique row is a query: Uq would be a copy of U -- the same pointers let the prefilter mode see that
    // the queries are the targets)
    const bool all_q = nuq == nu;
    KnnArgs u = a;
    u.Qhat = all_q ? W.U : W.Uq;
    u.qzero = all_q ? W.uzero : W.uqz;
    u.nq = nuq;
    u.That = W.U;
    u.tzero = W.uzero;
    u.nt = nu;
    u.t_base = 0;
    u.idx = W.idx_u;
    u.dist = W.dist_u;
    u.ws_bytes = W.inner_bytes;
    if ((rc = launch_knn_mode(ctx, u))) return rc;
    if ((trc = timing_begin(ctx, FDR_KERNEL_KNN_DEDUP, st))) return trc;
    const auto &inner = ctx->last.paths;  // the unique rows' codes, carried to the rows of their classes
    if ((rc = launch_expand(W, q0, nq, k, a.t_base, W.uqpos, W.idx_u, W.dist_u, k, a.idx, a.dist,
                            inner.n == nuq ? inner.dev : nullptr, inner.all, W.rowpath, st)))
        return rc;
    ctx->last.paths = {W.rowpath, nq, FDR_PATH_NONE, st};
    return timing_end(ctx, FDR_KERNEL_KNN_DEDUP, st);
}

// ---- duplicate-row classes across ranks ---------------------------------------------------------
// A row-sharded run searches a duplicate QUERY row once per rank that holds a member of its class (8 ranks
// at 1 M reads: 7816 query blocks instead of 6494).  These three calls let the ranks split the UNIQUE rows
// instead: every rank builds the classes of the (all-gathered) target set -- the same tables on every rank --
// searches its share of the unique rows, the shares are exchanged (nu x k indices and distances), and every
// rank expands its own rows from the complete result.
FDR_EXPORT int fdr_knn_classes_dev(fdr_ctx *ctx, const float *d_That, const uint8_t *d_tzero, int64_t nt, int32_t d,
                                   int32_t k, int64_t nq_max, void *d_ws, size_t ws_bytes, void *stream,
                                   int32_t *n_unique_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    hipStream_t st = (hipStream_t)stream;
    ctx->cls.valid = false;
    if (!n_unique_out) return fail(FDR_E_ARG, "knn_classes: n_unique_out is null");
    *n_unique_out = 0;
    const int dp = fdr_padded_dim(d);
    if (dp < 0 || k < 1 || k > FDR_MAX_K || nt < k || nq_max <= 0 || nq_max > nt || !d_That || !d_tzero || !d_ws ||
        nt > 0x7fffffffll)
        return fail(FDR_E_ARG, "knn_classes: bad argument");
    if (knn_route(dp, k, nt) != FDR_ROUTE_FAST) return FDR_OK;  // (no classes beyond k <= 64, d <= 512: the callers use fdr_knn_dev)
    if (!knn_dedup_wanted(ctx->dedup_mode, nq_max, nt)) return FDR_OK;  // (small sets: the callers use fdr_knn_dev)
    const DedupWs W = dedup_ws(ws_env(ctx), d_ws, nq_max, nt, d, k);
    if (ws_bytes < W.total) return fail(FDR_E_ARG, "knn_classes: workspace %zu < required %zu bytes", ws_bytes, W.total);
    const int n = (int)nt;
    const unsigned g16 = (unsigned)(((size_t)n * 16 + 255) / 256);
    int trc = timing_begin(ctx, FDR_KERNEL_KNN_DEDUP, st);
    if (trc) return trc;
    hipLaunchKernelGGL(hash_rows_kernel, dim3(g16), dim3(256), 0, st, d_That, n, dp, W.hash, W.idx);
    HIP_TRY(hipGetLastError());
    // No hash-table probe here (launch_knn's shortcut for small sets): its count depends on the order in which
    // the table fills, and every rank of a row-sharded run must take the SAME decision from the same gathered
    // rows or their collectives no longer match.  The exact unique count after the sort is deterministic.
    if ((rc = queue_class_tables(W, d_That, n, dp, st))) return rc;
    int nu = 0;
    HIP_TRY(hipMemcpyAsync(&nu, W.cid + (n - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (every unique row may be a query of some rank: launch_knn's rule with nuq = nu, nq = nt)
    if (!dedup_worth(nu, nu, nt, nt, k, ctx->dedup_mode)) return timing_end(ctx, FDR_KERNEL_KNN_DEDUP, st);
    hipLaunchKernelGGL(gather_unique_rows_kernel, dim3(g16), dim3(256), 0, st, d_That, d_tzero, n, dp,
                       (const int *)W.isrep, (const int *)W.upos, W.U, W.uzero);
    HIP_TRY(hipGetLastError());
    if ((trc = timing_end(ctx, FDR_KERNEL_KNN_DEDUP, st))) return trc;
    ctx->cls.valid = true;
    ctx->cls.That = d_That;
    ctx->cls.tzero = d_tzero;
    ctx->cls.nt = nt;
    ctx->cls.nq_max = nq_max;
    ctx->cls.d = d;
    ctx->cls.k = k;
    ctx->cls.nu = nu;
    ctx->cls.ws = d_ws;
    ctx->cls.ws_bytes = ws_bytes;
    ctx->last.unique_targets = nu;
    *n_unique_out = nu;
    return FDR_OK;
}

// the tables fdr_knn_classes_dev left in the caller's workspace: the same layout, from what it recorded
static DedupWs classes_ws(const fdr_ctx *ctx) {
    return dedup_ws(ws_env(ctx), ctx->cls.ws, ctx->cls.nq_max, ctx->cls.nt, ctx->cls.d, ctx->cls.k);
}

FDR_EXPORT int fdr_knn_unique_dev(fdr_ctx *ctx, int64_t u_lo, int64_t u_hi, int32_t *d_idx_u, float *d_dist_u,
                                  void *stream) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    if (!ctx->cls.valid) return fail(FDR_E_STATE, "knn_unique: no classes (call fdr_knn_classes_dev first)");
    if (u_lo < 0 || u_hi < u_lo || u_hi > ctx->cls.nu || u_hi - u_lo > ctx->cls.nq_max)
        return fail(FDR_E_ARG, "knn_unique: bad range [%lld, %lld) of %d unique rows (at most %lld per call)",
                    (long long)u_lo, (long long)u_hi, ctx->cls.nu, (long long)ctx->cls.nq_max);
    if (u_hi == u_lo) return FDR_OK;
    if (!d_idx_u || !d_dist_u) return fail(FDR_E_ARG, "knn_unique: null output");
    const int dp = fdr_padded_dim(ctx->cls.d);
    const DedupWs W = classes_ws(ctx);
    ctx->last.unique_queries = (int)(u_hi - u_lo);
    // the unique rows are stored in ascending representative order; a share of them is a block of U
    rc = launch_knn_mode(ctx, KnnArgs{W.U + (size_t)u_lo * dp, W.uzero + u_lo, u_hi - u_lo, W.U, W.uzero, ctx->cls.nu, 0,
                                      ctx->cls.d, ctx->cls.k, d_idx_u, d_dist_u, ctx->cls.ws, W.inner_bytes,
                                      (hipStream_t)stream});
    ctx->last.paths = {};  // (fdr_last_query_paths covers whole calls; a share of the unique rows is not one)
    return rc;
}

FDR_EXPORT int fdr_knn_expand_dev(fdr_ctx *ctx, int64_t q0, int64_t nq, int64_t t_base, const int32_t *d_idx_u_all,
                                  const float *d_dist_u_all, int64_t u_row_stride, int32_t *d_idx, float *d_dist,
                                  void *stream) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);  // (no path codes: the unique rows were searched by several ranks)
    if (!ctx->cls.valid) return fail(FDR_E_STATE, "knn_expand: no classes (call fdr_knn_classes_dev first)");
    if (q0 < 0 || nq < 0 || q0 + nq > ctx->cls.nt) return fail(FDR_E_ARG, "knn_expand: bad row range");
    if (nq == 0) return FDR_OK;
    if (!d_idx_u_all || !d_dist_u_all || !d_idx || !d_dist) return fail(FDR_E_ARG, "knn_expand: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int k = ctx->cls.k;
    if (u_row_stride == 0) u_row_stride = k;
    if (u_row_stride < k || u_row_stride > 0x7fffffffll) return fail(FDR_E_ARG, "knn_expand: bad row stride");
    int trc = timing_begin(ctx, FDR_KERNEL_KNN_DEDUP, st);
    if (trc) return trc;
    if ((rc = launch_expand(classes_ws(ctx), q0, nq, k, t_base, nullptr, d_idx_u_all, d_dist_u_all, u_row_stride, d_idx,
                            d_dist, nullptr, 0, nullptr, st)))
        return rc;
    return timing_end(ctx, FDR_KERNEL_KNN_DEDUP, st);
}

// ---- device-pointer API ----------------------------------------------------------------------
FDR_EXPORT int fdr_embed_dev(fdr_ctx *ctx, int64_t n_rows, const int64_t *d_indptr,
                             const int32_t *d_indices, float *d_E, void *stream) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (n_rows > 0 && (!d_indptr || !d_E)) return fail(FDR_E_ARG, "embed: null device pointer");
    return launch_embed(ctx, n_rows, d_indptr, d_indices, d_E, (hipStream_t)stream);
}

FDR_EXPORT int fdr_normalize_dev(fdr_ctx *ctx, const float *d_E, int64_t n_rows, int32_t d,
                                 float *d_Ehat, uint8_t *d_zero, void *stream) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if (n_rows > 0 && (!d_E || !d_Ehat || !d_zero)) return fail(FDR_E_ARG, "normalize: null device pointer");
    return launch_normalize(ctx, d_E, n_rows, d, d_Ehat, d_zero, (hipStream_t)stream);
}

FDR_EXPORT int fdr_knn_dev(fdr_ctx *ctx, const float *d_Qhat, const uint8_t *d_qzero, int64_t nq,
                           const float *d_That, const uint8_t *d_tzero, int64_t nt, int64_t t_base,
                           int32_t d, int32_t k, int32_t *d_idx, float *d_dist, void *d_workspace,
                           size_t workspace_bytes, void *stream) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    if (d_workspace == ctx->cls.ws) ctx->cls.valid = false;  // (this call overwrites the tables fdr_knn_classes_dev left there)
    return launch_knn(ctx, KnnArgs{d_Qhat, d_qzero, nq, d_That, d_tzero, nt, t_base, d, k, d_idx, d_dist, d_workspace,
                                   workspace_bytes, (hipStream_t)stream});
}

// ---- host-pointer API ------------------------------------------------------------------------
static int check_csr(int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices) {
    if (n_rows < 0 || !a_indptr) return fail(FDR_E_ARG, "embed: bad CSR (n_rows=%lld)", (long long)n_rows);
    if (a_indptr[0] != 0 || a_indptr[n_rows] < 0) return fail(FDR_E_ARG, "embed: bad indptr");
    if (a_indptr[n_rows] > 0 && !a_indices) return fail(FDR_E_ARG, "embed: indices is null");
    return FDR_OK;
}

static int upload_csr(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr,
                      const int32_t *a_indices) {
    int rc;
    CsrUpload &up = ctx->up;
    const int64_t nnz = a_indptr[n_rows];
    if ((rc = up.a_indptr.reserve((size_t)(n_rows + 1)))) return rc;
    if ((rc = up.a_indices.reserve((size_t)std::max<int64_t>(nnz, 1)))) return rc;
    HIP_TRY(upload(up.a_indptr, a_indptr, (size_t)(n_rows + 1), ctx->stream));
    if (nnz > 0) HIP_TRY(upload(up.a_indices, a_indices, (size_t)nnz, ctx->stream));
    return FDR_OK;
}

// How the upload's scheduler (host_upload.inc) reaches the device: its three operations on ctx->stream.
struct UploadLink {
    fdr_ctx *ctx;
    int64_t n_rows;
    const int64_t *a_indptr;
    const int32_t *a_indices;
    float *d_E;
    int64_t stage_cap;
    // rows [r0, r1) as they are, the embed kernel behind them
    int send_raw(int64_t r0, int64_t r1, int slot) {
        hipStream_t st = ctx->stream;
        const CsrUpload &up = ctx->up;
        const int64_t o = a_indptr[r0], len = a_indptr[r1] - o;
        if (len > 0)
            HIP_TRY(hipMemcpyAsync(up.a_indices.ptr() + o, a_indices + o, (size_t)len * sizeof *a_indices, hipMemcpyHostToDevice, st));
        int erc = launch_embed(ctx, r1 - r0, up.a_indptr.ptr() + r0, up.a_indices.ptr(), d_E + (size_t)r0 * ctx->proj.d, st);
        if (erc) return erc;
        if (slot >= 0) HIP_TRY(hipEventRecord(up.ev[slot], st));
        return FDR_OK;
    }
    int wait_slot(int slot) {
        HIP_TRY(hipEventSynchronize(ctx->up.ev[slot]));
        return FDR_OK;
    }
    // what the helpers staged, rows [rb, n_rows): two copies and one launch
    int send_staged(int64_t rb, int64_t used) {
        hipStream_t st = ctx->stream;
        const CsrUpload &up = ctx->up;
        const int32_t *stage_ids = up.stage_ids.ptr();
        const int64_t *stage_ptr = up.stage_ptr.ptr();
        if (used > 0)
            HIP_TRY(hipMemcpyAsync(up.c_indices.ptr() + (stage_cap - used), stage_ids + (stage_cap - used),
                                   (size_t)used * sizeof *stage_ids, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(up.c_indptr.ptr() + rb, stage_ptr + rb, (size_t)(n_rows - rb + 1) * sizeof *stage_ptr,
                               hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(up.ev[2], st));  // (the next call's helpers write the staging again: it waits for this)
        return launch_embed(ctx, n_rows - rb, up.c_indptr.ptr() + rb, up.c_indices.ptr(), d_E + (size_t)rb * ctx->proj.d, st);
    }
};

// Host CSR -> E (device, [n_rows, d]) on ctx->stream: see host_upload.inc.  Small inputs take the plain path.
static int upload_embed_pipelined(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices,
                                  float *d_E) {
    int rc;
    CsrUpload &up = ctx->up;
    const Projection &P = ctx->proj;
    const int64_t nnz = a_indptr[n_rows];
    const hup::Tuning tune;
    if (nnz < tune.min_ids || P.h_bits.empty()) {
        if ((rc = upload_csr(ctx, n_rows, a_indptr, a_indices))) return rc;
        return launch_embed(ctx, n_rows, up.a_indptr.ptr(), up.a_indices.ptr(), d_E, ctx->stream);
    }
    if ((rc = up.begin())) return rc;
    const int64_t stage_cap = hup::Tuning::stage_cap(nnz);
    if ((rc = up.a_indptr.reserve((size_t)(n_rows + 1)))) return rc;
    if ((rc = up.a_indices.reserve((size_t)nnz))) return rc;
    if ((rc = up.c_indptr.reserve((size_t)(n_rows + 1)))) return rc;
    if ((rc = up.c_indices.reserve((size_t)stage_cap))) return rc;
    if ((rc = up.stage_ids.reserve((size_t)stage_cap))) return rc;
    if ((rc = up.stage_ptr.reserve((size_t)(n_rows + 1)))) return rc;
    HIP_TRY(upload(up.a_indptr, a_indptr, (size_t)(n_rows + 1), ctx->stream));
    UploadLink link{ctx, n_rows, a_indptr, a_indices, d_E, stage_cap};
    return hup::upload(tune, n_rows, a_indptr, a_indices, P.h_bits.data(), (uint64_t)P.n_features, up.stage_ids.ptr(),
                       up.stage_ptr.ptr(), stage_cap, up.pool, hup::Tuning::helpers(host_cpu_budget()), link)
        .rc;
}

FDR_EXPORT int fdr_embed(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr,
                         const int32_t *a_indices, float *E_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    if ((rc = check_csr(n_rows, a_indptr, a_indices))) return rc;
    if (!ctx->proj.loaded()) return fail(FDR_E_STATE, "embed: no projection loaded");
    if (n_rows == 0) return FDR_OK;
    if (!E_out) return fail(FDR_E_ARG, "embed: E_out is null");
    DevArray<float> &E = ctx->call.E;
    const size_t ecount = (size_t)n_rows * ctx->proj.d;
    if ((rc = E.reserve(ecount))) return rc;
    if ((rc = upload_embed_pipelined(ctx, n_rows, a_indptr, a_indices, E.ptr()))) return rc;
    HIP_TRY(download(E_out, E, ecount, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FDR_OK;
}

// E (device, [n,d]) -> idx/dist on the host
static int knn_from_device_E(fdr_ctx *ctx, const float *d_E, int64_t n, int d, int k,
                             int32_t *idx_out, float *dist_out) {
    int rc;
    const int dp = fdr_padded_dim(d);
    if (dp < 0) return fail(FDR_E_ARG, "knn: dimension %d unsupported (1..%d)", d, FDR_MAX_DIM);
    if (k < 1 || k > FDR_MAX_K) return fail(FDR_E_ARG, "knn: k=%d unsupported (1..%d)", k, FDR_MAX_K);
    if (n < k) return fail(FDR_E_ARG, "knn: need n (%lld) >= k (%d)", (long long)n, k);
    if (!idx_out || !dist_out) return fail(FDR_E_ARG, "knn: null output pointer");
    CallScratch &cs = ctx->call;
    ResultStaging &res = ctx->res;
    if ((rc = cs.Ehat.reserve((size_t)n * dp))) return rc;
    if ((rc = cs.zero.reserve((size_t)n))) return rc;
    if ((rc = res.idx.reserve((size_t)n * k))) return rc;
    if ((rc = res.dist.reserve((size_t)n * k))) return rc;
    const size_t wsb = fdr_knn_workspace_bytes(ctx, n, n, d, k);
    if ((rc = cs.ws.reserve(wsb))) return rc;
    if ((rc = launch_normalize(ctx, d_E, n, d, cs.Ehat.ptr(), cs.zero.ptr(), ctx->stream))) return rc;
    const KnnArgs a = {cs.Ehat.ptr(), cs.zero.ptr(), n, cs.Ehat.ptr(), cs.zero.ptr(), n, 0, d, k, res.idx.ptr(), res.dist.ptr(),
                       cs.ws.ptr(), wsb, ctx->stream};
    if ((rc = launch_knn(ctx, a))) return rc;
    HIP_TRY(download(idx_out, res.idx, (size_t)n * k, ctx->stream));
    HIP_TRY(download(dist_out, res.dist, (size_t)n * k, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return FDR_OK;
}

FDR_EXPORT int fdr_knn(fdr_ctx *ctx, const float *E, int64_t n, int32_t d, int32_t k,
                       int32_t *idx_out, float *dist_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    if (!E || n <= 0) return fail(FDR_E_ARG, "knn: empty input");
    if (fdr_padded_dim(d) < 0) return fail(FDR_E_ARG, "knn: dimension %d unsupported (1..%d)", d, FDR_MAX_DIM);
    if ((rc = ctx->call.E.reserve((size_t)n * d))) return rc;
    HIP_TRY(upload(ctx->call.E, E, (size_t)n * d, ctx->stream));
    return knn_from_device_E(ctx, ctx->call.E.ptr(), n, d, k, idx_out, dist_out);
}

FDR_EXPORT int fdr_embed_knn(fdr_ctx *ctx, int64_t n_rows, const int64_t *a_indptr,
                             const int32_t *a_indices, int32_t k, int32_t *idx_out, float *dist_out,
                             float *E_out) {
    int rc = use_device(ctx);
    if (rc) return rc;
    knn_call_begin(ctx);
    if ((rc = check_csr(n_rows, a_indptr, a_indices))) return rc;
    if (!ctx->proj.loaded()) return fail(FDR_E_STATE, "embed: no projection loaded");
    if (n_rows <= 0) return fail(FDR_E_ARG, "embed_knn: empty input");
    DevArray<float> &E = ctx->call.E;
    const size_t ecount = (size_t)n_rows * ctx->proj.d;
    if ((rc = E.reserve(ecount))) return rc;
    if ((rc = upload_embed_pipelined(ctx, n_rows, a_indptr, a_indices, E.ptr()))) return rc;
    if (E_out) HIP_TRY(download(E_out, E, ecount, ctx->stream));
    return knn_from_device_E(ctx, E.ptr(), n_rows, ctx->proj.d, k, idx_out, dist_out);
}

#include "knn_sparse.inc"  // S1 .. S4: exact cosine / Jaccard k-NN on sparse feature rows (fdr_knn_sparse[_metric])
#include "knn_radius_common.inc"  // the count / scan / emit / hold protocol of both radius searches, on a RadiusResult
#include "knn_sparse_radius.inc"  // R1 .. R3: every row within a distance bound (fdr_sparse_index_radius_*)
#include "knn_dense_radius.inc"  // D-R1 .. D-R3: the same on the projected rows, through the fp16 range pass (fdr_dense_index_*)
#include "topk_merge.inc"  // T1: the exact merge of the ranks' candidate lists of a target-sharded sparse search
#include "radius_merge.inc"  // M1: the exact merge of the ranks' ragged rows of a target-sharded sparse radius search
#include "sparse_rescore.inc"  // X1 / X2: candidate lists re-scored by exact distance on the sparse rows (fdr_sparse_rescore)
#include "graph_symmetrize.inc"  // G1 .. G4: union, mutual and transposed rows of a neighbour graph (fdr_graph_symmetrize)
#include "graph_expand.inc"  // E1 .. E6: the distinct rows within two hops of a block of rows (fdr_graph_expand)
#include "graph_components.inc"  // C0 .. C3: connected components of a neighbour graph, cut at a distance (fdr_graph_components)
#include "kmer_search.inc"
#include "kmer_output_loader.inc"
#include "reads_parser.inc"
#include "overlaps_writer.inc"
