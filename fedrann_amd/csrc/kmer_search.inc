// GPU replacement of the reference's kmer_searcher (kmer_searcher/kmer_searcher.cpp:232-375), the step
// upstream of the hot path: reads x k-mer library -> per-read SET of library indices.
// Included by fedrann_hip.hip; exported through include/fedrann_hip.h (fdr_kmer_search*).
//
// Semantics restated (quirks included; oracle: oracle/fedrann_oracle.c orc_kmer_search):
//   code of a k-mer = 2 bits per base (A C G T = 0 1 2 3, either case), rolling
//   cur = ((cur << 2) & mask) | base; any other character sets cur = all ones and the following characters
//   keep shifting into that (the window reads T..T + the characters since); no look-up AT an invalid
//   character; first look-up of a read after min(k, len) characters (reads shorter than k: one look-up of
//   the A-padded partial code; an empty read looks up code 0); a read's hits form a set.
//
// Byte / integer work, HBM- and cache-bound:
//   * library: open-addressing table (code+1 -> index, linear probing, load <= 1/2) behind a blocked
//     Bloom filter (two bits of one 64-bit word per key, 16 bits per key): most window codes are not in
//     the sampled library, and the filter (<= 50 MB at 25 M keys: Infinity-Cache resident) rejects ~95 %
//     of them with one 8-byte load;
//   * reads: the concatenated bytes are staged through LDS in 4 KiB chunks (16-byte loads); a thread
//     owns 16 consecutive window ends, builds the first code from k bytes and rolls the other 15;
//   * hits are appended as (read << 32 | index) with one wave-aggregated atomic per wave, sorted with
//     rocprim's radix sort, de-duplicated, and cut into rows by a binary search per read.
//
// Device scratch and state (fedrann_hip.hip): ctx->ks (struct KmerSearchScratch) is the search's -- inputs, table and
// filter, the hits, their sorted copy, flags, scan, the unique hits' indices and rows, indptr, and `nnz` until
// fdr_kmer_search_indices fetches them; ctx->kc (struct KmerCountScratch) is the count's -- a block's characters, codes
// and runs, the two accumulated tables with `k`, `acc`, `na`, the merge and threshold arrays, the small tables of the
// W-way merge and the export, and `n` until fdr_kmer_count_fetch.  One typed array per job; two arrays of the count
// serve two jobs in turn and say so where they are declared (codes: a block's window codes, then its run codes; sorted:
// a block's sorted codes, at the end the kept codes).  The two stages share nothing.  Either fetch releases both
// (kmer_release_scratch), arrays and state together: a count whose table a fetch has freed is no longer under way.
// Every rocprim call goes through rocprim_run with the stage's `tmp`; a sequence is sized by rocprim_reserve first.
#define KS_CHUNK 4096
#define KS_PER_THREAD 16

__device__ __forceinline__ int ks_base_code(unsigned c) {
    c |= 0x20u;  // lower case
    return c == 'a' ? 0 : c == 'c' ? 1 : c == 'g' ? 2 : c == 't' ? 3 : -1;
}

__device__ __forceinline__ void ks_bloom_pos(u64 hv, u64 nwords_mask, u64 &word, u64 &bits) {
    word = (hv >> 12) & nwords_mask;
    bits = (1ull << (hv & 63)) | (1ull << ((hv >> 6) & 63));
}

__global__ __launch_bounds__(256) void ks_build_kernel(const u64 *__restrict__ codes, long long n,
                                                       u64 *__restrict__ keys, unsigned *__restrict__ vals,
                                                       u64 tmask, u64 *__restrict__ bloom, u64 bmask) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 code = codes[i], hv = mix64(code);
    u64 slot = hv & tmask;
    for (;;) {  // (codes are unique and the table is at most half full: terminates)
        const u64 old = atomicCAS(reinterpret_cast<unsigned long long *>(keys + slot), 0ull,
                                  (unsigned long long)(code + 1));
        if (old == 0ull) {
            vals[slot] = (unsigned)i;
            break;
        }
        slot = (slot + 1) & tmask;
    }
    u64 w, b;
    ks_bloom_pos(hv, bmask, w, b);
    atomicOr(reinterpret_cast<unsigned long long *>(bloom + w), (unsigned long long)b);
}

// look `code` up; returns the library index or -1
__device__ __forceinline__ int ks_lookup(u64 code, const u64 *__restrict__ keys, const unsigned *__restrict__ vals,
                                         u64 tmask, const u64 *__restrict__ bloom, u64 bmask) {
    const u64 hv = mix64(code);
    u64 w, b;
    ks_bloom_pos(hv, bmask, w, b);
    if ((bloom[w] & b) != b) return -1;
    u64 slot = hv & tmask;
    for (;;) {
        const u64 kv = keys[slot];
        if (kv == 0ull) return -1;
        if (kv == code + 1) return (int)vals[slot];
        slot = (slot + 1) & tmask;
    }
}

// wave-aggregated append of (read, index) pairs; `pairs` holds `cap` slots, `counter` keeps counting past it
__device__ __forceinline__ void ks_emit(bool hit, u64 pair, u64 *__restrict__ pairs, long long cap,
                                        unsigned long long *__restrict__ counter) {
    const u64 m = __ballot(hit);
    if (m == 0ull) return;
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == (int)__ffsll((long long)m) - 1) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = __shfl(base, (int)__ffsll((long long)m) - 1);
    if (hit) {
        const unsigned long long pos = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if ((long long)pos < cap) pairs[pos] = pair;
    }
}

// window ends of reads with at least k characters.  Per 4 KiB chunk of the concatenated reads:
//  1. stage the bytes (+ 32 of history) in LDS; find the read of the chunk's first position once per
//     workgroup (binary search) and, per thread, gallop from there to the read of its own first position;
//  2. a thread owns KS_PER_THREAD consecutive window ends, in batches of 8: the 8 codes (rolling, VALU
//     only), then the 8 Bloom-filter words back to back (independent loads in flight together);
//  3. windows that pass the filter (~5 % false positives + the real hits) are COMPACTED into an LDS list
//     and probed in the table by consecutive threads afterwards.  Probing inside step 2 put a divergent
//     chain of dependent loads on the path of every step, because some lane of 64 nearly always passes;
//  4. hits go to an LDS buffer (it reuses the candidate list's slots: a hit never outruns its candidate)
//     and leave with ONE global atomic per workgroup and chunk -- a global atomic per wave and step (3 M on
//     one address at 200 Mbases) serialised the whole kernel (30 ms -> 2.4 ms).
// A chunk with more than KS_CAND filter passes probes the excess on the spot and appends to global memory.
#define KS_CAND 2048
__global__ __launch_bounds__(256) void ks_search_kernel(const unsigned char *__restrict__ seq, long long total,
                                                        const long long *__restrict__ off, int n_reads, int k,
                                                        const u64 *__restrict__ keys,
                                                        const unsigned *__restrict__ vals, u64 tmask,
                                                        const u64 *__restrict__ bloom, u64 bmask,
                                                        u64 *__restrict__ pairs, long long cap,
                                                        unsigned long long *__restrict__ counter) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[KS_CHUNK + 48];  // 32 bytes of history in front
    __shared__ u64 cbuf[KS_CAND];   // candidate codes, then (step 4) the hits
    __shared__ int crid[KS_CAND];   // candidate read numbers
    __shared__ int ccnt, hitcnt, chunk_read;
    __shared__ unsigned long long hitbase;
    const u64 mask = (1ull << (2 * k)) - 1ull;
    const int lane = threadIdx.x & 63;
    auto probe = [&](u64 code, u64 hv, unsigned &idx) -> bool {
        u64 slot = hv & tmask;
        for (;;) {
            const u64 kv = keys[slot];
            if (kv == 0ull) return false;
            if (kv == code + 1) {
                idx = vals[slot];
                return true;
            }
            slot = (slot + 1) & tmask;
        }
    };
    for (long long c0 = (long long)blockIdx.x * KS_CHUNK; c0 < total; c0 += (long long)gridDim.x * KS_CHUNK) {
        __syncthreads();
        if (threadIdx.x == 0) {
            ccnt = 0;
            hitcnt = 0;
            int lo = 0, hi = n_reads - 1;  // last read with off[r] <= c0
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= c0) lo = mid; else hi = mid - 1;
            }
            chunk_read = lo;
        }
        for (int i = threadIdx.x; i < (KS_CHUNK + 32) / 16; i += 256) {  // (the host pads the array)
            const long long g = c0 - 32 + 16ll * i;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g >= 0 && g < total) v = *reinterpret_cast<const uint4 *>(seq + g);
            reinterpret_cast<uint4 *>(tile)[i] = v;
        }
        __syncthreads();
        const long long p0 = c0 + (long long)threadIdx.x * KS_PER_THREAD;  // this thread's first window end
        // read that contains p0: gallop + bisect from the chunk's read (long reads: no step at all)
        int r = chunk_read;
        long long r_begin = 0, r_end = 0;
        if (p0 < total) {
            int lo = r, step = 1;
            while (lo + step < n_reads && off[lo + step] <= p0) {
                lo += step;
                step <<= 1;
            }
            int hi = min(n_reads - 1, lo + step - 1);
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= p0) lo = mid; else hi = mid - 1;
            }
            r = lo;
            r_begin = off[r];
            r_end = off[r + 1];
            while (r_end <= p0 && r + 1 < n_reads) {  // (empty reads share their offset with the next one)
                ++r;
                r_begin = r_end;
                r_end = off[r + 1];
            }
        }
        u64 cur = 0;
        bool primed = false;  // cur holds the window ending at the previous position of the same read
#pragma unroll 1
        for (int s0 = 0; s0 < KS_PER_THREAD; s0 += 8) {
            u64 code[8];
            int rid[8];
            unsigned look = 0;  // bit j: position s0 + j has a valid window to look up
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const long long p = p0 + s0 + j;
                code[j] = 0;
                rid[j] = r;
                if (p < total) {
                    while (p >= r_end && r + 1 < n_reads) {
                        ++r;
                        r_begin = r_end;
                        r_end = off[r + 1];
                        primed = false;
                    }
                    rid[j] = r;
                    if (p < r_end && p - r_begin >= k - 1) {  // a full window inside read r
                        const int t = (int)(p - c0) + 32;      // tile index of position p
                        if (!primed) {
                            cur = 0;
                            for (int q = t - k + 1; q < t; ++q) {
                                const int bc = ks_base_code(tile[q]);
                                cur = (cur << 2) & mask;
                                if (bc < 0) cur = ~0ull; else cur |= (u64)bc;
                            }
                            primed = true;
                        }
                        const int bc = ks_base_code(tile[t]);
                        cur = (cur << 2) & mask;
                        if (bc < 0) cur = ~0ull; else cur |= (u64)bc;
                        code[j] = cur;
                        if (cur != ~0ull) look |= 1u << j;
                    }
                }
            }
            u64 hv[8], word[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // the eight filter words, in flight together
                hv[j] = mix64(code[j]);
                word[j] = ((look >> j) & 1u) ? bloom[(hv[j] >> 12) & bmask] : 0ull;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const u64 bits = (1ull << (hv[j] & 63)) | (1ull << ((hv[j] >> 6) & 63));
                const bool pass = ((look >> j) & 1u) && (word[j] & bits) == bits;
                const u64 m = __ballot(pass);
                if (m == 0ull) continue;
                const int leader = (int)__ffsll((long long)m) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&ccnt, (int)__popcll(m));
                base = __shfl(base, leader);
                if (pass) {
                    const int pos = base + (int)__popcll(m & ((1ull << lane) - 1ull));
                    if (pos < KS_CAND) {
                        cbuf[pos] = code[j];
                        crid[pos] = rid[j];
                    } else {  // more filter passes than list slots in this chunk: probe on the spot
                        unsigned idx;
                        if (probe(code[j], hv[j], idx)) {
                            const unsigned long long g = atomicAdd(counter, 1ull);
                            if ((long long)g < cap) pairs[g] = ((u64)(unsigned)rid[j] << 32) | idx;
                        }
                    }
                }
            }
        }
        __syncthreads();
        // dense probing: candidate i by thread i (mod 256); hit i' <= i overwrites slot i' after a barrier
        const int nc = min(ccnt, KS_CAND);
        for (int i0 = 0; i0 < nc; i0 += 256) {
            const int i = i0 + threadIdx.x;
            bool hit = false;
            u64 pair = 0;
            if (i < nc) {
                const u64 code = cbuf[i];
                unsigned idx;
                if (probe(code, mix64(code), idx)) {
                    hit = true;
                    pair = ((u64)(unsigned)crid[i] << 32) | idx;
                }
            }
            __syncthreads();  // every candidate of this round is in registers: its slots may be reused
            const u64 m = __ballot(hit);
            if (m != 0ull) {
                const int leader = (int)__ffsll((long long)m) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&hitcnt, (int)__popcll(m));
                base = __shfl(base, leader);
                if (hit) cbuf[base + (int)__popcll(m & ((1ull << lane) - 1ull))] = pair;  // (<= i0 + 255)
            }
            __syncthreads();
        }
        const int nh = hitcnt;
        if (threadIdx.x == 0 && nh) hitbase = atomicAdd(counter, (unsigned long long)nh);
        __syncthreads();
        if (nh) {
            const unsigned long long b0 = hitbase;
            for (int i = threadIdx.x; i < nh; i += 256)
                if ((long long)(b0 + i) < cap) pairs[b0 + i] = cbuf[i];
        }
    }
}

// reads shorter than k (one look-up of the A-padded partial code; code 0 for an empty read)
__global__ __launch_bounds__(256) void ks_short_reads_kernel(const unsigned char *__restrict__ seq,
                                                             const long long *__restrict__ off, int n_reads,
                                                             int k, const u64 *__restrict__ keys,
                                                             const unsigned *__restrict__ vals, u64 tmask,
                                                             const u64 *__restrict__ bloom, u64 bmask,
                                                             u64 *__restrict__ pairs, long long cap,
                                                             unsigned long long *__restrict__ counter) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool hit = false;
    u64 pair = 0;
    if (r < n_reads) {
        const long long b = off[r], e = off[r + 1];
        if (e - b < k) {
            const u64 mask = (1ull << (2 * k)) - 1ull;
            u64 cur = 0;
            for (long long p = b; p < e; ++p) {
                const int bc = ks_base_code(seq[p]);
                cur = (cur << 2) & mask;
                if (bc < 0) cur = ~0ull; else cur |= (u64)bc;
            }
            if (cur != ~0ull) {
                const int idx = ks_lookup(cur, keys, vals, tmask, bloom, bmask);
                if (idx >= 0) {
                    hit = true;
                    pair = ((u64)(unsigned)r << 32) | (unsigned)idx;
                }
            }
        }
    }
    ks_emit(hit, pair, pairs, cap, counter);
}

// flag[i] = 1 if sorted pair i differs from its predecessor
__global__ __launch_bounds__(256) void ks_mark_unique_kernel(const u64 *__restrict__ sorted, long long n,
                                                             int *__restrict__ flag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

// compact the unique pairs: indices[pos - 1] = index part, rows[pos - 1] = read part
__global__ __launch_bounds__(256) void ks_compact_kernel(const u64 *__restrict__ sorted, long long n,
                                                         const int *__restrict__ flag,
                                                         const int *__restrict__ pos_incl,
                                                         int *__restrict__ indices, int *__restrict__ rows) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flag[i]) {
        const int p = pos_incl[i] - 1;
        indices[p] = (int)(unsigned)(sorted[i] & 0xffffffffull);
        rows[p] = (int)(unsigned)(sorted[i] >> 32);
    }
}

// indptr[r] = first unique pair whose read is >= r (rows ascending)
__global__ __launch_bounds__(256) void ks_indptr_kernel(const int *__restrict__ rows, long long nu, int n_reads,
                                                        long long *__restrict__ indptr) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > n_reads) return;
    long long lo = 0, hi = nu;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (rows[mid] < r) lo = mid + 1; else hi = mid;
    }
    indptr[r] = lo;
}

// ---- host side ---------------------------------------------------------------------------------
FDR_EXPORT int fdr_kmer_search(fdr_ctx *ctx, const uint8_t *seqs, const int64_t *seq_off, int64_t n_reads,
                               const uint64_t *lib_codes, int64_t n_lib, int32_t k, int64_t *indptr_out,
                               int64_t *nnz_out) {
    if (int rc = use_device(ctx)) return rc;
    if (!seq_off || !indptr_out || !nnz_out || n_reads < 0 || n_lib < 0 || (n_lib > 0 && !lib_codes))
        return fail(FDR_E_ARG, "fdr_kmer_search: bad argument");
    if (k <= 0 || k > 31) return fail(FDR_E_ARG, "fdr_kmer_search: k must be in [1, 31] (got %d)", k);
    if (n_reads >= 0x7fffffffll || n_lib >= 0x7fffffffll)
        return fail(FDR_E_ARG, "fdr_kmer_search: read and library counts must be below 2^31");
    if (seq_off[0] != 0) return fail(FDR_E_ARG, "fdr_kmer_search: seq_off[0] must be 0");
    for (int64_t r = 0; r < n_reads; ++r)
        if (seq_off[r + 1] < seq_off[r]) return fail(FDR_E_ARG, "fdr_kmer_search: seq_off is not monotone");
    const int64_t total = seq_off[n_reads];
    if (total > 0 && !seqs) return fail(FDR_E_ARG, "fdr_kmer_search: seqs is null");
    KmerSearchScratch &ks = ctx->ks;
    ks.nnz = 0;
    indptr_out[0] = 0;
    *nnz_out = 0;
    if (n_reads == 0) return FDR_OK;
    hipStream_t st = ctx->stream;

    // inputs
    if (int rc = ks.seq.reserve((size_t)total + 64)) return rc;
    if (int rc = ks.off.reserve((size_t)(n_reads + 1))) return rc;
    HIP_TRY(hipMemsetAsync(ks.seq.ptr() + total, 0, 64, st));
    if (total) HIP_TRY(hipMemcpyAsync(ks.seq.ptr(), seqs, (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ks.off.ptr(), seq_off, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
    // library table + Bloom filter
    u64 tsize = 1024, bwords = 1024;
    while (tsize < 2ull * (u64)n_lib) tsize <<= 1;
    while (bwords < (u64)n_lib / 4) bwords <<= 1;  // 16 bits per key
    if (int rc = ks.lib_codes.reserve((size_t)std::max<int64_t>(n_lib, 1))) return rc;
    if (int rc = ks.keys.reserve((size_t)tsize)) return rc;
    if (int rc = ks.vals.reserve((size_t)tsize)) return rc;
    if (int rc = ks.bloom.reserve((size_t)bwords)) return rc;
    if (int rc = ks.counter.reserve(32)) return rc;
    HIP_TRY(hipMemsetAsync(ks.keys.ptr(), 0, (size_t)tsize * 8, st));
    HIP_TRY(hipMemsetAsync(ks.bloom.ptr(), 0, (size_t)bwords * 8, st));
    int trc = timing_begin(ctx, FDR_KERNEL_KMER_SEARCH, st);
    if (trc) return trc;
    if (n_lib) {
        HIP_TRY(hipMemcpyAsync(ks.lib_codes.ptr(), lib_codes, (size_t)n_lib * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(ks_build_kernel, dim3((unsigned)((n_lib + 255) / 256)), dim3(256), 0, st, ks.lib_codes.ptr(),
                           (long long)n_lib, ks.keys.ptr(), ks.vals.ptr(), tsize - 1, ks.bloom.ptr(), bwords - 1);
        HIP_TRY(hipGetLastError());
    }
    // search; the hit buffer is sized by a guess and the pass repeated once if it was too small
    long long cap = std::max<long long>(1 << 20, total / 4 + n_reads);
    unsigned long long count = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (int rc = ks.pairs.reserve((size_t)cap)) return rc;
        HIP_TRY(hipMemsetAsync(ks.counter.ptr(), 0, 8, st));
        if (total > 0) {
            const long long chunks = (total + KS_CHUNK - 1) / KS_CHUNK;
            const unsigned grid = (unsigned)std::min<long long>(chunks, (long long)ctx->num_cus * 8);
            hipLaunchKernelGGL(ks_search_kernel, dim3(grid), dim3(256), 0, st, ks.seq.ptr(), (long long)total,
                               ks.off.ptr(), (int)n_reads, (int)k, ks.keys.ptr(), ks.vals.ptr(), tsize - 1,
                               ks.bloom.ptr(), bwords - 1, ks.pairs.ptr(), cap, ks.counter.ptr());
        }
        hipLaunchKernelGGL(ks_short_reads_kernel, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, st,
                           ks.seq.ptr(), ks.off.ptr(), (int)n_reads, (int)k, ks.keys.ptr(), ks.vals.ptr(), tsize - 1,
                           ks.bloom.ptr(), bwords - 1, ks.pairs.ptr(), cap, ks.counter.ptr());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&count, ks.counter.ptr(), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if ((long long)count <= cap) break;
        if (attempt == 1) return fail(FDR_E_STATE, "fdr_kmer_search: hit count changed between passes");
        cap = (long long)count;
    }
    if ((trc = timing_end(ctx, FDR_KERNEL_KMER_SEARCH, st))) return trc;
    if (count >= 0x7fffffffull) return fail(FDR_E_ARG, "fdr_kmer_search: %llu hits (limit 2^31)", count);
    const long long n = (long long)count;
    if ((trc = timing_begin(ctx, FDR_KERNEL_KMER_COMPACT, st))) return trc;
    if (int rc = ks.indptr.reserve((size_t)(n_reads + 1))) return rc;
    long long nu = 0;
    if (n > 0) {
        // sort (read, index), drop repeats, cut into rows
        if (int rc = ks.sorted.reserve((size_t)n)) return rc;
        if (int rc = ks.flag.reserve((size_t)n)) return rc;
        if (int rc = ks.scan.reserve((size_t)n)) return rc;
        if (int rc = ks.indices.reserve((size_t)n)) return rc;
        if (int rc = ks.rows.reserve((size_t)n)) return rc;
        auto sort_hits = [&](void *tmp, size_t &bytes) {
            return rocprim::radix_sort_keys(tmp, bytes, ks.pairs.ptr(), ks.sorted.ptr(), (size_t)n, 0, 64, st);
        };
        auto scan_flags = [&](void *tmp, size_t &bytes) {
            return rocprim::inclusive_scan(tmp, bytes, ks.flag.ptr(), ks.scan.ptr(), (size_t)n, rocprim::plus<int>(), st);
        };
        if (int rc = rocprim_reserve(ks.tmp, sort_hits, scan_flags)) return rc;  // (for both: the scan regrows nothing)
        if (int rc = rocprim_run(ks.tmp, "rocprim::radix_sort_keys", sort_hits)) return rc;
        const unsigned g = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(ks_mark_unique_kernel, dim3(g), dim3(256), 0, st, ks.sorted.ptr(), n, ks.flag.ptr());
        if (int rc = rocprim_run(ks.tmp, "rocprim::inclusive_scan", scan_flags)) return rc;
        hipLaunchKernelGGL(ks_compact_kernel, dim3(g), dim3(256), 0, st, ks.sorted.ptr(), n, ks.flag.ptr(),
                           ks.scan.ptr(), ks.indices.ptr(), ks.rows.ptr());
        HIP_TRY(hipGetLastError());
        int last = 0;
        HIP_TRY(hipMemcpyAsync(&last, ks.scan.ptr() + (n - 1), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        nu = last;
        hipLaunchKernelGGL(ks_indptr_kernel, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, st,
                           ks.rows.ptr(), nu, (int)n_reads, ks.indptr.ptr());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(indptr_out, ks.indptr.ptr(), (size_t)(n_reads + 1) * 8, hipMemcpyDeviceToHost, st));
    } else {
        memset(indptr_out, 0, (size_t)(n_reads + 1) * 8);
    }
    if ((trc = timing_end(ctx, FDR_KERNEL_KMER_COMPACT, st))) return trc;
    HIP_TRY(hipStreamSynchronize(st));
    ks.nnz = nu;
    *nnz_out = nu;
    return FDR_OK;
}

// A fetch releases all k-mer scratch, the search's and the count's (~28 B per base: not to be held through the embed /
// k-NN stages), each with its state: what a released array held cannot be fetched again or, for a count under way,
// resumed (fdr_kmer_count_add then asks for fdr_kmer_count_begin)
static void kmer_release_scratch(fdr_ctx *ctx) {
    ctx->ks.release();
    ctx->kc.release();
}

FDR_EXPORT int fdr_kmer_search_indices(fdr_ctx *ctx, int32_t *indices_out) {
    if (int rc = use_device(ctx)) return rc;
    const long long nnz = ctx->ks.nnz;
    if (nnz > 0 && !indices_out) return fail(FDR_E_ARG, "fdr_kmer_search_indices: null output");
    if (nnz > 0) {
        HIP_TRY(hipMemcpyAsync(indices_out, ctx->ks.indices.ptr(), (size_t)nnz * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    kmer_release_scratch(ctx);
    return FDR_OK;
}

// ------------------------------------------------------------------------------------------------
// Canonical k-mer counting (`jellyfish count -m k -C` + `jellyfish dump -L min`, count_kmers.py:80-121):
// every window of k characters inside one read, all of them in ACGTacgt, counts once under the smaller
// of its 2-bit code and the code of its reverse complement.  One code per window end (all ones = no
// valid window), radix sort, run-length encoding, threshold, compaction -- ascending code order
// (jellyfish dumps in its hash order; the order only names the features).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kc_codes_kernel(const unsigned char *__restrict__ seq, long long total,
                                                       const long long *__restrict__ off, int n_reads, int k,
                                                       u64 *__restrict__ codes) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[KS_CHUNK + 48];
    __shared__ int chunk_read;
    const u64 mask = (1ull << (2 * k)) - 1ull;
    const int top = 2 * (k - 1);
    for (long long c0 = (long long)blockIdx.x * KS_CHUNK; c0 < total; c0 += (long long)gridDim.x * KS_CHUNK) {
        __syncthreads();
        if (threadIdx.x == 0) {
            int lo = 0, hi = n_reads - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= c0) lo = mid; else hi = mid - 1;
            }
            chunk_read = lo;
        }
        for (int i = threadIdx.x; i < (KS_CHUNK + 32) / 16; i += 256) {
            const long long g = c0 - 32 + 16ll * i;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (g >= 0 && g < total) v = *reinterpret_cast<const uint4 *>(seq + g);
            reinterpret_cast<uint4 *>(tile)[i] = v;
        }
        __syncthreads();
        const long long p0 = c0 + (long long)threadIdx.x * KS_PER_THREAD;
        int r = chunk_read;
        long long r_begin = 0, r_end = 0;
        if (p0 < total) {
            int lo = r, step = 1;
            while (lo + step < n_reads && off[lo + step] <= p0) {
                lo += step;
                step <<= 1;
            }
            int hi = min(n_reads - 1, lo + step - 1);
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (off[mid] <= p0) lo = mid; else hi = mid - 1;
            }
            r = lo;
            r_begin = off[r];
            r_end = off[r + 1];
            while (r_end <= p0 && r + 1 < n_reads) {
                ++r;
                r_begin = r_end;
                r_end = off[r + 1];
            }
        }
        u64 fw = 0, rc = 0;
        int run = 0;          // valid characters in a row ending at the previous position (saturates at k)
        bool primed = false;
        for (int s = 0; s < KS_PER_THREAD; ++s) {
            const long long p = p0 + s;
            if (p >= total) break;
            while (p >= r_end && r + 1 < n_reads) {
                ++r;
                r_begin = r_end;
                r_end = off[r + 1];
                primed = false;
            }
            u64 out = ~0ull;
            if (p < r_end && p - r_begin >= k - 1) {
                const int t = (int)(p - c0) + 32;
                if (!primed) {
                    fw = rc = 0;
                    run = 0;
                    for (int q = t - k + 1; q < t; ++q) {
                        const int bc = ks_base_code(tile[q]);
                        fw = ((fw << 2) | (u64)(bc & 3)) & mask;
                        rc = (rc >> 2) | ((u64)(3 - (bc & 3)) << top);
                        run = bc < 0 ? 0 : min(run + 1, k);
                    }
                    primed = true;
                }
                const int bc = ks_base_code(tile[t]);
                fw = ((fw << 2) | (u64)(bc & 3)) & mask;
                rc = (rc >> 2) | ((u64)(3 - (bc & 3)) << top);
                run = bc < 0 ? 0 : min(run + 1, k);
                if (run >= k) out = fw < rc ? fw : rc;
            }
            codes[p] = out;
        }
    }
}

// keep[i] = 1 for an accumulated k-mer with count >= min_count whose code is a real one
__global__ __launch_bounds__(256) void kc_flag64_kernel(const u64 *__restrict__ ucodes, const u64 *__restrict__ cnt,
                                                        long long n, u64 min_count, int *__restrict__ keep) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keep[i] = (ucodes[i] != ~0ull && cnt[i] >= min_count) ? 1 : 0;
}

__global__ __launch_bounds__(256) void kc_compact64_kernel(const u64 *__restrict__ ucodes, const u64 *__restrict__ cnt,
                                                           long long n, const int *__restrict__ keep,
                                                           const int *__restrict__ pos_incl, u64 *__restrict__ codes_out,
                                                           u64 *__restrict__ counts_out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && keep[i]) {
        codes_out[pos_incl[i] - 1] = ucodes[i];
        counts_out[pos_incl[i] - 1] = cnt[i];
    }
}

__global__ __launch_bounds__(256) void kc_widen_kernel(const unsigned *__restrict__ in, long long n, u64 *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i];
}

// One block of reads (`total` < 2^32 characters): canonical codes of every position, sorted, run-length encoded.
// Leaves the run codes (ascending; the "no k-mer here" marker ~0 last, if any) in kc.codes and their lengths in
// kc.run_len; *nruns_out = number of runs.
static int kc_block_runs(fdr_ctx *ctx, const uint8_t *seqs, const int64_t *off_rel, int64_t n_reads, int64_t total,
                         int k, unsigned *nruns_out) {
    hipStream_t st = ctx->stream;
    KmerCountScratch &kc = ctx->kc;
    if (int rc = kc.seq.reserve((size_t)total + 64)) return rc;
    if (int rc = kc.off.reserve((size_t)(n_reads + 1))) return rc;
    HIP_TRY(hipMemsetAsync(kc.seq.ptr() + total, 0, 64, st));
    HIP_TRY(hipMemcpyAsync(kc.seq.ptr(), seqs, (size_t)total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(kc.off.ptr(), off_rel, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice, st));
    if (int rc = kc.codes.reserve((size_t)total)) return rc;
    if (int rc = kc.sorted.reserve((size_t)total)) return rc;
    if (int rc = kc.run_len.reserve((size_t)total)) return rc;
    if (int rc = kc.n_runs.reserve(1)) return rc;
    auto sort_codes = [&](void *tmp, size_t &bytes) {  // (the all-ones marker needs bit 2k: codes use 2k bits)
        return rocprim::radix_sort_keys(tmp, bytes, kc.codes.ptr(), kc.sorted.ptr(), (size_t)total, 0, 2 * k + 1, st);
    };
    auto encode_runs = [&](void *tmp, size_t &bytes) {  // (the sorted codes in, the run codes over the unsorted ones)
        return rocprim::run_length_encode(tmp, bytes, kc.sorted.ptr(), (unsigned)total, kc.codes.ptr(),
                                          kc.run_len.ptr(), kc.n_runs.ptr(), st);
    };
    if (int rc = rocprim_reserve(kc.tmp, sort_codes, encode_runs)) return rc;  // (for both: nothing regrows under way)
    int trc = timing_begin(ctx, FDR_KERNEL_KMER_SEARCH, st);
    if (trc) return trc;
    const long long chunks = (total + KS_CHUNK - 1) / KS_CHUNK;
    hipLaunchKernelGGL(kc_codes_kernel, dim3((unsigned)std::min<long long>(chunks, (long long)ctx->num_cus * 8)),
                       dim3(256), 0, st, kc.seq.ptr(), (long long)total, kc.off.ptr(), (int)n_reads, (int)k,
                       kc.codes.ptr());
    HIP_TRY(hipGetLastError());
    if ((trc = timing_end(ctx, FDR_KERNEL_KMER_SEARCH, st))) return trc;
    if ((trc = timing_begin(ctx, FDR_KERNEL_KMER_COMPACT, st))) return trc;
    if (int rc = rocprim_run(kc.tmp, "rocprim::radix_sort_keys", sort_codes)) return rc;
    if (int rc = rocprim_run(kc.tmp, "rocprim::run_length_encode", encode_runs)) return rc;
    HIP_TRY(hipMemcpyAsync(nruns_out, kc.n_runs.ptr(), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return timing_end(ctx, FDR_KERNEL_KMER_COMPACT, st);
}

// Canonical k-mer counting (the reference runs `jellyfish count -C` + `dump -L`, count_kmers.py:76-101).  Read sets
// of 2^31 characters and more (1 M ONT reads are ~1e10) are counted in blocks of whole reads; the blocks' sorted
// (code, count) runs are merged into an accumulated table on the device (rocprim merge + reduce_by_key), and the
// multiplicity threshold is applied to the totals at the end.
// Incremental form (a streaming reader hands the reads over in pieces and never holds the whole read set):
//   fdr_kmer_count_begin   forgets the accumulated table
//   fdr_kmer_count_add     counts these whole reads (in blocks of < block-limit characters) and merges their sorted
//                          (code, count) runs into the accumulated device-resident table
//   fdr_kmer_count_finish  applies the multiplicity threshold to the totals; then fdr_kmer_count_fetch
FDR_EXPORT int fdr_kmer_count_begin(fdr_ctx *ctx, int32_t k) {
    if (int rc = use_device(ctx)) return rc;
    if (k <= 0 || k > 31) return fail(FDR_E_ARG, "fdr_kmer_count: k must be in [1, 31] (got %d)", k);
    ctx->kc.k = k;
    ctx->kc.na = 0;
    ctx->kc.acc = 0;
    ctx->kc.blocks = 0;
    ctx->kc.n = 0;
    return FDR_OK;
}

FDR_EXPORT int fdr_kmer_count_add(fdr_ctx *ctx, const uint8_t *seqs, const int64_t *seq_off, int64_t n_reads) {
    if (int rc = use_device(ctx)) return rc;
    if (ctx->kc.k <= 0) return fail(FDR_E_STATE, "fdr_kmer_count_add: call fdr_kmer_count_begin first");
    if (!seq_off || n_reads < 0) return fail(FDR_E_ARG, "fdr_kmer_count: bad argument");
    if (n_reads >= 0x7fffffffll) return fail(FDR_E_ARG, "fdr_kmer_count: read count must be below 2^31");
    if (n_reads > 0 && seq_off[0] != 0) return fail(FDR_E_ARG, "fdr_kmer_count: seq_off[0] must be 0");
    for (int64_t r = 0; r < n_reads; ++r)
        if (seq_off[r + 1] < seq_off[r]) return fail(FDR_E_ARG, "fdr_kmer_count: seq_off is not monotone");
    const int64_t total = n_reads > 0 ? seq_off[n_reads] : 0;
    if (total > 0 && !seqs) return fail(FDR_E_ARG, "fdr_kmer_count: seqs is null");
    if (total == 0) return FDR_OK;
    KmerCountScratch &kc = ctx->kc;
    const int k = kc.k;
    hipStream_t st = ctx->stream;
    const int64_t limit = kc.block_chars > 0 ? kc.block_chars : (int64_t)1 << 31;  // characters per block
    int trc;
    for (int64_t r0 = 0; r0 < n_reads;) {
        // whole reads, fewer than `limit` characters (a single longer read cannot be counted)
        int64_t r1 = r0;
        while (r1 < n_reads && seq_off[r1 + 1] - seq_off[r0] < limit) ++r1;
        if (r1 == r0)
            return fail(FDR_E_ARG, "fdr_kmer_count: read %lld has %lld characters (limit %lld per read)", (long long)r0,
                        (long long)(seq_off[r0 + 1] - seq_off[r0]), (long long)limit);
        const int64_t btotal = seq_off[r1] - seq_off[r0];
        std::vector<int64_t> off_rel((size_t)(r1 - r0 + 1));
        for (int64_t r = r0; r <= r1; ++r) off_rel[(size_t)(r - r0)] = seq_off[r] - seq_off[r0];
        unsigned nruns = 0;
        if (btotal > 0) {
            if (int rc = kc_block_runs(ctx, seqs + seq_off[r0], off_rel.data(), r1 - r0, btotal, k, &nruns)) return rc;
        }
        r0 = r1;
        if (nruns == 0) continue;
        ++kc.blocks;
        DevArray<u64> &acc_codes = kc.acc_codes[kc.acc], &acc_counts = kc.acc_counts[kc.acc];
        DevArray<u64> &nxt_codes = kc.acc_codes[kc.acc ^ 1], &nxt_counts = kc.acc_counts[kc.acc ^ 1];
        if ((trc = timing_begin(ctx, FDR_KERNEL_KMER_COMPACT, st))) return trc;
        if (int rc = kc.run_counts.reserve(nruns)) return rc;
        hipLaunchKernelGGL(kc_widen_kernel, dim3((nruns + 255) / 256), dim3(256), 0, st, kc.run_len.ptr(),
                           (long long)nruns, kc.run_counts.ptr());
        HIP_TRY(hipGetLastError());
        if (kc.na == 0) {  // the first block: its runs are the table so far
            if (int rc = acc_codes.reserve(nruns)) return rc;
            if (int rc = acc_counts.reserve(nruns)) return rc;
            HIP_TRY(hipMemcpyAsync(acc_codes.ptr(), kc.codes.ptr(), (size_t)nruns * 8, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(acc_counts.ptr(), kc.run_counts.ptr(), (size_t)nruns * 8, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));  // (the next block reuses the run buffers)
            kc.na = nruns;
        } else {
            const long long na = kc.na;
            const size_t nm = (size_t)na + nruns;
            if (int rc = kc.merged_codes.reserve(nm)) return rc;
            if (int rc = kc.merged_counts.reserve(nm)) return rc;
            if (int rc = nxt_codes.reserve(nm)) return rc;
            if (int rc = nxt_counts.reserve(nm)) return rc;
            if (int rc = kc.n_table.reserve(1)) return rc;
            auto merge_runs = [&](void *tmp, size_t &bytes) {
                return rocprim::merge(tmp, bytes, acc_codes.ptr(), kc.codes.ptr(), kc.merged_codes.ptr(), acc_counts.ptr(),
                                      kc.run_counts.ptr(), kc.merged_counts.ptr(), (size_t)na, (size_t)nruns,
                                      rocprim::less<u64>(), st);
            };
            auto sum_equal = [&](void *tmp, size_t &bytes) {
                return rocprim::reduce_by_key(tmp, bytes, kc.merged_codes.ptr(), kc.merged_counts.ptr(), nm,
                                              nxt_codes.ptr(), nxt_counts.ptr(), kc.n_table.ptr(), rocprim::plus<u64>(),
                                              rocprim::equal_to<u64>(), st);
            };
            if (int rc = rocprim_reserve(kc.tmp, merge_runs, sum_equal)) return rc;  // (for both)
            if (int rc = rocprim_run(kc.tmp, "rocprim::merge", merge_runs)) return rc;
            if (int rc = rocprim_run(kc.tmp, "rocprim::reduce_by_key", sum_equal)) return rc;
            unsigned long long nu = 0;
            HIP_TRY(hipMemcpyAsync(&nu, kc.n_table.ptr(), 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            kc.na = (long long)nu;
            kc.acc ^= 1;
        }
        if ((trc = timing_end(ctx, FDR_KERNEL_KMER_COMPACT, st))) return trc;
    }
    return FDR_OK;
}

FDR_EXPORT int fdr_kmer_count_finish(fdr_ctx *ctx, int64_t min_count, int64_t *n_out) {
    if (int rc = use_device(ctx)) return rc;
    if (!n_out) return fail(FDR_E_ARG, "fdr_kmer_count: bad argument");
    if (ctx->kc.k <= 0) return fail(FDR_E_STATE, "fdr_kmer_count_finish: call fdr_kmer_count_begin first");
    KmerCountScratch &kc = ctx->kc;
    hipStream_t st = ctx->stream;
    const u64 minc = (u64)std::max<int64_t>(1, min_count);
    const u64 *d_codes = kc.acc_codes[kc.acc].ptr();    // the table the threshold is applied to
    const u64 *d_counts = kc.acc_counts[kc.acc].ptr();  // (64-bit counts)
    const long long n_table = kc.na;
    kc.k = 0;
    kc.n = 0;
    *n_out = 0;
    int trc;
    long long kept = 0;
    if (n_table > 0) {
        if (n_table >= 0x7fffffffll) return fail(FDR_E_ARG, "fdr_kmer_count: %lld distinct k-mers (limit 2^31)", n_table);
        if ((trc = timing_begin(ctx, FDR_KERNEL_KMER_COMPACT, st))) return trc;
        if (int rc = kc.keep.reserve((size_t)n_table)) return rc;
        if (int rc = kc.keep_scan.reserve((size_t)n_table)) return rc;
        auto scan_keep = [&](void *tmp, size_t &bytes) {
            return rocprim::inclusive_scan(tmp, bytes, kc.keep.ptr(), kc.keep_scan.ptr(), (size_t)n_table,
                                           rocprim::plus<int>(), st);
        };
        if (int rc = rocprim_reserve(kc.tmp, scan_keep)) return rc;  // (ahead of the launch)
        const unsigned g = (unsigned)((n_table + 255) / 256);
        hipLaunchKernelGGL(kc_flag64_kernel, dim3(g), dim3(256), 0, st, d_codes, d_counts, n_table, minc, kc.keep.ptr());
        if (int rc = rocprim_run(kc.tmp, "rocprim::inclusive_scan", scan_keep)) return rc;
        int last = 0;
        HIP_TRY(hipMemcpyAsync(&last, kc.keep_scan.ptr() + (n_table - 1), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        kept = last;
        if (kept > 0) {
            if (int rc = kc.sorted.reserve((size_t)kept)) return rc;  // (no block is under way: the kept codes)
            if (int rc = kc.kept_counts.reserve((size_t)kept)) return rc;
            hipLaunchKernelGGL(kc_compact64_kernel, dim3(g), dim3(256), 0, st, d_codes, d_counts, n_table, kc.keep.ptr(),
                               kc.keep_scan.ptr(), kc.sorted.ptr(), kc.kept_counts.ptr());
            HIP_TRY(hipGetLastError());
        }
        if ((trc = timing_end(ctx, FDR_KERNEL_KMER_COMPACT, st))) return trc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    kc.n = kept;
    *n_out = kept;
    return FDR_OK;
}

FDR_EXPORT int fdr_kmer_count(fdr_ctx *ctx, const uint8_t *seqs, const int64_t *seq_off, int64_t n_reads,
                              int32_t k, int64_t min_count, int64_t *n_out) {
    if (!n_out) return fail(FDR_E_ARG, "fdr_kmer_count: bad argument");
    *n_out = 0;
    if (int rc = fdr_kmer_count_begin(ctx, k)) return rc;
    if (int rc = fdr_kmer_count_add(ctx, seqs, seq_off, n_reads)) return rc;
    return fdr_kmer_count_finish(ctx, min_count, n_out);
}

// Characters per block of fdr_kmer_count (0 = the default, 2^31; at most 2^32 - 1).  For tests: small blocks
// exercise the merge on small inputs.
FDR_EXPORT int fdr_set_kmer_count_block(fdr_ctx *ctx, int64_t chars) {
    if (!ctx) return fail(FDR_E_ARG, "null context");
    if (chars < 0 || chars > 0xffffffffll) return fail(FDR_E_ARG, "fdr_set_kmer_count_block: 0 .. 2^32 - 1 characters");
    ctx->kc.block_chars = chars;
    return FDR_OK;
}

FDR_EXPORT int fdr_last_kmer_count_blocks(fdr_ctx *ctx) { return ctx ? ctx->kc.blocks : 0; }

FDR_EXPORT int fdr_kmer_count_fetch(fdr_ctx *ctx, uint64_t *codes_out, uint64_t *counts_out) {
    if (int rc = use_device(ctx)) return rc;
    const long long n = ctx->kc.n;
    if (n > 0 && (!codes_out || !counts_out)) return fail(FDR_E_ARG, "fdr_kmer_count_fetch: null output");
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(codes_out, ctx->kc.sorted.ptr(), (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(counts_out, ctx->kc.kept_counts.ptr(), (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    kmer_release_scratch(ctx);
    return FDR_OK;
}

// ---- counting over several ranks: export by code range, W-way merge of the received runs -------------------------
// A rank of a sharded stage 1 counts its byte range of the reads (fdr_kmer_count_begin / _add), exports its
// unthresholded table cut at W - 1 splitter codes (fdr_kmer_count_export_dev), the parts are exchanged (rank p gets
// every rank's part p), and fdr_kmer_count_merge_dev folds the W received runs into one table with the threshold
// applied; fdr_kmer_count_fetch returns it as after fdr_kmer_count_finish.
//
// The merge is one pass over the runs (no chain of pairwise merges re-streaming the growing table):
//   1. every KM_STRIDE-th code of every run is a sample; the sorted samples are the tile boundaries, so a tile holds
//      about KM_STRIDE elements of all runs together (at most W x KM_STRIDE);
//   2. km_bounds_kernel binary-searches every run for every boundary: tile t's slice of run r;
//   3. km_tile_kernel, one workgroup per tile: the tile's slices go to LDS (when they fit; else the searches below
//      read them from global memory), and every element's place in the merged sequence is its index in its own
//      run plus its lower bound in every other run (+1 in a run before its own that holds the same code: ties go
//      by run number).  A code's copy in the lowest run holding it owns the code: it sums the counts of all copies
//      (at most W: every run is unique) and flags the total if it reaches min_count;
//   4. an inclusive scan of the flags compacts the owners' (code, total) in ascending code order.
#define KM_STRIDE 1024
#define KM_CACHE 4096  // codes of a tile held in LDS (32 KiB)
#define KM_MAX_RUNS 256

__device__ __forceinline__ long long km_lower_bound(const u64 *a, long long n, u64 c) {
    long long lo = 0;
    while (n > 0) {
        const long long h = n >> 1;
        if (a[lo + h] < c) {
            lo += h + 1;
            n -= h + 1;
        } else {
            n = h;
        }
    }
    return lo;
}

// samples: code KM_STRIDE * (q + 1) of run r for q < samp_pre[r + 1] - samp_pre[r]
__global__ __launch_bounds__(256) void km_sample_kernel(const u64 *__restrict__ codes, const long long *__restrict__ roff,
                                                        const long long *__restrict__ samp_pre, int n_runs, long long n_s,
                                                        u64 *__restrict__ samples) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_s) return;
    int r = 0;
    while (samp_pre[r + 1] <= s) ++r;  // (n_runs <= KM_MAX_RUNS)
    samples[s] = codes[roff[r] + (s - samp_pre[r] + 1) * KM_STRIDE];
}

// slice[t * W + r] = index in run r of tile t's first element, t = 0 .. T (row T = the run's length)
__global__ __launch_bounds__(256) void km_bounds_kernel(const u64 *__restrict__ codes, const long long *__restrict__ roff,
                                                        const u64 *__restrict__ bounds, long long n_tiles, int n_runs,
                                                        long long *__restrict__ slice) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (n_tiles + 1) * n_runs) return;
    const long long t = i / n_runs;
    const int r = (int)(i - t * n_runs);
    const long long len = roff[r + 1] - roff[r];
    slice[i] = t == 0 ? 0 : t == n_tiles ? len : km_lower_bound(codes + roff[r], len, bounds[t - 1]);
}

__global__ __launch_bounds__(256) void km_tile_kernel(const u64 *__restrict__ codes, const u64 *__restrict__ counts,
                                                      const long long *__restrict__ roff, const long long *__restrict__ slice,
                                                      int n_runs, u64 min_count, u64 *__restrict__ m_codes,
                                                      u64 *__restrict__ m_tot, int *__restrict__ keep) {
    __shared__ long long s_lo[KM_MAX_RUNS], s_base[KM_MAX_RUNS], s_pre[KM_MAX_RUNS + 1];
    __shared__ u64 s_cache[KM_CACHE];
    const long long t = blockIdx.x;
    const int tid = threadIdx.x;
    for (int r = tid; r < n_runs; r += 256) {
        s_lo[r] = slice[t * n_runs + r];
        s_base[r] = roff[r];
    }
    __syncthreads();
    if (tid == 0) {  // (n_runs <= KM_MAX_RUNS: a short serial prefix)
        long long acc = 0;
        for (int r = 0; r < n_runs; ++r) {
            s_pre[r] = acc;
            acc += max(0ll, slice[(t + 1) * n_runs + r] - s_lo[r]);  // (> 0 for ascending runs; a bad run reads nothing out of bounds)
        }
        s_pre[n_runs] = acc;
    }
    __syncthreads();
    const long long tot = s_pre[n_runs];
    const bool in_lds = tot <= KM_CACHE;
    auto run_of = [&](long long q) {  // the run of the tile's q-th element (upper bound in s_pre, minus one)
        int lo = 0, n = n_runs;
        while (n > 0) {
            const int h = n >> 1;
            if (s_pre[lo + h + 1] <= q) {
                lo += h + 1;
                n -= h + 1;
            } else {
                n = h;
            }
        }
        return lo;
    };
    if (in_lds) {
        for (long long q = tid; q < tot; q += 256) {
            const int r = run_of(q);
            s_cache[q] = codes[s_base[r] + s_lo[r] + (q - s_pre[r])];
        }
        __syncthreads();
    }
    for (long long q = tid; q < tot; q += 256) {
        const int j = run_of(q);
        const long long gi = s_lo[j] + (q - s_pre[j]);  // index in run j
        const u64 c = in_lds ? s_cache[q] : codes[s_base[j] + gi];
        u64 total = counts[s_base[j] + gi];
        long long pos = gi;
        bool owner = true;
        for (int r = 0; r < n_runs; ++r) {
            if (r == j) continue;
            const long long n = s_pre[r + 1] - s_pre[r];
            const u64 *a = in_lds ? s_cache + s_pre[r] : codes + s_base[r] + s_lo[r];
            const long long lb = km_lower_bound(a, n, c);
            pos += s_lo[r] + lb;
            if (lb < n && a[lb] == c) {
                if (r < j) {
                    owner = false;
                    ++pos;
                } else if (owner) {
                    total += counts[s_base[r] + s_lo[r] + lb];
                }
            }
        }
        keep[pos] = owner && total >= min_count ? 1 : 0;
        if (owner) {
            m_codes[pos] = c;
            m_tot[pos] = total;
        }
    }
}

// part_off[p] = first index of the table with code >= splitters[p - 1] (p = 1 .. n_parts - 1)
__global__ __launch_bounds__(256) void km_parts_kernel(const u64 *__restrict__ table, long long n,
                                                       const u64 *__restrict__ splitters, int n_parts,
                                                       long long *__restrict__ part_off) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p > n_parts) return;
    part_off[p] = p == 0 ? 0 : p == n_parts ? n : km_lower_bound(table, n, splitters[p - 1]);
}

FDR_EXPORT int fdr_kmer_count_export_dev(fdr_ctx *ctx, const uint64_t *d_splitters, int32_t n_parts,
                                         uint64_t *d_codes_out, uint64_t *d_counts_out, int64_t *part_off_out,
                                         void *stream) {
    if (int rc = use_device(ctx)) return rc;
    if (ctx->kc.k <= 0) return fail(FDR_E_STATE, "fdr_kmer_count_export_dev: call fdr_kmer_count_begin first");
    if (n_parts < 1 || !part_off_out || (n_parts > 1 && !d_splitters) || (!d_codes_out != !d_counts_out))
        return fail(FDR_E_ARG, "fdr_kmer_count_export_dev: bad argument");
    KmerCountScratch &kc = ctx->kc;
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    const u64 *d_codes = kc.acc_codes[kc.acc].ptr();
    const u64 *d_counts = kc.acc_counts[kc.acc].ptr();
    long long n = kc.na;
    if (n > 0) {  // the "no k-mer here" marker ~0 sorts last and is no k-mer: not exported
        u64 last = 0;
        HIP_TRY(hipMemcpyAsync(&last, d_codes + (n - 1), 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (last == ~0ull) --n;
    }
    if (int rc = kc.part_off.reserve((size_t)(n_parts + 1))) return rc;
    hipLaunchKernelGGL(km_parts_kernel, dim3((unsigned)((n_parts + 256) / 256)), dim3(256), 0, st, d_codes, n,
                       (const u64 *)d_splitters, (int)n_parts, kc.part_off.ptr());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(part_off_out, kc.part_off.ptr(), (size_t)(n_parts + 1) * 8, hipMemcpyDeviceToHost, st));
    if (d_codes_out && n > 0) {
        HIP_TRY(hipMemcpyAsync(d_codes_out, d_codes, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_counts_out, d_counts, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return FDR_OK;
}

// the merge of n_runs runs already on the device (d_codes / d_counts at run_off[r] .. run_off[r + 1])
static int km_merge(fdr_ctx *ctx, int32_t n_runs, const int64_t *run_off, const u64 *d_codes, const u64 *d_counts,
                    int64_t min_count, int64_t *n_out, hipStream_t st) {
    KmerCountScratch &kc = ctx->kc;
    const long long M = run_off[n_runs];
    kc.k = 0;
    kc.n = 0;
    *n_out = 0;
    if (M == 0) return FDR_OK;
    if (M >= 0x7fffffffll) return fail(FDR_E_ARG, "fdr_kmer_count_merge: %lld entries (limit 2^31)", M);
    const u64 minc = (u64)std::max<int64_t>(1, min_count);
    std::vector<long long> samp_pre((size_t)n_runs + 1, 0);
    for (int r = 0; r < n_runs; ++r) {
        const long long len = run_off[r + 1] - run_off[r];
        samp_pre[(size_t)r + 1] = samp_pre[(size_t)r] + (len > 0 ? (len - 1) / KM_STRIDE : 0);
    }
    const long long n_s = samp_pre[(size_t)n_runs], n_tiles = n_s + 1;
    if (int rc = kc.run_off.reserve((size_t)n_runs + 1)) return rc;
    if (int rc = kc.samp_pre.reserve((size_t)n_runs + 1)) return rc;
    if (int rc = kc.samples.reserve((size_t)std::max(n_s, 1ll))) return rc;
    if (int rc = kc.bounds.reserve((size_t)std::max(n_s, 1ll))) return rc;
    if (int rc = kc.slices.reserve((size_t)(n_tiles + 1) * n_runs)) return rc;
    if (int rc = kc.merged_codes.reserve((size_t)M)) return rc;   // owners' codes at their merged place
    if (int rc = kc.merged_counts.reserve((size_t)M)) return rc;  // ... their totals
    if (int rc = kc.keep.reserve((size_t)M)) return rc;
    if (int rc = kc.keep_scan.reserve((size_t)M)) return rc;
    auto sort_samples = [&](void *tmp, size_t &bytes) {
        return rocprim::radix_sort_keys(tmp, bytes, kc.samples.ptr(), kc.bounds.ptr(), (size_t)n_s, 0, 64, st);
    };
    auto scan_keep = [&](void *tmp, size_t &bytes) {
        return rocprim::inclusive_scan(tmp, bytes, kc.keep.ptr(), kc.keep_scan.ptr(), (size_t)M, rocprim::plus<int>(), st);
    };
    if (int rc = rocprim_reserve(kc.tmp, sort_samples, scan_keep)) return rc;  // (for both: nothing regrows under way)
    HIP_TRY(hipMemcpyAsync(kc.run_off.ptr(), run_off, (size_t)(n_runs + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(kc.samp_pre.ptr(), samp_pre.data(), (size_t)(n_runs + 1) * 8, hipMemcpyHostToDevice, st));
    int trc = timing_begin(ctx, FDR_KERNEL_KMER_COMPACT, st);
    if (trc) return trc;
    if (n_s > 0) {
        hipLaunchKernelGGL(km_sample_kernel, dim3((unsigned)((n_s + 255) / 256)), dim3(256), 0, st, d_codes,
                           kc.run_off.ptr(), kc.samp_pre.ptr(), (int)n_runs, n_s, kc.samples.ptr());
        HIP_TRY(hipGetLastError());
        if (int rc = rocprim_run(kc.tmp, "rocprim::radix_sort_keys", sort_samples)) return rc;
    }
    const long long nb = (n_tiles + 1) * n_runs;
    hipLaunchKernelGGL(km_bounds_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, d_codes, kc.run_off.ptr(),
                       kc.bounds.ptr(), n_tiles, (int)n_runs, kc.slices.ptr());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(km_tile_kernel, dim3((unsigned)n_tiles), dim3(256), 0, st, d_codes, d_counts, kc.run_off.ptr(),
                       kc.slices.ptr(), (int)n_runs, minc, kc.merged_codes.ptr(), kc.merged_counts.ptr(), kc.keep.ptr());
    HIP_TRY(hipGetLastError());
    if (int rc = rocprim_run(kc.tmp, "rocprim::inclusive_scan", scan_keep)) return rc;
    int kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, kc.keep_scan.ptr() + (M - 1), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (kept > 0) {
        if (int rc = kc.sorted.reserve((size_t)kept)) return rc;  // (no block is under way: the kept codes)
        if (int rc = kc.kept_counts.reserve((size_t)kept)) return rc;
        hipLaunchKernelGGL(kc_compact64_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st,
                           kc.merged_codes.ptr(), kc.merged_counts.ptr(), M, kc.keep.ptr(), kc.keep_scan.ptr(),
                           kc.sorted.ptr(), kc.kept_counts.ptr());
        HIP_TRY(hipGetLastError());
    }
    if ((trc = timing_end(ctx, FDR_KERNEL_KMER_COMPACT, st))) return trc;
    HIP_TRY(hipStreamSynchronize(st));
    kc.n = kept;
    *n_out = kept;
    return FDR_OK;
}

static int km_check_runs(int32_t n_runs, const int64_t *run_off, int64_t *n_out) {
    if (!n_out || !run_off || n_runs < 1 || n_runs > KM_MAX_RUNS)
        return fail(FDR_E_ARG, "fdr_kmer_count_merge: bad argument (1 .. %d runs)", KM_MAX_RUNS);
    if (run_off[0] != 0) return fail(FDR_E_ARG, "fdr_kmer_count_merge: run_off[0] must be 0");
    for (int r = 0; r < n_runs; ++r)
        if (run_off[r + 1] < run_off[r]) return fail(FDR_E_ARG, "fdr_kmer_count_merge: run_off is not monotone");
    return FDR_OK;
}

FDR_EXPORT int fdr_kmer_count_merge_dev(fdr_ctx *ctx, int32_t n_runs, const int64_t *run_off, const uint64_t *d_codes,
                                        const uint64_t *d_counts, int64_t min_count, int64_t *n_out, void *stream) {
    if (int rc = use_device(ctx)) return rc;
    if (int rc = km_check_runs(n_runs, run_off, n_out)) return rc;
    if (run_off[n_runs] > 0 && (!d_codes || !d_counts)) return fail(FDR_E_ARG, "fdr_kmer_count_merge_dev: null input");
    return km_merge(ctx, n_runs, run_off, (const u64 *)d_codes, (const u64 *)d_counts, min_count, n_out,
                    stream ? (hipStream_t)stream : ctx->stream);
}

FDR_EXPORT int fdr_kmer_count_merge(fdr_ctx *ctx, int32_t n_runs, const int64_t *run_off, const uint64_t *codes,
                                    const uint64_t *counts, int64_t min_count, int64_t *n_out) {
    if (int rc = use_device(ctx)) return rc;
    if (int rc = km_check_runs(n_runs, run_off, n_out)) return rc;
    const int64_t M = run_off[n_runs];
    if (M > 0 && (!codes || !counts)) return fail(FDR_E_ARG, "fdr_kmer_count_merge: null input");
    hipStream_t st = ctx->stream;
    DevArray<u64> &d_codes = ctx->kc.acc_codes[0], &d_counts = ctx->kc.acc_counts[0];  // (the merge replaces that table anyway)
    if (M > 0) {
        if (int rc = d_codes.reserve((size_t)M)) return rc;
        if (int rc = d_counts.reserve((size_t)M)) return rc;
        HIP_TRY(hipMemcpyAsync(d_codes.ptr(), codes, (size_t)M * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_counts.ptr(), counts, (size_t)M * 8, hipMemcpyHostToDevice, st));
    }
    return km_merge(ctx, n_runs, run_off, d_codes.ptr(), d_counts.ptr(), min_count, n_out, st);
}
