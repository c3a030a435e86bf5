// Part of libfedrann_hip.so (included by fedrann_hip.hip) and of the host-only sanitizer build
// (tests/host_san/host_san.cpp, case `upload`: ASan + UBSan, and ThreadSanitizer).  Plain C++, no HIP.
// ------------------------------------------------------------------------------------------
// Host CSR -> E in HBM for the host-pointer calls (fdr_embed, fdr_embed_knn): SURVEY.md 8(d)'s span starts with
// the CSR in host memory, and at 1 M rows its 0.69 GB of column ids are 12 ms of PCIe (57 GB/s) in front of a
// 100 ms search that cannot start before the last row has arrived.  >= 90 % of those ids have no entry in P
// (density 1 / sqrt(F), precompute.py:80-84) -- dropping them on the host (csr_compact.inc) leaves 31 MB to send,
// but costs the host about as long as the link takes for the raw ids.  So both run at once:
//
//   the rows are cut into chunks of ~1 MB of ids; the calling thread sends runs of up to eight chunks from the FRONT as
//   they are (hipMemcpyAsync, at most two in flight, so it claims chunks at the link's pace) and launches the embed
//   kernel on each run behind its copy; host threads (a pool that stays with the context) take single chunks from the
//   BACK, drop the dead ids into pinned staging memory, and the few surviving bytes follow once the two fronts have met
//   (a helper's last chunk is a quarter of a millisecond of work: the link does not wait long for it).
//
// Whatever the ratio of link to host speed on the machine, the two fronts meet where both are done (12 ms ->
// ~5-7 ms at 1 M rows on the 16 host threads of a one-GPU share).  E is bit for bit the same: a surviving id
// keeps its place in its row, and the embed kernel tests the bitmap for raw ids itself.
//
// This file decides WHAT is sent and when; HOW it reaches the device is the caller's `link` object (upload() below):
// fedrann_hip.hip's makes the HIP calls, the sanitizer harness's records what it is handed.
// ------------------------------------------------------------------------------------------
namespace hup {

struct Tuning {
    int64_t ids_per_chunk = 1 << 18;  // (1 MB of ids: ~0.25 ms for a helper, 18 us on the link; helpers' chunks cost no launch each)
    int run = 8;                      // chunks the link takes at once (two such runs in flight)
    int64_t min_ids = 1 << 20;        // below 4 MB of ids there is nothing to overlap: the caller takes its plain path
    static int64_t stage_cap(int64_t nnz) { return std::max<int64_t>(1 << 20, nnz / 6); }  // ids of pinned staging (P keeps ~5 % of them)
    static int helpers(int cpu_budget) { return std::max(1, std::min(cpu_budget - 1, 31)); }  // (the calling thread drives the link)
};

struct Chunk {
    int64_t r0, r1;            // rows
    bool checked = false;      // a helper claimed it and found its rows well-formed
    bool staged = false;       // ... and its surviving ids are in the staging buffer
};

// chunks of ~ids_per_chunk ids, cut at row boundaries by bisection of the row pointers (in bounds whatever they hold: the
// search stays inside [r + 1, n_rows] and the sum saturates -- on pointers that do not ascend std::upper_bound's
// precondition does not hold and the cut is arbitrary, but it is a cut; whoever claims a chunk checks its rows before it
// reads their ids)
static std::vector<Chunk> cut_chunks(const int64_t *a_indptr, int64_t n_rows, int64_t ids_per_chunk) {
    std::vector<Chunk> chunks;
    for (int64_t r = 0; r < n_rows;) {
        const int64_t room = std::numeric_limits<int64_t>::max() - ids_per_chunk;
        const int64_t want = a_indptr[r] > room ? std::numeric_limits<int64_t>::max() : a_indptr[r] + ids_per_chunk;
        int64_t r1 = std::upper_bound(a_indptr + r + 1, a_indptr + n_rows + 1, want) - a_indptr;  // first row END beyond `want`
        r1 = std::min(n_rows, std::max(r + 1, r1 - 1 > r ? r1 - 1 : r + 1));
        Chunk c;
        c.r0 = r;
        c.r1 = r1;
        chunks.push_back(c);
        r = r1;
    }
    return chunks;
}

// The two fronts over the chunks [0, nch), nch < 2^32: chunks [front, back) are unclaimed; the link claimed [0, front),
// the helpers [back, nch).  Both ends live in one word, so a claim is one compare-exchange and the fronts cannot cross.
struct TwoFronts {
    std::atomic<uint64_t> ends{0};  // front << 32 | back
    void reset(int64_t nch) { ends.store((uint64_t)nch); }
    int64_t back() const { return (int64_t)(ends.load() & 0xffffffffull); }
    // up to `want` chunks from one end: returns the first of them and sets `got`, or -1 when none is left
    int64_t claim(bool from_back, int want, int &got) {
        uint64_t v = ends.load();
        for (;;) {
            const uint64_t f = v >> 32, b = v & 0xffffffffull;
            if (f >= b) return -1;
            const uint64_t m = std::min<uint64_t>((uint64_t)want, b - f);
            const uint64_t nv = from_back ? (f << 32 | (b - m)) : ((f + m) << 32 | b);
            if (ends.compare_exchange_weak(v, nv)) {
                got = (int)m;
                return (int64_t)(from_back ? b - m : f);
            }
        }
    }
};

// A few host threads that stay with the context: fdr_embed_knn at 100 k rows is a 5 ms call, and starting fifteen threads
// costs a few tenths of one.
class WorkerPool {
public:
    ~WorkerPool() { stop(); }
    void ensure(int n) {  // (grows only; a thread that cannot be started is simply missing)
        try {
            while ((int)threads_.size() < n) threads_.emplace_back([this]() { loop(); });
        } catch (...) {
        }
    }
    // start the workers on fn and return at once; wait() joins them (the caller works meanwhile)
    template <typename F>
    void start(F &&fn) {
        held_ = std::function<void()>(std::forward<F>(fn));
        {
            std::unique_lock<std::mutex> lk(m_);
            job_ = &held_;
            pending_ = (int)threads_.size();
            ++gen_;
        }
        cv_.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this]() { return pending_ == 0; });
        job_ = nullptr;
    }
    void stop() {
        {
            std::unique_lock<std::mutex> lk(m_);
            quit_ = true;
            ++gen_;
        }
        cv_.notify_all();
        for (std::thread &t : threads_) t.join();
        threads_.clear();
    }

private:
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            std::function<void()> *f;
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&]() { return gen_ != seen; });
                seen = gen_;
                if (quit_) return;
                f = job_;
            }
            if (f) (*f)();
            {
                std::unique_lock<std::mutex> lk(m_);
                if (--pending_ == 0) done_.notify_all();
            }
        }
    }
    std::vector<std::thread> threads_;
    std::mutex m_;
    std::condition_variable cv_, done_;
    std::function<void()> *job_ = nullptr;
    std::function<void()> held_;
    int pending_ = 0;
    unsigned long long gen_ = 0;
    bool quit_ = false;
};

// What one call's threads share: the input, the staging the helpers fill, and the state of the two fronts.
struct Job {
    int64_t n_rows;
    const int64_t *a_indptr;
    const int32_t *a_indices;
    const uint32_t *bits;  // ftab's bitmap words, n_features bits
    uint64_t n_features;
    int32_t *stage_ids;    // [stage_cap]
    int64_t *stage_ptr;    // [n_rows + 1]
    int64_t stage_cap;
    std::vector<Chunk> chunks;
    TwoFronts fronts;
    std::vector<std::atomic<int64_t>> cum;  // [nch + 1], see help()
    std::atomic<bool> overflow{false};      // the helpers' ids do not fit the staging buffer: their chunks go raw after all
    std::atomic<int64_t> bad_row{-1};       // the first malformed row anybody met

    // true when 0 <= indptr[r] <= indptr[r + 1] <= nnz holds for the rows [r0, r1), so that their ids may be read; if not,
    // the first such row is noted in bad_row.  Relies on nnz = indptr[n_rows] >= 0 (the caller's check_csr).
    // Blocks are tested without a branch per row first.  While no pointer of a block is negative, no difference of two
    // of them overflows, so the sign bit of `neg` gathers negative pointers and negative row lengths.  Only the last
    // difference involves indptr[e], which `neg` does not cover: it is compared with nnz as unsigned, which refuses a
    // negative value too, and ascending pointers are largest at the block's end.  A block that fails this test is walked
    // row by row with the condition as written above.
    bool rows_ok(int64_t r0, int64_t r1) {
        const int64_t nnz = a_indptr[n_rows];
        for (int64_t b = r0; b < r1; b += 4096) {
            const int64_t e = std::min(r1, b + 4096);
            uint64_t neg = 0;
            for (int64_t r = b; r < e; ++r) {
                const uint64_t lo = (uint64_t)a_indptr[r], hi = (uint64_t)a_indptr[r + 1];
                neg |= lo | (hi - lo);
            }
            if ((int64_t)neg >= 0 && (uint64_t)a_indptr[e] <= (uint64_t)nnz) continue;
            for (int64_t r = b; r < e; ++r) {
                if (a_indptr[r] >= 0 && a_indptr[r] <= a_indptr[r + 1] && a_indptr[r + 1] <= nnz) continue;
                int64_t none = -1;
                bad_row.compare_exchange_strong(none, r);
                return false;
            }
        }
        return true;
    }
};

// A helper: single chunks from the back, until the fronts have met.
// The helpers' chunks end up in ROW ORDER at the END of the staging buffer, without gaps -- chunk ci right below
// chunk ci + 1 -- so that what they produced is one copy of ids, one of row pointers and ONE embed launch, however
// small the chunks.  A helper that has compacted chunk ci (into a buffer of its own) waits for cum[ci + 1], the ids
// of all chunks above it (a chained scan: that chunk was claimed just before this one and takes as long), publishes
// cum[ci] and copies its ids to stage_ids + stage_cap - cum[ci]; its rows' pointers are absolute positions there.
static void help(Job &j) {
    std::vector<int32_t> scratch;
    std::vector<int64_t> lptr;
    for (;;) {
        int got = 0;
        const int64_t ci = j.fronts.claim(true, 1, got);
        if (ci < 0) break;
        Chunk &c = j.chunks[(size_t)ci];
        const int64_t rows = c.r1 - c.r0;
        int64_t n = 0;
        // (its rows are looked at even when the chunk goes raw after all: by all helpers at once, not by the link alone)
        c.checked = j.bad_row.load() < 0 && j.rows_ok(c.r0, c.r1);
        bool ok = c.checked && !j.overflow.load();
        if (ok) {
            const int64_t raw = j.a_indptr[c.r1] - j.a_indptr[c.r0];
            try {
                if ((int64_t)scratch.size() < raw + 16) scratch.resize((size_t)raw + 16);  // (+ 16: the vector loop stores whole registers)
                if ((int64_t)lptr.size() < rows + 1) lptr.resize((size_t)rows + 1);
                n = csrc::compact_chunk(j.bits, j.n_features, j.a_indptr, j.a_indices, c.r0, c.r1, scratch.data(), raw, lptr.data());
            } catch (...) {  // (no memory for the private buffers: the chunk goes raw; no exception leaves a helper thread)
                ok = false;
            }
        }
        int64_t above;  // (every claimed chunk publishes, whatever happened to it: the chain must not break)
        while ((above = j.cum[(size_t)ci + 1].load(std::memory_order_acquire)) < 0) std::this_thread::yield();
        const int64_t mine = above + (ok ? n : 0);
        if (ok && mine > j.stage_cap) {  // (P keeps far more ids than expected: the helpers' chunks go raw after all)
            j.overflow.store(true);
            ok = false;
        }
        j.cum[(size_t)ci].store(ok ? mine : above, std::memory_order_release);
        if (!ok) continue;  // (c.staged stays false: the helpers' rows go raw)
        const int64_t base = j.stage_cap - mine;
        memcpy(j.stage_ids + base, scratch.data(), (size_t)n * 4);
        for (int64_t r = 0; r < rows; ++r) j.stage_ptr[c.r0 + r] = base + lptr[(size_t)r];
        c.staged = true;
    }
}

struct Outcome {
    int rc = FDR_OK;       // FDR_E_ARG for a malformed row (bad_row), else what the link returned
    int64_t raw_rows = 0, staged_rows = 0;  // rows handed to link.send_raw / link.send_staged
    bool overflow = false;
    int64_t bad_row = -1;
};

// The whole upload of a CSR with nnz >= 1 ids; the calling thread is the link side.  `link` has exactly three operations,
// each returning FDR_OK or the error that ends the call:
//   send_raw(r0, r1, slot)        rows [r0, r1) as they are, the embed kernel behind them; slot 0 / 1: remember the run as
//                                 that slot's, slot -1: nothing to remember
//   wait_slot(slot)               return when the link has taken the ids of that slot's run
//   send_staged(first_row, used)  rows [first_row, n_rows) from the staging buffers: the last `used` ids of stage_ids,
//                                 stage_ptr[first_row .. n_rows] (absolute positions in stage_ids), one embed launch
// What it sees for valid input: raw runs of up to `run` chunks from the front, at most two not waited for, then either one
// send_staged, or -- after an overflow or a dropped chunk -- one send_raw of the helpers' rows.  Whoever claims a chunk
// checks its rows first: no id of a malformed row is read by anybody.
template <typename Link>
static Outcome upload(const Tuning &tune, int64_t n_rows, const int64_t *a_indptr, const int32_t *a_indices, const uint32_t *bits,
                      uint64_t n_features, int32_t *stage_ids, int64_t *stage_ptr, int64_t stage_cap, WorkerPool &pool,
                      int helpers, Link &link) {
    Job j{n_rows, a_indptr, a_indices, bits, n_features, stage_ids, stage_ptr, stage_cap};
    j.chunks = cut_chunks(a_indptr, n_rows, tune.ids_per_chunk);
    const int64_t nch = (int64_t)j.chunks.size();
    j.fronts.reset(nch);
    j.cum = std::vector<std::atomic<int64_t>>((size_t)nch + 1);
    for (auto &c : j.cum) c.store(-1, std::memory_order_relaxed);
    j.cum[(size_t)nch].store(0);
    pool.ensure(helpers);  // (fewer helpers than hoped: the link carries more)
    pool.start([&j]() { help(j); });

    Outcome out;
    for (int64_t sent = 0; out.rc == FDR_OK; ++sent) {
        const int slot = (int)(sent & 1);
        // two runs in flight: the next is claimed when the link has taken the one before the last
        if (sent >= 2 && (out.rc = link.wait_slot(slot))) break;
        int got = 0;
        const int64_t ci = j.fronts.claim(false, tune.run, got);
        if (ci < 0) break;
        const int64_t r0 = j.chunks[(size_t)ci].r0, r1 = j.chunks[(size_t)(ci + got - 1)].r1;
        if (!j.rows_ok(r0, r1)) break;
        if ((out.rc = link.send_raw(r0, r1, slot)) == FDR_OK) out.raw_rows += r1 - r0;
    }
    pool.wait();
    out.overflow = j.overflow.load();
    // what the helpers left: chunks [first, nch), in row order at the end of the staging buffer -- two copies and one
    // launch; if the staging buffer overflowed (a dense P) or a chunk was dropped, their rows go raw after all
    const int64_t first = j.fronts.back();
    if (out.rc == FDR_OK && j.bad_row.load() < 0 && first < nch) {
        bool all_staged = !out.overflow;
        bool all_checked = true;  // (a helper skips the look at its rows only once the call has failed)
        for (int64_t ci = first; ci < nch; ++ci) {
            const Chunk &c = j.chunks[(size_t)ci];
            all_staged = all_staged && c.staged;
            all_checked = all_checked && (c.checked || j.rows_ok(c.r0, c.r1));
        }
        const int64_t rb = j.chunks[(size_t)first].r0;
        if (all_staged) {
            stage_ptr[n_rows] = stage_cap;
            if ((out.rc = link.send_staged(rb, j.cum[(size_t)first].load())) == FDR_OK) out.staged_rows = n_rows - rb;
        } else if (all_checked) {
            if ((out.rc = link.send_raw(rb, n_rows, -1)) == FDR_OK) out.raw_rows += n_rows - rb;
        }
    }
    out.bad_row = j.bad_row.load();
    if (out.rc == FDR_OK && out.bad_row >= 0)
        out.rc = fail(FDR_E_ARG, "embed: indptr not monotone at row %lld", (long long)out.bad_row);
    return out;
}

}  // namespace hup
