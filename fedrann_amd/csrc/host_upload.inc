// Part of libfedrann_hip.so: included by fedrann_hip.hip (one translation unit), not compiled on its own.
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
// ------------------------------------------------------------------------------------------
namespace hup {

struct Chunk {
    int64_t r0, r1;            // rows
    int64_t staged_off = -1;   // compacted: offset of its ids in the staging buffer (ids), -1 = sent raw
    int64_t staged_n = 0;      // ... surviving ids
};

struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return FDR_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(FDR_E_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        }
        cap = bytes;
        return FDR_OK;
    }
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
};

// A few host threads that stay with the context: fdr_embed_knn at 100 k rows is a 5 ms call, and starting fifteen threads
// costs a few tenths of one.  run(fn) has every worker call fn() once and returns when all have.
class WorkerPool {
public:
    ~WorkerPool() { stop(); }
    int size() const { return (int)threads_.size(); }
    void ensure(int n) {  // (grows only; a thread that cannot be started is simply missing)
        try {
            while ((int)threads_.size() < n) threads_.emplace_back([this]() { loop(); });
        } catch (...) {
        }
    }
    template <typename F>
    void run(F &&fn) {
        std::function<void()> f(std::forward<F>(fn));
        {
            std::unique_lock<std::mutex> lk(m_);
            job_ = &f;
            pending_ = (int)threads_.size();
            ++gen_;
        }
        cv_.notify_all();
        std::unique_lock<std::mutex> lk(m_);
        done_.wait(lk, [this]() { return pending_ == 0; });
        job_ = nullptr;
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

}  // namespace hup
