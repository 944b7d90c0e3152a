// multi_host.hip -- dnagpu_multi_*, dnagpu_count_multi*.  Host side only.
// Multi-GPU count from ONE process (what a PostgreSQL backend's glue can call): N contexts, one per
// rank, the sequence resident as contiguous word chunks, one all-gather of the packed words (RCCL
// over xGMI, or peer copies), then every rank counts the key range it owns in its own host thread.
// Same algorithm and ownership rule as the process-per-GPU path of sharded.py (bench.py --gpus N).
#include <dlfcn.h>
#include <pthread.h>
#include <rccl/rccl.h>
#include <signal.h>

#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>

#include "host_common.hpp"
#include "multi_math.hpp"

using namespace dnagpu;

namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    bool load()
    {
        if (lib)
            return true;
        // loaded on demand: a single-GPU backend never maps RCCL
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib)
                break;
        }
        if (!lib)
            return false;
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(lib, "ncclAllGather"));
        Reduce = reinterpret_cast<decltype(Reduce)>(dlsym(lib, "ncclReduce"));
        Send = reinterpret_cast<decltype(Send)>(dlsym(lib, "ncclSend"));
        Recv = reinterpret_cast<decltype(Recv)>(dlsym(lib, "ncclRecv"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(lib, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        if (!CommInitAll || !CommDestroy || !AllGather || !Reduce || !Send || !Recv || !GroupStart || !GroupEnd || !GetErrorString) {
            dlclose(lib);
            lib = nullptr;
            return false;
        }
        return true;
    }
};
}  // namespace

// One host thread per rank >= 1, kept for the life of the dnagpu_multi (rank 0's work runs on the caller's thread): a
// count drives every rank from its own thread because the level loops read counters back between launches.  No
// exception leaves a worker (std::terminate would take the PostgreSQL backend down): a job that throws marks its rank
// failed.  If the threads cannot be created the ranks' jobs run one after the other on the caller's thread.
struct MultiPool {
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    const std::function<void(int)> *job = nullptr;
    std::vector<int> threw;               // per rank: the job ended in a C++ exception (1 = bad_alloc, 2 = other)
    unsigned long long gen = 0;
    int pending = 0;
    bool stop = false, started = false, serial = false;

    static int run_guarded(const std::function<void(int)> &f, int r) noexcept
    {
        try {
            f(r);
            return 0;
        } catch (const std::bad_alloc &) {
            return 1;
        } catch (...) {
            return 2;
        }
    }
    void worker(int r)
    {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(int)> *f = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return stop || gen != seen; });
                if (stop)
                    return;
                seen = gen;
                f = job;
            }
            const int t = run_guarded(*f, r);
            {
                std::lock_guard<std::mutex> lk(mu);
                threw[(size_t)r] = t;
                if (--pending == 0)
                    cv_done.notify_all();
            }
        }
    }
    void start(int n) noexcept
    {
        if (started)
            return;
        started = true;
        // The workers must never run the host program's signal handlers: a PostgreSQL backend's handlers (SIGINT cancel,
        // SIGUSR1 latch, SIGTERM) are not thread-safe, and the kernel may deliver a process-directed signal to ANY thread
        // that does not block it.  Threads inherit the creating thread's mask: every signal is blocked around the creation
        // and the caller's mask restored right after, so the workers block everything for their whole life.
        sigset_t all, old_mask;
        sigfillset(&all);
        const bool masked = pthread_sigmask(SIG_BLOCK, &all, &old_mask) == 0;
        try {
            threw.assign((size_t)n, 0);
            th.reserve((size_t)n);
            for (int r = 1; r < n; r++)
                th.emplace_back(&MultiPool::worker, this, r);
        } catch (...) {
            shutdown();                       // joins the threads that did start
            serial = true;
        }
        if (masked)
            (void)pthread_sigmask(SIG_SETMASK, &old_mask, nullptr);
    }
    // runs f(r) for r = 0 .. n-1, rank 0 here; returns 0, or DNAGPU_ERR_OOM / DNAGPU_ERR_INTERNAL if a job threw
    int run(int n, const std::function<void(int)> &f) noexcept
    {
        start(n);
        int bad = 0;
        if (serial || n == 1) {
            for (int r = 0; r < n; r++)
                bad = std::max(bad, run_guarded(f, r));
        } else {
            {
                std::lock_guard<std::mutex> lk(mu);
                job = &f;
                pending = n - 1;
                gen++;
            }
            cv_go.notify_all();
            bad = run_guarded(f, 0);
            std::unique_lock<std::mutex> lk(mu);
            cv_done.wait(lk, [&] { return pending == 0; });
            for (int r = 1; r < n; r++)
                bad = std::max(bad, threw[(size_t)r]);
        }
        return bad == 0 ? DNAGPU_OK : (bad == 1 ? DNAGPU_ERR_OOM : DNAGPU_ERR_INTERNAL);
    }
    void shutdown() noexcept
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_go.notify_all();
        for (std::thread &t : th)
            if (t.joinable())
                t.join();
        th.clear();
        stop = false;
    }
};

struct dnagpu_multi {
    MultiPool workers;
    int n;
    std::vector<int> dev;
    std::vector<dnagpu_ctx *> ctx;
    bool rccl;
    RcclApi api;
    std::vector<ncclComm_t> comms;
    dnagpu_multi_times last{};            // host clock of the most recent dnagpu_count_multi_unordered
    std::vector<hipStream_t> xfer;        // per rank: the stream its inbound record copies are queued on
    int parts = DNAGPU_MULTI_DEFAULT_PARTS;   // bucket groups per owner of the pipelined exchange
    double emulate_gbs = 0;               // rehearsal: same-device "transfers" are held to this rate (0 = off)
    int probe_owner = -1;                 // rehearsal: only this owner pulls and counts (-1 = all), so that its time is its own
    int exchange_rccl = 0;                // record exchange: 0 = owners pull with peer copies, 1 = ncclSend / ncclRecv per piece,
                                          // 2 = as 1 and a rank's own pieces travel through RCCL too (tests with one rank)
    const char *last_exchange = "none";   // what the most recent dnagpu_count_multi_unordered moved its records with
    std::vector<dnagpu_phase_times> rec_phases;   // per rank: device phases of its record pass (most recent unordered count)
};

struct dnagpu_multi_dna {
    u64 n_bases, n_words, per;            // per = words per rank chunk; every rank's buffer holds per * n words
    std::vector<u64 *> full;              // rank r: chunk r resident at full[r] + r * per; the rest is gather space
    std::vector<dnagpu_dna *> view;       // full[r] as a dnagpu_dna of n_bases bases
};

extern "C" void dnagpu_multi_destroy(dnagpu_multi *m)
{
    if (!m)
        return;
    m->workers.shutdown();
    for (size_t r = 0; r < m->xfer.size(); r++)
        if (hipSetDevice(m->ctx[r]->device) == hipSuccess) {
            (void)hipStreamSynchronize(m->xfer[r]);
            (void)hipStreamDestroy(m->xfer[r]);
        }
    for (size_t r = 0; r < m->comms.size(); r++)
        if (m->comms[r])
            m->api.CommDestroy(m->comms[r]);
    for (dnagpu_ctx *c : m->ctx)
        dnagpu_destroy(c);
    delete m;
}

extern "C" int dnagpu_multi_init(const int *devices, int n_gpus, int transport, dnagpu_multi **out)
{
    return guarded([&]() -> int {
    if (!out || n_gpus < 1 || n_gpus > 64 || transport < DNAGPU_MULTI_AUTO || transport > DNAGPU_MULTI_COPY)
        return DNAGPU_ERR_BAD_ARG;
    *out = nullptr;
    dnagpu_multi *m = new (std::nothrow) dnagpu_multi();
    if (!m)
        return DNAGPU_ERR_OOM;
    m->n = n_gpus;
    m->rccl = false;
    bool distinct = true;
    for (int r = 0; r < n_gpus; r++) {
        const int d = devices ? devices[r] : r;
        for (int q = 0; q < r; q++)
            distinct = distinct && m->dev[q] != d;
        m->dev.push_back(d);
    }
    for (int r = 0; r < n_gpus; r++) {
        dnagpu_ctx *c = nullptr;
        const int rc = dnagpu_init(m->dev[r], &c);
        if (rc != DNAGPU_OK) {
            dnagpu_multi_destroy(m);
            return rc;
        }
        m->ctx.push_back(c);
        // the rank's transfer stream, made right behind its context's stream: the runtime hands its hardware queues out
        // round-robin in creation order, and two streams on one queue would not overlap (seen in the one-device rehearsal
        // with eight ranks: the pipelined exchange hid nothing when the streams were made in two batches)
        hipStream_t xs = nullptr;
        if (hipSetDevice(m->dev[r]) != hipSuccess || hipStreamCreateWithFlags(&xs, hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            dnagpu_multi_destroy(m);
            return DNAGPU_ERR_HIP;
        }
        m->xfer.push_back(xs);
    }
    // peer access for the copy transport and for RCCL's direct xGMI paths (failure is not fatal: copies stage)
    for (int a = 0; a < n_gpus; a++)
        for (int b = 0; b < n_gpus; b++)
            if (m->dev[a] != m->dev[b]) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, m->dev[a], m->dev[b]) == hipSuccess && can) {
                    (void)hipSetDevice(m->dev[a]);
                    const hipError_t e = hipDeviceEnablePeerAccess(m->dev[b], 0);
                    if (e != hipSuccess)
                        (void)hipGetLastError();      // already enabled, or not supported
                }
            }
    const bool want_rccl = transport == DNAGPU_MULTI_RCCL || (transport == DNAGPU_MULTI_AUTO && n_gpus > 1 && distinct);
    if (want_rccl) {
        if (!distinct) {
            set_err("RCCL transport needs %d distinct devices", n_gpus);
            dnagpu_multi_destroy(m);
            return DNAGPU_ERR_BAD_ARG;
        }
        if (!m->api.load()) {
            if (transport == DNAGPU_MULTI_RCCL) {
                set_err("librccl.so could not be loaded: %s", dlerror());
                dnagpu_multi_destroy(m);
                return DNAGPU_ERR_HIP;
            }
        } else {
            m->comms.assign((size_t)n_gpus, nullptr);
            const ncclResult_t nr = m->api.CommInitAll(m->comms.data(), n_gpus, m->dev.data());
            if (nr != ncclSuccess) {
                set_err("ncclCommInitAll: %s", m->api.GetErrorString(nr));
                m->comms.clear();
                (void)hipGetLastError();
                if (transport == DNAGPU_MULTI_RCCL) {
                    dnagpu_multi_destroy(m);
                    return DNAGPU_ERR_HIP;
                }
                // DNAGPU_MULTI_AUTO: "RCCL when ... the library loads, else copies" -- a communicator that cannot be made
                // (e.g. another ROCm runtime already in the process) leaves the copy transport
            } else {
                m->rccl = true;
            }
        }
    }
    *out = m;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_multi_size(const dnagpu_multi *m) { return m ? m->n : 0; }
extern "C" dnagpu_ctx *dnagpu_multi_ctx(dnagpu_multi *m, int rank)
{
    return (m && rank >= 0 && rank < m->n) ? m->ctx[(size_t)rank] : nullptr;
}
extern "C" const char *dnagpu_multi_transport(const dnagpu_multi *m) { return !m ? "" : (m->rccl ? "rccl" : "copy"); }
extern "C" const char *dnagpu_multi_exchange_transport(const dnagpu_multi *m) { return !m ? "" : m->last_exchange; }
extern "C" int dnagpu_multi_rccl_ranks(const dnagpu_multi *m) { return (m && m->rccl) ? m->n : 0; }
extern "C" int dnagpu_multi_last_phase_times(dnagpu_multi *m, int rank, dnagpu_phase_times *out)
{
    if (!m || !out || rank < 0 || rank >= m->n)
        return DNAGPU_ERR_BAD_ARG;
    // the record pass's phases (kept by the call: the owner phase starts a new session on the rank's context), then the
    // owner phase's
    dnagpu_phase_times t{};
    if ((size_t)rank < m->rec_phases.size())
        t = m->rec_phases[(size_t)rank];
    const dnagpu_phase_times &o = m->ctx[(size_t)rank]->last_times;
    for (int i = 0; i < o.n && t.n < DNAGPU_MAX_PHASES; i++) {
        t.names[t.n] = o.names[i];
        t.ms[t.n] = o.ms[i];
        t.n++;
    }
    *out = t;
    return DNAGPU_OK;
}
extern "C" int dnagpu_multi_last_times(const dnagpu_multi *m, dnagpu_multi_times *out)
{
    if (!m || !out)
        return DNAGPU_ERR_BAD_ARG;
    *out = m->last;
    return DNAGPU_OK;
}

extern "C" void dnagpu_multi_dna_free(dnagpu_multi *m, dnagpu_multi_dna *d)
{
    if (!d)
        return;
    for (size_t r = 0; r < d->view.size(); r++)
        if (d->view[r])
            dnagpu_dna_free(m ? m->ctx[r] : nullptr, d->view[r]);
    if (m)
        for (size_t r = 0; r < d->full.size(); r++)
            pool_free(m->ctx[r], d->full[r]);
    delete d;
}

// allocates every rank's buffer and wraps it; fill(r, w_lo, w_hi) makes rank r's own chunk resident
template <typename Fill>
static int multi_dna_make(dnagpu_multi *m, u64 n_bases, dnagpu_multi_dna **out, Fill &&fill)
{
    dnagpu_multi_dna *d = new (std::nothrow) dnagpu_multi_dna();
    if (!d)
        return DNAGPU_ERR_OOM;
    d->n_bases = n_bases;
    d->n_words = words_for(n_bases);
    d->per = (d->n_words + (u64)m->n - 1) / (u64)m->n;
    if (d->per == 0)
        d->per = 1;
    int rc = DNAGPU_OK;
    for (int r = 0; r < m->n && rc == DNAGPU_OK; r++) {
        dnagpu_ctx *c = m->ctx[(size_t)r];
        hipError_t e = hipSetDevice(c->device);
        u64 *buf = nullptr;
        if (e == hipSuccess)
            rc = pool_alloc_t(c, (size_t)(d->per * (u64)m->n), &buf);
        if (e != hipSuccess || rc != DNAGPU_OK) {
            if (e != hipSuccess) {
                set_err("hipSetDevice: %s", hipGetErrorString(e));
                rc = DNAGPU_ERR_HIP;
            }
            break;
        }
        d->full.push_back(buf);
        d->view.push_back(nullptr);
        const u64 lo = std::min((u64)r * d->per, d->n_words), hi = std::min((u64)(r + 1) * d->per, d->n_words);
        // gather space behind the last word of the sequence stays zero (never read as bases: n_words bounds every sweep)
        e = hipMemsetAsync(buf + d->n_words, 0, (size_t)(d->per * (u64)m->n - d->n_words) * 8, c->stream);
        if (e == hipSuccess)
            e = fill(r, c, buf, lo, hi);
        if (e != hipSuccess) {
            set_err("multi dna: %s", hipGetErrorString(e));
            rc = DNAGPU_ERR_HIP;
            break;
        }
        rc = dnagpu_dna_wrap(c, buf, d->per * (u64)m->n, n_bases, &d->view[(size_t)r]);
    }
    for (int r = 0; r < m->n && rc == DNAGPU_OK; r++)
        if (hipSetDevice(m->ctx[(size_t)r]->device) != hipSuccess || hipStreamSynchronize(m->ctx[(size_t)r]->stream) != hipSuccess)
            rc = DNAGPU_ERR_HIP;
    if (rc != DNAGPU_OK) {
        dnagpu_multi_dna_free(m, d);
        return rc;
    }
    *out = d;
    return DNAGPU_OK;
}

extern "C" int dnagpu_multi_dna_upload(dnagpu_multi *m, const uint64_t *words, uint64_t n_bases, dnagpu_multi_dna **out)
{
    return guarded([&]() -> int {
    if (!m || !out || (n_bases && !words))
        return DNAGPU_ERR_BAD_ARG;
    return multi_dna_make(m, n_bases, out, [&](int, dnagpu_ctx *c, u64 *buf, u64 lo, u64 hi) -> hipError_t {
        if (hi <= lo)
            return hipSuccess;
        return hipMemcpyAsync(buf + lo, words + lo, (size_t)(hi - lo) * 8, hipMemcpyHostToDevice, c->stream);
    });
    });
}

extern "C" int dnagpu_multi_dna_synth(dnagpu_multi *m, uint64_t seed, uint64_t n_bases, uint64_t motif_len,
                                      dnagpu_multi_dna **out)
{
    return guarded([&]() -> int {
    if (!m || !out)
        return DNAGPU_ERR_BAD_ARG;
    return multi_dna_make(m, n_bases, out, [&](int, dnagpu_ctx *c, u64 *buf, u64 lo, u64 hi) -> hipError_t {
        return launch_synth(buf, lo, hi, n_bases, seed, motif_len, c->stream);
    });
    });
}

extern "C" uint64_t dnagpu_multi_dna_length(const dnagpu_multi_dna *d) { return d ? d->n_bases : 0; }

// a copy between two ranks, queued on `st` (a stream of dst_rank's device): device-to-device when they share a device, a
// peer copy otherwise
static hipError_t rank_copy(const dnagpu_multi *m, int dst_rank, void *to, int src_rank, const void *from, size_t bytes, hipStream_t st)
{
    const int dd = m->dev[(size_t)dst_rank], sd = m->dev[(size_t)src_rank];
    return dd == sd ? hipMemcpyAsync(to, from, bytes, hipMemcpyDeviceToDevice, st) : hipMemcpyPeerAsync(to, dd, from, sd, bytes, st);
}

// Rank r's rows of [first, first + count) and, where they reach into the next chunk, the neighbour's first word (its chunk
// is resident since the upload; gather space on this rank), copied on the rank's stream
static hipError_t rank_rows_with_halo(const dnagpu_multi *m, const dnagpu_multi_dna *d, int r, u64 first, u64 count, RankRows *rows)
{
    *rows = rank_rows(d->n_words, d->per, r, first, count);
    if (!rows->halo)
        return hipSuccess;
    return rank_copy(m, r, d->full[(size_t)r] + rows->w_hi, r + 1, d->full[(size_t)r + 1] + rows->w_hi, 8, m->ctx[(size_t)r]->stream);
}

// Runs job(r) -> its code on every rank, each on its own host thread (MultiPool::run).  The error text is per thread: a
// failing rank's is kept beside its code, and the first failing rank becomes the call's error, "rank R (what): text"
// ("rank R: text" without a `what`).  On any failure every rank's histogram is freed.
static int run_ranks(dnagpu_multi *m, const char *what, const char *threw, dnagpu_hist **hists, const std::function<int(int)> &job)
{
    std::vector<int> rcs((size_t)m->n, DNAGPU_OK);
    std::vector<std::string> errs((size_t)m->n);
    const std::function<void(int)> work = [&](int r) {
        rcs[(size_t)r] = job(r);
        if (rcs[(size_t)r] != DNAGPU_OK)
            errs[(size_t)r] = dnagpu_last_error();
    };
    int rc = m->workers.run(m->n, work);
    if (rc != DNAGPU_OK)
        set_err("%s", threw);
    for (int r = 0; r < m->n && rc == DNAGPU_OK; r++)
        if (rcs[(size_t)r] != DNAGPU_OK) {
            if (what)
                set_err("rank %d (%s): %s", r, what, errs[(size_t)r].c_str());
            else
                set_err("rank %d: %s", r, errs[(size_t)r].c_str());
            rc = rcs[(size_t)r];
        }
    if (rc == DNAGPU_OK)
        return rc;
    for (int r = 0; r < m->n; r++) {
        (void)hipSetDevice(m->ctx[(size_t)r]->device);
        dnagpu_hist_free(m->ctx[(size_t)r], hists[r]);
        hists[r] = nullptr;
    }
    (void)hipSetDevice(m->ctx[0]->device);
    return rc;
}

// every rank's buffer receives the other ranks' chunks, ordered on each rank's own stream
static int multi_gather(dnagpu_multi *m, const dnagpu_multi_dna *d)
{
    if (m->n == 1)
        return DNAGPU_OK;
    const size_t per_bytes = (size_t)d->per * 8;
    if (m->rccl) {
        ncclResult_t nr = m->api.GroupStart();
        for (int r = 0; r < m->n && nr == ncclSuccess; r++)     // in place: send = recv + rank * count
            nr = m->api.AllGather(d->full[(size_t)r] + (u64)r * d->per, d->full[(size_t)r], (size_t)d->per, ncclUint64,
                                  m->comms[(size_t)r], m->ctx[(size_t)r]->stream);
        const ncclResult_t ne = m->api.GroupEnd();
        if (nr != ncclSuccess || ne != ncclSuccess) {
            set_err("ncclAllGather: %s", m->api.GetErrorString(nr != ncclSuccess ? nr : ne));
            return DNAGPU_ERR_HIP;
        }
        return DNAGPU_OK;
    }
    for (int dst = 0; dst < m->n; dst++) {
        dnagpu_ctx *c = m->ctx[(size_t)dst];
        HIP_TRY(hipSetDevice(c->device));
        for (int q = 1; q < m->n; q++) {                          // start at the neighbour: spreads the link load
            const int src = (dst + q) % m->n;
            u64 *to = d->full[(size_t)dst] + (u64)src * d->per;
            const u64 *from = d->full[(size_t)src] + (u64)src * d->per;
            HIP_TRY(rank_copy(m, dst, to, src, from, per_bytes, c->stream));
        }
    }
    return DNAGPU_OK;
}

// rank 0: the summed table -> ascending (key, count) groups, one segment; hists[r > 0] are empty
static int multi_dense_compact(dnagpu_multi *m, const u32 *table, int bits, u64 count, dnagpu_hist **hists)
{
    dnagpu_ctx *c0 = m->ctx[0];
    PoolScope ps(c0);
    const size_t n_bins = (size_t)1 << bits;
    u32 *oc = nullptr;
    u64 *ok = nullptr, *n_out = nullptr;
    HIP_TRY(hipSetDevice(c0->device));
    RC_TRY(ps.alloc(n_bins, &ok));
    RC_TRY(ps.alloc(n_bins, &oc));
    RC_TRY(ps.alloc(1, &n_out));
    HIP_TRY(launch_dense_compact(table, bits, ok, oc, n_out, c0->stream));
    u64 D = 0;
    HIP_TRY(hipMemcpyAsync(&D, n_out, 8, hipMemcpyDeviceToHost, c0->stream));
    HIP_TRY(hipStreamSynchronize(c0->stream));
    std::vector<HistPtr> made((size_t)m->n);
    for (HistPtr &h : made)
        if (!(h = hist_new(0)))
            return DNAGPU_ERR_OOM;
    made[0]->total = count;
    RC_TRY(hist_adopt_one_segment(c0, ps, made[0].get(), ok, oc, D, true));
    for (int r = 0; r < m->n; r++)
        hists[r] = made[(size_t)r].release();
    return DNAGPU_OK;
}

// Short k-mers on N ranks (a sum-reduce of the 4^k table): nothing is gathered.  Rank r counts the
// rows that START in its own chunk into a table of 4^k counters (the k-1 <= 8 bases a row may reach into the next
// chunk are one word, copied from the neighbour), the tables are summed onto rank 0 (ncclReduce, or peer copies and
// adds), and rank 0 compacts: hists[0] holds the whole result in ascending key order, the other ranks' are empty.
static int multi_count_dense(dnagpu_multi *m, const dnagpu_multi_dna *d, int k, u64 first, u64 count, dnagpu_hist **hists)
{
    const int bits = 2 * k;
    const size_t n_bins = (size_t)1 << bits;
    std::vector<u32 *> table((size_t)m->n, nullptr);
    u32 *scratch = nullptr;
    int rc = DNAGPU_OK;
    auto cleanup = [&]() {
        for (int r = 0; r < m->n; r++)
            pool_free(m->ctx[(size_t)r], table[(size_t)r]);
        pool_free(m->ctx[0], scratch);
    };
    for (int r = 0; r < m->n && rc == DNAGPU_OK; r++) {
        dnagpu_ctx *c = m->ctx[(size_t)r];
        hipError_t e = hipSetDevice(c->device);
        if (e == hipSuccess)
            rc = pool_alloc_t(c, n_bins, &table[(size_t)r]);
        if (e == hipSuccess && rc == DNAGPU_OK) {
            RankRows rows;
            e = rank_rows_with_halo(m, d, r, first, count, &rows);
            if (e == hipSuccess)
                e = launch_dense_table(d->full[(size_t)r], d->n_words, rows.row_lo, rows.n(), bits, table[(size_t)r], c->stream);
        }
        if (e != hipSuccess) {
            set_err("dense multi count (rank %d): %s", r, hipGetErrorString(e));
            rc = DNAGPU_ERR_HIP;
        }
    }
    if (rc == DNAGPU_OK && m->n > 1) {
        if (m->rccl) {
            ncclResult_t nr = m->api.GroupStart();
            for (int r = 0; r < m->n && nr == ncclSuccess; r++)
                nr = m->api.Reduce(table[(size_t)r], table[(size_t)r], n_bins, ncclUint32, ncclSum, 0, m->comms[(size_t)r],
                                   m->ctx[(size_t)r]->stream);
            const ncclResult_t ne = m->api.GroupEnd();
            if (nr != ncclSuccess || ne != ncclSuccess) {
                set_err("ncclReduce: %s", m->api.GetErrorString(nr != ncclSuccess ? nr : ne));
                rc = DNAGPU_ERR_HIP;
            }
        } else {
            dnagpu_ctx *c0 = m->ctx[0];
            hipError_t e = hipSuccess;
            for (int r = 1; r < m->n && e == hipSuccess; r++) {       // (the partial table of rank r is complete)
                e = hipSetDevice(m->ctx[(size_t)r]->device);
                if (e == hipSuccess)
                    e = hipStreamSynchronize(m->ctx[(size_t)r]->stream);
            }
            if (e == hipSuccess)
                e = hipSetDevice(c0->device);
            if (e == hipSuccess)
                rc = pool_alloc_t(c0, n_bins, &scratch);
            for (int r = 1; r < m->n && e == hipSuccess && rc == DNAGPU_OK; r++) {
                e = rank_copy(m, 0, scratch, r, table[(size_t)r], n_bins * 4, c0->stream);
                if (e == hipSuccess)
                    e = launch_table_add(table[0], scratch, (u32)n_bins, c0->stream);
            }
            if (e != hipSuccess) {
                set_err("dense multi count (sum): %s", hipGetErrorString(e));
                rc = DNAGPU_ERR_HIP;
            }
        }
    }
    if (rc == DNAGPU_OK)
        rc = multi_dense_compact(m, table[0], bits, count, hists);
    // the other ranks' streams may still hold the reduce: their tables go back to the pools behind it
    for (int r = 1; r < m->n; r++)
        if (hipSetDevice(m->ctx[(size_t)r]->device) == hipSuccess)
            (void)hipStreamSynchronize(m->ctx[(size_t)r]->stream);
    (void)hipSetDevice(m->ctx[0]->device);
    cleanup();
    return rc;
}

extern "C" int dnagpu_count_multi(dnagpu_multi *m, const dnagpu_multi_dna *dna, int k, uint64_t first, uint64_t count,
                                  dnagpu_hist **hists)
{
    return guarded([&]() -> int {
    if (!m || !dna || !hists || (int)dna->view.size() != m->n)
        return DNAGPU_ERR_BAD_ARG;
    for (int r = 0; r < m->n; r++)
        hists[r] = nullptr;
    RC_TRY(check_range(dna->view[0], k, first, count));
    if (dense_pays(count, k)) {
        m->last_exchange = m->n == 1 ? "none" : (m->rccl ? "rccl-reduce" : "peer-copy");
        return multi_count_dense(m, dna, k, first, count, hists);
    }
    m->last_exchange = m->n == 1 ? "none" : (m->rccl ? "rccl-allgather" : "peer-copy");
    RC_TRY(multi_gather(m, dna));
    // one host thread per rank: the level loop of a count reads counters back between levels, so the ranks
    // only run concurrently when each is driven by its own thread (device selection is per thread)
    return run_ranks(m, nullptr, "a rank's count ended in a C++ exception", hists, [&](int r) {
        return dnagpu_count_kmers_owned(m->ctx[(size_t)r], dna->view[(size_t)r], k, first, count, r, m->n, &hists[r]);
    });
    });
}

// ---- the same count without any order promise, for long k-mers (k >= 21): the record exchange from one process.
// Rank r cuts the records of the rows that start in its own chunk (one word of halo from its neighbour), every coarse
// bucket's pieces are pulled by the bucket's owner (peer copies of 16-byte records, 1.8 B per k-mer at k = 31; nothing is
// gathered and no rank sweeps rows of another), and the owner counts them.  The exchange is PIPELINED with the count: an
// owner's buckets are cut into `parts` groups; all copies are queued at once on the owner's transfer stream, group after
// group with an event behind each, and the counting of group g (on the context's stream) waits for event g only -- the
// pieces of group g + 1 arrive while group g is counted.  hists[r] = the groups of rank r's buckets (a histogram of
// `parts` parts): disjoint between ranks, in no key order.

// rehearsal aid: holds a stream for `ticks` of the 100 MHz wall clock (the time a copy of that size would take on a link
// of the emulated bandwidth); one wave, every lane leaves the loop when the clock passes the deadline
__global__ __launch_bounds__(64) void link_delay_kernel(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks)
        __builtin_amdgcn_s_sleep(32);
}

extern "C" int dnagpu_multi_set_option(dnagpu_multi *m, int option, double value)
{
    if (!m)
        return DNAGPU_ERR_BAD_ARG;
    switch (option) {
    case DNAGPU_MULTI_OPT_PARTS:
        if (value < 1 || value > DNAGPU_MULTI_MAX_PARTS)
            return DNAGPU_ERR_BAD_ARG;
        m->parts = (int)value;
        return DNAGPU_OK;
    case DNAGPU_MULTI_OPT_EMULATE_LINK_GBS:
        if (value < 0)
            return DNAGPU_ERR_BAD_ARG;
        m->emulate_gbs = value;
        return DNAGPU_OK;
    case DNAGPU_MULTI_OPT_PROBE_OWNER:
        if (value < -1 || value >= m->n)
            return DNAGPU_ERR_BAD_ARG;
        m->probe_owner = (int)value;
        return DNAGPU_OK;
    case DNAGPU_MULTI_OPT_EXCHANGE_RCCL:
        if (value < 0 || value > 2)
            return DNAGPU_ERR_BAD_ARG;
        if (value > 0 && !m->rccl) {
            set_err("the RCCL record exchange needs the RCCL transport (dnagpu_multi_transport() is \"%s\")", m->rccl ? "rccl" : "copy");
            return DNAGPU_ERR_BAD_ARG;
        }
        m->exchange_rccl = (int)value;
        return DNAGPU_OK;
    }
    return DNAGPU_ERR_BAD_ARG;
}

namespace {
double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
struct EventSet {                               // timing events of one owner, destroyed with the scope
    std::vector<hipEvent_t> ev;
    ~EventSet()
    {
        for (hipEvent_t e : ev)
            (void)hipEventDestroy(e);
    }
    hipError_t make(hipEvent_t *out)
    {
        hipEvent_t e;
        const hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess)
            return r;
        ev.push_back(e);
        *out = e;
        return hipSuccess;
    }
};

// ---- the record exchange as stages: one Exchange per call, one Owner per owner's job, the stages in the order they run

using Clock = std::chrono::steady_clock;

// one dnagpu_count_multi_unordered call
struct Exchange {
    dnagpu_multi *m;
    const dnagpu_multi_dna *dna;
    int k;
    u64 first, count;
    dnagpu_hist **hists;
    int W, P = 1;                                   // ranks; bucket groups per owner
    std::vector<dnagpu_records *> recs;             // per rank: the records of its own rows, grouped by coarse bucket
    std::vector<u64> wgt;                           // per bucket: its records on all ranks
    std::vector<u32> cuts;                          // exchange_cuts: owner o's group p = buckets [cuts[o * P + p], cuts[o * P + p + 1])
    SkGeom g{};
    u32 n_coarse = 0;
    bool via_rccl = false, rccl_self = false;       // pieces travel through ncclSend / ncclRecv; a rank's own pieces too
    std::vector<double> t_rec, t_xfer, t_hidden;    // per rank: record pass (host clock); transfer, and its part beside the count (events)
    std::vector<u64> moved;                         // per owner: bytes received from other ranks

    Exchange(dnagpu_multi *m_, const dnagpu_multi_dna *dna_, int k_, u64 first_, u64 count_, dnagpu_hist **hists_)
        : m(m_), dna(dna_), k(k_), first(first_), count(count_), hists(hists_), W(m_->n), recs((size_t)W, nullptr),
          t_rec((size_t)W, 0.0), t_xfer((size_t)W, 0.0), t_hidden((size_t)W, 0.0), moved((size_t)W, 0)
    {
    }
    ~Exchange()                                     // the records are freed on every exit, an exception's included
    {
        for (int r = 0; r < W; r++) {
            (void)hipSetDevice(m->ctx[(size_t)r]->device);
            dnagpu_records_free(m->ctx[(size_t)r], recs[(size_t)r]);
        }
        (void)hipSetDevice(m->ctx[0]->device);
    }
    u32 group_lo(int o, int p) const { return cuts[(size_t)o * P + p]; }
    u32 group_hi(int o, int p) const { return std::max(cuts[(size_t)o * P + p + 1], group_lo(o, p)); }
    u64 piece_len(int rank, u32 b) const { return recs[(size_t)rank]->off[b + 1] - recs[(size_t)rank]->off[b]; }
    const char *piece(int rank, u32 b) const { return static_cast<const char *>(recs[(size_t)rank]->recs) + recs[(size_t)rank]->off[b] * 16; }
};

// One owner's pulls and counts.  The destructor is the error exit: whatever stage returns early, nothing of this owner's
// buffers is in flight afterwards -- the transfer stream, then the context's stream are waited for before the landing
// buffers the owner still holds go back to the pool.  (A buffer handed to count_sk_received has left bufs[]; after
// owner_finish has waited for both streams there is nothing to wait for.)
struct Owner {
    const int o;
    dnagpu_ctx *const c;
    const hipStream_t xs;                           // the owner's transfer stream; the counting runs on c->stream
    EventSet evs;
    hipEvent_t ready = nullptr, x0 = nullptr, x1 = nullptr, c0 = nullptr;
    std::vector<hipEvent_t> landed;                 // per group: its last piece has arrived
    std::vector<void *> bufs;                       // per group: the landing buffer (null: the group holds no record)
    std::vector<GroupLayout> lay;                   // per group: blen[] / boff[] of its landing buffer
    dnagpu_hist *head = nullptr;                    // hists[o] owns it: freed with the others when a rank fails
    bool drained = false;                           // both streams have been waited for behind everything this owner queued

    Owner(const Exchange &x, int o_)
        : o(o_), c(x.m->ctx[(size_t)o_]), xs(x.m->xfer[(size_t)o_]), landed((size_t)x.P, nullptr), bufs((size_t)x.P, nullptr), lay((size_t)x.P)
    {
    }
    ~Owner()
    {
        if (!drained) {
            (void)hipStreamSynchronize(xs);
            (void)hipStreamSynchronize(c->stream);
        }
        for (void *b : bufs)
            pool_free(c, b);
    }
};
}  // namespace

// a stage's error exit: the text becomes the thread's error (run_ranks reads it there)
static int fail(int rc, const char *text)
{
    set_err("%s", text);
    return rc;
}
static int fail(hipError_t e) { return fail(DNAGPU_ERR_HIP, hipGetErrorString(e)); }

// stage 1, every rank: the records of the rows that start in its own chunk
static int exchange_records(Exchange &x, int r)
{
    const auto t0 = Clock::now();
    dnagpu_ctx *c = x.m->ctx[(size_t)r];
    RankRows rows;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess)
        e = rank_rows_with_halo(x.m, x.dna, r, x.first, x.count, &rows);   // the k-1 <= 31 bases a row reaches into the next chunk
    if (e != hipSuccess)
        return fail(e);
    const int rc = dnagpu_sk_records(c, x.dna->view[(size_t)r], x.k, rows.n() ? rows.row_lo : 0, rows.n(), x.count, &x.recs[(size_t)r]);
    x.m->rec_phases[(size_t)r] = c->last_times;    // (the owner phase starts a new profiling session on this context)
    x.t_rec[(size_t)r] = ms_since(t0);
    return rc;
}

// stage 2, the caller's thread: who owns which buckets, in which groups, and how the pieces travel
static void exchange_plan(Exchange &x)
{
    dnagpu_multi *m = x.m;
    x.g = sk_geometry(m->ctx[0], x.count, x.k);
    x.n_coarse = 1u << x.g.r0bits;
    x.wgt.assign(dnagpu_records_buckets(x.recs[0]), 0);
    for (int r = 0; r < x.W; r++)
        for (u32 b = 0; b < x.wgt.size(); b++)
            x.wgt[b] += x.piece_len(r, b);
    x.P = std::max(1, std::min(m->parts, (int)DNAGPU_MULTI_MAX_PARTS));
    x.cuts = exchange_cuts(x.wgt, x.W, x.P);
    m->last.parts = x.P;
    // How the remote pieces travel.  Default: the owner PULLS every piece with a peer copy on its transfer stream.
    // DNAGPU_MULTI_OPT_EXCHANGE_RCCL: every piece is one ncclSend on its rank's transfer stream and one ncclRecv on its
    // owner's, a group call per bucket group (round p: a rank sends what the other owners' groups p hold of its records
    // and receives its own group p; between two ranks the pieces are issued in ascending bucket order on both sides).
    // Needs every rank driven by its own thread (the ranks' group calls meet each other) and all owners active.
    x.via_rccl = m->exchange_rccl > 0 && m->rccl && !m->workers.serial && m->probe_owner < 0;
    x.rccl_self = x.via_rccl && m->exchange_rccl == 2;
    m->last_exchange = x.via_rccl ? "rccl-sendrecv" : "peer-copy";
}

// Stage 3: everything of an owner that can fail without work in flight -- its histogram, EVERY event, EVERY group's landing
// buffer and the too-large check -- before stage 4 queues the first copy.  An owner that returns from here with an error
// has not touched its transfer stream.
static int owner_setup(const Exchange &x, Owner &ow)
{
    ow.head = hist_new(0, false).release();
    if (!ow.head)
        return fail(DNAGPU_ERR_OOM, "host allocation failed");
    x.hists[ow.o] = ow.head;
    hipError_t e = ow.evs.make(&ow.x0);
    if (e == hipSuccess) e = ow.evs.make(&ow.x1);
    if (e == hipSuccess) e = ow.evs.make(&ow.c0);
    if (e == hipSuccess) e = ow.evs.make(&ow.ready);
    for (int p = 0; p < x.P && e == hipSuccess; p++)
        e = ow.evs.make(&ow.landed[(size_t)p]);
    if (e != hipSuccess)
        return fail(e);
    for (int p = 0; p < x.P; p++) {
        GroupLayout &l = ow.lay[(size_t)p];
        l = group_layout(x.wgt, x.group_lo(ow.o, p), x.group_hi(ow.o, p), x.n_coarse);
        if (l.n_recs > 0xFFFFFFFFull)
            return fail(DNAGPU_ERR_TOO_LARGE, "too many records for one owner");
        if (l.n_recs)
            RC_TRY(pool_alloc(ow.c, (size_t)sk_received_cap(l.blen, x.n_coarse, x.g) * 16, &ow.bufs[(size_t)p]));
    }
    return DNAGPU_OK;
}

// The pieces of the owner's group p in the order they are queued and laid out: bucket ascending; within a bucket the owner's
// own piece first, then round the ranks, (o + q) % W (spreads the link load); empty pieces skipped.  fn(src, b, n_b, to):
// n_b records of rank src's bucket b land at `to`; false from fn ends the walk.
template <typename Fn>
static void for_each_piece(const Exchange &x, const Owner &ow, int p, Fn &&fn)
{
    for (u32 b = x.group_lo(ow.o, p); b < x.group_hi(ow.o, p); b++) {
        u64 at = ow.lay[(size_t)p].boff[b];
        for (int q = 0; q < x.W; q++) {
            const int src = (ow.o + q) % x.W;
            const u64 n_b = x.piece_len(src, b);
            if (!n_b)
                continue;
            if (!fn(src, b, n_b, static_cast<char *>(ow.bufs[(size_t)p]) + at * 16))
                return;
            at += n_b;
        }
    }
}

// stage 4 (copy transport): the owner pulls group p's pieces; in the rehearsal the emulated link's delay follows them
static int owner_pull_group(Exchange &x, Owner &ow, int p)
{
    if (!ow.bufs[(size_t)p])
        return DNAGPU_OK;
    hipError_t e = hipSuccess;
    u64 inbound = 0;
    for_each_piece(x, ow, p, [&](int src, u32 b, u64 n_b, char *to) {
        e = rank_copy(x.m, ow.o, to, src, x.piece(src, b), (size_t)n_b * 16, ow.xs);
        if (src != ow.o)
            inbound += n_b * 16;
        return e == hipSuccess;
    });
    if (e != hipSuccess)
        return fail(e);
    x.moved[(size_t)ow.o] += inbound;
    if (x.m->emulate_gbs > 0 && inbound) {
        // rehearsal on one device: the group's inbound bytes at the emulated rate, on the transfer stream
        const double us = (double)inbound / (x.m->emulate_gbs * 1e3);
        const unsigned long long ticks = (unsigned long long)std::min(us, 50000.0) * 100ull;
        hipLaunchKernelGGL(link_delay_kernel, dim3(1), dim3(64), 0, ow.xs, ticks);
    }
    return DNAGPU_OK;
}

// stage 5 (RCCL transport): one group call -- the sends of this rank's records of every owner's group p, then the
// receives of its own group p
static int owner_rccl_group(Exchange &x, Owner &ow, int p)
{
    const RcclApi &api = x.m->api;
    const ncclComm_t comm = x.m->comms[(size_t)ow.o];
    ncclResult_t nr = api.GroupStart();
    // this rank's records of the other owners' groups p (its own pieces too when asked: one-rank tests)
    for (int q = 0; q < x.W && nr == ncclSuccess; q++) {
        const int dst = (ow.o + q) % x.W;
        if (dst == ow.o && !x.rccl_self)
            continue;
        for (u32 b = x.group_lo(dst, p); b < x.group_hi(dst, p) && nr == ncclSuccess; b++)
            if (const u64 n_b = x.piece_len(ow.o, b))
                nr = api.Send(x.piece(ow.o, b), (size_t)n_b * 2, ncclUint64, dst, comm, ow.xs);
    }
    if (nr == ncclSuccess && ow.bufs[(size_t)p])
        for_each_piece(x, ow, p, [&](int src, u32 b, u64 n_b, char *to) {
            if (src == ow.o && !x.rccl_self) {
                if (hipMemcpyAsync(to, x.piece(src, b), (size_t)n_b * 16, hipMemcpyDeviceToDevice, ow.xs) != hipSuccess)
                    nr = ncclUnhandledCudaError;
            } else {
                nr = api.Recv(to, (size_t)n_b * 2, ncclUint64, src, comm, ow.xs);
                if (src != ow.o)
                    x.moved[(size_t)ow.o] += n_b * 16;
            }
            return nr == ncclSuccess;
        });
    const ncclResult_t ne = api.GroupEnd();
    if (nr != ncclSuccess || ne != ncclSuccess) {
        (void)hipGetLastError();
        return fail(DNAGPU_ERR_HIP, api.GetErrorString(nr != ncclSuccess ? nr : ne));
    }
    return DNAGPU_OK;
}

// stages 4 / 5: all transfers of the owner at once on its transfer stream, group after group, an event behind each group
static int owner_queue_transfers(Exchange &x, Owner &ow)
{
    // The pool orders reuse on the context's stream only (and poisons there when asked to): the transfer stream
    // starts behind everything queued on it so far -- the owner's own record pass included, whose pieces are read
    // from this device; the other ranks' passes were synchronised by dnagpu_sk_records.
    hipError_t e = hipEventRecord(ow.ready, ow.c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ow.xs, ow.ready, 0);
    if (e == hipSuccess) e = hipEventRecord(ow.x0, ow.xs);
    for (int p = 0; p < x.P && e == hipSuccess; p++) {
        RC_TRY(x.via_rccl ? owner_rccl_group(x, ow, p) : owner_pull_group(x, ow, p));
        e = hipEventRecord(ow.landed[(size_t)p], ow.xs);
    }
    if (e == hipSuccess) e = hipEventRecord(ow.x1, ow.xs);
    if (e == hipSuccess) e = hipEventRecord(ow.c0, ow.c->stream);
    return e == hipSuccess ? DNAGPU_OK : fail(e);
}

// stage 6: group p is counted on the context's stream behind its event, into a part of the owner's histogram
static int owner_count_groups(const Exchange &x, Owner &ow)
{
    prof_begin(ow.c);
    for (int p = 0; p < x.P; p++) {
        if (!ow.bufs[(size_t)p])
            continue;
        const hipError_t e = hipStreamWaitEvent(ow.c->stream, ow.landed[(size_t)p], 0);
        if (e != hipSuccess)
            return fail(e);
        HistPtr part = hist_new(0, false);
        if (!part)
            return fail(DNAGPU_ERR_OOM, "host allocation failed");
        void *buf = ow.bufs[(size_t)p];
        ow.bufs[(size_t)p] = nullptr;               // (count_sk_received takes the buffer over)
        const GroupLayout &l = ow.lay[(size_t)p];
        RC_TRY(count_sk_received(ow.c, buf, l.boff, l.blen, x.g, x.k, part.get(), sk_received_cap(l.blen, x.n_coarse, x.g)));
        ow.head->parts.push_back(part.get());
        ow.head->n_distinct += part->n_distinct;
        ow.head->total += part->total;
        ow.head->extent += part->extent ? part->extent : part->n_distinct;
        part.release();                             // (the head owns it now)
    }
    prof_end(ow.c);
    return DNAGPU_OK;
}

// stage 7: both streams drained; the owner's times, and a head of one part becomes a plain histogram
static int owner_finish(Exchange &x, Owner &ow)
{
    hipError_t e = hipStreamSynchronize(ow.xs);
    if (e == hipSuccess) e = hipStreamSynchronize(ow.c->stream);
    if (e != hipSuccess)
        return fail(e);
    ow.drained = true;
    float x_ms = 0, c_at = 0, first_ms = 0;
    (void)hipEventElapsedTime(&x_ms, ow.x0, ow.x1);             // first copy queued -> last piece landed
    (void)hipEventElapsedTime(&c_at, ow.x0, ow.c0);             // ... -> the owner's stream was free to count
    (void)hipEventElapsedTime(&first_ms, ow.x0, ow.landed[0]);
    x.t_xfer[(size_t)ow.o] = x_ms;
    // the counting starts when the first group has landed; what the transfer stream did after that ran beside it
    x.t_hidden[(size_t)ow.o] = std::max(0.0f, x_ms - std::max(first_ms, c_at));
    if (ow.head->parts.size() == 1) {                           // one group: a plain histogram, no head
        x.hists[ow.o] = ow.head->parts[0];
        ow.head->parts.clear();
        dnagpu_hist_free(ow.c, ow.head);                        // (it owns no arrays)
        ow.head = nullptr;
    }
    return DNAGPU_OK;
}

// stages 3 - 7, every owner on its own thread: its buckets' pieces from all ranks, group by group, counted as they land
static int exchange_owner(Exchange &x, int o)
{
    if (x.m->probe_owner >= 0 && o != x.m->probe_owner) {       // rehearsal probe: this owner's buckets are not counted
        x.hists[o] = hist_new(0, false).release();
        return x.hists[o] ? DNAGPU_OK : fail(DNAGPU_ERR_OOM, "host allocation failed");
    }
    const hipError_t e = hipSetDevice(x.m->ctx[(size_t)o]->device);
    if (e != hipSuccess)
        return fail(e);
    Owner ow(x, o);
    RC_TRY(owner_setup(x, ow));
    RC_TRY(owner_queue_transfers(x, ow));
    RC_TRY(owner_count_groups(x, ow));
    return owner_finish(x, ow);
}

// stage 8: the call's times, from the ranks'
static void exchange_times(const Exchange &x, Clock::time_point t_own)
{
    dnagpu_multi_times &t = x.m->last;
    t.records_ms = *std::max_element(x.t_rec.begin(), x.t_rec.end());
    t.exchange_ms = *std::max_element(x.t_xfer.begin(), x.t_xfer.end());
    t.hidden_ms = x.m->probe_owner >= 0 ? x.t_hidden[(size_t)x.m->probe_owner] : *std::min_element(x.t_hidden.begin(), x.t_hidden.end());
    t.count_ms = ms_since(t_own);
    for (u64 b : x.moved)
        t.bytes_moved += b;
}

extern "C" int dnagpu_count_multi_unordered(dnagpu_multi *m, const dnagpu_multi_dna *dna, int k, uint64_t first, uint64_t count,
                                            dnagpu_hist **hists)
{
    return guarded([&]() -> int {
    if (!m || !dna || !hists || (int)dna->view.size() != m->n)
        return DNAGPU_ERR_BAD_ARG;
    for (int r = 0; r < m->n; r++)
        hists[r] = nullptr;
    m->last = dnagpu_multi_times{};
    RC_TRY(check_range(dna->view[0], k, first, count));
    if (k < sk_min_k() || count == 0)
        return dnagpu_count_multi(m, dna, k, first, count, hists);         // (short k-mers: the ordered paths)
    const auto t_call = Clock::now();
    int rc;
    {
        Exchange x(m, dna, k, first, count, hists);
        m->rec_phases.assign((size_t)m->n, dnagpu_phase_times{});
        rc = run_ranks(m, "records", "a rank's record pass ended in a C++ exception", hists, [&](int r) { return exchange_records(x, r); });
        if (rc == DNAGPU_OK) {
            exchange_plan(x);
            const auto t_own = Clock::now();
            rc = run_ranks(m, "count", "an owner's count ended in a C++ exception", hists, [&](int o) { return exchange_owner(x, o); });
            exchange_times(x, t_own);
        }
    }       // (the records are freed here; the histograms were freed by run_ranks if a rank failed)
    m->last.total_ms = ms_since(t_call);
    return rc;
    });
}
