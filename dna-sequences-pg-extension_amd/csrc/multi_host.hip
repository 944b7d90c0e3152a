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
            if (m->dev[(size_t)src] == m->dev[(size_t)dst])
                HIP_TRY(hipMemcpyAsync(to, from, per_bytes, hipMemcpyDeviceToDevice, c->stream));
            else
                HIP_TRY(hipMemcpyPeerAsync(to, m->dev[(size_t)dst], from, m->dev[(size_t)src], per_bytes, c->stream));
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
            const u64 w_lo = std::min((u64)r * d->per, d->n_words), w_hi = std::min((u64)(r + 1) * d->per, d->n_words);
            const u64 row_lo = std::max(first, w_lo * 32), row_hi = std::min(first + count, w_hi * 32);
            if (r + 1 < m->n && w_hi < d->n_words && row_hi > row_lo) {
                // the neighbour's first word (its chunk is resident since the upload; gather space on this rank)
                const int src = r + 1;
                u64 *to = d->full[(size_t)r] + w_hi;
                const u64 *from = d->full[(size_t)src] + w_hi;
                e = m->dev[(size_t)src] == m->dev[(size_t)r]
                        ? hipMemcpyAsync(to, from, 8, hipMemcpyDeviceToDevice, c->stream)
                        : hipMemcpyPeerAsync(to, m->dev[(size_t)r], from, m->dev[(size_t)src], 8, c->stream);
            }
            if (e == hipSuccess)
                e = launch_dense_table(d->full[(size_t)r], d->n_words, row_lo, row_hi > row_lo ? row_hi - row_lo : 0, bits,
                                       table[(size_t)r], c->stream);
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
                e = m->dev[(size_t)r] == m->dev[0]
                        ? hipMemcpyAsync(scratch, table[(size_t)r], n_bins * 4, hipMemcpyDeviceToDevice, c0->stream)
                        : hipMemcpyPeerAsync(scratch, m->dev[0], table[(size_t)r], m->dev[(size_t)r], n_bins * 4, c0->stream);
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
    std::vector<int> rcs((size_t)m->n, DNAGPU_OK);
    std::vector<std::string> errs((size_t)m->n);
    const std::function<void(int)> work = [&](int r) {
        rcs[(size_t)r] = dnagpu_count_kmers_owned(m->ctx[(size_t)r], dna->view[(size_t)r], k, first, count, r, m->n,
                                                 &hists[r]);
        if (rcs[(size_t)r] != DNAGPU_OK)
            errs[(size_t)r] = dnagpu_last_error();                // the error text is per thread
    };
    const int wrc = m->workers.run(m->n, work);
    if (wrc != DNAGPU_OK) {
        set_err("a rank's count ended in a C++ exception");
        for (int q = 0; q < m->n; q++) {
            dnagpu_hist_free(m->ctx[(size_t)q], hists[q]);
            hists[q] = nullptr;
        }
        return wrc;
    }
    for (int r = 0; r < m->n; r++)
        if (rcs[(size_t)r] != DNAGPU_OK) {
            set_err("rank %d: %s", r, errs[(size_t)r].c_str());
            for (int q = 0; q < m->n; q++) {
                dnagpu_hist_free(m->ctx[(size_t)q], hists[q]);
                hists[q] = nullptr;
            }
            return rcs[(size_t)r];
        }
    return DNAGPU_OK;
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
}  // namespace

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
    const auto t_call = std::chrono::steady_clock::now();
    const int W = m->n;
    std::vector<dnagpu_records *> recs((size_t)W, nullptr);
    std::vector<int> rcs((size_t)W, DNAGPU_OK);
    std::vector<std::string> errs((size_t)W);
    std::vector<double> t_rec((size_t)W, 0.0), t_cnt((size_t)W, 0.0), t_xfer((size_t)W, 0.0), t_hidden((size_t)W, 0.0);
    std::vector<u64> moved((size_t)W, 0);
    auto fail = [&](int r, int rc, const char *what) {
        rcs[(size_t)r] = rc;
        errs[(size_t)r] = what;
    };
    // ---- every rank: the records of its own rows
    const std::function<void(int)> cut = [&](int r) {
        const auto t0 = std::chrono::steady_clock::now();
        dnagpu_ctx *c = m->ctx[(size_t)r];
        const u64 w_lo = std::min((u64)r * dna->per, dna->n_words), w_hi = std::min((u64)(r + 1) * dna->per, dna->n_words);
        const u64 row_lo = std::max<u64>(first, w_lo * 32), row_hi = std::min<u64>(first + count, w_hi * 32);
        hipError_t e = hipSetDevice(c->device);
        if (e == hipSuccess && r + 1 < W && w_hi < dna->n_words && row_hi > row_lo) {
            const int src = r + 1;                 // the k-1 <= 31 bases a row reaches into the next chunk: one word
            u64 *to = dna->full[(size_t)r] + w_hi;
            const u64 *from = dna->full[(size_t)src] + w_hi;
            e = m->dev[(size_t)src] == m->dev[(size_t)r] ? hipMemcpyAsync(to, from, 8, hipMemcpyDeviceToDevice, c->stream)
                                                        : hipMemcpyPeerAsync(to, m->dev[(size_t)r], from, m->dev[(size_t)src], 8, c->stream);
        }
        if (e != hipSuccess)
            return fail(r, DNAGPU_ERR_HIP, hipGetErrorString(e));
        rcs[(size_t)r] = dnagpu_sk_records(c, dna->view[(size_t)r], k, row_hi > row_lo ? row_lo : 0, row_hi > row_lo ? row_hi - row_lo : 0,
                                           count, &recs[(size_t)r]);
        if (rcs[(size_t)r] != DNAGPU_OK)
            errs[(size_t)r] = dnagpu_last_error();
        m->rec_phases[(size_t)r] = c->last_times;  // (the owner phase below starts a new profiling session on this context)
        t_rec[(size_t)r] = ms_since(t0);
    };
    m->rec_phases.assign((size_t)W, dnagpu_phase_times{});
    int rc = m->workers.run(W, cut);
    if (rc != DNAGPU_OK)
        set_err("a rank's record pass ended in a C++ exception");
    for (int r = 0; r < W && rc == DNAGPU_OK; r++)
        if (rcs[(size_t)r] != DNAGPU_OK) {
            set_err("rank %d (records): %s", r, errs[(size_t)r].c_str());
            rc = rcs[(size_t)r];
        }
    // ---- every owner: its buckets' pieces from all ranks, group by group, counted as they land
    if (rc == DNAGPU_OK) {
        const SkGeom g = sk_geometry(m->ctx[0], count, k);
        const u32 nb = dnagpu_records_buckets(recs[0]);
        const u32 n_coarse = 1u << g.r0bits;
        // owners: contiguous bucket ranges balanced by the records the buckets hold on all ranks (shard_math.py:
        // bucket_owner_ranges_weighted -- a bucket goes to the side its middle falls on)
        std::vector<u64> wgt(nb, 0);
        u64 wtotal = 0;
        for (int r = 0; r < W; r++)
            for (u32 b = 0; b < nb; b++) {
                wgt[b] += recs[(size_t)r]->off[b + 1] - recs[(size_t)r]->off[b];
                wtotal += recs[(size_t)r]->off[b + 1] - recs[(size_t)r]->off[b];
            }
        // cuts[j] for j = 0 .. W * P: owner o's group p = buckets [cuts[o * P + p], cuts[o * P + p + 1])
        const int P = std::max(1, std::min(m->parts, (int)DNAGPU_MULTI_MAX_PARTS));
        const int WP = W * P;
        std::vector<u32> cuts((size_t)WP + 1, 0);
        cuts[(size_t)WP] = nb;
        if (wtotal == 0) {
            for (int j = 1; j < WP; j++)
                cuts[(size_t)j] = (u32)(((u64)j * nb + (u64)WP - 1) / (u64)WP);
        } else {
            // owners first (the rule the process-per-GPU path uses), then every owner's range into P groups the same way
            std::vector<u32> ocut((size_t)W + 1, 0);
            ocut[(size_t)W] = nb;
            auto split = [&](u32 lo, u32 hi, int ways, u32 *out /* ways + 1 entries, out[0] = lo, out[ways] = hi */) {
                u64 tot = 0;
                for (u32 b = lo; b < hi; b++)
                    tot += wgt[b];
                out[0] = lo;
                out[ways] = hi;
                u64 run = 0;
                u32 b = lo;
                for (int j = 1; j < ways; j++) {
                    const double target = (double)tot * j / ways;
                    while (b < hi && (double)run + (double)wgt[b] / 2 <= target) {
                        run += wgt[b];
                        b++;
                    }
                    out[j] = b;
                }
            };
            split(0, nb, W, ocut.data());
            // An owner's groups grow geometrically (1 : 3 : 9 ...): the first one lands -- and its counting starts --
            // after a small share of the transfer, and every later group is still in flight while a group a third of its
            // size is being counted.
            for (int o = 0; o < W; o++) {
                const u32 lo = ocut[(size_t)o], hi = std::max(ocut[(size_t)o + 1], ocut[(size_t)o]);
                u64 tot = 0;
                for (u32 b = lo; b < hi; b++)
                    tot += wgt[b];
                double wsum = 0, acc = 0, wp = 1;
                for (int p = 0; p < P; p++, wp *= 3)
                    wsum += wp;
                u32 *out = &cuts[(size_t)o * P];
                out[0] = lo;
                u64 run = 0;
                u32 b = lo;
                wp = 1;
                for (int p = 1; p < P; p++, wp *= 3) {
                    acc += wp;
                    const double target = (double)tot * acc / wsum;
                    while (b < hi && (double)run + (double)wgt[b] / 2 <= target) {
                        run += wgt[b];
                        b++;
                    }
                    out[p] = b;
                }
                cuts[(size_t)(o + 1) * P] = hi;
            }
        }
        m->last.parts = P;
        // How the remote pieces travel.  Default: the owner PULLS every piece with a peer copy on its transfer stream.
        // DNAGPU_MULTI_OPT_EXCHANGE_RCCL: every piece is one ncclSend on its rank's transfer stream and one ncclRecv on its
        // owner's, a group call per bucket group (round p: a rank sends what the other owners' groups p hold of its records
        // and receives its own group p; between two ranks the pieces are issued in ascending bucket order on both sides).
        // Needs every rank driven by its own thread (the ranks' group calls meet each other) and all owners active.
        const bool via_rccl = m->exchange_rccl > 0 && m->rccl && !m->workers.serial && m->probe_owner < 0;
        const bool rccl_self = via_rccl && m->exchange_rccl == 2;
        m->last_exchange = via_rccl ? "rccl-sendrecv" : "peer-copy";
        const std::function<void(int)> own = [&](int o) {
            const auto t0 = std::chrono::steady_clock::now();
            dnagpu_ctx *c = m->ctx[(size_t)o];
            if (m->probe_owner >= 0 && o != m->probe_owner) {     // rehearsal probe: this owner's buckets are not counted
                hists[o] = hist_new(0, false).release();
                if (!hists[o])
                    fail(o, DNAGPU_ERR_OOM, "host allocation failed");
                return;
            }
            hipStream_t xs = m->xfer[(size_t)o];
            hipError_t e = hipSetDevice(c->device);
            if (e != hipSuccess)
                return fail(o, DNAGPU_ERR_HIP, hipGetErrorString(e));
            dnagpu_hist *head = hist_new(0, false).release();      // (hists[] owns it: freed with the others when a rank fails)
            if (!head)
                return fail(o, DNAGPU_ERR_OOM, "host allocation failed");
            hists[o] = head;
            EventSet evs;
            hipEvent_t x0 = nullptr, x1 = nullptr, c0 = nullptr;
            std::vector<hipEvent_t> landed((size_t)P, nullptr);
            std::vector<void *> bufs((size_t)P, nullptr);
            std::vector<std::vector<u64>> boffs((size_t)P), blens((size_t)P);
            auto drop = [&](int rc_, const char *what) {          // error exit: nothing of this owner's buffers is in flight afterwards
                (void)hipStreamSynchronize(xs);
                (void)hipStreamSynchronize(c->stream);
                for (void *b : bufs)
                    pool_free(c, b);
                fail(o, rc_, what);
            };
            hipEvent_t ready = nullptr;
            e = evs.make(&x0);
            if (e == hipSuccess) e = evs.make(&x1);
            if (e == hipSuccess) e = evs.make(&c0);
            if (e == hipSuccess) e = evs.make(&ready);
            for (int p = 0; p < P && e == hipSuccess; p++)
                e = evs.make(&landed[(size_t)p]);
            if (e != hipSuccess)
                return drop(DNAGPU_ERR_HIP, hipGetErrorString(e));
            // ---- every group's landing buffer
            for (int p = 0; p < P; p++) {
                const u32 b_lo = cuts[(size_t)o * P + p], b_hi = std::max(cuts[(size_t)o * P + p + 1], b_lo);
                std::vector<u64> &blen = blens[(size_t)p], &boff = boffs[(size_t)p];
                blen.assign(n_coarse, 0);
                boff.assign((size_t)n_coarse + 1, 0);
                for (u32 b = b_lo; b < b_hi; b++)
                    blen[b] = wgt[b];
                for (u32 d = 0; d < n_coarse; d++)
                    boff[d + 1] = boff[d] + blen[d];
                const u64 n_recs = boff[n_coarse];
                if (n_recs > 0xFFFFFFFFull)
                    return drop(DNAGPU_ERR_TOO_LARGE, "too many records for one owner");
                if (n_recs) {
                    const int arc = pool_alloc(c, (size_t)sk_received_cap(blen, n_coarse, g) * 16, &bufs[(size_t)p]);
                    if (arc != DNAGPU_OK)
                        return drop(arc, dnagpu_last_error());
                }
            }
            // The pool orders reuse on the context's stream only (and poisons there when asked to): the transfer stream
            // starts behind everything queued on it so far -- the owner's own record pass included, whose pieces are read
            // from this device; the other ranks' passes were synchronised by dnagpu_sk_records.
            e = hipEventRecord(ready, c->stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(xs, ready, 0);
            if (e == hipSuccess) e = hipEventRecord(x0, xs);
            if (e != hipSuccess)
                return drop(DNAGPU_ERR_HIP, hipGetErrorString(e));
            // ---- all copies, group after group, an event behind each group
            for (int p = 0; p < P; p++) {
                const u32 b_lo = cuts[(size_t)o * P + p], b_hi = std::max(cuts[(size_t)o * P + p + 1], b_lo);
                const std::vector<u64> &boff = boffs[(size_t)p];
                if (via_rccl) {
                    ncclResult_t nr = m->api.GroupStart();
                    // this rank's records of the other owners' groups p (its own pieces too when asked: one-rank tests)
                    const dnagpu_records *mine = recs[(size_t)o];
                    for (int q = 0; q < W && nr == ncclSuccess; q++) {
                        const int dst = (o + q) % W;
                        if (dst == o && !rccl_self)
                            continue;
                        const u32 d_lo = cuts[(size_t)dst * P + p], d_hi = std::max(cuts[(size_t)dst * P + p + 1], d_lo);
                        for (u32 b = d_lo; b < d_hi && nr == ncclSuccess; b++) {
                            const u64 n_b = mine->off[b + 1] - mine->off[b];
                            if (n_b)
                                nr = m->api.Send(static_cast<const char *>(mine->recs) + mine->off[b] * 16, (size_t)n_b * 2, ncclUint64,
                                                 dst, m->comms[(size_t)o], xs);
                        }
                    }
                    for (u32 b = b_lo; b < b_hi && nr == ncclSuccess && bufs[(size_t)p]; b++) {
                        u64 at = boff[b];
                        for (int q = 0; q < W && nr == ncclSuccess; q++) {
                            const int src = (o + q) % W;
                            const dnagpu_records *rr = recs[(size_t)src];
                            const u64 n_b = rr->off[b + 1] - rr->off[b];
                            if (!n_b)
                                continue;
                            char *to = static_cast<char *>(bufs[(size_t)p]) + at * 16;
                            if (src == o && !rccl_self) {
                                if (hipMemcpyAsync(to, static_cast<const char *>(rr->recs) + rr->off[b] * 16, (size_t)n_b * 16,
                                                   hipMemcpyDeviceToDevice, xs) != hipSuccess)
                                    nr = ncclUnhandledCudaError;
                            } else {
                                nr = m->api.Recv(to, (size_t)n_b * 2, ncclUint64, src, m->comms[(size_t)o], xs);
                                if (src != o)
                                    moved[(size_t)o] += n_b * 16;
                            }
                            at += n_b;
                        }
                    }
                    const ncclResult_t ne = m->api.GroupEnd();
                    if (nr != ncclSuccess || ne != ncclSuccess) {
                        (void)hipGetLastError();
                        return drop(DNAGPU_ERR_HIP, m->api.GetErrorString(nr != ncclSuccess ? nr : ne));
                    }
                } else if (bufs[(size_t)p]) {
                    u64 delay_bytes = 0;
                    for (u32 b = b_lo; b < b_hi; b++) {
                        u64 at = boff[b];
                        for (int q = 0; q < W; q++) {
                            const int src = (o + q) % W;             // own pieces first, then round the ranks: spreads the link load
                            const dnagpu_records *rr = recs[(size_t)src];
                            const u64 n_b = rr->off[b + 1] - rr->off[b];
                            if (!n_b)
                                continue;
                            char *to = static_cast<char *>(bufs[(size_t)p]) + at * 16;
                            const char *from = static_cast<const char *>(rr->recs) + rr->off[b] * 16;
                            if (m->dev[(size_t)src] == m->dev[(size_t)o])
                                e = hipMemcpyAsync(to, from, (size_t)n_b * 16, hipMemcpyDeviceToDevice, xs);
                            else
                                e = hipMemcpyPeerAsync(to, m->dev[(size_t)o], from, m->dev[(size_t)src], (size_t)n_b * 16, xs);
                            if (e != hipSuccess)
                                return drop(DNAGPU_ERR_HIP, hipGetErrorString(e));
                            if (src != o) {
                                moved[(size_t)o] += n_b * 16;
                                delay_bytes += n_b * 16;
                            }
                            at += n_b;
                        }
                    }
                    if (m->emulate_gbs > 0 && delay_bytes) {
                        // rehearsal on one device: the group's inbound bytes at the emulated rate, on the transfer stream
                        const double us = (double)delay_bytes / (m->emulate_gbs * 1e3);
                        const unsigned long long ticks = (unsigned long long)std::min(us, 50000.0) * 100ull;
                        hipLaunchKernelGGL(link_delay_kernel, dim3(1), dim3(64), 0, xs, ticks);
                    }
                }
                e = hipEventRecord(landed[(size_t)p], xs);
                if (e != hipSuccess)
                    return drop(DNAGPU_ERR_HIP, hipGetErrorString(e));
            }
            e = hipEventRecord(x1, xs);
            if (e == hipSuccess) e = hipEventRecord(c0, c->stream);
            if (e != hipSuccess)
                return drop(DNAGPU_ERR_HIP, hipGetErrorString(e));
            // ---- count group p behind its event
            prof_begin(c);
            for (int p = 0; p < P; p++) {
                if (!bufs[(size_t)p])
                    continue;
                e = hipStreamWaitEvent(c->stream, landed[(size_t)p], 0);
                if (e != hipSuccess)
                    return drop(DNAGPU_ERR_HIP, hipGetErrorString(e));
                HistPtr part = hist_new(0, false);
                if (!part)
                    return drop(DNAGPU_ERR_OOM, "host allocation failed");
                void *buf = bufs[(size_t)p];
                bufs[(size_t)p] = nullptr;                        // (count_sk_received takes the buffer over)
                const int crc = count_sk_received(c, buf, boffs[(size_t)p], blens[(size_t)p], g, k, part.get(),
                                                  sk_received_cap(blens[(size_t)p], n_coarse, g));
                if (crc != DNAGPU_OK)
                    return drop(crc, dnagpu_last_error());
                head->parts.push_back(part.get());
                head->n_distinct += part->n_distinct;
                head->total += part->total;
                head->extent += part->extent ? part->extent : part->n_distinct;
                part.release();                                   // (the head owns it now)
            }
            prof_end(c);
            e = hipStreamSynchronize(xs);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess)
                return drop(DNAGPU_ERR_HIP, hipGetErrorString(e));
            float x_ms = 0, c_at = 0;
            (void)hipEventElapsedTime(&x_ms, x0, x1);             // first copy queued -> last piece landed
            (void)hipEventElapsedTime(&c_at, x0, c0);             // ... -> the owner's stream was free to count
            t_xfer[(size_t)o] = x_ms;
            // the counting starts when the first group has landed; what the transfer stream did after that ran beside it
            float first_ms = 0;
            (void)hipEventElapsedTime(&first_ms, x0, landed[0]);
            t_hidden[(size_t)o] = std::max(0.0f, x_ms - std::max(first_ms, c_at));
            if (head->parts.size() == 1) {                        // one group: a plain histogram, no head
                dnagpu_hist *only = head->parts[0];
                head->parts.clear();
                dnagpu_hist_free(c, head);                        // (it owns no arrays)
                hists[o] = only;
            }
            t_cnt[(size_t)o] = ms_since(t0);
        };
        const auto t_own = std::chrono::steady_clock::now();
        rc = m->workers.run(W, own);
        if (rc != DNAGPU_OK)
            set_err("an owner's count ended in a C++ exception");
        for (int r = 0; r < W && rc == DNAGPU_OK; r++)
            if (rcs[(size_t)r] != DNAGPU_OK) {
                set_err("rank %d (count): %s", r, errs[(size_t)r].c_str());
                rc = rcs[(size_t)r];
            }
        m->last.records_ms = *std::max_element(t_rec.begin(), t_rec.end());
        m->last.exchange_ms = *std::max_element(t_xfer.begin(), t_xfer.end());
        m->last.hidden_ms = m->probe_owner >= 0 ? t_hidden[(size_t)m->probe_owner] : *std::min_element(t_hidden.begin(), t_hidden.end());
        m->last.count_ms = ms_since(t_own);
        for (int r = 0; r < W; r++)
            m->last.bytes_moved += moved[(size_t)r];
    }
    for (int r = 0; r < W; r++) {
        (void)hipSetDevice(m->ctx[(size_t)r]->device);
        dnagpu_records_free(m->ctx[(size_t)r], recs[(size_t)r]);
        if (rc != DNAGPU_OK) {
            dnagpu_hist_free(m->ctx[(size_t)r], hists[r]);
            hists[r] = nullptr;
        }
    }
    (void)hipSetDevice(m->ctx[0]->device);
    m->last.total_ms = ms_since(t_call);
    return rc;
    });
}

