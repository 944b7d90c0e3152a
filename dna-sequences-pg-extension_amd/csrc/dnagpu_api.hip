// dnagpu_api.hip -- the C-ABI of include/dnagpu.h over the gfx950 kernels.
//
// Host side only: argument checks in the reference's terms (same conditions, same message text as
// the ereport() sites of dna.c), device buffer pool, event timing; the counts are driven from count_host.hip, sk_host.hip
// and multi_host.hip, and host_common.hpp declares what the four files share.
// There is no CPU fallback: without a HIP device every entry point fails with DNAGPU_ERR_NO_DEVICE.
#include "host_common.hpp"

using namespace dnagpu;

// ------------------------------------------------------------------------------------------------
// errors
static thread_local char g_err[512] = "";

void dnagpu::set_err(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

extern "C" const char *dnagpu_strerror(int status)
{
    switch (status) {
    case DNAGPU_OK: return "ok";
    case DNAGPU_ERR_INVALID_K: return "Invalid k value: must be between 1 and 32";             // dna.c:773
    case DNAGPU_ERR_QKMER_LEN_MISMATCH: return "Qkmer pattern and kmer lengths do not match";   // dna.c:1107
    case DNAGPU_ERR_PREFIX_TOO_LONG: return "Prefix length cannot exceed kmer length";         // dna.c:855
    case DNAGPU_ERR_QKMER_INVALID: return "Invalid Qkmer sequence: must contain valid IUPAC nucleotide codes";  // dna.c:916
    case DNAGPU_ERR_BAD_ARG: return "bad argument";
    case DNAGPU_ERR_TOO_LARGE: return "too many k-mers for one call (limit 2^32 - 1)";
    case DNAGPU_ERR_NO_DEVICE: return "no usable HIP device (gfx950 required)";
    case DNAGPU_ERR_OOM: return "out of memory";
    case DNAGPU_ERR_HIP: return "HIP runtime or kernel failure";
    case DNAGPU_ERR_INTERNAL: return "internal error";
    case DNAGPU_ERR_DNA_EMPTY: return "DNA sequence cannot be empty";                         // dna.c:161
    case DNAGPU_ERR_DNA_INVALID_CHAR: return "Invalid character in DNA sequence";              // dna.c:166 (+ ": %c")
    }
    return "unknown status";
}

extern "C" const char *dnagpu_last_error(void) { return g_err; }
extern "C" int dnagpu_abi_version(void) { return DNAGPU_ABI_VERSION; }
extern "C" int dnagpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n > 0 ? n : 0;
}

// ------------------------------------------------------------------------------------------------
// context + device buffer pool
// Up to 32 bytes from the host into device memory as a kernel argument: no staging copy, and no wait for a stack
// variable to be consumed.
struct Poke32 {
    u32 w[8];
};
__global__ void poke_kernel(u32 *dst, Poke32 v, int n_words)
{
    if ((int)threadIdx.x < n_words)
        dst[threadIdx.x] = v.w[threadIdx.x];
}
hipError_t dnagpu::poke(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    Poke32 v;
    memset(&v, 0, sizeof v);
    memcpy(&v, src, bytes <= sizeof v ? bytes : sizeof v);
    hipLaunchKernelGGL(poke_kernel, dim3(1), dim3(8), 0, st, static_cast<u32 *>(dst), v, (int)((bytes + 3) / 4));
    return hipGetLastError();
}

// Small results the host needs between launches (level counters, child lists, totals): copied into the context's pinned
// mailbox and read from there.  A copy into pageable memory (a stack variable, a std::vector) goes through the
// runtime's staging path, which costs tens of microseconds per call -- a count makes about ten of them.  Waits for
// the stream.
// up to 256 bytes go by a one-wave kernel that stores them into the mailbox and then raises a flag word there (system
// scope): the host polls the flag for a few tens of microseconds -- no completion signal, no wake-up: the copy + wait
// of a tiny result costs ~20 us through the runtime and a third of that this way -- and falls back to waiting for the
// stream when the work queued before it takes longer (so a backend does not burn a core through millisecond kernels).
constexpr size_t MAILBOX_FLAG_WORD = MAILBOX_BYTES / 8 - 1;    // the mailbox's last word
__global__ void mailbox_kernel(u64 *mailbox, const u32 *src, int n_words, u64 flag_word, u64 seq)
{
    u32 *dst = reinterpret_cast<u32 *>(mailbox);
    if ((int)threadIdx.x < n_words)
        __hip_atomic_store(&dst[threadIdx.x], src[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        __hip_atomic_store(&mailbox[flag_word], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

int dnagpu::read_back(dnagpu_ctx *ctx, void *host, const void *dev, size_t bytes)
{
    if (bytes == 0)
        return DNAGPU_OK;
    if (bytes <= 256 && (bytes & 3) == 0 && (reinterpret_cast<uintptr_t>(dev) & 3) == 0) {
        const u64 seq = ++ctx->mailbox_seq;
        hipLaunchKernelGGL(mailbox_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->mailbox, static_cast<const u32 *>(dev),
                           (int)(bytes / 4), (u64)MAILBOX_FLAG_WORD, seq);
        HIP_TRY(hipGetLastError());
        volatile u64 *flag = ctx->mailbox + MAILBOX_FLAG_WORD;
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        for (u32 spins = 0;; spins++) {
            if (*flag == seq) {
                seen = true;
                break;
            }
            if ((spins & 63) == 63 &&
                std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() > 60.0)
                break;
        }
        if (!seen)
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (*flag != seq) {
            set_err("mailbox: the result of a read-back did not arrive");
            return DNAGPU_ERR_INTERNAL;
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        memcpy(host, ctx->mailbox, bytes);
        return DNAGPU_OK;
    }
    void *to = bytes <= MAILBOX_BYTES - 8 ? static_cast<void *>(ctx->mailbox) : host;
    HIP_TRY(hipMemcpyAsync(to, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (to != host)
        memcpy(host, to, bytes);
    return DNAGPU_OK;
}

// DNAGPU_DEBUG_POISON_POOL: no work buffer starts out zeroed (fresh hipMalloc memory) or holding a
// previous call's values (a recycled block); both hide reads of data the call never wrote
static int pool_poison(dnagpu_ctx *ctx, void *p, size_t bytes)
{
    if (ctx->debug_flags & DNAGPU_DEBUG_POISON_POOL)
        HIP_TRY(hipMemsetAsync(p, 0xFF, bytes, ctx->stream));
    return DNAGPU_OK;
}

int dnagpu::pool_alloc(dnagpu_ctx *ctx, size_t bytes, void **out)
{
    if (bytes == 0)
        bytes = 256;
    const size_t asked = bytes;
    const bool guard = (ctx->debug_flags & DNAGPU_DEBUG_GUARD_POOL) != 0;
    bytes = (bytes + (guard ? POOL_GUARD : 0) + 255) & ~(size_t)255;
    // size classes (eight per power of two above 64 KB: at most 12.5 % more than asked): a work buffer whose size moves a
    // little from call to call (key ranges of the oversize buckets, sampled regions) finds the block of the call before
    // instead of a hipMalloc -- which costs milliseconds to a second for buffers of gigabytes
    if (bytes > ((size_t)1 << 16)) {
        const size_t g = (size_t)1 << (60 - __builtin_clzll((unsigned long long)bytes));
        bytes = (bytes + g - 1) & ~(g - 1);
    }
    const size_t want = bytes;
    auto finish = [&](PoolBlock &b) -> int {
        b.in_use = true;
        b.guard_at = 0;
        *out = b.ptr;
        RC_TRY(pool_poison(ctx, b.ptr, b.size));
        if (guard) {      // the band sits right behind the bytes asked for (a recycled block may be larger)
            HIP_TRY(hipMemsetAsync(static_cast<char *>(b.ptr) + asked, 0xA5, POOL_GUARD, ctx->stream));
            b.guard_at = asked;
        }
        return DNAGPU_OK;
    };
    int best = -1;
    for (size_t i = 0; i < ctx->pool.size(); i++) {
        PoolBlock &b = ctx->pool[i];
        if (!b.in_use && b.size >= want && b.size <= want * 2 + (1u << 20))
            if (best < 0 || b.size < ctx->pool[best].size)
                best = (int)i;
    }
    if (best >= 0)
        return finish(ctx->pool[best]);
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, want);
#ifdef DNAGPU_STAMPS
    fprintf(stderr, "[pool] hipMalloc %zu bytes (%zu blocks pooled)\n", want, ctx->pool.size());
#endif
    if (e != hipSuccess) {
        // give pooled-but-idle memory back and retry once
        (void)hipGetLastError();
        hipStreamSynchronize(ctx->stream);
        for (size_t i = 0; i < ctx->pool.size();) {
            if (!ctx->pool[i].in_use) {
                hipFree(ctx->pool[i].ptr);
                ctx->pool.erase(ctx->pool.begin() + i);
            } else {
                i++;
            }
        }
        e = hipMalloc(&p, want);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_err("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
        return DNAGPU_ERR_OOM;
    }
    ctx->pool.push_back(PoolBlock{p, want, true});
    return finish(ctx->pool.back());
}

// DNAGPU_DEBUG_GUARD_POOL: every guard band must still hold its pattern (checked with the stream idle)
static int pool_check_guards(dnagpu_ctx *ctx)
{
    if (!(ctx->debug_flags & DNAGPU_DEBUG_GUARD_POOL))
        return DNAGPU_OK;
    unsigned char band[POOL_GUARD];
    for (const PoolBlock &b : ctx->pool) {
        if (!b.guard_at)
            continue;
        HIP_TRY(hipMemcpy(band, static_cast<const char *>(b.ptr) + b.guard_at, POOL_GUARD, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < POOL_GUARD; i++)
            if (band[i] != 0xA5) {
                set_err("pool guard: a kernel wrote %zu bytes past the end of a %zu-byte work buffer (%s)", i + 1, b.guard_at,
                        b.in_use ? "in use" : "already returned");
                return DNAGPU_ERR_INTERNAL;
            }
    }
    return DNAGPU_OK;
}

void dnagpu::pool_free(dnagpu_ctx *ctx, void *p)
{
    if (!p)
        return;
    for (PoolBlock &b : ctx->pool)
        if (b.ptr == p) {
            b.in_use = false;
            return;
        }
}

int dnagpu::side_stream(dnagpu_ctx *ctx, size_t n_events)
{
    if (!ctx->stream2)
        HIP_TRY(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    while (ctx->sync_ev.size() < n_events) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->sync_ev.push_back(e);
    }
    return DNAGPU_OK;
}

HistPtr dnagpu::hist_new(u64 total, bool sorted)
{
    HistPtr h(new (std::nothrow) dnagpu_hist());
    if (h) {
        h->total = total;
        h->sorted = sorted;
    }
    return h;
}

void dnagpu::hist_adopt(PoolScope &ps, dnagpu_hist *h, u64 *keys, u32 *counts, u64 *seg_off, u32 *seg_cnt, u32 n_segs, u64 n_distinct,
                        bool sorted, u64 extent)
{
    h->keys = keys;
    h->counts = counts;
    h->seg_off = seg_off;
    h->seg_cnt = seg_cnt;
    h->n_segs = n_segs;
    h->n_distinct = n_distinct;
    h->sorted = sorted;
    h->extent = extent;
    ps.release(keys);
    ps.release(counts);
    ps.release(seg_off);
    ps.release(seg_cnt);
}

int dnagpu::hist_adopt_one_segment(dnagpu_ctx *ctx, PoolScope &ps, dnagpu_hist *h, u64 *keys, u32 *counts, u64 n_groups, bool sorted)
{
    u64 *dir = nullptr;
    RC_TRY(ps.alloc(2, &dir));
    const u32 words[3] = {0, 0, (u32)n_groups};
    HIP_TRY(poke(dir, words, sizeof words, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    hist_adopt(ps, h, keys, counts, dir, reinterpret_cast<u32 *>(dir + 1), 1, n_groups, sorted, 0);
    return DNAGPU_OK;
}

extern "C" int dnagpu_init(int device, dnagpu_ctx **out_ctx)
{
    return guarded([&]() -> int {
    if (!out_ctx)
        return DNAGPU_ERR_BAD_ARG;
    *out_ctx = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_err("hipGetDeviceCount: %s (%d devices)", hipGetErrorString(e), n);
        return DNAGPU_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_err("device %d out of range (%d devices)", device, n);
        return DNAGPU_ERR_NO_DEVICE;
    }
    HIP_TRY(hipSetDevice(device));
    dnagpu_ctx *ctx = new (std::nothrow) dnagpu_ctx();
    if (!ctx)
        return DNAGPU_ERR_OOM;
    ctx->device = device;
    ctx->profiling = false;
    ctx->last_times.n = 0;
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        set_err("hipStreamCreate: %s", hipGetErrorString(e));
        delete ctx;
        return DNAGPU_ERR_HIP;
    }
    ctx->mailbox = nullptr;
    ctx->debug_flags = 0;
    e = hipHostMalloc(reinterpret_cast<void **>(&ctx->mailbox), MAILBOX_BYTES, hipHostMallocDefault);
    if (e == hipSuccess)
        memset(ctx->mailbox, 0, MAILBOX_BYTES);
    if (e != hipSuccess) {
        set_err("hipHostMalloc: %s", hipGetErrorString(e));
        hipStreamDestroy(ctx->stream);
        delete ctx;
        return DNAGPU_ERR_OOM;
    }
    *out_ctx = ctx;
    return DNAGPU_OK;
    });
}

extern "C" void dnagpu_destroy(dnagpu_ctx *ctx)
{
    if (!ctx)
        return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (ctx->stream2)
        hipStreamSynchronize(ctx->stream2);
    for (PoolBlock &b : ctx->pool)
        hipFree(b.ptr);
    for (hipEvent_t e : ctx->ev)
        hipEventDestroy(e);
    for (hipEvent_t e : ctx->sync_ev)
        hipEventDestroy(e);
    if (ctx->stream2)
        hipStreamDestroy(ctx->stream2);
    hipStreamDestroy(ctx->stream);
    if (ctx->mailbox)
        hipHostFree(ctx->mailbox);
    delete ctx;
}

extern "C" int dnagpu_synchronize(dnagpu_ctx *ctx)
{
    return guarded([&]() -> int {
    if (!ctx)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return pool_check_guards(ctx);                  // (DNAGPU_DEBUG_GUARD_POOL only)
    });
}

extern "C" void *dnagpu_stream(dnagpu_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int dnagpu_trim(dnagpu_ctx *ctx)
{
    return guarded([&]() -> int {
    if (!ctx)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < ctx->pool.size();) {
        if (!ctx->pool[i].in_use) {
            hipFree(ctx->pool[i].ptr);
            ctx->pool.erase(ctx->pool.begin() + i);
        } else {
            i++;
        }
    }
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_device_bytes(dnagpu_ctx *ctx)
{
    uint64_t t = 0;
    if (ctx)
        for (PoolBlock &b : ctx->pool)
            t += b.size;
    return t;
}

extern "C" int dnagpu_buffer_alloc(dnagpu_ctx *ctx, uint64_t bytes, void **dev_ptr)
{
    return guarded([&]() -> int {
    if (!ctx || !dev_ptr)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    return pool_alloc(ctx, (size_t)bytes, dev_ptr);
    });
}

extern "C" void dnagpu_buffer_free(dnagpu_ctx *ctx, void *dev_ptr)
{
    if (ctx)
        pool_free(ctx, dev_ptr);
}

extern "C" int dnagpu_buffer_download(dnagpu_ctx *ctx, const void *dev_ptr, uint64_t bytes, void *host)
{
    return guarded([&]() -> int {
    if (!ctx || (bytes && (!dev_ptr || !host)))
        return DNAGPU_ERR_BAD_ARG;
    if (bytes == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(host, dev_ptr, (size_t)bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_buffer_upload(dnagpu_ctx *ctx, void *dev_ptr, const void *host, uint64_t bytes)
{
    return guarded([&]() -> int {
    if (!ctx || (bytes && (!dev_ptr || !host)))
        return DNAGPU_ERR_BAD_ARG;
    if (bytes == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipMemcpyAsync(dev_ptr, host, (size_t)bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// profiling helpers
void dnagpu::prof_begin(dnagpu_ctx *ctx)
{
    ctx->ev_names.clear();
}

void dnagpu::prof_mark(dnagpu_ctx *ctx, const char *name)
{
    if (!ctx->profiling)
        return;
    size_t i = ctx->ev_names.size();
    if (i >= ctx->ev.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess)
            return;
        ctx->ev.push_back(e);
    }
    hipEventRecord(ctx->ev[i], ctx->stream);
    ctx->ev_names.push_back(name);
}

void dnagpu::prof_end(dnagpu_ctx *ctx)
{
    ctx->last_times.n = 0;
    if (!ctx->profiling || ctx->ev_names.size() < 2)
        return;
    hipStreamSynchronize(ctx->stream);
    int n = 0;
    for (size_t i = 0; i + 1 < ctx->ev_names.size() && n < DNAGPU_MAX_PHASES; i++) {
        float ms = 0;
        hipEventElapsedTime(&ms, ctx->ev[i], ctx->ev[i + 1]);
        // merge intervals that carry the same label (levels beyond the table of names)
        if (n > 0 && ctx->last_times.names[n - 1] == ctx->ev_names[i]) {
            ctx->last_times.ms[n - 1] += ms;
        } else {
            ctx->last_times.names[n] = ctx->ev_names[i];
            ctx->last_times.ms[n] = ms;
            n++;
        }
    }
    ctx->last_times.n = n;
}

extern "C" int dnagpu_set_debug(dnagpu_ctx *ctx, unsigned flags)
{
    if (!ctx)
        return DNAGPU_ERR_BAD_ARG;
    ctx->debug_flags = flags;
    return DNAGPU_OK;
}

extern "C" int dnagpu_last_phase_times(dnagpu_ctx *ctx, dnagpu_phase_times *out)
{
    return guarded([&]() -> int {
    if (!ctx || !out)
        return DNAGPU_ERR_BAD_ARG;
    *out = ctx->last_times;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_set_profiling(dnagpu_ctx *ctx, int enabled)
{
    return guarded([&]() -> int {
    if (!ctx)
        return DNAGPU_ERR_BAD_ARG;
    ctx->profiling = enabled != 0;
    return DNAGPU_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// dna

extern "C" int dnagpu_dna_upload(dnagpu_ctx *ctx, const uint64_t *words, uint64_t n_bases, dnagpu_dna **out)
{
    return guarded([&]() -> int {
    if (!ctx || !out || (!words && n_bases))
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    u64 nw = words_for(n_bases);
    u64 *d = nullptr;
    RC_TRY(pool_alloc_t(ctx, (size_t)std::max<u64>(nw, 1), &d));
    if (nw) {
        hipError_t e = hipMemcpyAsync(d, words, nw * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            pool_free(ctx, d);
            set_err("upload: %s", hipGetErrorString(e));
            return DNAGPU_ERR_HIP;
        }
    }
    dnagpu_dna *h = new (std::nothrow) dnagpu_dna{d, nw, n_bases, true};
    if (!h) {
        pool_free(ctx, d);
        return DNAGPU_ERR_OOM;
    }
    *out = h;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_dna_wrap(dnagpu_ctx *ctx, const uint64_t *dev_words, uint64_t n_words,
                               uint64_t n_bases, dnagpu_dna **out)
{
    return guarded([&]() -> int {
    if (!ctx || !out || (!dev_words && n_bases) || n_words < words_for(n_bases))
        return DNAGPU_ERR_BAD_ARG;
    dnagpu_dna *h = new (std::nothrow) dnagpu_dna{const_cast<u64 *>(dev_words), n_words, n_bases, false};
    if (!h)
        return DNAGPU_ERR_OOM;
    *out = h;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_dna_synth(dnagpu_ctx *ctx, uint64_t seed, uint64_t n_bases, uint64_t motif_len,
                                dnagpu_dna **out)
{
    return guarded([&]() -> int {
    if (!ctx || !out)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    u64 nw = words_for(n_bases);
    u64 *d = nullptr;
    RC_TRY(pool_alloc_t(ctx, (size_t)std::max<u64>(nw, 1), &d));
    hipError_t e = launch_synth(d, 0, nw, n_bases, seed, motif_len, ctx->stream);
    if (e != hipSuccess) {
        pool_free(ctx, d);
        set_err("synth: %s", hipGetErrorString(e));
        return DNAGPU_ERR_HIP;
    }
    dnagpu_dna *h = new (std::nothrow) dnagpu_dna{d, nw, n_bases, true};
    if (!h) {
        pool_free(ctx, d);
        return DNAGPU_ERR_OOM;
    }
    *out = h;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_dna_download(dnagpu_ctx *ctx, const dnagpu_dna *dna, uint64_t *words)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || !words)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    u64 nw = words_for(dna->n_bases);
    if (nw) {
        HIP_TRY(hipMemcpyAsync(words, dna->words, nw * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_dna_pack(dnagpu_ctx *ctx, const char *text, uint64_t n_bases, int text_on_device,
                               dnagpu_dna **out, uint64_t *bad_pos, char *bad_char)
{
    return guarded([&]() -> int {
    if (!ctx || !out)
        return DNAGPU_ERR_BAD_ARG;
    if (n_bases == 0)
        return DNAGPU_ERR_DNA_EMPTY;
    if (!text)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    const unsigned char *dtext = reinterpret_cast<const unsigned char *>(text);
    if (!text_on_device) {
        unsigned char *stage = nullptr;
        RC_TRY(ps.alloc((size_t)n_bases, &stage));
        HIP_TRY(hipMemcpyAsync(stage, text, n_bases, hipMemcpyHostToDevice, ctx->stream));
        dtext = stage;
    }
    u64 nw = words_for(n_bases);
    u64 *words = nullptr, *bad = nullptr;
    RC_TRY(ps.alloc((size_t)nw, &words));
    RC_TRY(ps.alloc(1, &bad));
    HIP_TRY(hipMemsetAsync(bad, 0xff, 8, ctx->stream));
    HIP_TRY(launch_pack(dtext, n_bases, words, bad, ctx->stream));
    u64 hbad = 0;
    HIP_TRY(hipMemcpyAsync(&hbad, bad, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (hbad != ~(u64)0) {
        char c = 0;
        HIP_TRY(hipMemcpy(&c, dtext + hbad, 1, hipMemcpyDeviceToHost));
        if (bad_pos) *bad_pos = hbad;
        if (bad_char) *bad_char = c;
        set_err("Invalid character in DNA sequence: %c", c);
        return DNAGPU_ERR_DNA_INVALID_CHAR;
    }
    dnagpu_dna *h = new (std::nothrow) dnagpu_dna{words, nw, n_bases, true};
    if (!h)
        return DNAGPU_ERR_OOM;
    ps.release(words);
    *out = h;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_dna_unpack(dnagpu_ctx *ctx, const dnagpu_dna *dna, uint64_t first, uint64_t count,
                                 char *out_text, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || (count && !out_text))
        return DNAGPU_ERR_BAD_ARG;
    if (first > dna->n_bases || count > dna->n_bases - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    unsigned char *dt = reinterpret_cast<unsigned char *>(out_text);
    if (!out_on_device)
        RC_TRY(ps.alloc((size_t)count, &dt));
    HIP_TRY(launch_unpack(dna->words, first, count, dt, ctx->stream));
    if (!out_on_device)
        HIP_TRY(hipMemcpyAsync(out_text, dt, count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

// bases [first, first+count) reverse-complemented as a new dna (strand_kernels.hip)
extern "C" int dnagpu_dna_revcomp(dnagpu_ctx *ctx, const dnagpu_dna *dna, uint64_t first, uint64_t count, dnagpu_dna **out)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || !out)
        return DNAGPU_ERR_BAD_ARG;
    if (first > dna->n_bases || count > dna->n_bases - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0)
        return DNAGPU_ERR_DNA_EMPTY;               // (the type has no empty value: dna.c:160-161)
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    const u64 nw = words_for(count);
    u64 *words = nullptr;
    RC_TRY(ps.alloc((size_t)nw, &words));
    HIP_TRY(launch_dna_revcomp(dna->words, first, count, words, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    dnagpu_dna *h = new (std::nothrow) dnagpu_dna{words, nw, count, true};
    if (!h)
        return DNAGPU_ERR_OOM;
    ps.release(words);
    *out = h;
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_dna_wire_size(uint64_t n_bases) { return 8 + 8 * words_for(n_bases); }

extern "C" int dnagpu_dna_from_wire(dnagpu_ctx *ctx, const void *wire, uint64_t wire_bytes, int wire_on_device,
                                    dnagpu_dna **out)
{
    return guarded([&]() -> int {
    if (!ctx || !wire || !out || wire_bytes < 8)
        return DNAGPU_ERR_BAD_ARG;
    if (wire_on_device && (reinterpret_cast<uintptr_t>(wire) & 7))
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    unsigned char hdr[8];
    if (wire_on_device) {
        HIP_TRY(hipMemcpyAsync(hdr, wire, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    } else {
        memcpy(hdr, wire, 8);
    }
    u64 n_bases = 0;
    for (int i = 0; i < 8; i++)
        n_bases = (n_bases << 8) | hdr[i];                  // pq_getmsgint64: network byte order (dna.c:251)
    if (n_bases == 0)
        return DNAGPU_ERR_DNA_EMPTY;
    if (n_bases > ((u64)1 << 40) || wire_bytes != dnagpu_dna_wire_size(n_bases))
        return DNAGPU_ERR_BAD_ARG;
    const u64 nw = words_for(n_bases);
    u64 *d = nullptr;
    RC_TRY(pool_alloc_t(ctx, (size_t)nw, &d));
    int rc = DNAGPU_OK;
    {
        PoolScope ps(ctx);
        const u64 *src = reinterpret_cast<const u64 *>(static_cast<const unsigned char *>(wire) + 8);
        u64 *stage = nullptr;
        hipError_t e = hipSuccess;
        if (!wire_on_device) {
            rc = ps.alloc((size_t)nw, &stage);
            if (rc == DNAGPU_OK)
                e = hipMemcpyAsync(stage, src, nw * 8, hipMemcpyHostToDevice, ctx->stream);
            src = stage;
        }
        const u64 last_mask = (n_bases % 32) ? (((u64)1 << (2 * (n_bases % 32))) - 1) : ~(u64)0;
        if (rc == DNAGPU_OK && e == hipSuccess)
            e = launch_wire_swap(src, d, nw, last_mask, ctx->stream);
        if (rc == DNAGPU_OK && e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream);
        if (rc == DNAGPU_OK && e != hipSuccess) {
            set_err("from_wire: %s", hipGetErrorString(e));
            rc = DNAGPU_ERR_HIP;
        }
    }
    dnagpu_dna *h = rc == DNAGPU_OK ? new (std::nothrow) dnagpu_dna{d, nw, n_bases, true} : nullptr;
    if (!h) {
        pool_free(ctx, d);
        return rc == DNAGPU_OK ? DNAGPU_ERR_OOM : rc;
    }
    *out = h;
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_dna_to_wire(dnagpu_ctx *ctx, const dnagpu_dna *dna, void *wire, uint64_t wire_cap,
                                  int wire_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || !wire || wire_cap < dnagpu_dna_wire_size(dna->n_bases))
        return DNAGPU_ERR_BAD_ARG;
    if (wire_on_device && (reinterpret_cast<uintptr_t>(wire) & 7))
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    unsigned char hdr[8];
    for (int i = 0; i < 8; i++)
        hdr[i] = (unsigned char)(dna->n_bases >> (56 - 8 * i));     // pq_sendint64 (dna.c:282, as an int64)
    const u64 nw = words_for(dna->n_bases);
    PoolScope ps(ctx);
    u64 *dst = reinterpret_cast<u64 *>(static_cast<unsigned char *>(wire) + 8);
    u64 *stage = nullptr;
    if (!wire_on_device) {
        RC_TRY(ps.alloc((size_t)std::max<u64>(nw, 1), &stage));
        memcpy(wire, hdr, 8);
    } else {
        HIP_TRY(hipMemcpyAsync(wire, hdr, 8, hipMemcpyHostToDevice, ctx->stream));
    }
    // (a wrapped view's last word may carry the caller's neighbouring data behind the last base: not part of the image)
    const u64 last_mask = (dna->n_bases % 32) ? (((u64)1 << (2 * (dna->n_bases % 32))) - 1) : ~(u64)0;
    // (the kernel masks what it stores, i.e. the swapped word: swapped mask)
    HIP_TRY(launch_wire_swap(dna->words, wire_on_device ? dst : stage, nw, __builtin_bswap64(last_mask), ctx->stream));
    if (!wire_on_device && nw)
        HIP_TRY(hipMemcpyAsync(dst, stage, nw * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_kmers_to_text(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, int k, char *out_text,
                                    int on_device)
{
    return guarded([&]() -> int {
    if (!ctx || (n && (!keys || !out_text)))
        return DNAGPU_ERR_BAD_ARG;
    if (k <= 0 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    if (n == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    const u64 *dk = keys;
    unsigned char *dt = reinterpret_cast<unsigned char *>(out_text);
    if (!on_device) {
        u64 *tk = nullptr;
        RC_TRY(ps.alloc((size_t)n, &tk));
        RC_TRY(ps.alloc((size_t)n * (k + 1), &dt));
        HIP_TRY(hipMemcpyAsync(tk, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
        dk = tk;
    }
    HIP_TRY(launch_kmers_to_text(dk, n, k, dt, ctx->stream));
    if (!on_device)
        HIP_TRY(hipMemcpyAsync(out_text, dt, n * (u64)(k + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_dna_length(const dnagpu_dna *dna) { return dna ? dna->n_bases : 0; }
extern "C" const uint64_t *dnagpu_dna_device_words(const dnagpu_dna *dna) { return dna ? dna->words : nullptr; }

extern "C" void dnagpu_dna_free(dnagpu_ctx *ctx, dnagpu_dna *dna)
{
    if (!dna)
        return;
    if (dna->owned && ctx)
        pool_free(ctx, dna->words);
    if (ctx && dna->seq_starts)
        pool_free(ctx, dna->seq_starts);
    if (ctx && dna->seq_marks)
        pool_free(ctx, dna->seq_marks);
    delete dna;
}

// ------------------------------------------------------------------------------------------------
// generate_kmers
extern "C" int dnagpu_kmer_count(uint64_t n_bases, int k, uint64_t *n_kmers)
{
    return guarded([&]() -> int {
    if (k <= 0 || k > 32)                      // dna.c:772
        return DNAGPU_ERR_INVALID_K;
    if (!n_kmers)
        return DNAGPU_ERR_BAD_ARG;
    *n_kmers = n_bases >= (u64)k ? n_bases - (u64)k + 1 : 0;   // dna.c:781 without the underflow
    return DNAGPU_OK;
    });
}

int dnagpu::check_range(const dnagpu_dna *dna, int k, u64 first, u64 count)
{
    u64 total = 0;
    RC_TRY(dnagpu_kmer_count(dna->n_bases, k, &total));
    if (first > total || count > total - first) {
        set_err("rows [%llu, +%llu) outside generate_kmers' %llu rows", (unsigned long long)first,
                (unsigned long long)count, (unsigned long long)total);
        return DNAGPU_ERR_BAD_ARG;
    }
    return DNAGPU_OK;
}

extern "C" int dnagpu_generate_kmers(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, uint64_t first,
                                     uint64_t count, uint64_t *out_keys, int out_on_device)
{
    return guarded([&]() -> int {
    if (!ctx || !dna)
        return DNAGPU_ERR_BAD_ARG;
    RC_TRY(check_range(dna, k, first, count));
    if (count == 0)
        return DNAGPU_OK;
    if (!out_keys)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    if (out_on_device) {
        HIP_TRY(launch_extract(dna->words, dna->n_words, first, count, k, out_keys, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DNAGPU_OK;
    }
    // host destination: batches through a device staging buffer, so a PostgreSQL caller can
    // CHECK_FOR_INTERRUPTS between batches by asking for windows itself
    PoolScope ps(ctx);
    const u64 BATCH = (u64)1 << 26;            // 64 Mi keys = 512 MiB staging
    u64 *stage = nullptr;
    RC_TRY(ps.alloc((size_t)std::min(count, BATCH), &stage));
    for (u64 done = 0; done < count; done += BATCH) {
        u64 nb = std::min(BATCH, count - done);
        HIP_TRY(launch_extract(dna->words, dna->n_words, first + done, nb, k, stage, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out_keys + done, stage, nb * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return DNAGPU_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// batched operators
extern "C" int dnagpu_kmer_hash(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, uint32_t *out, int on_device)
{
    return guarded([&]() -> int {
    if (!ctx || (n && (!keys || !out)))
        return DNAGPU_ERR_BAD_ARG;
    if (n == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (on_device) {
        HIP_TRY(launch_hash_batch(keys, n, out, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DNAGPU_OK;
    }
    PoolScope ps(ctx);
    u64 *dk = nullptr;
    u32 *dh = nullptr;
    RC_TRY(ps.alloc((size_t)n, &dk));
    RC_TRY(ps.alloc((size_t)n, &dh));
    HIP_TRY(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_hash_batch(dk, n, dh, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, dh, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_kmer_strand(dnagpu_ctx *ctx, const uint64_t *keys, uint64_t n, int k, int mode, uint64_t *out,
                                  uint8_t *flipped, int on_device)
{
    return guarded([&]() -> int {
    if (mode != DNAGPU_STRAND_REVCOMP && mode != DNAGPU_STRAND_CANONICAL)
        return DNAGPU_ERR_BAD_ARG;
    if (k < 1 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    if (!ctx || (n && (!keys || !out)))
        return DNAGPU_ERR_BAD_ARG;
    if (n == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const int canonical = mode == DNAGPU_STRAND_CANONICAL;
    if (on_device) {
        HIP_TRY(launch_kmer_strand(keys, n, k, canonical, out, flipped, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        return DNAGPU_OK;
    }
    PoolScope ps(ctx);
    u64 *dk = nullptr;
    uint8_t *df = nullptr;
    RC_TRY(ps.alloc((size_t)n, &dk));
    if (flipped)
        RC_TRY(ps.alloc((size_t)n, &df));
    HIP_TRY(hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(launch_kmer_strand(dk, n, k, canonical, dk, df, ctx->stream));      // (in place on the staging copy)
    HIP_TRY(hipStreamSynchronize(ctx->stream));    // (out may be keys: the upload has read them before the download writes)
    HIP_TRY(hipMemcpyAsync(out, dk, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (flipped)
        HIP_TRY(hipMemcpyAsync(flipped, df, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_hist_is_sorted(const dnagpu_hist *h) { return h && h->sorted ? 1 : 0; }

extern "C" uint64_t dnagpu_hist_distinct(const dnagpu_hist *h) { return h ? h->n_distinct : 0; }
extern "C" uint64_t dnagpu_hist_total(const dnagpu_hist *h) { return h ? h->total : 0; }
extern "C" const uint64_t *dnagpu_hist_device_keys(const dnagpu_hist *h) { return h ? h->keys : nullptr; }
extern "C" uint64_t dnagpu_hist_extent(const dnagpu_hist *h) { return !h ? 0 : (h->extent ? h->extent : h->n_distinct); }
extern "C" const uint32_t *dnagpu_hist_device_counts(const dnagpu_hist *h) { return h ? h->counts : nullptr; }
extern "C" uint32_t dnagpu_hist_parts(const dnagpu_hist *h) { return !h ? 0 : (h->parts.empty() ? 1u : (uint32_t)h->parts.size()); }
extern "C" const dnagpu_hist *dnagpu_hist_part(const dnagpu_hist *h, uint32_t i)
{
    if (!h)
        return nullptr;
    if (h->parts.empty())
        return i == 0 ? h : nullptr;
    return i < h->parts.size() ? h->parts[i] : nullptr;
}

// Ascending-key order through the segment directory: groups are gathered on the device into a
// staging window, then copied to the host.
// exclusive scan of the segment sizes, built on the first ordered read of a histogram
static int ensure_seg_pre(dnagpu_ctx *ctx, dnagpu_hist *h)
{
    if (h->seg_pre)
        return DNAGPU_OK;
    PoolScope ps(ctx);
    u32 *pre = nullptr, *tmp = nullptr;
    RC_TRY(ps.alloc((size_t)h->n_segs + 1, &pre));
    RC_TRY(ps.alloc((size_t)scan_tmp_words(h->n_segs), &tmp));
    HIP_TRY(launch_scan_u32(h->seg_cnt, pre, h->n_segs, tmp, pre + h->n_segs, ctx->stream));
    ps.release(pre);
    h->seg_pre = pre;
    return DNAGPU_OK;
}

// groups [first, first + count) of a histogram in its read order = the same range cut along the parts
template <typename F>
static int for_parts(dnagpu_hist *h, u64 first, u64 count, F &&f)
{
    if (h->parts.empty())
        return f(h, first, count, (u64)0);
    u64 base = 0, done = 0;
    for (dnagpu_hist *p : h->parts) {
        const u64 lo = std::max(first, base), hi = std::min(first + count, base + p->n_distinct);
        if (hi > lo) {
            RC_TRY(f(p, lo - base, hi - lo, done));
            done += hi - lo;
        }
        base += p->n_distinct;
    }
    return DNAGPU_OK;
}

extern "C" int dnagpu_hist_sorted_view(dnagpu_ctx *ctx, const dnagpu_hist *h_c, uint64_t first, uint64_t count,
                                       uint64_t *dev_keys, uint64_t *dev_counts)
{
    return guarded([&]() -> int {
    dnagpu_hist *h = const_cast<dnagpu_hist *>(h_c);
    if (!ctx || !h)
        return DNAGPU_ERR_BAD_ARG;
    if (first > h->n_distinct || count > h->n_distinct - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0 || (!dev_keys && !dev_counts))
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    RC_TRY(for_parts(h, first, count, [&](dnagpu_hist *p, u64 pf, u64 pc, u64 out_at) -> int {
        RC_TRY(ensure_seg_pre(ctx, p));
        HIP_TRY(launch_gather_sorted(p->seg_off, p->seg_cnt, p->seg_pre, p->n_segs, pf, pc, p->keys, p->counts,
                                     dev_keys ? dev_keys + out_at : nullptr, dev_counts ? dev_counts + out_at : nullptr, ctx->stream));
        return DNAGPU_OK;
    }));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_hist_download(dnagpu_ctx *ctx, const dnagpu_hist *h_c, uint64_t first, uint64_t count,
                                    uint64_t *keys, uint64_t *counts)
{
    return guarded([&]() -> int {
    dnagpu_hist *h = const_cast<dnagpu_hist *>(h_c);
    if (!ctx || !h)
        return DNAGPU_ERR_BAD_ARG;
    if (first > h->n_distinct || count > h->n_distinct - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0 || (!keys && !counts))
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    const u64 BATCH = (u64)1 << 25;            // 32 Mi groups = 2 x 256 MiB staging
    u64 *sk = nullptr, *sc = nullptr;
    if (keys)
        RC_TRY(ps.alloc((size_t)std::min(count, BATCH), &sk));
    if (counts)
        RC_TRY(ps.alloc((size_t)std::min(count, BATCH), &sc));
    return for_parts(h, first, count, [&](dnagpu_hist *p, u64 pf, u64 pc, u64 out_at) -> int {
        RC_TRY(ensure_seg_pre(ctx, p));
        for (u64 done = 0; done < pc; done += BATCH) {
            u64 nb = std::min(BATCH, pc - done);
            HIP_TRY(launch_gather_sorted(p->seg_off, p->seg_cnt, p->seg_pre, p->n_segs, pf + done, nb, p->keys,
                                         p->counts, sk, sc, ctx->stream));
            if (keys)
                HIP_TRY(hipMemcpyAsync(keys + out_at + done, sk, nb * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (counts)
                HIP_TRY(hipMemcpyAsync(counts + out_at + done, sc, nb * 8, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
        }
        return DNAGPU_OK;
    });
    });
}

extern "C" int dnagpu_hist_summary(dnagpu_ctx *ctx, const dnagpu_hist *h, uint64_t *total, uint64_t *unique,
                                   uint64_t *checksum)
{
    return guarded([&]() -> int {
    if (!ctx || !h)
        return DNAGPU_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    PoolScope ps(ctx);
    u64 *res = nullptr;
    RC_TRY(ps.alloc(4, &res));
    HIP_TRY(hipMemsetAsync(res, 0, 32, ctx->stream));
    if (h->parts.empty()) {
        HIP_TRY(launch_hist_summary(h->keys, h->counts, h->extent ? h->extent : h->n_distinct, res, ctx->stream));
    } else {
        for (const dnagpu_hist *p : h->parts)       // (the kernel adds into res: wrapping sums over all parts)
            HIP_TRY(launch_hist_summary(p->keys, p->counts, p->extent ? p->extent : p->n_distinct, res, ctx->stream));
    }
    u64 r[3] = {0, 0, 0};
    RC_TRY(read_back(ctx, r, res, 24));
    if (total) *total = r[0];
    if (unique) *unique = r[1];
    if (checksum) *checksum = r[2];
    return DNAGPU_OK;
    });
}

// The groups of a and b added up: equal keys' counts are summed.  Both histograms must live on ctx's device; they are
// left as they are.  Histograms counted with different k are refused (BAD_ARG); the result carries their k.
extern "C" int dnagpu_hist_merge(dnagpu_ctx *ctx, const dnagpu_hist *a, const dnagpu_hist *b, dnagpu_hist **out)
{
    return guarded([&]() -> int {
    if (!ctx || !a || !b || !out)
        return DNAGPU_ERR_BAD_ARG;
    *out = nullptr;
    if (a->k && b->k && a->k != b->k)
        return DNAGPU_ERR_BAD_ARG;                 // (keys of different k: equal values would be different k-mers)
    if (a->total + b->total > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;               // (counts are 32-bit in device memory)
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    const u64 n_max = a->n_distinct + b->n_distinct;
    u64 t_slots = 1024;
    while (t_slots < 2 * n_max)
        t_slots <<= 1;
    u64 *tkeys = nullptr, *ok = nullptr;
    u32 *tcnt = nullptr, *oc = nullptr;
    unsigned long long *ctr = nullptr;             // [0] the all-ones key's count, [1] the groups written
    RC_TRY(ps.alloc((size_t)t_slots, &tkeys));
    RC_TRY(ps.alloc((size_t)t_slots, &tcnt));
    RC_TRY(ps.alloc(2, &ctr));
    RC_TRY(ps.alloc((size_t)std::max<u64>(n_max, 1), &ok));
    RC_TRY(ps.alloc((size_t)std::max<u64>(n_max, 1), &oc));
    HIP_TRY(hipMemsetAsync(tkeys, 0xFF, (size_t)t_slots * 8, st));
    HIP_TRY(hipMemsetAsync(tcnt, 0, (size_t)t_slots * 4, st));
    HIP_TRY(hipMemsetAsync(ctr, 0, 16, st));
    for (const dnagpu_hist *h : {a, b}) {
        if (h->parts.empty()) {
            HIP_TRY(launch_merge_insert(h->keys, h->counts, h->extent ? h->extent : h->n_distinct, tkeys, tcnt, t_slots, ctr, st));
        } else {
            for (const dnagpu_hist *p : h->parts)
                HIP_TRY(launch_merge_insert(p->keys, p->counts, p->extent ? p->extent : p->n_distinct, tkeys, tcnt, t_slots, ctr, st));
        }
    }
    HIP_TRY(launch_merge_compact(tkeys, tcnt, t_slots, ok, oc, ctr + 1, st));
    u64 res[2] = {0, 0};
    RC_TRY(read_back(ctx, res, ctr, 16));
    u64 D = res[1];
    if (D > n_max) {
        set_err("hist merge: %llu groups out of %llu", (unsigned long long)D, (unsigned long long)n_max);
        return DNAGPU_ERR_INTERNAL;
    }
    if (D + (res[0] ? 1 : 0) > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    if (res[0]) {                                  // the all-ones key goes last (n_max has room: it was a group of a or b)
        const u64 kk = ~(u64)0;
        const u32 cc = (u32)res[0];
        HIP_TRY(poke(ok + D, &kk, 8, st));
        HIP_TRY(poke(oc + D, &cc, 4, st));
        D++;
    }
    HistPtr h = hist_new(a->total + b->total);
    if (!h)
        return DNAGPU_ERR_OOM;
    // group order: the table's -- unspecified, like every unordered histogram's (one segment, not ascending inside)
    RC_TRY(hist_adopt_one_segment(ctx, ps, h.get(), ok, oc, D, false));
    h->k = a->k ? a->k : b->k;
    *out = h.release();
    return DNAGPU_OK;
    });
}

extern "C" void dnagpu_hist_free(dnagpu_ctx *ctx, dnagpu_hist *h)
{
    if (!h)
        return;
    for (dnagpu_hist *p : h->parts)
        dnagpu_hist_free(ctx, p);
    if (ctx) {
        pool_free(ctx, h->keys);
        pool_free(ctx, h->counts);
        pool_free(ctx, h->seg_off);
        pool_free(ctx, h->seg_cnt);
        pool_free(ctx, h->seg_pre);
    }
    delete h;
}

// ------------------------------------------------------------------------------------------------
// the k-mer accumulator (acc_kernels.hip; DESIGN.md "accumulator"): 2^pbits partitions of ACC_SLOTS 16-byte slots.  A table
// grows -- every partition split on the next hash bits, into new buffers -- when its mean load would pass 3/4; a merge runs
// only when no partition can end above ACC_BOUND.
constexpr int ACC_MIN_BITS = 4;
constexpr u32 ACC_BOUND = ACC_SLOTS / 8 * 7;

// (AccTable and dnagpu_acc: host_common.hpp -- query_host.hip reads the table too)
static void acc_table_free(dnagpu_ctx *ctx, AccTable &t)
{
    pool_free(ctx, t.table);
    pool_free(ctx, t.occ);
    t = AccTable{};
}

static int acc_table_alloc(dnagpu_ctx *ctx, int pbits, AccTable &t)
{
    const u64 P = (u64)1 << pbits;
    t.pbits = pbits;
    int rc = pool_alloc_t(ctx, (size_t)(P * ACC_SLOTS * 2), &t.table);
    if (rc == DNAGPU_OK)
        rc = pool_alloc_t(ctx, (size_t)P, &t.occ);
    if (rc != DNAGPU_OK)
        acc_table_free(ctx, t);
    return rc;
}

// the fewest partitions (at least 2^at_least) that hold `groups` at a mean load of 3/4
static int acc_bits_for(u64 groups, int at_least)
{
    int b = std::max(at_least, ACC_MIN_BITS);
    while (b < 40 && groups > (((u64)ACC_SLOTS << b) / 4) * 3)
        b++;
    return b;
}

static void acc_drop_view(dnagpu_ctx *ctx, dnagpu_acc *acc)
{
    acc->pre.clear();
    pool_free(ctx, acc->dev_pre);
    acc->dev_pre = nullptr;
}

extern "C" int dnagpu_acc_create(dnagpu_ctx *ctx, int k, dnagpu_acc **out)
{
    return guarded([&]() -> int {
    if (k < 1 || k > 32)
        return DNAGPU_ERR_INVALID_K;
    if (!ctx || !out)
        return DNAGPU_ERR_BAD_ARG;
    *out = nullptr;
    dnagpu_acc *a = new (std::nothrow) dnagpu_acc;
    if (!a)
        return DNAGPU_ERR_OOM;
    a->k = k;
    *out = a;
    return DNAGPU_OK;
    });
}

extern "C" uint64_t dnagpu_acc_distinct(const dnagpu_acc *acc) { return acc ? acc->distinct : 0; }
extern "C" uint64_t dnagpu_acc_total(const dnagpu_acc *acc) { return acc ? acc->total : 0; }

// canonical != 0: every key is folded into its canonical form on the way into the bins; the bins, the
// growth and the take-over are the same
static int acc_add(dnagpu_ctx *ctx, dnagpu_acc *acc, const dnagpu_hist *h, int canonical)
{
    return guarded([&]() -> int {
    if (!ctx || !acc || !h)
        return DNAGPU_ERR_BAD_ARG;
    if (h->k && h->k != acc->k)
        return DNAGPU_ERR_BAD_ARG;                 // (keys of different k: equal values would be different k-mers)
    const u64 n_in = h->n_distinct;
    if (n_in == 0)
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PoolScope ps(ctx);
    // the table the add goes into: the accumulator's own, or a larger one in new buffers that takes over on success
    AccTable cur = acc->t;
    struct Fresh {
        dnagpu_ctx *ctx;
        AccTable *t;
        bool on = false;
        ~Fresh()
        {
            if (on)
                acc_table_free(ctx, *t);
        }
    } fresh{ctx, &cur};
    u32 *stats = nullptr;
    RC_TRY(ps.alloc(4, &stats));
    if (acc->distinct == 0) {                      // an empty accumulator is sized from the histogram: no growth later
        const int b = acc_bits_for(n_in, acc->t.pbits);
        if (b != acc->t.pbits) {
            RC_TRY(acc_table_alloc(ctx, b, cur));
            fresh.on = true;
            HIP_TRY(hipMemsetAsync(cur.occ, 0, ((size_t)1 << b) * 4, st));
        }
    }
    const dnagpu_hist *const one[1] = {h};
    const dnagpu_hist *const *parts = h->parts.empty() ? one : h->parts.data();
    const size_t n_parts = h->parts.empty() ? 1 : h->parts.size();
    u64 want_cap = 0, n_new = 0;
    for (int round = 0;; round++) {
        if (round > 64) {
            set_err("accumulator: no table size fits the add");
            return DNAGPU_ERR_INTERNAL;
        }
        const u64 P = (u64)1 << cur.pbits;
        // bins: the expected arrivals per partition + 8 standard deviations (grown to what a round saw if that overflowed)
        const u64 mean = (n_in + P - 1) / P;
        u64 cap = mean + 8 * (u64)std::sqrt((double)mean) + 32;
        cap = std::min<u64>(ACC_SLOTS, (std::max(cap, want_cap) + 31) & ~(u64)31);
        u32 *cursor = nullptr;
        u64 *bins = nullptr;
        RC_TRY(ps.alloc((size_t)P, &cursor));
        RC_TRY(ps.alloc((size_t)(P * cap * 2), &bins));
        HIP_TRY(hipMemsetAsync(cursor, 0, (size_t)P * 4, st));
        HIP_TRY(hipMemsetAsync(stats, 0, 16, st));
        for (size_t i = 0; i < n_parts; i++) {
            const dnagpu_hist *q = parts[i];
            HIP_TRY(launch_acc_bin(q->keys, q->counts, q->extent ? q->extent : q->n_distinct, cur.pbits, cursor, bins, (u32)cap,
                                   canonical ? acc->k : 0, st));
        }
        HIP_TRY(launch_acc_bin_stats(cur.occ, cursor, P, stats, st));
        u32 m[4] = {0, 0, 0, 0};
        RC_TRY(read_back(ctx, m, stats, 8));
        bool commit = m[1] <= cap && m[0] <= ACC_BOUND;
        u64 grow_for = acc->distinct + n_in;       // (an upper bound of the groups after the add)
        if (!commit && m[1] > cap && m[1] <= ACC_SLOTS && m[0] <= ACC_BOUND) {
            want_cap = m[1];                       // a bin overflowed, the table has room: bin again, wider
            ps.free_now(cursor);
            ps.free_now(bins);
            continue;
        }
        if (!commit && m[1] <= cap) {              // dry run: how many arrivals are new keys (the rest only add counts)
            HIP_TRY(hipMemsetAsync(stats, 0, 16, st));
            HIP_TRY(launch_acc_merge(cur.table, cur.occ, P, cursor, bins, (u32)cap, 0, canonical, stats, st));
            RC_TRY(read_back(ctx, m, stats, 16));
            commit = m[0] <= ACC_BOUND;
            grow_for = acc->distinct + ((u64)m[2] | (u64)m[3] << 32);
        }
        if (!commit) {                             // grow: every partition split on the next hash bits, into new buffers
            AccTable next;
            RC_TRY(acc_table_alloc(ctx, acc_bits_for(grow_for, cur.pbits + 1), next));
            hipError_t e = hipMemsetAsync(stats, 0, 16, st);
            if (e == hipSuccess)
                e = launch_acc_split(cur.table, cur.occ, cur.pbits, next.table, next.occ, next.pbits, stats, st);
            int rc = DNAGPU_OK;
            if (e != hipSuccess) {
                set_err("accumulator split: %s", hipGetErrorString(e));
                rc = e == hipErrorOutOfMemory ? DNAGPU_ERR_OOM : DNAGPU_ERR_HIP;
            } else {
                rc = read_back(ctx, m, stats, 8);
                if (rc == DNAGPU_OK && m[1]) {
                    set_err("accumulator split: a partition ran full");
                    rc = DNAGPU_ERR_INTERNAL;
                }
            }
            if (rc != DNAGPU_OK) {
                acc_table_free(ctx, next);
                return rc;
            }
            if (fresh.on)
                acc_table_free(ctx, cur);          // (a grown copy of an earlier round)
            cur = next;
            fresh.on = true;
            want_cap = 0;
            ps.free_now(cursor);
            ps.free_now(bins);
            continue;
        }
        HIP_TRY(hipMemsetAsync(stats, 0, 16, st));
        HIP_TRY(launch_acc_merge(cur.table, cur.occ, P, cursor, bins, (u32)cap, 1, canonical, stats, st));
        RC_TRY(read_back(ctx, m, stats, 16));
        if (m[1]) {
            set_err("accumulator merge: a partition ran full");
            return DNAGPU_ERR_INTERNAL;
        }
        n_new = (u64)m[2] | (u64)m[3] << 32;
        break;
    }
    if (fresh.on) {                                // the new table takes over
        acc_table_free(ctx, acc->t);
        acc->t = cur;
        fresh.on = false;
    }
    acc->distinct += n_new;
    acc->total += h->total;
    acc_drop_view(ctx, acc);
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_acc_add(dnagpu_ctx *ctx, dnagpu_acc *acc, const dnagpu_hist *h) { return acc_add(ctx, acc, h, 0); }
extern "C" int dnagpu_acc_add_canonical(dnagpu_ctx *ctx, dnagpu_acc *acc, const dnagpu_hist *h) { return acc_add(ctx, acc, h, 1); }

extern "C" int dnagpu_acc_summary(dnagpu_ctx *ctx, const dnagpu_acc *acc, uint64_t *total, uint64_t *unique, uint64_t *checksum)
{
    return guarded([&]() -> int {
    if (!ctx || !acc)
        return DNAGPU_ERR_BAD_ARG;
    u64 r[3] = {0, 0, 0};
    if (acc->distinct) {
        HIP_TRY(hipSetDevice(ctx->device));
        PoolScope ps(ctx);
        u64 *res = nullptr;
        RC_TRY(ps.alloc(4, &res));
        HIP_TRY(hipMemsetAsync(res, 0, 32, ctx->stream));
        HIP_TRY(launch_acc_summary(acc->t.table, acc->t.occ, (u64)1 << acc->t.pbits, res, ctx->stream));
        RC_TRY(read_back(ctx, r, res, 24));
    }
    if (total) *total = r[0];
    if (unique) *unique = r[1];
    if (checksum) *checksum = r[2];
    return DNAGPU_OK;
    });
}

extern "C" int dnagpu_acc_download(dnagpu_ctx *ctx, dnagpu_acc *acc, uint64_t first, uint64_t count, uint64_t *keys,
                                   uint64_t *counts)
{
    return guarded([&]() -> int {
    if (!ctx || !acc)
        return DNAGPU_ERR_BAD_ARG;
    if (first > acc->distinct || count > acc->distinct - first)
        return DNAGPU_ERR_BAD_ARG;
    if (count == 0 || (!keys && !counts))
        return DNAGPU_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 P = (u64)1 << acc->t.pbits;
    if (acc->pre.empty()) {                        // the partitions' group offsets: the order of every window until the next add
        std::vector<u32> occ((size_t)P);
        HIP_TRY(hipMemcpyAsync(occ.data(), acc->t.occ, (size_t)P * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<u64> pre((size_t)P + 1);
        pre[0] = 0;
        for (u64 p = 0; p < P; p++)
            pre[p + 1] = pre[p] + occ[p];
        if (pre[P] != acc->distinct) {
            set_err("accumulator: %llu groups in the partitions, %llu counted", (unsigned long long)pre[P],
                    (unsigned long long)acc->distinct);
            return DNAGPU_ERR_INTERNAL;
        }
        u64 *dp = nullptr;
        RC_TRY(pool_alloc_t(ctx, (size_t)P, &dp));
        hipError_t e = hipMemcpyAsync(dp, pre.data(), (size_t)P * 8, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            pool_free(ctx, dp);
            set_err("accumulator download: %s", hipGetErrorString(e));
            return DNAGPU_ERR_HIP;
        }
        acc->pre.swap(pre);
        acc->dev_pre = dp;
    }
    PoolScope ps(ctx);
    const u64 BATCH = (u64)1 << 25;
    u64 *sk = nullptr, *sc = nullptr;
    if (keys)
        RC_TRY(ps.alloc((size_t)std::min(count, BATCH), &sk));
    if (counts)
        RC_TRY(ps.alloc((size_t)std::min(count, BATCH), &sc));
    for (u64 done = 0; done < count; done += BATCH) {
        const u64 nb = std::min(BATCH, count - done), f = first + done;
        // partitions [p_lo, p_hi) hold groups [f, f + nb): pre[p_lo] <= f < pre[p_lo + 1], pre[p_hi] >= f + nb
        const u64 p_lo = (u64)(std::upper_bound(acc->pre.begin(), acc->pre.end(), f) - acc->pre.begin()) - 1;
        const u64 p_hi = (u64)(std::lower_bound(acc->pre.begin(), acc->pre.end(), f + nb) - acc->pre.begin());
        HIP_TRY(launch_acc_gather(acc->t.table, acc->t.occ, acc->dev_pre, p_lo, p_hi - p_lo, f, nb, sk, sc, st));
        if (keys)
            HIP_TRY(hipMemcpyAsync(keys + done, sk, nb * 8, hipMemcpyDeviceToHost, st));
        if (counts)
            HIP_TRY(hipMemcpyAsync(counts + done, sc, nb * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return DNAGPU_OK;
    });
}

extern "C" void dnagpu_acc_free(dnagpu_ctx *ctx, dnagpu_acc *acc)
{
    if (!acc)
        return;
    if (ctx) {
        acc_table_free(ctx, acc->t);
        pool_free(ctx, acc->dev_pre);
    }
    delete acc;
}

// ------------------------------------------------------------------------------------------------
// multi-GPU step 1: one forced level over the dna root, children grouped by owner
extern "C" int dnagpu_partition_kmers(dnagpu_ctx *ctx, const dnagpu_dna *dna, int k, uint64_t first,
                                      uint64_t count, int n_owners, uint64_t **dev_keys,
                                      uint64_t *owner_offsets)
{
    return guarded([&]() -> int {
    if (!ctx || !dna || !dev_keys || !owner_offsets || n_owners < 1 || n_owners > (1 << MAX_SPLIT_BITS))
        return DNAGPU_ERR_BAD_ARG;
    *dev_keys = nullptr;
    RC_TRY(check_range(dna, k, first, count));
    const int bits = std::min(2 * k, MAX_SPLIT_BITS);
    if (2 * k == bits) {
        // the forced level would be terminal: nothing is scattered (children carry key = prefix, count = len); expanding
        // them is not needed by any caller today: k <= 5 counts run on one GPU.  Refused before any device work
        set_err("partition: k too small to shard (2k <= %d bits)", MAX_SPLIT_BITS);
        return DNAGPU_ERR_BAD_ARG;
    }
    if (count > 0xFFFFFFFFull)
        return DNAGPU_ERR_TOO_LARGE;
    HIP_TRY(hipSetDevice(ctx->device));
    for (int o = 0; o <= n_owners; o++)
        owner_offsets[o] = 0;
    if (count == 0)
        return DNAGPU_OK;
    const u32 R = 1u << bits;
    prof_begin(ctx);
    PoolScope ps(ctx);
    TreeResult tr;
    RC_TRY(run_tree(ctx, ps, dna, first, count, k, nullptr, bits, &tr));
    if (tr.n_nodes != R) {
        set_err("partition: expected %u children, got %u", R, tr.n_nodes);
        return DNAGPU_ERR_INTERNAL;
    }
    std::vector<Node> kids(R);
    HIP_TRY(hipMemcpyAsync(kids.data(), tr.nodes, (size_t)R * sizeof(Node), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // owner o owns digits d with (d * n_owners) >> bits == o: first digit = ceil(o * R / n_owners)
    for (int o = 0; o <= n_owners; o++) {
        u64 d0 = ((u64)o * R + n_owners - 1) / n_owners;
        owner_offsets[o] = d0 >= R ? count : kids[d0].start;
    }
    ps.release(tr.buf0);
    *dev_keys = tr.buf0;
    prof_end(ctx);
    return DNAGPU_OK;
    });
}

