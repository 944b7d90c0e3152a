// sk_tail_kernels.hip -- the tail of the super-k-mer engine (sk_device.hpp; the host's count_sk_tail): what becomes of the
// final buckets.  The selection sorts them into small, big and over (sk_select_*, sk_over_*); a small bucket is counted from
// its records (sk_count_clean, which tests records before k-mers and takes every small bucket first, then sk_count, an LDS
// hash table of k-mers, for what that leaves); an over bucket, like a heavy mid bucket, leaves the record path and is
// expanded to keys (sk_slice_*, sk_expand_flat, sk_unmix, sk_take_heavy, sk_heavy_finals).  The big buckets' kernels
// (sk_count_big) are in sk_level0_kernels.hip: see the note there.
//   sk_expand_flat shares this file with sk_count for the same reason: alone, with calls of funnel() that all have a small
//   shift, the compiler gives it other instructions (profiles/refactor_sk_kernels.md).
#include "sk_device.hpp"

namespace dnagpu {

// ------------------------------------------------------------------------------------------------
// selection of the final buckets.  class 1 "small": sk_count takes it (k-mers, records and quads within its stage); class 2
// "big": more than twice sk_count's k-mers and up to big_limit, tried by sk_count_big; class 3 "over": expanded to keys
// for the ordinary levels.
__device__ __forceinline__ u32 sk_bucket_class(const Node &nd, u32 cap, u32 big_limit)
{
    const u32 km = nd.child_base;
    if (km == 0)
        return 0u;
    if (km <= cap && nd.len <= (u32)SKC_MAXREC && nd.chunk_base <= (u32)SKC_MAXQ)
        return 1u;
    // (buckets just over sk_count's stage -- the tail of the size distribution of non-repetitive sequence, mostly distinct
    // keys -- are cheaper through the expansion: 0.55 against 0.8 ms at 3 Gbase uniform)
    return km > 2 * cap && km <= big_limit ? 2u : 3u;
}

// flags (to be scanned in place) and the k-mers that take output slots (small and big buckets: k_range) / key slots (over)
// f_over3 / k_over3: what sk_over_flags writes when there is no big bucket -- class 3 alone -- so that the selection of the
// over buckets needs no sweep and no wait of its own then
__global__ __launch_bounds__(256) void sk_select_flags_kernel(const Node *__restrict__ fin, u32 n_fin, u32 cap, u32 big_limit,
                                                              u32 *__restrict__ f_small, u32 *__restrict__ f_big,
                                                              u32 *__restrict__ k_range, u32 *__restrict__ k_big,
                                                              u32 *__restrict__ f_over3, u32 *__restrict__ k_over3)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_fin)
        return;
    const u32 c = sk_bucket_class(fin[i], cap, big_limit);
    f_small[i] = c == 1u ? 1u : 0u;
    f_big[i] = c == 2u ? 1u : 0u;
    k_range[i] = c == 1u || c == 2u ? fin[i].child_base : 0u;
    k_big[i] = c == 2u ? fin[i].child_base : 0u;
    f_over3[i] = c == 3u ? 1u : 0u;
    k_over3[i] = c == 3u ? fin[i].child_base : 0u;
}

__global__ __launch_bounds__(256) void sk_select_lists_kernel(const Node *__restrict__ fin, u32 n_fin, u32 cap, u32 big_limit,
                                                              const u32 *__restrict__ p_small, const u32 *__restrict__ p_big,
                                                              const u32 *__restrict__ kb_range, u32 *__restrict__ list_small,
                                                              u32 *__restrict__ off_small, u32 *__restrict__ list_big,
                                                              u32 *__restrict__ off_big)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_fin)
        return;
    const u32 c = sk_bucket_class(fin[i], cap, big_limit);
    if (c == 1u) {
        list_small[p_small[i]] = i;
        off_small[p_small[i]] = kb_range[i];
    } else if (c == 2u) {
        list_big[p_big[i]] = i;
        off_big[p_big[i]] = kb_range[i];
    }
}

// the buckets that go through the expansion: class 3, and the big ones sk_count_big gave up on
__global__ __launch_bounds__(256) void sk_over_flags_kernel(const Node *__restrict__ fin, u32 n_fin, u32 cap, u32 big_limit,
                                                            const u32 *__restrict__ p_big, const u32 *__restrict__ big_status,
                                                            u32 *__restrict__ f_over, u32 *__restrict__ k_over)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_fin)
        return;
    const u32 c = sk_bucket_class(fin[i], cap, big_limit);
    const bool over = c == 3u || (c == 2u && big_status[p_big[i]] != 0);
    f_over[i] = over ? 1u : 0u;
    k_over[i] = over ? fin[i].child_base : 0u;
}

__global__ __launch_bounds__(256) void sk_over_list_kernel(const Node *__restrict__ fin, u32 n_fin, const u32 *__restrict__ f_raw,
                                                           const u32 *__restrict__ p_over, const u32 *__restrict__ kb_over,
                                                           Node *__restrict__ over_nodes, u32 *__restrict__ over_kbase)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_fin || !f_raw[i])
        return;
    over_nodes[p_over[i]] = fin[i];
    over_kbase[p_over[i]] = kb_over[i];
}

hipError_t launch_sk_select_flags(const Node *fin, u32 n_fin, u32 cap, u32 big_limit, u32 *f_small, u32 *f_big, u32 *k_range,
                                  u32 *k_big, u32 *f_over3, u32 *k_over3, hipStream_t s)
{
    if (n_fin == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_select_flags_kernel, dim3((n_fin + 255) / 256), dim3(256), 0, s, fin, n_fin, cap, big_limit, f_small, f_big,
                       k_range, k_big, f_over3, k_over3);
    return hipGetLastError();
}

hipError_t launch_sk_select_lists(const Node *fin, u32 n_fin, u32 cap, u32 big_limit, const u32 *p_small, const u32 *p_big,
                                  const u32 *kb_range, u32 *list_small, u32 *off_small, u32 *list_big, u32 *off_big, hipStream_t s)
{
    if (n_fin == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_select_lists_kernel, dim3((n_fin + 255) / 256), dim3(256), 0, s, fin, n_fin, cap, big_limit, p_small, p_big,
                       kb_range, list_small, off_small, list_big, off_big);
    return hipGetLastError();
}

hipError_t launch_sk_over_flags(const Node *fin, u32 n_fin, u32 cap, u32 big_limit, const u32 *p_big, const u32 *big_status,
                                u32 *f_over, u32 *k_over, hipStream_t s)
{
    if (n_fin == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_over_flags_kernel, dim3((n_fin + 255) / 256), dim3(256), 0, s, fin, n_fin, cap, big_limit, p_big, big_status,
                       f_over, k_over);
    return hipGetLastError();
}

hipError_t launch_sk_over_list(const Node *fin, u32 n_fin, const u32 *f_raw, const u32 *p_over, const u32 *kb_over, Node *over_nodes,
                               u32 *over_kbase, hipStream_t s)
{
    if (n_fin == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_over_list_kernel, dim3((n_fin + 255) / 256), dim3(256), 0, s, fin, n_fin, f_raw, p_over, kb_over, over_nodes,
                       over_kbase);
    return hipGetLastError();
}

int sk_count_cap() { return 4096; }              // distinct keys of a bucket <= its k-mers <= half the 8128-slot table

// ------------------------------------------------------------------------------------------------
// sk_count: the leaves of the super-k-mer engine for the buckets that may hold COPIES (round 4: sk_count_clean below takes
// every small bucket first and leaves these).  A final bucket of at most sk_count_cap() k-mers in at most
// SKC_MAXREC records is counted straight from its records in the workgroup's LDS hash table: linear probing over
// four-byte slots claimed by a 32-bit compare-and-swap, a slot holding 19 bits of fingerprint and the 12-bit id of the
// k-mer that claimed it; a probe that meets its own fingerprint re-derives the claimant's key from the staged records and
// compares in full (a copy is counted in a 16-bit counter at the claimant's id).  The keys a thread was first to insert
// stay in its registers and leave, with their counts, one bucket later; a bucket's output range is the exclusive scan of
// the buckets' k-mer counts -- no cursor.  No key of such a bucket ever reaches HBM as a key.
//   Work split: a record's k-mers are cut into groups of SKC_KPT ("quads"); a prefix sum over the records' quad counts
//   gives every quad a thread, and every record writes its quads' owner entries itself -- no search.  Records and
//   owner table live in LDS, so that nothing between two barriers waits for global memory: the next bucket's records
//   are requested a whole bucket ahead.
//   What bounds it (PMC of three variants, round 3): the time follows the kernel's VALU + SALU instruction count
//   (9.3 G wave instructions at 3 Gbase: VALU issue 77 % busy, the CU's scalar unit 47 %), not the LDS (23 % busy).
//   Measured and dropped: the quad's four first probes issued back to back (more registers live, a spill); eight k-mers
//   per thread at 512 threads (half the waves); a binary search over the prefix instead of the owner table; branch-free
//   probe loops that keep finished lanes probing a private word (more VALU than the SALU they save: 12.7 vs 12.1 ms);
//   a per-lane `claimed` flag as a bool (it lives in scalar registers: +44 % SALU, 13.8 ms).
// Other buckets (flagged by the host's selection) are expanded to keys and counted by the ordinary levels.
constexpr int SKC_SLOTS = 236 * 64;              // 15104 four-byte slots (load 0.2 at 3000 keys): with the tables below 79.0 KiB, two workgroups per CU

__global__ __launch_bounds__(SKC_NT, 8) void sk_count_kernel(const Node *__restrict__ fin, const u32 *__restrict__ list,
                                                             const u32 *__restrict__ list_off, u32 n_list_arg,
                                                             const u32 *__restrict__ n_list_dev /* or null */,
                                                             const ull2_t *__restrict__ recs, int k,
                                                             unsigned long long *__restrict__ n_groups,
                                                             u64 *__restrict__ seg_off, u32 *__restrict__ seg_cnt,
                                                             u64 *__restrict__ out_keys, u32 *__restrict__ out_counts, int dbg)
{
    constexpr int WAVES = SKC_NT / 64;
    constexpr int RWAVES = SKC_MAXREC / 64;        // waves that hold records
    // A slot holds 19 bits of fingerprint (under a clear top bit: no word equals the all-ones of a free slot) and the
    // 12-bit id of the k-mer that claimed it (thread << 2 | position in its quad) -- four bytes instead of the key's
    // eight, so the same LDS gives twice the slots and probe chains half as long.  An insert that meets its own
    // fingerprint re-derives the claimant's key from the staged records (owner table -> record -> shift) and compares in
    // full: equal = a copy, counted at the claimant's id; different = a fingerprint collision (one comparison in 2^19),
    // which just probes on.  No key value is reserved.
    __shared__ __attribute__((aligned(16))) u32 tab[SKC_SLOTS];
    __shared__ __attribute__((aligned(16))) u32 cop2[SKC_NT * SKC_KPT / 2];    // copies per claimant id, 16-bit halves
    unsigned short *cop16 = reinterpret_cast<unsigned short *>(cop2);
    __shared__ __attribute__((aligned(16))) ull2_t lrec[SKC_MAXREC];
    __shared__ unsigned short ownq[SKC_MAXQ];      // quad -> record | first k-mer / SKC_KPT << 9
    __shared__ u32 wclaim[2][WAVES], wq[RWAVES];
    __shared__ u32 copy_seen[2];
    int tid = threadIdx.x;
    int lane = tid & 63, wave = tid >> 6;
    const u32 n_list = n_list_dev ? *n_list_dev : n_list_arg;      // (the buckets sk_count_clean left: counted on the device)
    u32 lq = blockIdx.x;
    if (lq >= n_list)
        return;
    for (int q = tid; q < SKC_SLOTS; q += SKC_NT)
        tab[q] = SKC_FREE;
    for (int q = tid; q < SKC_NT * SKC_KPT / 2; q += SKC_NT)
        cop2[q] = 0;
    if (tid < 2)
        copy_seen[tid] = 0;
    const u64 kmask = kmer_mask(k);
    u32 li = list[lq];
    u32 off = list_off[lq];                        // the bucket's output range is [off, off + its k-mers): the exclusive scan of
    Node nd = fin[li];                             // the buckets' k-mer counts, so no cursor is involved
    ull2_t myrec;                                  // record tid of the bucket (threads 0 .. SKC_MAXREC-1)
    myrec.x = myrec.y = 0;
    if ((u32)tid < nd.len)
        myrec = recs[(u64)nd.start + tid];

    // What a thread keeps of a bucket until its output range has arrived: the keys of its quad whose slots it claimed,
    // their counts, its wave's offset.
    constexpr int KEEP = SKC_KPT;
    u32 pkl[KEEP], pkh[KEEP];
    u32 pc[KEEP];
    u32 p_mask = 0, p_before = 0, p_groups = 0, p_li = 0, p_off = 0, p_kmers = 0;
    bool have_prev = false, p_copy = false;
    u64 my_groups = 0;                             // (thread 0: groups of all this workgroup's buckets)
    int par = 0;

    auto emit_prev = [&]() {
        // every wave's claimed keys go out position by position: lanes that claimed their q-th key write one
        // contiguous run per store instruction (wave-uniform base pointers, 32-bit offsets)
        const u64 obase = p_off;
        u64 *ok = out_keys + obase;
        u32 *oc = out_counts + obase;
        u32 run = p_before;
#pragma unroll
        for (int q = 0; q < KEEP; q++) {
            const bool mine = (p_mask >> q) & 1u;
            const u64 b = __ballot(mine);
            if (mine && !SK_DBG(64)) {
                const u32 o = run + __builtin_amdgcn_mbcnt_hi((u32)(b >> 32), __builtin_amdgcn_mbcnt_lo((u32)b, 0u));
                ok[o] = ((u64)pkh[q] << 32) | pkl[q];
                oc[o] = pc[q];
            }
            run += (u32)__popcll(b);
        }
        if (p_copy)                                // a bucket that held copies: the rest of its range is count-0 padding
            for (u32 i = p_groups + (u32)tid; i < p_kmers; i += SKC_NT)
                oc[i] = 0;
        if (tid == 0) {
            seg_off[p_li] = obase;
            seg_cnt[p_li] = p_groups;
        }
    };

    // Two barriers per bucket.  The bucket's records and owner table are staged (registers -> LDS) right behind the
    // previous bucket's barrier B, from records requested a bucket earlier and a quad prefix the record waves computed
    // at the end of the previous insert phase; descriptors run two buckets ahead.
    const u32 step = gridDim.x;
    u32 n_quads = 0;
    {   // the first bucket: staged here (one extra barrier)
        const u32 len = (u32)tid < nd.len ? (u32)((myrec.y >> 44) & 31) + 1u : 0u;
        const u32 nq = (len + SKC_KPT - 1) / SKC_KPT;
        u32 qinc = 0;
        if (tid < SKC_MAXREC) {
            lrec[tid] = myrec;
            qinc = wave_incl_scan(nq);
            if (lane == 63)
                wq[wave] = qinc;
        }
        __syncthreads();
        u32 qb = 0;
        sk_wave_prefix16(wq, RWAVES, wave, lane, qb, n_quads);
        if (tid < SKC_MAXREC) {
            const u32 q0 = qb + qinc - nq;
            for (u32 q = 0; q < nq; q++)
                ownq[q0 + q] = (unsigned short)((u32)tid | (q << 9));
        }
    }
    bool has_next = lq + step < n_list;
    u32 ln = has_next ? list[lq + step] : li;
    u32 off_next = has_next ? list_off[lq + step] : off;
    Node nn = fin[ln];
    myrec.x = myrec.y = 0;
    if (has_next && (u32)tid < nn.len)
        myrec = recs[(u64)nn.start + tid];         // the second bucket's records: in flight
    for (;;) {
        const u32 lq2 = lq + 2 * step;
        const bool has_next2 = lq2 < n_list;
        const u32 ln2 = has_next2 ? list[lq2] : ln;                     // (used at the end of this iteration)
        const u32 off2 = has_next2 ? list_off[lq2] : off_next;
        const Node nn2 = fin[ln2];
        // (opaque per bucket: the LDS addresses and masks derived from the thread index are then recomputed -- one or two
        // operations each -- instead of being held across the loop: 21 of the 64 VGPRs were such invariants; 54 are used
        // now, and the kernel issues fewer instructions: 11.47 -> 11.29 ms with the next item in an A/B on one box)
        asm volatile("" : "+v"(tid));
        lane = tid & 63;
        wave = tid >> 6;
        __syncthreads();                           // A2: lrec[] and ownq[] complete, every slot of the previous bucket reset
        // ---- this thread's quad.  32-bit arithmetic throughout (the kernel's time follows its instruction count: 343 vector
        // + 214 scalar instructions per wave and bucket in round 2's form): the quad's k-mers are cut
        // from a three-dword window of the record that moves on two bits per k-mer (three v_alignbit), slot and
        // fingerprint come from one 32-bit product (the slot through a full-rate 24-bit multiply), and the probe loop
        // carries the slot's byte address only -- what a claim leaves behind is assigned once, after the loop.
        u32 ckl[KEEP], ckh[KEEP];
        u32 cslot[KEEP];                           // byte address of the claimed slot
        u32 c_mask = 0;
        // (only positions whose c_mask bit is set are ever used: the others stay whatever their registers hold -- defined
        // for the compiler by an empty asm, so that no instruction initialises them: 12 moves per thread and bucket)
#pragma unroll
        for (int q = 0; q < SKC_KPT; q++) {
            asm volatile("" : "=v"(ckl[q]));
            asm volatile("" : "=v"(ckh[q]));
            asm volatile("" : "=v"(cslot[q]));
        }
        if ((u32)tid < n_quads) {
            const u32 e = ownq[tid];
            const ull2_t rec = lrec[e & 511u];
            const u32 p0 = (u32)rec.x, p1 = (u32)(rec.x >> 32), p2 = (u32)rec.y, p3h = (u32)(rec.y >> 32);
            const u32 rl = ((p3h >> 12) & 31u) + 1u;
            const u32 p3 = p3h & 0xFFFu;
            const u32 j0 = (e >> 9) * SKC_KPT;
            const bool up = j0 >= 16;                            // the quad starts in the record's second dword
            const u32 sh = (2 * j0) & 31u;
            const u32 a0 = up ? p1 : p0, a1 = up ? p2 : p1, a2 = up ? p3 : p2, a3 = up ? 0u : p3;
            u32 w0 = __builtin_amdgcn_alignbit(a1, a0, sh), w1 = __builtin_amdgcn_alignbit(a2, a1, sh),
                w2 = __builtin_amdgcn_alignbit(a3, a2, sh);
            const u32 hmask = (u32)(kmask >> 32);                // (k >= 21: the low dword is whole)
            const u32 id0 = (u32)tid << 2;
            // all four keys of the quad first, straight into the registers that keep them (the window moves on two bits per
            // k-mer whether the position exists or not: no copies where the branches of the inserts meet)
#pragma unroll
            for (int q = 0; q < SKC_KPT; q++) {
                ckl[q] = w0;
                ckh[q] = w1 & hmask;
                w0 = __builtin_amdgcn_alignbit(w1, w0, 2);
                w1 = __builtin_amdgcn_alignbit(w2, w1, 2);
                w2 >>= 2;
            }
#pragma unroll
            for (int q = 0; q < SKC_KPT; q++) {
                if (j0 + (u32)q < rl) {
                    const u32 kl = ckl[q], kh = ckh[q];
                    if (SK_DBG(32)) {
                        c_mask |= (kl & 1) ? 1u << q : 0u;
                    } else {
                        const u32 x = (kl ^ kh) * 0x9E3779B1u;
                        u32 &sa = cslot[q];                      // byte address of the probed slot: where a claim leaves it, it stays
                        sa = ((u32)__umul24(x >> 16, (u32)SKC_SLOTS) >> 16) << 2;
                        const u32 y = x ^ (x >> 15);             // (the product's low bits alone depend on the key's low bits only)
                        // 19 bits of fingerprint under a clear top bit: no word equals the all-ones of a free slot
                        const u32 word = ((y & 0x7FFFFu) << 12) | id0 | (u32)q;
                        for (;;) {
                            const u32 old = atomicCAS(reinterpret_cast<u32 *>(reinterpret_cast<char *>(tab) + sa), SKC_FREE, word);
                            if (old == SKC_FREE) {
                                c_mask |= 1u << q;
                                break;
                            }
                            if ((old ^ word) < 4096u) {
                                // the claimant's key, from the staged records (its owner entry and record do not change before B)
                                const u32 oid = old & 0xFFFu;
                                const u32 oe = ownq[oid >> 2];
                                const u64 okey = sk_record_kmer(lrec[oe & 511u], (oe >> 9) * SKC_KPT + (oid & 3u), kmask);
                                if (okey == (((u64)kh << 32) | kl)) {  // a copy: counted at the claimant's id
                                    atomicAdd(&cop2[oid >> 1], 1u << ((oid & 1u) * 16u));
                                    copy_seen[par] = 1u;
                                    break;
                                }
                            }
                            sa = sa + 4 == (u32)SKC_SLOTS * 4u ? 0u : sa + 4;
                        }
                    }
                }
            }
        }
        const u32 wc = wave_sum((u32)__popc(c_mask));
        if (lane == 0)
            wclaim[par][wave] = wc;
        // the next bucket's quad prefix (record waves; its records were requested a bucket ago)
        const u32 len_n = has_next && (u32)tid < nn.len ? (u32)((myrec.y >> 44) & 31) + 1u : 0u;
        const u32 nq_n = (len_n + SKC_KPT - 1) / SKC_KPT;
        u32 qinc_n = 0;
        if (tid < SKC_MAXREC) {
            qinc_n = wave_incl_scan(nq_n);
            if (lane == 63)
                wq[wave] = qinc_n;
        }
        __syncthreads();                           // B: all inserts done
        if (have_prev)
            emit_prev();                           // (a bucket behind: its stores overlap this bucket's tail and the next one's head)
        // ---- this bucket: counts of the claimed slots, table cleaned; emitted next round
        u32 before = 0, D = 0;
        sk_wave_prefix16(wclaim[par], WAVES, wave, lane, before, D);
        const bool any_copy = copy_seen[par] != 0; // (random sequence: no bucket has one, and the copy counters are not read)
#pragma unroll
        for (int q = 0; q < KEEP; q++) {
            pkl[q] = ckl[q];
            pkh[q] = ckh[q];
            pc[q] = 0;
            if ((c_mask >> q) & 1u) {
                pc[q] = 1u;
                *reinterpret_cast<u32 *>(reinterpret_cast<char *>(tab) + cslot[q]) = SKC_FREE;
                if (any_copy) {
                    const u32 copies = cop16[(u32)tid * SKC_KPT + (u32)q];
                    pc[q] = 1u + copies;
                    if (copies)
                        cop16[(u32)tid * SKC_KPT + (u32)q] = 0;
                }
            }
        }
        p_mask = c_mask;
        p_before = before;
        p_groups = D;
        p_li = li;
        p_off = off;
        p_kmers = nd.child_base;
        p_copy = any_copy;
        if (tid == 0) {
            my_groups += D;
            copy_seen[par ^ 1] = 0;                // (the other parity's flag: its bucket is done with it)
        }
        have_prev = true;
        par ^= 1;
        if (!has_next)
            break;
        // ---- the next bucket is staged (nobody reads lrec / ownq between B and A2), the one after it requested
        {
            u32 qb = 0;
            sk_wave_prefix16(wq, RWAVES, wave, lane, qb, n_quads);
            if (tid < SKC_MAXREC) {
                lrec[tid] = myrec;
                const u32 q0 = qb + qinc_n - nq_n;
                for (u32 q = 0; q < nq_n; q++)
                    ownq[q0 + q] = (unsigned short)((u32)tid | (q << 9));
            }
            myrec.x = myrec.y = 0;
            if (has_next2 && (u32)tid < nn2.len)
                myrec = recs[(u64)nn2.start + tid];
        }
        lq += step;
        li = ln;
        off = off_next;
        nd = nn;
        has_next = has_next2;
        ln = ln2;
        off_next = off2;
        nn = nn2;
    }
    emit_prev();                                   // the last bucket's output
    if (tid == 0)
        atomicAdd(n_groups, (unsigned long long)my_groups);
}

// Could records A and B -- both cut from plain tiles (SK_REC_MULTI clear), their minimum m-mers equal, at offsets a and b --
// hold an equal k-mer?  All k-mers of such a record have their leftmost minimum m-mer at the record's one place, and that
// offset inside a k-mer is a function of the k-mer's content: equal k-mers K = A[j1 ..] = B[j2 ..] have a - j1 = b - j2.  So
// the records can only agree where they are aligned at their m-mers, and K covers the m-mer, L' bases before it and R'
// behind it with L' + R' = k - m: an equal k-mer exists iff the bases agree over L before and R behind the m-mer (as far
// as BOTH records reach: ML, MR) with L + R >= k - m.  Exact, not a filter.
__device__ __forceinline__ bool sk_records_share_kmer(const ull2_t A, u32 a, u32 nba, const ull2_t B, u32 b, u32 nbb, u32 m, u32 kmm)
{
    const u64 pm = ((u64)1 << 34) - 1;             // payload bits of the second word (at most 49 bases)
    const u64 ah = A.y & pm, bh = B.y & pm;
    const u32 ML = a < b ? a : b;
    const u32 ra = nba - a - m, rb = nbb - b - m;
    const u32 MR = ra < rb ? ra : rb;               // <= k - m <= 17
    const u64 xr = (sk_shr128(A.x, ah, 2u * (a + m)) ^ sk_shr128(B.x, bh, 2u * (b + m))) & (((u64)1 << (2u * MR)) - 1);
    const u32 R = xr ? (u32)__builtin_ctzll(xr) >> 1 : MR;
    if (R + ML < kmm)
        return false;
    const u64 xl = (funnel(A.x, ah, 2u * (a - ML)) ^ funnel(B.x, bh, 2u * (b - ML))) & (((u64)1 << (2u * ML)) - 1);
    const u32 L = xl ? ML - 1u - ((63u - (u32)__builtin_clzll(xl)) >> 1) : ML;
    return L + R >= kmm;
}


// ------------------------------------------------------------------------------------------------
// sk_count_clean (round 4): RECORDS ARE TESTED BEFORE K-MERS.  Equal k-mers share their minimum m-mer AND its offset inside
// the k-mer (both are functions of the k-mer's content), so two records cut from plain tiles can hold an equal k-mer only
// if their m-mers are equal and they agree around them -- over L bases before and R behind it with L + R >= k - m
// (sk_records_share_kmer: exact).  A bucket's ~300 records go into a small LDS table keyed by the m-mer: an entry is
//   low word  = 22 bits of a hash of the m-mer | record index << 22 (bit 31 clear: no entry is all ones)
//   high word = the F bases before the m-mer | the F bases behind it << 16, F = min(8, (k - m) / 2); a side the record
//               does not have F bases of holds a value of the record's own (0x8000 | index) instead
// (linear probing: a record passes every earlier entry of its m-mer on the way to its own slot: ~1.4 of them at 3 Gbase,
// 0.1 at 250 Mbase).  An equal k-mer covers the m-mer and k - m >= 2 F more bases around it, so it needs the m-mer's hash
// and one of the two halves equal: two XORs per passed entry; the few pairs that pass (4^-F per side) take the exact test.
// A bucket in which no two records share a k-mer holds every k-mer ONCE: its k-mers are cut from the records and leave as
// (key, 1) groups, one k-mer per thread and round, 8 + 4 bytes per lane to consecutive addresses -- no k-mer hash, no probe,
// no table.  A bucket in which SOME records share k-mers (a stretch that occurs again elsewhere: a handful of buckets per
// million on random sequence, nearly every bucket of a real genome) keeps that path for all its other records and counts
// only the sharing records' k-mers, up to SKQ_DIRTY_MAX of them, in the record table's slots once the records are done
// with them (a k-mer of a record that shares nothing has no copy; a copy of a sharing record's k-mer lies in a record that
// shares with it).  What is left -- a SK_REC_MULTI record of a low-complexity stretch, more copies than that -- is
// appended to a list that sk_count takes afterwards, exact as before.
//   Why: round 3's sk_count spent 265 vector + 200 scalar instructions per wave and bucket, a third of them probing the
//   k-mer table for k-mers that never had a copy, the rest bookkeeping around sixteen waves (quads, claim prefixes, keys
//   kept a bucket long, four ballot rounds of stores).  This kernel has eight waves per bucket, no table to clear, and
//   26 KB of LDS: four workgroups per CU.
constexpr int SKQ_NT = 512;
static_assert(SKQ_NT == SKC_MAXREC, "a thread per record");
constexpr int SKQ_KMERS = 4096;                  // sk_count_cap(): most k-mers of a small bucket
constexpr int SKQ_VSLOTS = 1024;                 // record table (at most 512 entries)
constexpr int SKQ_DIRTY_MAX = 640;               // most k-mers of sharing records that are counted in those slots

// (A/B builds only: tools/build_variant.sh WORK x.so -DSKQ_STORE_PLAIN / -DSKQ_KEYS_PLAIN / -DSKQ_COUNTS_PLAIN)
#if defined(SKQ_STORE_PLAIN) || defined(SKQ_KEYS_PLAIN)
#define SKQ_STORE(v, p) (*(p) = (v))
#else
#define SKQ_STORE(v, p) __builtin_nontemporal_store(v, p)
#endif
#if defined(SKQ_STORE_PLAIN) || defined(SKQ_COUNTS_PLAIN)
#define SKQ_STOREC(v, p) (*(p) = (v))
#else
#define SKQ_STOREC(v, p) __builtin_nontemporal_store(v, p)
#endif
__global__ __launch_bounds__(SKQ_NT, 8) void sk_count_clean_kernel(const Node *__restrict__ fin, const u32 *__restrict__ list,
                                                                   const u32 *__restrict__ list_off, u32 n_list,
                                                                   const ull2_t *__restrict__ recs, int k,
                                                                   unsigned long long *__restrict__ n_groups,
                                                                   u64 *__restrict__ seg_off, u32 *__restrict__ seg_cnt,
                                                                   u64 *__restrict__ out_keys, u32 *__restrict__ out_counts,
                                                                   u32 *__restrict__ left_list, u32 *__restrict__ left_off,
                                                                   u32 *__restrict__ n_left, int dbg)
{
    constexpr int WAVES = SKQ_NT / 64;
    __shared__ __attribute__((aligned(16))) ull2_t lrec[SKC_MAXREC];
    __shared__ __attribute__((aligned(16))) u64 vtab[SKQ_VSLOTS];
    __shared__ unsigned short own[SKQ_KMERS];      // k-mer of the bucket -> record | position in it << 9
    __shared__ u32 wk[WAVES], wk2[WAVES];
    __shared__ u32 shared_flag[2], multi_flag[2];  // by bucket parity: two records share a k-mer; a SK_REC_MULTI record
    __shared__ u32 dcnt2[SKQ_VSLOTS / 2];          // (buckets with copies) the counts beside vtab's k-mer keys, 16 bits each
    __shared__ unsigned short cpos[SKC_MAXREC];    // ... a record's first output slot, or 0xFFFF: its k-mers are counted
    __shared__ unsigned char rdb[SKC_MAXREC];      // ... the record shares a k-mer with another
    __shared__ u32 d_ones;
    unsigned short *dcnt = reinterpret_cast<unsigned short *>(dcnt2);
    int tid = threadIdx.x;
    u32 lq = blockIdx.x;
    if (lq >= n_list)
        return;
    vtab[tid] = ~(u64)0;
    vtab[tid + SKQ_NT] = ~(u64)0;
    dcnt2[tid] = 0;
    rdb[tid] = 0;
    if (tid < 2)
        shared_flag[tid] = multi_flag[tid] = 0;
    if (tid == 0)
        d_ones = 0;
    const u32 mlen = (u32)sk_mlen(k);
    const u32 vmask = (1u << (2u * mlen)) - 1u, kmm = (u32)k - mlen;
    const u32 flank = kmm / 2u < 8u ? kmm / 2u : 8u, fmask = (1u << (2u * flank)) - 1u;
    const u32 hmask = (u32)(kmer_mask(k) >> 32);   // (k >= 21: the low dword of a key is whole)
    const u32 step = gridDim.x;
    u32 li = list[lq];
    Node nd = fin[li];
    ull2_t myrec;
    myrec.x = myrec.y = 0;
    if ((u32)tid < nd.len)
        myrec = recs[(u64)nd.start + tid];
    u64 my_groups = 0;
    int par = 0;
    for (;;) {
        const u32 off = list_off[lq];
        const bool has_next = lq + step < n_list;
        const u32 ln = has_next ? list[lq + step] : li;
        const Node nn = fin[ln];
        asm volatile("" : "+v"(tid));              // (nothing derived from the thread index is held across buckets)
        const int lane = tid & 63, wave = tid >> 6;
        // ---- this bucket's records into LDS, the next bucket's requested
        const ull2_t me = myrec;
        lrec[tid] = me;
        myrec.x = myrec.y = 0;
        if (has_next && (u32)tid < nn.len)
            myrec = recs[(u64)nn.start + tid];
        const bool have = (u32)tid < nd.len;
        const u32 yh = (u32)(me.y >> 32);
        const u32 len = have ? ((yh >> 12) & 31u) + 1u : 0u;
        const u32 kinc = wave_incl_scan(len);
        if (lane == 63)
            wk[wave] = kinc;
        __syncthreads();                           // (1) lrec / wk complete; the previous bucket's readers are done (barrier 3)
        u32 kbase = 0, n_km = 0;
        sk_wave_prefix16(wk, WAVES, wave, lane, kbase, n_km);
        // ---- every k-mer's owner; the records against each other
        u32 vslot = ~0u;
        if (have) {
            const u32 k0 = kbase + kinc - len;
            if (!SK_DBG(1024))
                for (u32 j = 0; j < len; j++)
                    own[k0 + j] = (unsigned short)((u32)tid | (j << 9));
            if (SK_DBG(256)) {
            } else if (yh & (1u << (SK_REC_MULTI_BIT - 32))) {
                multi_flag[par] = 1u;              // (nothing is known about where this record's m-mer is)
            } else {
                const u32 p0 = (u32)me.x, p1 = (u32)(me.x >> 32), p2 = (u32)me.y, p3 = yh & 3u;
                const u32 a = (yh >> (SK_POS_SHIFT - 32)) & SK_POS_MASK;
                const u32 nba = len + (u32)k - 1u;                                // bases (<= 49: payload bits 0 .. 97)
                const u32 sv = 2u * a, sl = 2u * (a - flank), sr = 2u * (a + mlen);   // bit offsets (sl: only used if a >= flank)
                const u32 v = __builtin_amdgcn_alignbit(sv >= 32u ? p2 : p1, sv >= 32u ? p1 : p0, sv) & vmask;
                u32 fl = __builtin_amdgcn_alignbit(sl >= 32u ? p2 : p1, sl >= 32u ? p1 : p0, sl) & fmask;
                const u32 r_lo = sr >= 64u ? p2 : (sr >= 32u ? p1 : p0), r_hi = sr >= 64u ? p3 : (sr >= 32u ? p2 : p1);
                u32 fr = __builtin_amdgcn_alignbit(r_hi, r_lo, sr) & fmask;
                const u32 mine_own = 0x8000u | (u32)tid;
                fl = a >= flank ? fl : mine_own;
                fr = nba - a - mlen >= flank ? fr : mine_own;
                const u32 hv = (v ^ (v >> 13)) * 0x85EBCA6Bu;                    // (not sk_fine_word: the bucket's records share its top bits)
                const u32 lo32 = (hv >> 10) | ((u32)tid << 22), hi32 = fl | (fr << 16);
                const u64 mine = (u64)lo32 | ((u64)hi32 << 32);
                u32 slot = hv >> 22;
                for (;;) {
                    const u64 old = atomicCAS(reinterpret_cast<unsigned long long *>(&vtab[slot]), ~0ull, (unsigned long long)mine);
                    if (old == ~(u64)0)
                        break;
                    const u32 xl = (u32)old ^ lo32, xh = (u32)(old >> 32) ^ hi32;
                    if ((xl & 0x3FFFFFu) == 0 && ((xh & 0xFFFFu) == 0 || (xh >> 16) == 0)) {
                        // (rare: 4^-F per side and pair) the exact test
                        const u32 oid = ((u32)old >> 22) & 511u;
                        const ull2_t ot = lrec[oid];
                        const u32 oyh = (u32)(ot.y >> 32);
                        if (sk_records_share_kmer(me, a, nba, ot, (oyh >> (SK_POS_SHIFT - 32)) & SK_POS_MASK,
                                                  ((oyh >> 12) & 31u) + (u32)k, mlen, kmm)) {
                            shared_flag[par] = 1u;
                            rdb[tid] = 1;
                            rdb[oid] = 1;
                        }
                    }
                    slot = (slot + 1u) & (u32)(SKQ_VSLOTS - 1);
                }
                vslot = slot;
            }
        }
        __syncthreads();                           // (2) owners and the verdict complete
        if (vslot != ~0u)
            vtab[vslot] = ~(u64)0;                 // (the table is clean again for the next bucket)
        u64 *ok = out_keys + off;
        u32 *oc = out_counts + off;
        auto key_cut = [&](const ull2_t r, u32 e) -> u64 {
            const u32 p0 = (u32)r.x, p1 = (u32)(r.x >> 32), p2 = (u32)r.y, p3 = (u32)(r.y >> 32) & 3u;
            const u32 sh = 2u * (e >> 9);          // (<= 2 (w - 1) = 34)
            const bool up = sh >= 32u;
            const u32 a0 = up ? p1 : p0, a1 = up ? p2 : p1, a2 = up ? p3 : p2;
            const u32 kl = __builtin_amdgcn_alignbit(a1, a0, sh), kh = __builtin_amdgcn_alignbit(a2, a1, sh) & hmask;
            return ((u64)kh << 32) | kl;
        };
        auto key_of = [&](u32 i) -> u64 {
            const u32 e = own[i];
            return key_cut(lrec[e & 511u], e);
        };
        const u32 flag = shared_flag[par] | (multi_flag[par] << 1);
        if (flag) {
            // ---- some records share k-mers with others (a copy of a stretch elsewhere: the rule on real genomes, a handful
            // of buckets per million on random sequence).  Only THOSE records' k-mers can have copies: every other record's
            // k-mers leave as (key, 1) as below, compacted by a prefix over the records; the sharing records' k-mers -- up to
            // SKQ_DIRTY_MAX of them -- are counted in the record table's slots (empty again by now) and leave behind them.
            // A bucket with a SK_REC_MULTI record or with more k-mers to count goes to sk_count's list.
            const bool dirty = have && rdb[tid] != 0;
            rdb[tid] = 0;
            const u32 pk = dirty ? (len << 16) : len;
            const u32 pinc = wave_incl_scan(pk);
            if (lane == 63)
                wk2[wave] = pinc;
            __syncthreads();                       // (A) wk2; every slot of vtab is empty again
            u32 pbase = 0, ptot = 0;
            sk_wave_prefix16(wk2, WAVES, wave, lane, pbase, ptot);
            const u32 n_clean = ptot & 0xFFFFu, n_dirty = ptot >> 16;
            if ((flag & 2u) || n_dirty > (u32)SKQ_DIRTY_MAX) {
                if (tid == 0) {
                    const u32 d = atomicAdd(n_left, 1u);
                    left_list[d] = li;
                    left_off[d] = off;
                }
            } else {
                cpos[tid] = dirty ? (unsigned short)0xFFFFu : (unsigned short)((pbase + pinc - pk) & 0xFFFFu);
                __syncthreads();                   // (B) cpos
                for (u32 i = (u32)tid; i < n_km; i += SKQ_NT) {
                    const u32 e = own[i];
                    const u32 c = cpos[e & 511u];
                    const u64 key = key_of(i);
                    if (c != 0xFFFFu) {
                        SKQ_STORE(key, &ok[c + (e >> 9)]);
                        SKQ_STOREC(1u, &oc[c + (e >> 9)]);
                    } else if (key == ~(u64)0) {
                        atomicAdd(&d_ones, 1u);    // (the 32-base k-mer GG..G: the empty slot's value)
                    } else {
                        u32 slot = ((((u32)key ^ (u32)(key >> 32)) * 0x9E3779B1u) >> 22) & (u32)(SKQ_VSLOTS - 1);
                        for (;;) {
                            const u64 old = atomicCAS(reinterpret_cast<unsigned long long *>(&vtab[slot]), ~0ull, (unsigned long long)key);
                            if (old == ~(u64)0 || old == key)
                                break;
                            slot = (slot + 1u) & (u32)(SKQ_VSLOTS - 1);
                        }
                        atomicAdd(&dcnt2[slot >> 1], 1u << ((slot & 1u) * 16u));
                    }
                }
                __syncthreads();                   // (C) the table complete
                const u32 c0 = dcnt[tid], c1 = dcnt[tid + SKQ_NT], ones = d_ones;
                const u64 b0 = __ballot(c0 != 0), b1 = __ballot(c1 != 0);
                if (lane == 0)
                    wk2[wave] = (u32)__popcll(b0) + (u32)__popcll(b1);
                __syncthreads();                   // (D)
                u32 before = 0, D = 0;
                sk_wave_prefix16(wk2, WAVES, wave, lane, before, D);
                const u64 lt = ((u64)1 << lane) - 1;
                u64 *dk = ok + n_clean;
                u32 *dc = oc + n_clean;
                if (c0) {
                    const u32 r = before + (u32)__popcll(b0 & lt);
                    dk[r] = vtab[tid];
                    dc[r] = c0;
                    vtab[tid] = ~(u64)0;
                    dcnt[tid] = 0;
                }
                if (c1) {
                    const u32 r = before + (u32)__popcll(b0) + (u32)__popcll(b1 & lt);
                    dk[r] = vtab[tid + SKQ_NT];
                    dc[r] = c1;
                    vtab[tid + SKQ_NT] = ~(u64)0;
                    dcnt[tid + SKQ_NT] = 0;
                }
                const u32 groups = n_clean + D + (ones ? 1u : 0u);
                for (u32 i = groups + (u32)tid; i < n_km; i += SKQ_NT)
                    oc[i] = 0;                     // (the rest of the bucket's range is padding: count 0)
                if (tid == 0) {
                    if (ones) {
                        dk[D] = ~(u64)0;
                        dc[D] = ones;
                        d_ones = 0;
                    }
                    seg_off[li] = off;
                    seg_cnt[li] = groups;
                    my_groups += groups;
                }
            }
        } else {
            // ---- every k-mer of the bucket is the only one of its kind: (key, 1) groups, k-mer i at slot off + i
            // Two k-mers per thread and round: 16 bytes of keys and 8 of counts per lane, nontemporal (a plain store stream
            // tops out near 3.3 TB/s on this chip).
            // The pairs start on a 32-slot boundary of the arrays (256 bytes of keys, 128 of counts), so that a wave's stores
            // cover whole lines; the k-mers before that boundary leave one per thread.  (Measured, 3 Gbase, 14 runs each on
            // one box: pairs from the first even slot 8.07 - 8.34 ms with runs of 10.0 - 10.8 in between -- typically a box's
            // first -- against 7.93 - 8.04 with one of 8.7, when every kernel was 5 - 8 % slower; plain stores throughout
            // 8.45 - 9.3; plain stores for the partial lines at a bucket's ends: no gain.)
            const u32 head = (32u - (off & 31u)) & 31u;
            if ((u32)tid < head && (u32)tid < n_km) {
                SKQ_STORE(key_of((u32)tid), &ok[tid]);
                SKQ_STOREC(1u, &oc[tid]);
            }
            // (both owners, then both records: two LDS round trips per pair instead of four in a row -- and the NEXT pair's
            // reads are issued before this pair's keys are cut and stored)
            u32 i = head + 2u * (u32)tid;
            u32 e0 = 0, e1 = 0;
            ull2_t r0, r1;
            r0.x = r0.y = r1.x = r1.y = 0;
            auto fetch = [&](u32 at) {
                e0 = own[at];
                e1 = own[at + 1 < n_km ? at + 1 : at];
                asm volatile("" : "+v"(e0), "+v"(e1));
                r0 = lrec[e0 & 511u];
                r1 = lrec[e1 & 511u];
                asm volatile("" : "+v"(r0.x), "+v"(r0.y), "+v"(r1.x), "+v"(r1.y));
            };
            if (i < n_km)
                fetch(i);
            while (i < n_km) {
                const u32 ce0 = e0, ce1 = e1;
                const ull2_t c0 = r0, c1 = r1;
                const u32 nxt = i + 2u * SKQ_NT;
                if (nxt < n_km)
                    fetch(nxt);
                const u64 k0 = key_cut(c0, ce0);
                if (SK_DBG(512)) {
                    if (k0 == 0x123456789ull)
                        ok[0] = k0;
                } else if (i + 1 < n_km) {
                    ull2_t kk;
                    kk.x = k0;
                    kk.y = key_cut(c1, ce1);
                    SKQ_STORE(kk, reinterpret_cast<ull2_t *>(&ok[i]));
                    SKQ_STOREC((u64)0x100000001ull, reinterpret_cast<u64 *>(&oc[i]));
                } else {
                    SKQ_STORE(k0, &ok[i]);
                    SKQ_STOREC(1u, &oc[i]);
                }
                i = nxt;
            }
            if (tid == 0) {
                seg_off[li] = off;
                seg_cnt[li] = n_km;
                my_groups += n_km;
            }
        }
        if (tid == 0)
            shared_flag[par ^ 1] = multi_flag[par ^ 1] = 0;   // (the other parity's flags: its bucket is done with them)
        par ^= 1;
        if (!has_next)
            break;
        __syncthreads();                           // (3) lrec / own are rewritten by the next bucket
        lq += step;
        li = ln;
        nd = nn;
    }
    if (tid == 0 && my_groups)
        atomicAdd(n_groups, (unsigned long long)my_groups);
}

hipError_t launch_sk_count(const Node *fin, const u32 *list, const u32 *list_off, u32 n_list, const void *recs, int k, u64 *n_groups,
                           u64 *seg_off, u32 *seg_cnt, u64 *out_keys, u32 *out_counts, u32 *left /* 2 n_list + 1 words */,
                           hipStream_t s)
{
    if (n_list == 0)
        return hipSuccess;
    int dev = 0, n_cu = 256, v = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0)
        n_cu = v;
    // every small bucket through the record test first; the ones that may hold copies are listed (left[0 .. n), left[n_list ..
    // n_list + n) = their output offsets, left[2 n_list] = n) and counted by the k-mer table kernel behind it
    u32 *left_list = left, *left_off = left + n_list, *n_left = left + 2 * (size_t)n_list;
    hipError_t e = hipMemsetAsync(n_left, 0, sizeof(u32), s);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(sk_count_clean_kernel, dim3(std::min<u32>(n_list, (u32)n_cu * 4u)), dim3(SKQ_NT), 0, s, fin, list, list_off, n_list,
                       reinterpret_cast<const ull2_t *>(recs), k, reinterpret_cast<unsigned long long *>(n_groups), seg_off, seg_cnt,
                       out_keys, out_counts, left_list, left_off, n_left, sk_dbg());
    const u32 grid = std::min<u32>(n_list, (u32)n_cu * 2u);
    hipLaunchKernelGGL(sk_count_kernel, dim3(grid), dim3(SKC_NT), 0, s, fin, left_list, left_off, 0u, n_left,
                       reinterpret_cast<const ull2_t *>(recs), k, reinterpret_cast<unsigned long long *>(n_groups), seg_off, seg_cnt,
                       out_keys, out_counts, sk_dbg());
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Buckets that sk_count does not take (more k-mers, records or quads than its tables hold; the heavy mid buckets of long
// repeats with millions of k-mers) are expanded to keys in record order by many waves at once, with no host step
// in between: a bucket's records are cut into slices of SKF_SLICE records (sk_slice_count -> scan -> sk_slice_fill),
// sk_slice_kmers sums every slice's k-mers, a scan of the sums gives every slice its key offset and every bucket its
// key range (sk_slice_nodes: one key node per bucket, which the ordinary levels split with their skew paths), and
// sk_expand_flat expands slice by slice (64 records at a time: lengths -> wave prefix -> keys staged in LDS -> one
// contiguous copy).
constexpr int SKF_SLICE = 4096;
int sk_flat_slice() { return SKF_SLICE; }

__global__ __launch_bounds__(256) void sk_slice_count_kernel(const Node *__restrict__ buckets, u32 nb, u32 *__restrict__ n_slices)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nb)
        n_slices[i] = (buckets[i].len + (u32)SKF_SLICE - 1u) / (u32)SKF_SLICE;
}

// one wave per bucket: its slices' first records and record counts, at slice_first[bucket]
__global__ __launch_bounds__(256) void sk_slice_fill_kernel(const Node *__restrict__ buckets, u32 nb,
                                                            const u32 *__restrict__ slice_first, u32 *__restrict__ slice_rec0,
                                                            u32 *__restrict__ slice_nrec)
{
    const u32 lane = threadIdx.x & 63;
    const u32 i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nb)
        return;
    const u32 start = buckets[i].start, len = buckets[i].len, s0 = slice_first[i];
    const u32 ns = (len + (u32)SKF_SLICE - 1u) / (u32)SKF_SLICE;
    for (u32 j = lane; j < ns; j += 64) {
        slice_rec0[s0 + j] = start + j * (u32)SKF_SLICE;
        slice_nrec[s0 + j] = min((u32)SKF_SLICE, len - j * (u32)SKF_SLICE);
    }
}

__global__ __launch_bounds__(256) void sk_slice_kmers_kernel(const ull2_t *__restrict__ recs, const u32 *__restrict__ slice_rec0,
                                                             const u32 *__restrict__ slice_nrec, u32 n_slices,
                                                             u32 *__restrict__ slice_km)
{
    const int lane = threadIdx.x & 63;
    const u32 si = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (si >= n_slices)
        return;
    const u64 *hi = reinterpret_cast<const u64 *>(recs + (u64)slice_rec0[si]) + 1;
    const u32 n = slice_nrec[si];
    u32 sum = 0;
    for (u32 r = lane; r < n; r += 64)
        sum += (u32)((__builtin_nontemporal_load(&hi[(u64)r * 2]) >> 44) & 31) + 1u;
    sum = wave_sum(sum);
    if (lane == 0)
        slice_km[si] = sum;
}

// key node of bucket i: the keys of its slices, [key_base + slice_koff[first slice], ... of the next bucket).
// expect_kmers (buckets[i].child_base, the partition's own count) must agree: *n_bad counts the buckets where not.
__global__ __launch_bounds__(256) void sk_slice_nodes_kernel(const Node *__restrict__ buckets, u32 nb,
                                                             const u32 *__restrict__ slice_first, const u32 *__restrict__ slice_koff,
                                                             u32 n_slices, const u32 *__restrict__ total_keys, u32 key_base, int k,
                                                             int check_kmers, Node *__restrict__ out,
                                                             unsigned long long *__restrict__ n_bad)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb)
        return;
    const u32 s0 = slice_first[i], s1 = i + 1 < nb ? slice_first[i + 1] : n_slices;
    const u32 k0 = s0 < n_slices ? slice_koff[s0] : *total_keys, k1 = s1 < n_slices ? slice_koff[s1] : *total_keys;
    Node nd;
    nd.prefix = 0;
    nd.start = key_base + k0;
    nd.len = k1 - k0;
    nd.meta = (u32)(2 * k);                      // no key bit is fixed; buffer 0
    nd.split = 0;
    nd.child_base = 0;
    nd.chunk_base = 0;
    out[i] = nd;
    if (check_kmers && buckets[i].child_base != k1 - k0)
        atomicAdd(n_bad, 1ull);
}

__global__ __launch_bounds__(256) void sk_expand_flat_kernel(const ull2_t *__restrict__ recs, const u32 *__restrict__ slice_rec0,
                                                             const u32 *__restrict__ slice_nrec,
                                                             const u32 *__restrict__ slice_koff, u32 key_base, u32 n_slices, int k,
                                                             u32 lmax, u64 *__restrict__ keys)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char skf_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 si = blockIdx.x * 4 + (u32)wave;
    if (si >= n_slices)
        return;                                   // (whole waves: nothing below synchronises across waves)
    u64 *stage = reinterpret_cast<u64 *>(skf_smem) + (size_t)wave * 64 * lmax;
    const ull2_t *src = recs + (u64)slice_rec0[si];
    const u32 n = slice_nrec[si];
    const u64 kmask = kmer_mask(k);
    u64 out = (u64)key_base + slice_koff[si];
    ull2_t nxt;
    nxt.x = nxt.y = 0;
    if ((u32)lane < n)
        nxt = src[lane];
    for (u32 b0 = 0; b0 < n; b0 += 64) {
        const ull2_t rec = nxt;
        const bool have = b0 + (u32)lane < n;
        if (b0 + 64 + (u32)lane < n)
            nxt = src[b0 + 64 + lane];
        const u32 len = have ? (u32)((rec.y >> 44) & 31) + 1u : 0u;
        const u32 inc = wave_incl_scan(len);
        const u32 n_keys = (u32)__builtin_amdgcn_readlane((int)inc, 63);
        const u32 o = inc - len;
        const u64 hi = rec.y & (((u64)1 << 44) - 1);
        for (u32 j = 0; j < len; j++)
            stage[o + j] = key_mix(funnel(rec.x, hi, 2 * j) & kmask, k, kmask);   // (see key_mix: the levels split mixed keys)
        sk_wave_fence();
        for (u32 s = lane; s < n_keys; s += 64)
            __builtin_nontemporal_store(stage[s], &keys[out + s]);
        sk_wave_fence();
        out += n_keys;
    }
}

// the groups of the expansion's tree, keys[first .. *end), back from key_mix
__global__ __launch_bounds__(256) void sk_unmix_kernel(u64 *__restrict__ keys, u64 first, const unsigned long long *__restrict__ end,
                                                       int k)
{
    const u64 e = *end, mask = kmer_mask(k);
    for (u64 i = first + (u64)blockIdx.x * 256 + threadIdx.x; i < e; i += (u64)gridDim.x * 256)
        keys[i] = key_unmix(keys[i], k, mask);
}

hipError_t launch_sk_unmix(u64 *keys, u64 first, const u64 *end, u64 max_groups, int k, hipStream_t s)
{
    if (max_groups == 0)
        return hipSuccess;
    const u64 g = (max_groups + 1023) / 1024;
    hipLaunchKernelGGL(sk_unmix_kernel, dim3((u32)(g < 4096 ? g : 4096)), dim3(256), 0, s, keys, first,
                       reinterpret_cast<const unsigned long long *>(end), k);
    return hipGetLastError();
}

// heavy mid buckets leave the record path: out[j] = mids[idx[j]] with child_base = its k-mers; the list entry is emptied
__global__ __launch_bounds__(256) void sk_take_heavy_kernel(Node *__restrict__ mids, const u32 *__restrict__ idx, u32 n_heavy,
                                                            const u32 *__restrict__ kcount, Node *__restrict__ out)
{
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_heavy)
        return;
    const u32 i = idx[j];
    Node nd = mids[i];
    nd.child_base = kcount[i];
    out[j] = nd;
    mids[i].len = 0;
}

hipError_t launch_sk_take_heavy(Node *mids, const u32 *idx, u32 n_heavy, const u32 *kcount, Node *out, hipStream_t s)
{
    if (n_heavy == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_take_heavy_kernel, dim3((n_heavy + 255) / 256), dim3(256), 0, s, mids, idx, n_heavy, kcount, out);
    return hipGetLastError();
}

hipError_t launch_sk_slice_count(const Node *buckets, u32 nb, u32 *n_slices, hipStream_t s)
{
    if (nb == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_slice_count_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, buckets, nb, n_slices);
    return hipGetLastError();
}

hipError_t launch_sk_slice_fill(const Node *buckets, u32 nb, const u32 *slice_first, u32 *slice_rec0, u32 *slice_nrec, hipStream_t s)
{
    if (nb == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_slice_fill_kernel, dim3((nb + 3) / 4), dim3(256), 0, s, buckets, nb, slice_first, slice_rec0, slice_nrec);
    return hipGetLastError();
}

hipError_t launch_sk_slice_kmers(const void *recs, const u32 *slice_rec0, const u32 *slice_nrec, u32 n_slices, u32 *slice_km,
                                 hipStream_t s)
{
    if (n_slices == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_slice_kmers_kernel, dim3((n_slices + 3) / 4), dim3(256), 0, s, reinterpret_cast<const ull2_t *>(recs),
                       slice_rec0, slice_nrec, n_slices, slice_km);
    return hipGetLastError();
}

hipError_t launch_sk_slice_nodes(const Node *buckets, u32 nb, const u32 *slice_first, const u32 *slice_koff, u32 n_slices,
                                 const u32 *total_keys, u32 key_base, int k, bool check_kmers, Node *out, u64 *n_bad, hipStream_t s)
{
    if (nb == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_slice_nodes_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, buckets, nb, slice_first, slice_koff, n_slices,
                       total_keys, key_base, k, check_kmers ? 1 : 0, out, reinterpret_cast<unsigned long long *>(n_bad));
    return hipGetLastError();
}

hipError_t launch_sk_expand_flat(const void *recs, const u32 *slice_rec0, const u32 *slice_nrec, const u32 *slice_koff, u32 key_base,
                                 u32 n_slices, int k, u64 *keys, hipStream_t s)
{
    if (n_slices == 0)
        return hipSuccess;
    const u32 lmax = sk_lmax(k);
    const size_t smem = (size_t)4 * 64 * lmax * 8;
    const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void *>(sk_expand_flat_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)4 * 64 * 32 * 8));
    if (ae != hipSuccess)
        return ae;
    hipLaunchKernelGGL(sk_expand_flat_kernel, dim3((n_slices + 3) / 4), dim3(256), smem, s, reinterpret_cast<const ull2_t *>(recs),
                       slice_rec0, slice_nrec, slice_koff, key_base, n_slices, k, lmax, keys);
    return hipGetLastError();
}

// the 16 children of the heavy mid buckets (split by d2 with the chunked level kernels) as final-bucket nodes: start / len
// in records, child_base = k-mers; their quads are not counted (chunk_base = ~0: never sk_count's)
__global__ __launch_bounds__(256) void sk_heavy_finals_kernel(const Node *__restrict__ kids, u32 n, const u32 *__restrict__ kcount,
                                                              Node *__restrict__ out)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    Node o;
    o.start = kids[i].start;
    o.len = kids[i].len;
    o.meta = 0;
    o.split = 0;
    o.prefix = 0;
    o.child_base = kids[i].len ? kcount[i] : 0u;
    o.chunk_base = ~0u;
    out[i] = o;
}

hipError_t launch_sk_heavy_finals(const Node *kids, u32 n, const u32 *kcount, Node *out, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_heavy_finals_kernel, dim3((n + 255) / 256), dim3(256), 0, s, kids, n, kcount, out);
    return hipGetLastError();
}

}  // namespace dnagpu
