// seqeq_kernels.hip -- equal sequences on the device (dna.c:334-350, test.sql:1-20): the content fingerprint
// of every sequence of a table, the verify round over the fingerprint-sorted list, the class sizes, the match of a probe
// table against a built one, the two selects, and the comparison of two whole values.  Classes, items, the realigned word
// and the fingerprint are seqeq_math.hpp's; the sort between the sweep and the rounds is the index's (index_kernels.hip).
//
// Short sequences (at most SEQEQ_WAVE_BASES bases) are handled by groups of SEQEQ_GROUP lanes, eight sequences per wave:
// lane g of a group takes the realigned words g, g + 8, ... and the group reduces with three xor shuffles.  Neighbouring
// groups hold neighbouring sequences, so a wave reads one contiguous piece of the stream.  Long sequences are cut into
// items of SEQEQ_TILE_WORDS words, one workgroup each.  Control flow ahead of a shuffle is uniform inside a group.
#include <algorithm>

#include "kernels.hpp"
#include "seqeq_math.hpp"

namespace dnagpu {

namespace {

constexpr int SQ_THREADS = 256;
constexpr int SQ_GROUPS = SQ_THREADS / SEQEQ_GROUP;          // sequences per workgroup of a group kernel
constexpr int SQ_TILE = 2048;                                // entries per workgroup of a select sweep
constexpr int SQ_ITEMS = SQ_TILE / SQ_THREADS;
constexpr u32 SQ_NONE = 0xFFFFFFFFu;                         // no match (ids stop at 2^32 - 2)

__device__ __forceinline__ u64 group_sum(u64 v)
{
#pragma unroll
    for (int m = 1; m < SEQEQ_GROUP; m <<= 1)
        v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ u32 group_or(u32 v)
{
#pragma unroll
    for (int m = 1; m < SEQEQ_GROUP; m <<= 1)
        v |= __shfl_xor(v, m);
    return v;
}

// the first slot of fp[0 .. n) that holds a value >= f
__device__ __forceinline__ u64 lower_bound(const u64 *__restrict__ fp, u64 n, u64 f)
{
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (fp[mid] < f)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// does lane `sub` of a group see a difference between sequence (a, sa, len) and sequence (b, sb, len)?  len is short.
__device__ __forceinline__ u32 group_differs(const SeqTable &a, u64 sa, const SeqTable &b, u64 sb, u64 len, int sub)
{
    u32 neq = 0;
    const u64 nw = seqeq_words(len);
    for (u64 j = sub; j < nw; j += SEQEQ_GROUP)
        neq |= seqeq_word(a.words, a.n_words, sa, len, j) != seqeq_word(b.words, b.n_words, sb, len, j);
    return neq;
}

// ---- the fingerprint sweep

// fp[i] of every short sequence; of a long one the length's part, to which its items add.  ids[i] = i and items[i] = the
// sequence's item count (either may be null).
__global__ __launch_bounds__(SQ_THREADS) void seqeq_fp_short_kernel(SeqTable t, u64 n, u64 *__restrict__ fp, u32 *__restrict__ ids,
                                                                    u32 *__restrict__ items)
{
    const int sub = threadIdx.x & (SEQEQ_GROUP - 1);
    const u64 i = (u64)blockIdx.x * SQ_GROUPS + (threadIdx.x / SEQEQ_GROUP);
    const bool valid = i < n;
    u64 start = 0, len = 0, acc = 0;
    if (valid) {
        start = t.starts[i];
        len = t.starts[i + 1] - start;
        if (!seqeq_is_long(len)) {
            const u64 nw = seqeq_words(len);
            for (u64 j = sub; j < nw; j += SEQEQ_GROUP)
                acc += seqeq_fp_word(seqeq_word(t.words, t.n_words, start, len, j), j);
        }
    }
    acc = group_sum(acc);
    if (valid && sub == 0) {
        fp[i] = seqeq_fp_length(len) + acc;
        if (ids)
            ids[i] = (u32)i;
        if (items)
            items[i] = (u32)seqeq_items(len);
    }
}

__device__ __forceinline__ u64 block_sum_u64(u64 v, u64 *sh)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1)
        v += __shfl_xor(v, m);
    if ((threadIdx.x & 63) == 0)
        sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// one workgroup per item: fp[seq] += the item's partial sum, one 64-bit add
__global__ __launch_bounds__(SQ_THREADS) void seqeq_fp_long_kernel(SeqTable t, u64 n, const u32 *__restrict__ off, u64 *fp)
{
    __shared__ u64 sh[SQ_THREADS / 64];
    const u32 item = blockIdx.x;
    const u64 seq = profile_item_seq(off, n, item);
    const u64 start = t.starts[seq], len = t.starts[seq + 1] - start;
    u64 w0, w1;
    seqeq_item_words(len, item - off[seq], &w0, &w1);
    u64 acc = 0;
    for (u64 j = w0 + threadIdx.x; j < w1; j += SQ_THREADS)
        acc += seqeq_fp_word(seqeq_word(t.words, t.n_words, start, len, j), j);
    acc = block_sum_u64(acc, sh);
    if (threadIdx.x == 0)
        atomicAdd(reinterpret_cast<unsigned long long *>(&fp[seq]), (unsigned long long)acc);
}

__global__ __launch_bounds__(SQ_THREADS) void seqeq_weaken_kernel(u64 *__restrict__ fp, u64 n)
{
    const u64 i = (u64)blockIdx.x * SQ_THREADS + threadIdx.x;
    if (i < n)
        fp[i] &= SEQEQ_WEAK_MASK;
}

// ---- the verify round over a fingerprint-sorted list (lfp, lid)[0 .. m), ids ascending inside a run

// The heads of the runs without a search: head[i] = 1 where a run starts; with run = the exclusive scan of head, the entry
// at slot i belongs to run number run[i] + head[i] - 1, and every head stores its slot under its run's number.
__global__ __launch_bounds__(SQ_THREADS) void seqeq_head_flags_kernel(const u64 *__restrict__ lfp, u64 m, u32 *__restrict__ head)
{
    const u64 i = (u64)blockIdx.x * SQ_THREADS + threadIdx.x;
    if (i < m)
        head[i] = (i == 0 || lfp[i - 1] != lfp[i]) ? 1u : 0u;
}
__global__ __launch_bounds__(SQ_THREADS) void seqeq_head_slots_kernel(const u32 *__restrict__ head, const u32 *__restrict__ run, u64 m,
                                                                      u32 *__restrict__ slot)
{
    const u64 i = (u64)blockIdx.x * SQ_THREADS + threadIdx.x;
    if (i < m && head[i])
        slot[run[i]] = (u32)i;
}

// Entry i against the head of its run: hidx[i] = the head's slot, eq[i] = 1 for the head itself and for an entry whose
// length and bases equal the head's.  A long pair of equal lengths gets eq = 1 and items[i] = its item count: the item
// kernel clears eq where an item differs.  items[i] = 0 otherwise.
__global__ __launch_bounds__(SQ_THREADS) void seqeq_verify_kernel(SeqTable t, const u32 *__restrict__ lid, u64 m,
                                                                  const u32 *__restrict__ head, const u32 *__restrict__ run,
                                                                  const u32 *__restrict__ slot, u32 *__restrict__ hidx,
                                                                  u32 *__restrict__ eq, u32 *__restrict__ items)
{
    const int sub = threadIdx.x & (SEQEQ_GROUP - 1);
    const u64 i = (u64)blockIdx.x * SQ_GROUPS + (threadIdx.x / SEQEQ_GROUP);
    const bool valid = i < m;
    u64 h = 0;
    u32 e = 0, it = 0, neq = 0;
    bool compare = false;
    if (valid) {
        h = head[i] ? i : slot[run[i] - 1];
        if (h == i) {
            e = 1;
        } else {
            const u64 a = lid[i], b = lid[h];
            const u64 sa = t.starts[a], la = t.starts[a + 1] - sa;
            const u64 sb = t.starts[b], lb = t.starts[b + 1] - sb;
            if (la == lb) {
                if (seqeq_is_long(la)) {
                    e = 1;
                    it = (u32)seqeq_items(la);
                } else {
                    compare = true;
                    neq = group_differs(t, sa, t, sb, la, sub);
                }
            }
        }
    }
    neq = group_or(neq);
    if (compare)
        e = neq ? 0u : 1u;
    if (valid && sub == 0) {
        hidx[i] = (u32)h;
        eq[i] = e;
        items[i] = it;
    }
}

// One workgroup per item of a long pair.  Pair p = sequence (ia ? ia[p] : p) of table a against sequence ib[ib_slot[p]] of
// table b, equal lengths; off = the exclusive scan of the pairs' item counts.  An item that differs stores 0 into flag[p]:
// every writer stores the same value.
__global__ __launch_bounds__(SQ_THREADS) void seqeq_pair_items_kernel(SeqTable a, const u32 *__restrict__ ia, SeqTable b,
                                                                      const u32 *__restrict__ ib, const u32 *__restrict__ ib_slot,
                                                                      u64 n_pairs, const u32 *__restrict__ off, u32 *flag)
{
    const u32 item = blockIdx.x;
    const u64 p = profile_item_seq(off, n_pairs, item);
    const u64 qa = ia ? ia[p] : p, qb = ib[ib_slot[p]];
    const u64 sa = a.starts[qa], len = a.starts[qa + 1] - sa, sb = b.starts[qb];
    u64 w0, w1;
    seqeq_item_words(len, item - off[p], &w0, &w1);
    bool differs = false;
    for (u64 j = w0 + threadIdx.x; j < w1; j += SQ_THREADS)
        differs |= seqeq_word(a.words, a.n_words, sa, len, j) != seqeq_word(b.words, b.n_words, sb, len, j);
    if (differs)
        flag[p] = 0;
}

// pre = the exclusive scan of eq.  An equal entry takes its head as rep; the others move, in order, to (out_fp, out_id);
// the last entry of a run stores the run's equal entries as the head's class size -- one plain store per class, because a
// class is settled in exactly one round.
__global__ __launch_bounds__(SQ_THREADS) void seqeq_apply_kernel(const u64 *__restrict__ lfp, const u32 *__restrict__ lid, u64 m,
                                                                 const u32 *__restrict__ hidx, const u32 *__restrict__ eq,
                                                                 const u32 *__restrict__ pre, u32 *__restrict__ rep,
                                                                 u32 *__restrict__ copies, u64 *__restrict__ out_fp,
                                                                 u32 *__restrict__ out_id, u64 n_out)
{
    const u64 i = (u64)blockIdx.x * SQ_THREADS + threadIdx.x;
    if (i >= m)
        return;
    const u64 f = lfp[i];
    const u32 id = lid[i], h = hidx[i], e = eq[i], before = pre[i];
    const u32 head = lid[h];
    if (e) {
        rep[id] = head;
    } else {
        const u64 pos = i - before;
        if (pos < n_out) {                                 // (always: n_out = m - the sum of eq)
            out_fp[pos] = f;
            out_id[pos] = id;
        }
    }
    if (i + 1 == m || lfp[i + 1] != f)
        copies[head] = before + e - pre[h];
}

// copies[s] = copies[rep[s]] for every member that is not its class's representative; *distinct += the representatives
__global__ __launch_bounds__(SQ_THREADS) void seqeq_spread_kernel(const u32 *__restrict__ rep, u32 *copies, u64 n,
                                                                  unsigned long long *distinct)
{
    const u64 s = (u64)blockIdx.x * SQ_THREADS + threadIdx.x;
    bool is_rep = false;
    if (s < n) {
        const u32 r = rep[s];
        is_rep = r == s;
        if (!is_rep)
            copies[s] = copies[r];                         // (a representative's entry is never written here)
    }
    const int c = __syncthreads_count(is_rep);
    if (threadIdx.x == 0 && c)
        atomicAdd(distinct, (unsigned long long)c);
}

// ---- match

// One group per probe sequence.  first != 0: every probe starts at the lower bound of its fingerprint in the built side's
// sorted list.  first == 0: only the probes parked on a long candidate (items[p] != 0) go on -- flag[p] != 0: the candidate
// at slot cur[p] is the match; else the walk resumes behind it.  The walk visits the run's representatives of equal length:
// a short one is compared here; at a long one the probe parks (cur, flag = 1, items = its item count) for the item kernel.
__global__ __launch_bounds__(SQ_THREADS) void seqeq_match_walk_kernel(SeqTable pt, u64 np, const u64 *__restrict__ pfp, SeqTable bt,
                                                                      const u64 *__restrict__ sfp, const u32 *__restrict__ sid,
                                                                      u64 nb, const u32 *__restrict__ rep, int first, u32 *cur,
                                                                      u32 *flag, u32 *items, u32 *match)
{
    const int sub = threadIdx.x & (SEQEQ_GROUP - 1);
    const u64 p = (u64)blockIdx.x * SQ_GROUPS + (threadIdx.x / SEQEQ_GROUP);
    const bool walks = p < np && (first || items[p] != 0);
    bool pending = walks;
    u64 j = 0, f = 0, sp = 0, len = 0;
    u32 found = SQ_NONE, park_items = 0;
    if (pending) {
        f = pfp[p];
        sp = pt.starts[p];
        len = pt.starts[p + 1] - sp;
        if (first) {
            j = lower_bound(sfp, nb, f);
        } else {
            j = cur[p];
            if (flag[p]) {
                found = sid[j];
                pending = false;
            }
            j++;
        }
    }
    while (pending && j < nb && sfp[j] == f) {
        const u32 id = sid[j];
        bool candidate = false;
        u64 sb = 0;
        if (rep[id] == id) {
            sb = bt.starts[id];
            candidate = bt.starts[id + 1] - sb == len;
        }
        if (candidate && seqeq_is_long(len)) {
            park_items = (u32)seqeq_items(len);
            break;
        }
        const u32 neq = group_or(candidate ? group_differs(pt, sp, bt, sb, len, sub) : 1u);
        if (!neq) {
            found = id;
            break;
        }
        j++;
    }
    if (walks && sub == 0) {
        items[p] = park_items;
        if (park_items) {
            cur[p] = (u32)j;
            flag[p] = 1;
        } else {
            match[p] = found;
        }
    }
}

// match32 == nullptr: nothing was built, no probe matches.  *n_matched += the probes with a match.
__global__ __launch_bounds__(SQ_THREADS) void seqeq_match_out_kernel(const u32 *__restrict__ match32, const u32 *__restrict__ copies,
                                                                     u64 n, u64 *__restrict__ out_match, u64 *__restrict__ out_copies,
                                                                     unsigned long long *n_matched)
{
    const u64 p = (u64)blockIdx.x * SQ_THREADS + threadIdx.x;
    bool hit = false;
    if (p < n) {
        const u32 m = match32 ? match32[p] : SQ_NONE;
        hit = m != SQ_NONE;
        if (out_match)
            out_match[p] = hit ? (u64)m : ~(u64)0;
        if (out_copies)
            out_copies[p] = hit ? (u64)copies[m] : 0;
    }
    const int c = __syncthreads_count(hit);
    if (threadIdx.x == 0 && c)
        atomicAdd(n_matched, (unsigned long long)c);
}

// ---- the selects: the tile layout of the index's compaction (wave w owns a contiguous quarter of the tile, element (item
// i, lane l) at slice + 64 i + l); WRITE = false: tiles[tile] = the matches; WRITE = true: tiles = their exclusive scan
__device__ __forceinline__ bool selected(const SeqSelect &q, u32 s, u32 r, u32 c)
{
    return q.members ? r == q.target : (r == s && c >= q.lo && c <= q.hi);
}

template <bool WRITE>
__global__ __launch_bounds__(SQ_THREADS) void seqeq_select_kernel(const u32 *__restrict__ rep, const u32 *__restrict__ copies, u64 n,
                                                                  SeqSelect q, u32 *__restrict__ tiles, u64 *__restrict__ out_seq,
                                                                  u64 *__restrict__ out_copies, u64 cap)
{
    __shared__ u32 wsum[SQ_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 slice = (u64)blockIdx.x * SQ_TILE + (u64)wave * 64 * SQ_ITEMS;
    u32 rank[SQ_ITEMS], cop[SQ_ITEMS];
    u32 kept = 0, cnt = 0;
#pragma unroll
    for (int i = 0; i < SQ_ITEMS; i++) {
        const u64 s = slice + (u64)i * 64 + lane;
        bool keep = false;
        cop[i] = 0;
        if (s < n) {
            cop[i] = copies[s];
            keep = selected(q, (u32)s, rep[s], cop[i]);
        }
        const u64 bal = __ballot(keep);
        rank[i] = cnt + (u32)__popcll(bal & (((u64)1 << lane) - 1));
        cnt += (u32)__popcll(bal);
        kept |= keep ? 1u << i : 0u;
    }
    if (lane == 0)
        wsum[wave] = cnt;
    __syncthreads();
    if (!WRITE) {
        if (tid == 0)
            tiles[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        return;
    }
    u64 base = tiles[blockIdx.x];
    for (int w = 0; w < wave; w++)
        base += wsum[w];
#pragma unroll
    for (int i = 0; i < SQ_ITEMS; i++)
        if (kept & (1u << i)) {
            const u64 pos = base + rank[i];
            if (pos < cap) {
                if (out_seq)
                    out_seq[pos] = slice + (u64)i * 64 + lane;
                if (out_copies)
                    out_copies[pos] = cop[i];
            }
        }
}

// ---- two whole values of n_bases bases each, both from base 0: a word that differs stores 0 into *flag (the caller set it
// to a non-zero value); the last word is compared up to the last base only
__global__ __launch_bounds__(SQ_THREADS) void seqeq_whole_kernel(const u64 *__restrict__ a, u64 a_words, const u64 *__restrict__ b,
                                                                 u64 b_words, u64 n_bases, u32 *flag)
{
    const u64 nw = seqeq_words(n_bases);
    bool differs = false;
    for (u64 j = (u64)blockIdx.x * SQ_THREADS + threadIdx.x; j < nw; j += (u64)gridDim.x * SQ_THREADS)
        differs |= seqeq_word(a, a_words, 0, n_bases, j) != seqeq_word(b, b_words, 0, n_bases, j);
    if (differs)
        *flag = 0;
}

unsigned group_blocks(u64 n) { return (unsigned)((n + SQ_GROUPS - 1) / SQ_GROUPS); }
unsigned thread_blocks(u64 n) { return (unsigned)((n + SQ_THREADS - 1) / SQ_THREADS); }

}  // namespace

hipError_t launch_seqeq_fp_short(const SeqTable &t, u64 n, u64 *fp, u32 *ids, u32 *items, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_fp_short_kernel, dim3(group_blocks(n)), dim3(SQ_THREADS), 0, s, t, n, fp, ids, items);
    return hipGetLastError();
}

hipError_t launch_seqeq_fp_long(const SeqTable &t, u64 n, const u32 *off, u32 n_items, u64 *fp, hipStream_t s)
{
    if (n_items == 0)
        return hipSuccess;
    hipLaunchKernelGGL(seqeq_fp_long_kernel, dim3(n_items), dim3(SQ_THREADS), 0, s, t, n, off, fp);
    return hipGetLastError();
}

hipError_t launch_seqeq_weaken(u64 *fp, u64 n, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_weaken_kernel, dim3(thread_blocks(n)), dim3(SQ_THREADS), 0, s, fp, n);
    return hipGetLastError();
}

hipError_t launch_seqeq_head_flags(const u64 *lfp, u64 m, u32 *head, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_head_flags_kernel, dim3(thread_blocks(m)), dim3(SQ_THREADS), 0, s, lfp, m, head);
    return hipGetLastError();
}

hipError_t launch_seqeq_head_slots(const u32 *head, const u32 *run, u64 m, u32 *slot, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_head_slots_kernel, dim3(thread_blocks(m)), dim3(SQ_THREADS), 0, s, head, run, m, slot);
    return hipGetLastError();
}

hipError_t launch_seqeq_verify(const SeqTable &t, const u32 *lid, u64 m, const u32 *head, const u32 *run, const u32 *slot, u32 *hidx,
                               u32 *eq, u32 *items, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_verify_kernel, dim3(group_blocks(m)), dim3(SQ_THREADS), 0, s, t, lid, m, head, run, slot, hidx, eq,
                       items);
    return hipGetLastError();
}

hipError_t launch_seqeq_pair_items(const SeqTable &a, const u32 *ia, const SeqTable &b, const u32 *ib, const u32 *ib_slot,
                                   u64 n_pairs, const u32 *off, u32 n_items, u32 *flag, hipStream_t s)
{
    if (n_items == 0)
        return hipSuccess;
    hipLaunchKernelGGL(seqeq_pair_items_kernel, dim3(n_items), dim3(SQ_THREADS), 0, s, a, ia, b, ib, ib_slot, n_pairs, off, flag);
    return hipGetLastError();
}

hipError_t launch_seqeq_apply(const u64 *lfp, const u32 *lid, u64 m, const u32 *hidx, const u32 *eq, const u32 *pre, u32 *rep,
                              u32 *copies, u64 *out_fp, u32 *out_id, u64 n_out, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_apply_kernel, dim3(thread_blocks(m)), dim3(SQ_THREADS), 0, s, lfp, lid, m, hidx, eq, pre, rep, copies,
                       out_fp, out_id, n_out);
    return hipGetLastError();
}

hipError_t launch_seqeq_spread(const u32 *rep, u32 *copies, u64 n, u64 *distinct, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_spread_kernel, dim3(thread_blocks(n)), dim3(SQ_THREADS), 0, s, rep, copies, n,
                       reinterpret_cast<unsigned long long *>(distinct));
    return hipGetLastError();
}

hipError_t launch_seqeq_match_walk(const SeqTable &pt, u64 np, const u64 *pfp, const SeqTable &bt, const u64 *sfp, const u32 *sid,
                                   u64 nb, const u32 *rep, int first, u32 *cur, u32 *flag, u32 *items, u32 *match, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_match_walk_kernel, dim3(group_blocks(np)), dim3(SQ_THREADS), 0, s, pt, np, pfp, bt, sfp, sid, nb, rep,
                       first, cur, flag, items, match);
    return hipGetLastError();
}

hipError_t launch_seqeq_match_out(const u32 *match32, const u32 *copies, u64 n, u64 *out_match, u64 *out_copies, u64 *n_matched,
                                  hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_match_out_kernel, dim3(thread_blocks(n)), dim3(SQ_THREADS), 0, s, match32, copies, n, out_match,
                       out_copies, reinterpret_cast<unsigned long long *>(n_matched));
    return hipGetLastError();
}

u32 seqeq_select_tiles(u64 n)
{
    return (u32)((n + SQ_TILE - 1) / SQ_TILE);
}

hipError_t launch_seqeq_select_count(const u32 *rep, const u32 *copies, u64 n, const SeqSelect &q, u32 *tile_counts, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_select_kernel<false>, dim3(seqeq_select_tiles(n)), dim3(SQ_THREADS), 0, s, rep, copies, n, q, tile_counts,
                       (u64 *)nullptr, (u64 *)nullptr, (u64)0);
    return hipGetLastError();
}

hipError_t launch_seqeq_select_write(const u32 *rep, const u32 *copies, u64 n, const SeqSelect &q, const u32 *tile_offsets,
                                     u64 *out_seq, u64 *out_copies, u64 cap, hipStream_t s)
{
    hipLaunchKernelGGL(seqeq_select_kernel<true>, dim3(seqeq_select_tiles(n)), dim3(SQ_THREADS), 0, s, rep, copies, n, q,
                       const_cast<u32 *>(tile_offsets), out_seq, out_copies, cap);
    return hipGetLastError();
}

hipError_t launch_seqeq_whole(const u64 *a, u64 a_words, const u64 *b, u64 b_words, u64 n_bases, u32 *flag, hipStream_t s)
{
    const u64 nw = seqeq_words(n_bases);
    const unsigned blocks = (unsigned)std::min<u64>(std::max<u64>(thread_blocks(nw), 1), 2048);
    hipLaunchKernelGGL(seqeq_whole_kernel, dim3(blocks), dim3(SQ_THREADS), 0, s, a, a_words, b, b_words, n_bases, flag);
    return hipGetLastError();
}

}  // namespace dnagpu
