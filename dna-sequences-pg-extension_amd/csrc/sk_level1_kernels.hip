// sk_level1_kernels.hip -- the record levels of the super-k-mer engine (sk_device.hpp): level 1 moves a coarse bucket's
// records into mid buckets (sk_hist1 / sk_scatter1, or speculatively into regions: sk_spec_*, sk_sample1), sk_regroup
// regroups a mid bucket's records into its 16 final buckets.
#include "sk_device.hpp"

namespace dnagpu {

// ------------------------------------------------------------------------------------------------
// sk_hist1: records of a chunk of a coarse node by d1; also the k-mers of every (node, d1) = mid bucket
constexpr int SK1_NT = 1024;
__global__ __launch_bounds__(SK1_NT) void sk_hist1_kernel(const Node *__restrict__ nodes, const Chunk *__restrict__ chunks,
                                                          u32 n_chunks, const ull2_t *__restrict__ recs,
                                                          u32 *__restrict__ hist, u32 *__restrict__ kcount, int shift)
{
    __shared__ u32 h[ROW_STRIDE];
    __shared__ u32 kc[ROW_STRIDE];
    if (blockIdx.x >= n_chunks)
        return;
    const Chunk ch = chunks[blockIdx.x];
    const Node nd = nodes[ch.node];
    const u32 R = 1u << nd.split;
    for (u32 d = threadIdx.x; d < R; d += SK1_NT) {
        h[d] = 0;
        kc[d] = 0;
    }
    __syncthreads();
    const u64 *hi = reinterpret_cast<const u64 *>(recs + (u64)nd.start + ch.off) + 1;
    u32 i = threadIdx.x;
    for (; i + 3u * SK1_NT < ch.len; i += 4u * SK1_NT) {           // four loads in flight per thread
        u64 m[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            m[j] = __builtin_nontemporal_load(&hi[(u64)(i + (u32)j * SK1_NT) * 2]);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (m[j] >> 63)
                continue;                          // (a NULL record: an unused slot of a slab sweep)
            const u32 d1 = (u32)(m[j] >> shift) & (R - 1);
            atomicAdd(&h[d1], 1u);
            atomicAdd(&kc[d1], (u32)((m[j] >> 44) & 31) + 1u);
        }
    }
    for (; i < ch.len; i += SK1_NT) {
        const u64 m = __builtin_nontemporal_load(&hi[(u64)i * 2]);
        if (m >> 63)
            continue;
        const u32 d1 = (u32)(m >> shift) & (R - 1);
        atomicAdd(&h[d1], 1u);
        atomicAdd(&kc[d1], (u32)((m >> 44) & 31) + 1u);
    }
    __syncthreads();
    u32 *row = hist + (u64)blockIdx.x * ROW_STRIDE;
    for (u32 d = threadIdx.x; d < R; d += SK1_NT) {
        row[d] = h[d];
        if (kc[d])
            atomicAdd(&kcount[nd.child_base + d], kc[d]);
    }
}

// A SAMPLE of the same histogram, for the regions of a speculative level 1 over uneven coarse buckets (repeats): the chunks
// are pieces of SK1_SAMPLE_LEN records, one in every SK1_SAMPLE_EVERY of a node's records (the host lists them); est[mid
// bucket] += the records of the piece that fall into it.
constexpr u32 SK1_SAMPLE_LEN = 1024, SK1_SAMPLE_EVERY = 8;
u32 sk_sample1_len() { return SK1_SAMPLE_LEN; }
u32 sk_sample1_every() { return SK1_SAMPLE_EVERY; }
__global__ __launch_bounds__(SK1_NT) void sk_sample1_kernel(const Node *__restrict__ nodes, const Chunk *__restrict__ chunks,
                                                            u32 n_chunks, const ull2_t *__restrict__ recs, u32 *__restrict__ est)
{
    __shared__ u32 h[ROW_STRIDE];
    if (blockIdx.x >= n_chunks)
        return;
    const Chunk ch = chunks[blockIdx.x];
    const Node nd = nodes[ch.node];
    const u32 R = 1u << nd.split;
    for (u32 d = threadIdx.x; d < R; d += SK1_NT)
        h[d] = 0;
    __syncthreads();
    const u64 *hi = reinterpret_cast<const u64 *>(recs + (u64)nd.start + ch.off) + 1;
    for (u32 i = threadIdx.x; i < ch.len; i += SK1_NT) {
        const u64 m = __builtin_nontemporal_load(&hi[(u64)i * 2]);
        if (!(m >> 63))
            atomicAdd(&h[(u32)(m >> 49) & (R - 1)], 1u);
    }
    __syncthreads();
    for (u32 d = threadIdx.x; d < R; d += SK1_NT)
        if (h[d])
            atomicAdd(&est[nd.child_base + d], h[d]);
}

// Slots of a mid bucket whose sample held est records: the estimate, five standard deviations of it (a Poisson count
// scaled by the sampling factor) and 128, whole 128-byte lines.  (A region's unused slots cost memory only: the mid
// node's length is what the sweep drew.)
__global__ __launch_bounds__(256) void sk_sampled_caps_kernel(const u32 *__restrict__ est, u32 n_mid, u32 *__restrict__ rcap)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_mid)
        return;
    const u64 e = est[i];
    const u64 cap = e * SK1_SAMPLE_EVERY + 5ull * SK1_SAMPLE_EVERY * sk_isqrt(e) + 128ull + 7ull;
    rcap[i] = (u32)(cap < 0xFFFFFFF8ull ? cap : 0xFFFFFFF8ull) & ~7u;
}

// sk_scatter1: tiles of 8192 records, grouped by d1 in LDS and copied to their mid buckets in sorted order, 16 bytes per
// lane (16 records per digit and tile on average: 256-byte runs).  Full tiles keep their records in registers between the
// one read and the staging; the chunk's last, partial tile ranks an index list and gathers.
constexpr int SK1_ITEMS = 8;
constexpr int SK1_TILE = SK1_NT * SK1_ITEMS;
constexpr int SK1_STAGE = SK1_TILE / 2 + 64;     // records the stage holds: half a tile and a digit's worth of slack
// SPEC (level 1 without its histogram): the mid buckets are REGIONS of the destination buffer -- spec[2 node] = start of
// the node's first, spec[2 node + 1] = records each holds, the cursors start at the regions' starts (sk_spec_*_kernel below)
// -- and the sweep counts the k-mers per mid bucket itself (kcount).  A record that does not fit its region is dropped and
// raises *over: the caller then runs the exact level (histogram, prefix, this kernel without SPEC).
template <bool SPEC>
__global__ __launch_bounds__(SK1_NT, 8) void sk_scatter1_kernel(const Node *__restrict__ nodes, const Chunk *__restrict__ chunks,
                                                             u32 n_chunks, const ull2_t *__restrict__ src_all,
                                                             ull2_t *__restrict__ dst_all, const u32 *__restrict__ hist,
                                                             const u32 *__restrict__ tot, int shift, u32 *__restrict__ gcur,
                                                             const u32 *__restrict__ spec, u32 *__restrict__ kcount,
                                                             u32 *__restrict__ over, const u32 *__restrict__ rstart,
                                                             const u32 *__restrict__ rcapv /* or null: see sk_spec_* below */)
{
    __shared__ u32 cnt[ROW_STRIDE];
    __shared__ u32 glim[SPEC ? ROW_STRIDE : 1];    // SPEC: the end of digit d's region
    // gadj[d]: where the tile's sorted slot sl of digit d goes = gadj[d] + sl (the digit's base in the destination minus its
    // offset in the tile).  gpos[d] (only without global cursors: the by-d2 split of heavy buckets): the chunk's running
    // position in digit d.
    __shared__ u32 gadj[ROW_STRIDE];
    __shared__ u32 gpos[SPEC ? 1 : ROW_STRIDE];
    // a full tile: about half of its records at a time, in sorted order; a partial tile: the index list (16 KB of it)
    __shared__ __attribute__((aligned(16))) ull2_t stage[SK1_STAGE];
    unsigned short *idx = reinterpret_cast<unsigned short *>(stage);
    // SPEC: while a tile is counted the stage's first words hold, per digit, records | k-mers << 32 -- ONE 64-bit LDS add
    // per record counts both (round 3: two 32-bit adds); thread d keeps digit d's k-mers of the whole chunk in a register
    u64 *c64 = reinterpret_cast<u64 *>(stage);
    u32 kacc = 0;
    __shared__ u32 wtmp[SK1_NT / 64];
    __shared__ u32 split[4];                       // a full tile's halves: [0] first digit of the second, [1] its offset, [2] skew
    if (blockIdx.x >= n_chunks)
        return;
    int tid = threadIdx.x;
    const Chunk ch = chunks[blockIdx.x];
    const Node nd = nodes[ch.node];
    const u32 R = 1u << nd.split;
    const u32 *hrow = hist + (u64)blockIdx.x * ROW_STRIDE;
    const u32 *trow = tot + (u64)nd.chunk_base * ROW_STRIDE;          // absolute base of every digit of the node
    // gcur != null: the node's digits have GLOBAL cursors (a copy of `tot`: they start at the digits' absolute bases) and
    // every tile reserves its slots there, one returning add per digit, in flight while the tile is staged.  The chunks of a
    // node then fill a mid bucket in arrival order instead of each into a range of its own: a run's partial first and last
    // cache lines are completed by whichever workgroup writes to the bucket next, soon, while they are still in L2, and
    // the per-tile cursor update with its barrier is gone (3.27 -> 2.92 ms at 3 Gbase).  ~300 adds per address and count.
    u32 *gc = gcur ? gcur + (u64)nd.chunk_base * ROW_STRIDE : nullptr;
    if (!SPEC && !gc)
        for (u32 d = tid; d < R; d += SK1_NT)
            gpos[d] = trow[d] + hrow[d];
    const ull2_t *src = src_all + (u64)nd.start + ch.off;
    const u32 dmask = R - 1;
    bool dropped = false;
    if (SPEC) {
        // digit d's region: [reg0 + d rcap, reg0 + (d + 1) rcap) from its parent's size, or -- over uneven coarse buckets --
        // rstart / rcapv per mid bucket from a sampled histogram
        const u32 reg0 = spec[2 * ch.node], rcap = spec[2 * ch.node + 1];
        for (u32 d = tid; d < R; d += SK1_NT)
            glim[d] = rcapv ? rstart[nd.child_base + d] + rcapv[nd.child_base + d] : reg0 + (d + 1) * rcap;
    }
    // after the tile's digit counts have become offsets (cnt[d]; cnt[R] = the tile's records): digit tid's slots in the
    // destination -- reserved from its global cursor, or the chunk's own running position -- as gadj[tid]
    // The reservation is ISSUED here (a returning add on a global cursor: microseconds) and FINISHED -- gadj written -- only
    // where the tile's first write-out needs it: the staging of the first half runs while it is in flight.
    u32 pl_base = 0;
    bool pl_pending = false;
    auto place_issue = [&]() {
        if ((u32)tid < R) {
            const u32 lo = cnt[tid], c = cnt[tid + 1] - lo;
            pl_base = 0;
            if (gc) {
                if (c)
                    pl_base = atomicAdd(&gc[tid], c);
            } else if (!SPEC) {
                pl_base = gpos[tid];
                gpos[tid] = pl_base + c;
            }
            gadj[tid] = 0u - lo;
            pl_pending = true;
        }
    };
    auto place_finish = [&]() {
        if (pl_pending) {
            gadj[tid] += pl_base;                  // (SPEC: a record that falls behind its region's end is dropped, and
            pl_pending = false;                    // reported, where it is written)
        }
    };
    // the tile's digit counts (cnt[], or -- SPEC -- c64[] with the k-mers in the high words) -> exclusive offsets in cnt[],
    // cnt[R] = the tile's records
    auto scan_counts = [&]() {
        u32 v = 0;
        if ((u32)tid <= R) {
            if (SPEC) {
                const u64 w = c64[tid];
                v = (u32)w;
                kacc += (u32)(w >> 32);
            } else {
                v = cnt[tid];
            }
        }
        block_scan_value<SK1_NT>(v, cnt, (int)R + 1, wtmp, tid);       // (R + 1 <= 513)
    };
    for (u32 t0 = 0; t0 < ch.len; t0 += SK1_TILE) {
        const u32 n_tile = ch.len - t0 < (u32)SK1_TILE ? ch.len - t0 : (u32)SK1_TILE;
        asm volatile("" : "+v"(tid));              // (thread-derived addresses recomputed per tile, not held: the kernel lives on 64 registers)
        for (u32 d = tid; d <= R; d += SK1_NT) {   // (bin R: NULL records -- unused slots of a slab sweep -- sort behind all digits)
            if (SPEC)
                c64[d] = 0;
            else
                cnt[d] = 0;
        }
        if (tid == 0) {
            split[0] = R;                          // (a tile of at most SK1_STAGE records: one half)
            split[2] = 0;
        }
        __syncthreads();
        bool gather = n_tile != (u32)SK1_TILE, placed = false;
        if (!gather) {
            // ---- a full tile (all tiles of a chunk but its last): every record is read ONCE, 16 bytes per lane and all
            // eight of a thread in flight; it waits in registers while the tile's digits are counted, then takes its slot in
            // the sorted order from its digit's LDS cursor and goes through the stage, digits [0, s) first and [s, R) second
            // (s = the digit that holds sorted slot SK1_STAGE: both halves fit unless that one digit has more than 128
            // records in this tile -- skew, the gather below), and leaves in runs -- 16 bytes per lane, consecutive lanes to
            // consecutive addresses.  No sorted position is ever kept in a register (round 3 kept eight, and spilled 23
            // VGPRs around the scan: 96 bytes of scratch per lane and tile).  (Reading the digits first and gathering the
            // records by index afterwards -- the partial tile's way below -- brings every record in twice: 16 GB moved for 10.7.)
            ull2_t rec[SK1_ITEMS];
#pragma unroll
            for (int j = 0; j < SK1_ITEMS; j++)
                rec[j] = src[t0 + tid + j * SK1_NT];
#pragma unroll
            for (int j = 0; j < SK1_ITEMS; j++) {
                const bool null = (rec[j].y >> 63) != 0;
                const u32 dg = null ? R : (u32)(rec[j].y >> shift) & dmask;
                if (SPEC)
                    atomicAdd(reinterpret_cast<unsigned long long *>(&c64[dg]),
                              null ? 1ull : 1ull | ((unsigned long long)(((u32)(rec[j].y >> 44) & 31u) + 1u) << 32));
                else
                    atomicAdd(&cnt[dg], 1u);
            }
            __syncthreads();
            scan_counts();
            const u32 n_valid = cnt[R];
            if ((u32)tid < R && cnt[tid] <= (u32)SK1_STAGE && cnt[tid + 1] > (u32)SK1_STAGE) {
                split[0] = (u32)tid;               // (exactly one digit holds slot SK1_STAGE, if the tile has that many)
                split[1] = cnt[tid];
                split[2] = n_valid - cnt[tid] > (u32)SK1_STAGE ? 1u : 0u;
            }
            place_issue();
            placed = true;
            __syncthreads();                       // (the offsets have been read: the cursors below move them)
            const u32 s_dig = split[0];
            gather = split[2] != 0;
            if (!gather) {
                const u32 s_off = s_dig < R ? split[1] : n_valid;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const u32 lo = h ? s_off : 0u, hi = h ? n_valid : s_off;   // sorted slots of this half
                    if (lo == hi)
                        continue;                  // (wave-uniform, workgroup-uniform)
#pragma unroll
                    for (int j = 0; j < SK1_ITEMS; j++) {
                        const u32 dg = (u32)(rec[j].y >> shift) & dmask;
                        if (!(rec[j].y >> 63) && (dg >= s_dig) == (h != 0))
                            stage[atomicAdd(&cnt[dg], 1u) - lo] = rec[j];
                    }
                    place_finish();
                    __syncthreads();
#pragma unroll
                    for (int j = 0; j < (SK1_STAGE + SK1_NT - 1) / SK1_NT; j++) {
                        const u32 sl = lo + (u32)tid + (u32)j * SK1_NT;
                        if (sl >= hi)
                            continue;
                        const ull2_t r = stage[sl - lo];
                        const u32 d = (u32)(r.y >> shift) & dmask;
                        // (a plain store: a run's first and last cache lines are partial, and the same digit's next run --
                        // this workgroup's next tile -- completes them; kept in L2 they merge more often: 3.44 -> 3.30 ms)
                        const u32 p = gadj[d] + sl;
                        if (!SPEC || p < glim[d])
                            dst_all[p] = r;
                        else
                            dropped = true;
                    }
                    __syncthreads();
                }
            } else {
                place_finish();
                for (u32 d = tid; d <= R; d += SK1_NT)
                    cnt[d] = 0;                    // (the gather ranks the tile again; its slots are reserved already)
                __syncthreads();
            }
        }
        if (gather) {
            u32 dig[SK1_ITEMS], rank[SK1_ITEMS];
#pragma unroll
            for (int j = 0; j < SK1_ITEMS; j++) {
                const u32 i = tid + j * SK1_NT;
                dig[j] = 0;
                rank[j] = 0;
                if (i < n_tile) {
                    const u64 m = reinterpret_cast<const u64 *>(src + t0 + i)[1];
                    const bool null = (m >> 63) != 0;
                    dig[j] = null ? R : (u32)(m >> shift) & dmask;
                    if (SPEC && !placed) {         // (records | k-mers << 32: the returned low word is the rank)
                        rank[j] = (u32)atomicAdd(reinterpret_cast<unsigned long long *>(&c64[dig[j]]),
                                                 null ? 1ull : 1ull | ((unsigned long long)(((u32)(m >> 44) & 31u) + 1u) << 32));
                    } else {
                        rank[j] = atomicAdd(&cnt[dig[j]], 1u);
                    }
                }
            }
            __syncthreads();
            if (SPEC && !placed)
                scan_counts();
            else
                block_scan_small<SK1_NT>(cnt, (int)R + 1, wtmp, tid);  // cnt -> exclusive offsets; cnt[R] = the tile's records
            if (!placed) {
                place_issue();
                place_finish();
            }
#pragma unroll
            for (int j = 0; j < SK1_ITEMS; j++) {
                const u32 i = tid + j * SK1_NT;
                if (i < n_tile)
                    idx[cnt[dig[j]] + rank[j]] = (unsigned short)i;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SK1_ITEMS; j++) {
                const u32 sl = tid + j * SK1_NT;
                if (sl < cnt[R]) {
                    const ull2_t r = src[t0 + idx[sl]];
                    const u32 d = (u32)(r.y >> shift) & dmask;
                    const u32 p = gadj[d] + sl;
                    if (!SPEC || p < glim[d])
                        __builtin_nontemporal_store(r, &dst_all[p]);
                    else
                        dropped = true;
                }
            }
            __syncthreads();
        }
    }
    if (SPEC) {
        if ((u32)tid < R && kacc)
            atomicAdd(&kcount[nd.child_base + (u32)tid], kacc);
        if (dropped)
            *over = 1u;
    }
}

// The regions of a speculative level 1: a node of len records split R ways gives each child len / R + 12.5 % + 72 slots,
// whole 128-byte lines (on random sequence a mid bucket is Poisson around ~4,800: the slack is > 8 sigma).  Host and
// device use this one formula (the host sizes the buffers with it).
__host__ __device__ inline u32 sk_spec_cap(u32 len, u32 R)
{
    return ((u32)(((u64)len + (len >> 3)) / R) + 72u + 7u) & ~7u;
}
u64 sk_spec_span(u32 len, int bits) { return len ? (u64)sk_spec_cap(len, 1u << bits) << bits : 0; }

// spec[2 i] = first slot of node i's regions, spec[2 i + 1] = slots per child; out[0] = slots of all, out[1] = 1 if they
// pass 2^32.  One workgroup (at most 256 nodes: the coarse buckets).
__global__ __launch_bounds__(SK_MAX_C0) void sk_spec_caps_kernel(const Node *__restrict__ nodes, u32 n_nodes, u32 *__restrict__ spec,
                                                                u32 *__restrict__ out)
{
    __shared__ u64 span[SK_MAX_C0];
    const u32 i = threadIdx.x;
    u32 cap = 0;
    u64 sp = 0;
    if (i < n_nodes && nodes[i].split) {
        cap = sk_spec_cap(nodes[i].len, 1u << nodes[i].split);
        sp = (u64)cap << nodes[i].split;
    }
    span[i] = sp;
    __syncthreads();
    if (i == 0) {
        u64 run = 0;
        for (u32 q = 0; q < (u32)SK_MAX_C0; q++) {
            const u64 c = span[q];
            span[q] = run;
            run += c;
        }
        out[0] = (u32)(run < 0xFFFFFFFFull ? run : 0xFFFFFFFFull);
        out[1] = run > 0xFFFFFFFFull ? 1u : 0u;
        out[2] = 0;                                // (the sweep's overflow flag)
    }
    __syncthreads();
    if (i < n_nodes) {
        spec[2 * i] = (u32)(span[i] < 0xFFFFFFFFull ? span[i] : 0xFFFFFFFFull);
        spec[2 * i + 1] = cap;
    }
}

// the cursors at the regions' starts (a workgroup per node, a thread per child)
__global__ __launch_bounds__(ROW_STRIDE) void sk_spec_init_kernel(const Node *__restrict__ nodes, u32 n_nodes, const u32 *__restrict__ spec,
                                                                 u32 *__restrict__ gcur, const u32 *__restrict__ rstart)
{
    const u32 i = blockIdx.x, d = threadIdx.x;
    if (i >= n_nodes)
        return;
    const Node nd = nodes[i];
    if (nd.split && d < (1u << nd.split))
        gcur[(u64)nd.chunk_base * ROW_STRIDE + d] = rstart ? rstart[nd.child_base + d] : spec[2 * i] + d * spec[2 * i + 1];
}

// the mid nodes a speculative sweep leaves (what level_children makes of a histogram): start = region start, len = records
// drawn; a cursor past its region's end raises *over
__global__ __launch_bounds__(ROW_STRIDE) void sk_spec_nodes_kernel(const Node *__restrict__ nodes, u32 n_nodes, const u32 *__restrict__ spec,
                                                                  const u32 *__restrict__ gcur, Node *__restrict__ next,
                                                                  u32 *__restrict__ over, const u32 *__restrict__ rstart,
                                                                  const u32 *__restrict__ rcapv)
{
    const u32 i = blockIdx.x, d = threadIdx.x;
    if (i >= n_nodes)
        return;
    const Node nd = nodes[i];
    if (nd.split == 0) {
        if (d == 0) {
            Node o = nd;
            o.split = 0;
            next[nd.child_base] = o;
        }
        return;
    }
    if (d >= (1u << nd.split))
        return;
    const int bits = (int)nd.split, rem = (int)(nd.meta & 0xff);
    const u32 cap = rcapv ? rcapv[nd.child_base + d] : spec[2 * i + 1];
    const u32 start = rcapv ? rstart[nd.child_base + d] : spec[2 * i] + d * cap;
    u32 used = gcur[(u64)nd.chunk_base * ROW_STRIDE + d] - start;
    if (used > cap) {
        used = cap;
        *over = 1u;
    }
    Node c;
    c.start = start;
    c.len = used;
    c.meta = (u32)(rem - bits) | ((nd.meta & NODE_BUF) ^ NODE_BUF) | ((bits == rem) ? NODE_TERMINAL : 0u);
    c.split = 0;
    c.prefix = nd.prefix | ((u64)d << (rem - bits));
    c.child_base = 0;
    c.chunk_base = 0;
    next[nd.child_base + d] = c;
}

// ------------------------------------------------------------------------------------------------
// sk_regroup: inside every mid bucket the records are regrouped by d2 (16 final buckets), from one record buffer
// into the same range of the other: a workgroup per mid bucket counts d2 (records and k-mers), then copies tile
// by tile with the same index staging as sk_scatter1.  out_nodes[16 i + j] = final bucket j of mid bucket i:
// start / len in RECORDS, child_base = its k-mers, chunk_base = its quads (sk_count's work items).
constexpr int SKR_NT = 1024;
constexpr int SKR_ITEMS = 8;
constexpr int SKR_TILE = SKR_NT * SKR_ITEMS;
// LONG = false: the mid buckets of at most one tile (all of them on random sequence; the others are left alone);
// LONG = true: the longer ones only (launched when the host has seen one: the records per mid bucket are on the host).
// Two kernels, so that the common one carries neither the long path's code nor its registers (as one kernel it showed
// 76 bytes of scratch per lane: the records' registers spilled around the long path's loop).
template <bool LONG>
__global__ __launch_bounds__(SKR_NT, 8) void sk_regroup_kernel(const Node *__restrict__ mids, u32 n_mids,
                                                            const ull2_t *__restrict__ src_all, ull2_t *__restrict__ dst_all,
                                                            Node *__restrict__ out_nodes, const u32 *__restrict__ gate)
{
    __shared__ u32 rc[64][17], kc[64][17], qc[64][17];   // per-lane copies of the 16 record / k-mer / quad counters
    __shared__ u32 gpos[16], tcnt[17];
    // a bucket of one tile: half a tile of records at a time, in regrouped order (64 KB); longer buckets: the index list
    __shared__ __attribute__((aligned(16))) ull2_t stage[SKR_TILE / 2];
    unsigned short *idx = reinterpret_cast<unsigned short *>(stage);
    const u32 i = blockIdx.x;
    if (i >= n_mids)
        return;
    // launched before the host knew whether level 1 stands (launch_sk_l1_gate): if it does not, rec0 -- dst here -- is
    // still the input of the exact level 1, and nothing may be written
    if (!LONG && gate && *gate)
        return;
    const int tid = threadIdx.x, lane = tid & 63;
    const Node nd = mids[i];
    if ((nd.len > (u32)SKR_TILE) != LONG)
        return;
    const ull2_t *src = src_all + (u64)nd.start;
    for (int q = tid; q < 64 * 17; q += SKR_NT) {
        (&rc[0][0])[q] = 0;
        (&kc[0][0])[q] = 0;
        (&qc[0][0])[q] = 0;
    }
    if (tid < 17)
        tcnt[tid] = 0;
    __syncthreads();
    // A mid bucket of at most one tile (the planned size is ~5,000 records): its digit words are read ONCE -- counted
    // for the output nodes and ranked for the copy in the same sweep.
    constexpr bool one_tile = !LONG;
    const u32 last = nd.len ? nd.len - 1u : 0u;
    // A bucket of one tile reads every record ONCE, 16 bytes per lane, all of a thread's loads in flight (no bounds test:
    // a slot past the end reads the last record again and drops it); the records wait in registers while they are counted
    // and ranked, and leave through LDS in regrouped order (as sk_scatter1's full tiles do).
    ull2_t rec[LONG ? 1 : SKR_ITEMS];
    u32 pos[LONG ? 1 : SKR_ITEMS];
    if constexpr (one_tile) {
      if (nd.len) {
#pragma unroll
        for (int j = 0; j < SKR_ITEMS; j++) {
            const u32 r = tid + j * SKR_NT;
            rec[j] = src[r < nd.len ? r : last];
        }
#pragma unroll
        for (int j = 0; j < SKR_ITEMS; j++) {
            const u32 r = tid + j * SKR_NT;
            pos[j] = 0;
            if (r < nd.len) {
                const u64 m = rec[j].y;
                const u32 d2 = (u32)(m >> 59) & 15u;
                const u32 len = (u32)((m >> 44) & 31) + 1u;
                atomicAdd(&rc[lane][d2], 1u);
                atomicAdd(&kc[lane][d2], len);
                atomicAdd(&qc[lane][d2], (len + 3u) >> 2);
                pos[j] = atomicAdd(&tcnt[d2], 1u);
            }
        }
      }
    } else {
        for (u32 r = tid; r < nd.len; r += SKR_NT) {
            const u64 m = reinterpret_cast<const u64 *>(src + r)[1];
            const u32 d2 = (u32)(m >> 59) & 15u;
            const u32 len = (u32)((m >> 44) & 31) + 1u;
            atomicAdd(&rc[lane][d2], 1u);
            atomicAdd(&kc[lane][d2], len);
            atomicAdd(&qc[lane][d2], (len + 3u) >> 2);   // quads of sk_count: groups of four k-mers of one record
        }
    }
    __syncthreads();
    if (tid < 48) {                                // threads 0..15: records, 16..31: k-mers, 32..47: quads of d2 = tid % 16
        const u32 (*tab)[17] = tid < 16 ? rc : (tid < 32 ? kc : qc);
        u32 sum = 0;
        for (int q = 0; q < 64; q++)
            sum += tab[q][tid & 15];
        if (tid < 16)
            rc[0][tid] = sum;
        else if (tid < 32)
            kc[0][tid & 15] = sum;
        else
            qc[0][tid & 15] = sum;
    }
    __syncthreads();
    if (tid < 16) {                                // (a thread per final bucket: thread 0 alone held sixteen nodes' worth of
        const u32 c = rc[0][tid];                  // registers while every thread's records waited -- 18 of them spilled)
        const u32 run = row16_excl_scan(c);
        gpos[tid] = nd.start + run;
        Node o;
        o.start = nd.start + run;
        o.len = c;
        o.meta = 0;
        o.split = 0;
        o.prefix = 0;
        o.child_base = kc[0][tid];
        o.chunk_base = qc[0][tid];
        out_nodes[(u64)i * 16 + tid] = o;
        if (one_tile) {
            tcnt[tid] = run;                       // the tile's digit offsets (its counts are the bucket's)
            if (tid == 15)
                tcnt[16] = run + c;
        }
    }
    __syncthreads();
    if constexpr (one_tile) {
        if (nd.len == 0)
            return;
#pragma unroll
        for (int j = 0; j < SKR_ITEMS; j++)
            pos[j] += tcnt[(u32)(rec[j].y >> 59) & 15u];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if ((u32)h * (SKR_TILE / 2) >= nd.len)
                break;
#pragma unroll
            for (int j = 0; j < SKR_ITEMS; j++) {
                const u32 r = tid + j * SKR_NT;
                if (r < nd.len && (pos[j] >> 12) == (u32)h)
                    stage[pos[j] & 4095u] = rec[j];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < SKR_ITEMS / 2; j++) {
                const u32 s2 = (u32)h * (SKR_TILE / 2) + tid + j * SKR_NT;
                if (s2 < nd.len)                   // (the final buckets lie back to back in the mid bucket's own range)
                    __builtin_nontemporal_store(stage[tid + j * SKR_NT], &dst_all[nd.start + s2]);
            }
            __syncthreads();
        }
        return;
    }
    for (u32 t0 = 0; t0 < nd.len; t0 += SKR_TILE) {
        const u32 n_tile = nd.len - t0 < (u32)SKR_TILE ? nd.len - t0 : (u32)SKR_TILE;
        u32 dig[SKR_ITEMS], rank[SKR_ITEMS];
#pragma unroll
        for (int j = 0; j < SKR_ITEMS; j++) {
            const u32 r = tid + j * SKR_NT;
            dig[j] = 0;
            rank[j] = 0;
            const bool in = r < n_tile;
            if (in)
                dig[j] = (u32)(reinterpret_cast<const u64 *>(src + t0 + r)[1] >> 59) & 15u;
            // one atomic per wave and digit present: a long bucket is a repeat's, its records share the m-mer and with it
            // d2 -- a lane's own atomic would be 8,192 additions to ONE address per tile
            u64 todo = __ballot(in);
            while (todo) {
                const u32 d = (u32)__builtin_amdgcn_readlane((int)dig[j], (int)__builtin_ctzll(todo));
                const u64 same = __ballot(in && dig[j] == d);
                u32 base = 0;
                if (lane == (int)__builtin_ctzll(same))
                    base = atomicAdd(&tcnt[d], (u32)__popcll(same));
                base = (u32)__builtin_amdgcn_readlane((int)base, (int)__builtin_ctzll(same));
                if (in && dig[j] == d)
                    rank[j] = base + (u32)__popcll(same & (((u64)1 << lane) - 1));
                todo &= ~same;
            }
        }
        __syncthreads();
        if (tid == 0) {                             // counts -> exclusive offsets, tcnt[16] = n_tile
            u32 run = 0;
            for (int j = 0; j < 16; j++) {
                const u32 c = tcnt[j];
                tcnt[j] = run;
                run += c;
            }
            tcnt[16] = run;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SKR_ITEMS; j++) {
            const u32 r = tid + j * SKR_NT;
            if (r < n_tile)
                idx[tcnt[dig[j]] + rank[j]] = (unsigned short)r;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < SKR_ITEMS; j++) {
            const u32 s = tid + j * SKR_NT;
            if (s < n_tile) {
                const ull2_t r = src[t0 + idx[s]];
                const u32 d = (u32)(r.y >> 59) & 15u;
                __builtin_nontemporal_store(r, &dst_all[gpos[d] + (s - tcnt[d])]);
            }
        }
        __syncthreads();
        // (lane t reads tcnt[t + 1], which lane t + 1 is about to zero: both values into registers first, then the store)
        u32 adv = 0;
        if (tid < 16)
            adv = tcnt[tid + 1] - tcnt[tid];
        __syncthreads();
        if (tid < 16) {
            gpos[tid] += adv;
            tcnt[tid] = 0;
        }
        __syncthreads();
    }
}

// The gate word of an early level 2 (kernels.hpp: SkGateIn): one workgroup over the mid buckets' record and k-mer counts
// and the status words of the sweeps before it.
__global__ __launch_bounds__(1024) void sk_l1_gate_kernel(SkGateIn in, u32 *__restrict__ gate)
{
    __shared__ u32 wbits[16];
    __shared__ u64 wsum[16];
    u32 g = 0;
    u64 run = 0;
    // four buckets per load where both lists are 16-byte aligned (pool memory is), several loads in flight: one workgroup
    // reads 75 K buckets at 3 Gbase, and the regroup waits behind it
    const bool vec = ((reinterpret_cast<uintptr_t>(in.lens) | reinterpret_cast<uintptr_t>(in.kcount)) & 15) == 0;
    const u32 n4 = vec ? in.n_mid / 4 : 0;
    const uint4 *lens4 = reinterpret_cast<const uint4 *>(in.lens), *kc4 = reinterpret_cast<const uint4 *>(in.kcount);
#pragma unroll 4
    for (u32 q = threadIdx.x; q < n4; q += 1024) {
        const uint4 l = lens4[q], c = kc4[q];
        run += (u64)c.x + c.y + c.z + c.w;
        g |= sk_gate_bucket(l.x, c.x, in.mid_limit, in.rec_limit, in.tile) | sk_gate_bucket(l.y, c.y, in.mid_limit, in.rec_limit, in.tile) |
             sk_gate_bucket(l.z, c.z, in.mid_limit, in.rec_limit, in.tile) | sk_gate_bucket(l.w, c.w, in.mid_limit, in.rec_limit, in.tile);
    }
    for (u32 i = 4 * n4 + threadIdx.x; i < in.n_mid; i += 1024) {
        const u32 kmers = in.kcount[i];
        run += kmers;
        g |= sk_gate_bucket(in.lens[i], kmers, in.mid_limit, in.rec_limit, in.tile);
    }
    for (int o = 32; o; o >>= 1) {
        g |= __shfl_xor(g, o);
        run += __shfl_xor(run, o);
    }
    if ((threadIdx.x & 63) == 0) {
        wbits[threadIdx.x >> 6] = g;
        wsum[threadIdx.x >> 6] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        g = 0;
        run = 0;
        for (int w = 0; w < 16; w++) {
            g |= wbits[w];
            run += wsum[w];
        }
        g |= sk_gate_status(in.status1, in.span1, in.sampled, in.status0, in.span0);
        if ((in.n_expected != 0 && run != in.n_expected) || run > 0xFFFFFFFFull)
            g |= SK_GATE_KMERS;
        *gate = g;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers
hipError_t launch_sk_l1_gate(const SkGateIn &in, u32 *gate, hipStream_t s)
{
    hipLaunchKernelGGL(sk_l1_gate_kernel, dim3(1), dim3(1024), 0, s, in, gate);
    return hipGetLastError();
}

hipError_t launch_sk_hist1(const Node *nodes, const Chunk *chunks, u32 n_chunks, const void *recs, u32 *hist, u32 *kcount,
                           hipStream_t s, bool by_d2)
{
    if (n_chunks == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_hist1_kernel, dim3(n_chunks), dim3(SK1_NT), 0, s, nodes, chunks, n_chunks,
                       reinterpret_cast<const ull2_t *>(recs), hist, kcount, by_d2 ? 59 : 49);
    return hipGetLastError();
}

hipError_t launch_sk_scatter1(const Node *nodes, const Chunk *chunks, u32 n_chunks, const void *src, void *dst, const u32 *hist,
                              const u32 *tot, hipStream_t s, bool by_d2, u32 *gcur)
{
    if (n_chunks == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_scatter1_kernel<false>, dim3(n_chunks), dim3(SK1_NT), 0, s, nodes, chunks, n_chunks,
                       reinterpret_cast<const ull2_t *>(src), reinterpret_cast<ull2_t *>(dst), hist, tot, by_d2 ? 59 : 49, gcur,
                       nullptr, nullptr, nullptr, nullptr, nullptr);
    return hipGetLastError();
}

// level 1 without its histogram: regions (spec: 2 words per node; out: 3 words -- slots of all regions, 1 if past 2^32, the
// sweep's overflow flag), cursors, the sweep (k-mers per mid bucket into kcount), the mid nodes
// (rstart != null: the regions are per mid bucket -- launch_sk_sampled_regions -- and spec / out are only cleared)
hipError_t launch_sk_spec_regions(const Node *nodes, u32 n_nodes, u32 *spec, u32 *out, u32 *gcur, hipStream_t s, const u32 *rstart)
{
    if (n_nodes == 0 || n_nodes > (u32)SK_MAX_C0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sk_spec_caps_kernel, dim3(1), dim3(SK_MAX_C0), 0, s, nodes, n_nodes, spec, out);
    hipLaunchKernelGGL(sk_spec_init_kernel, dim3(n_nodes), dim3(ROW_STRIDE), 0, s, nodes, n_nodes, spec, gcur, rstart);
    return hipGetLastError();
}

// The regions of a speculative level 1 from a SAMPLED histogram (uneven coarse buckets: repeats): est[] (zeroed here) <- the
// records of the sample pieces per mid bucket, rcap[] <- slots per mid bucket, rstart[] <- their exclusive scan, *total <-
// slots of all (saturating).  scan_tmp: scan_tmp_words(n_mid) words.
hipError_t launch_sk_sampled_regions(const Node *nodes, const Chunk *samples, u32 n_samples, const void *recs, u32 n_mid, u32 *est,
                                     u32 *rcap, u32 *rstart, u32 *scan_tmp, u32 *total, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(est, 0, (size_t)n_mid * sizeof(u32), s);
    if (e != hipSuccess)
        return e;
    if (n_samples)
        hipLaunchKernelGGL(sk_sample1_kernel, dim3(n_samples), dim3(SK1_NT), 0, s, nodes, samples, n_samples,
                           reinterpret_cast<const ull2_t *>(recs), est);
    hipLaunchKernelGGL(sk_sampled_caps_kernel, dim3((n_mid + 255) / 256), dim3(256), 0, s, est, n_mid, rcap);
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    return launch_scan_u32(rcap, rstart, n_mid, scan_tmp, total, s);
}

hipError_t launch_sk_scatter1_spec(const Node *nodes, const Chunk *chunks, u32 n_chunks, const void *src, void *dst, u32 *gcur,
                                   const u32 *spec, u32 *kcount, u32 *over, hipStream_t s, const u32 *rstart, const u32 *rcap)
{
    if (n_chunks == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_scatter1_kernel<true>, dim3(n_chunks), dim3(SK1_NT), 0, s, nodes, chunks, n_chunks,
                       reinterpret_cast<const ull2_t *>(src), reinterpret_cast<ull2_t *>(dst), nullptr, nullptr, 49, gcur, spec,
                       kcount, over, rstart, rcap);
    return hipGetLastError();
}

hipError_t launch_sk_spec_nodes(const Node *nodes, u32 n_nodes, const u32 *spec, const u32 *gcur, Node *next, u32 *over,
                                hipStream_t s, const u32 *rstart, const u32 *rcap)
{
    if (n_nodes == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_spec_nodes_kernel, dim3(n_nodes), dim3(ROW_STRIDE), 0, s, nodes, n_nodes, spec, gcur, next, over, rstart,
                       rcap);
    return hipGetLastError();
}

int sk_regroup_tile() { return SKR_TILE; }

hipError_t launch_sk_regroup(const Node *mids, u32 n_mids, const void *src, void *dst, Node *out_nodes, bool any_long, hipStream_t s,
                             const u32 *gate)
{
    if (n_mids == 0)
        return hipSuccess;
    hipLaunchKernelGGL(sk_regroup_kernel<false>, dim3(n_mids), dim3(SKR_NT), 0, s, mids, n_mids, reinterpret_cast<const ull2_t *>(src),
                       reinterpret_cast<ull2_t *>(dst), out_nodes, gate);
    if (any_long)
        hipLaunchKernelGGL(sk_regroup_kernel<true>, dim3(n_mids), dim3(SKR_NT), 0, s, mids, n_mids, reinterpret_cast<const ull2_t *>(src),
                           reinterpret_cast<ull2_t *>(dst), out_nodes, nullptr);
    return hipGetLastError();
}

}  // namespace dnagpu
