// index_math.hpp -- the arithmetic of the index over a stored kmer column, shared by the kernels
// (index_kernels.hip), the host driver (index_host.hip) and the host check tests/host/index_math_check.cpp: the order, the
// range of a prefix, and the prune depth of a filter given as per-position sets (FilterBits).
#pragma once
#include "kmer_device.hpp"

namespace dnagpu {

constexpr u32 INDEX_MAX_RANGES = 1024;      // DNAGPU_INDEX_MAX_RANGES

// the 32 two-bit fields of x in reverse order, each field intact: bit reversal, then the two bits of every pair swapped back
__host__ __device__ __forceinline__ u64 rev2(u64 x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    x = __brevll(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    x = (x >> 32) | (x << 32);
#endif
    return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
}

// The index orders keys by r: base 0 of the k-mer in the TOP field of the 2k bits, so that ascending r is text order under
// A < T < C < G and the keys that share a prefix are one range of r.  Bits of key above 2k are dropped.
__host__ __device__ __forceinline__ u64 index_r_of_key(u64 key, int k)
{
    return rev2(key & kmer_mask(k)) >> (64 - 2 * k);
}
__host__ __device__ __forceinline__ u64 index_key_of_r(u64 r, int k)
{
    return rev2(r << (64 - 2 * k));
}

// [*lo, *hi], both inclusive, = the r of every k-mer whose first p bases are the fields of pr (base 0 in the top field of its
// 2p bits), 0 <= p <= k.  Inclusive, so that p = 0 at k = 32 -- the whole 64-bit range -- needs no 1 << 64.
__host__ __device__ __forceinline__ void index_prefix_range(u64 pr, int p, int k, u64 *lo, u64 *hi)
{
    const int free_bits = 2 * (k - p);
    const u64 low = free_bits >= 64 ? ~(u64)0 : (((u64)1 << free_bits) - 1);
    *lo = free_bits >= 64 ? 0 : pr << free_bits;
    *hi = *lo | low;
}

__host__ __device__ __forceinline__ u32 index_set_at(const FilterBits &fb, int i)
{
    return (fb.sets[i >> 3] >> ((i & 7) * 4)) & 15u;
}
__host__ __device__ __forceinline__ u32 index_popc4(u32 set)
{
    return (set & 1) + ((set >> 1) & 1) + ((set >> 2) & 1) + ((set >> 3) & 1);
}

// Prune depth: the largest p in 0..k with prod_{i<p} |S_i| <= INDEX_MAX_RANGES; *n_ranges = that product, the concrete
// prefixes of p bases the scan looks up.  An empty set makes every longer product 0: p = k, no range.
__host__ __device__ inline int index_prune_depth(const FilterBits &fb, u32 *n_ranges)
{
    u64 prod = 1;
    int p = 0;
    while (p < fb.k) {
        const u64 next = prod * index_popc4(index_set_at(fb, p));
        if (next > INDEX_MAX_RANGES)
            break;
        prod = next;
        p++;
    }
    *n_ranges = (u32)prod;
    return p;
}

// The j-th of those prefixes in ascending r order (position 0 is the most significant digit of the mixed-radix number j, and
// a position's codes ascend): its 2p bits, base 0 in the top field.
__host__ __device__ inline u64 index_prefix_at(const FilterBits &fb, int p, u32 j)
{
    u64 pr = 0;
    for (int i = p - 1; i >= 0; i--) {
        const u32 set = index_set_at(fb, i), sz = index_popc4(set);
        u32 pick = j % sz;
        j /= sz;
        u32 code = 0;
        for (u32 c = 0; c < 4; c++)
            if (set & (1u << c)) {
                if (pick == 0) {
                    code = c;
                    break;
                }
                pick--;
            }
        pr |= (u64)code << (2 * (p - 1 - i));
    }
    return pr;
}

// Are positions p .. k-1 all "any"?  Then the candidates of the ranges are the answer and no key is tested.
__host__ __device__ inline bool index_rest_is_any(const FilterBits &fb, int p)
{
    for (int i = p; i < fb.k; i++)
        if (index_set_at(fb, i) != 15u)
            return false;
    return true;
}

// Merge path (the append: a stable merge of the sorted runs A, the index, and B, the sorted batch).  The split of diagonal
// d, 0 <= d <= na + nb: the a in [0, na] (b = d - a in [0, nb]) with A[a-1] <= B[b] and B[b-1] < A[a] wherever both sides
// exist -- the first d outputs of the merge are A[0 .. a) and B[0 .. b), ties taken from A.  a_at(i) / b_at(i) read A[i] /
// B[i] and are only called with i < na / i < nb: neither run is read past its end and no value of r is special.
template <typename AAt, typename BAt>
__host__ __device__ __forceinline__ u64 index_merge_split(AAt a_at, u64 na, BAt b_at, u64 nb, u64 d)
{
    u64 lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const u64 mid = lo + ((hi - lo) >> 1);      // lo <= mid < hi: mid < na, and 0 <= d - 1 - mid < nb
        if (a_at(mid) <= b_at(d - 1 - mid))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

}  // namespace dnagpu
