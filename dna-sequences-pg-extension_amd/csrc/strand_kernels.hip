// strand_kernels.hip -- the reverse complement of a packed dna and the strand forms of a key array.  The
// arithmetic is strand_math.hpp's; the canonical add of the accumulator is in acc_kernels.hip.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "strand_math.hpp"

namespace dnagpu {

// One thread per output word: out[j] = bases [first, first + count) of `words` reverse-complemented, bases 32 j ..  The
// thread reads one or two words of [first / 32, ceil((first + count) / 32)) -- revcomp_source says which -- and nothing
// outside; the bits behind the window's last base never reach the result, and the bits behind the result's last base are
// zero.
__global__ __launch_bounds__(256) void dna_revcomp_kernel(const u64 *__restrict__ words, u64 first, u64 count, u64 n_out,
                                                          u64 *__restrict__ out)
{
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_out)
        return;
    const RevcompSource s = revcomp_source(first, count, j);
    const u64 lo = words[s.word];
    const u64 hi = s.two_words ? words[s.word + 1] : 0;
    out[j] = revcomp_finish(funnel(lo, hi, s.shift), s.nb);
}

// One thread per key: out[i] = rc(keys[i]) or canonical(keys[i]) (bits above 2k dropped); flipped[i] (may be null) = the
// result differs from the masked key.  out may be keys: a thread reads its key before it writes.
__global__ __launch_bounds__(256) void kmer_strand_kernel(const u64 *keys, u64 n, int k, int canonical, u64 *out,
                                                          uint8_t *__restrict__ flipped)
{
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 mask = kmer_mask(k);
    for (; i < n; i += stride) {
        const u64 key = keys[i] & mask;
        const u64 res = canonical ? kmer_canonical(key, k) : kmer_revcomp(key, k);
        out[i] = res;
        if (flipped)
            flipped[i] = res != key;
    }
}

hipError_t launch_dna_revcomp(const u64 *words, u64 first, u64 count, u64 *out, hipStream_t s)
{
    const u64 n_out = (count + 31) / 32;
    if (n_out == 0)
        return hipSuccess;
    hipLaunchKernelGGL(dna_revcomp_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, words, first, count, n_out, out);
    return hipGetLastError();
}

hipError_t launch_kmer_strand(const u64 *keys, u64 n, int k, int canonical, u64 *out, uint8_t *flipped, hipStream_t s)
{
    if (n == 0)
        return hipSuccess;
    const u64 blocks = (n + 255) / 256;
    hipLaunchKernelGGL(kmer_strand_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, keys, n, k, canonical,
                       out, flipped);
    return hipGetLastError();
}

}  // namespace dnagpu
