// acc_device.hpp -- device helpers of the kernels that hold one accumulator partition in LDS (acc_kernels.hip: merge and
// split; join_kernels.hip: the partition path of the join): the 16-byte slot accesses, a key's home slot, and the load of a
// partition by a workgroup of ACC_NT threads.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace dnagpu {

constexpr int ACC_NT = 512;                                // threads of a partition's workgroup
constexpr int ACC_PER_T = ACC_SLOTS / ACC_NT;              // slots per thread: 8

__device__ __forceinline__ u32 acc_home(u64 h) { return (u32)h & (ACC_SLOTS - 1); }

// 16-byte slot load / store as one dwordx4
__device__ __forceinline__ void ld_slot(const u64 *p, u64 &k, u64 &c)
{
    const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(p);
    k = v.x;
    c = v.y;
}
__device__ __forceinline__ void st_slot(u64 *p, u64 k, u64 c)
{
    ulonglong2 v;
    v.x = k;
    v.y = c;
    *reinterpret_cast<ulonglong2 *>(p) = v;
}

// lds[2 s] = key, lds[2 s + 1] = count of slot s.  A partition that is occupied is loaded whole; else zeroed.
__device__ __forceinline__ void load_region(u64 *lds, const u64 *__restrict__ region, bool occupied)
{
#pragma unroll
    for (int j = 0; j < ACC_PER_T; j++) {
        const int s = j * ACC_NT + (int)threadIdx.x;
        u64 k = 0, c = 0;
        if (occupied)
            ld_slot(region + 2 * (u64)s, k, c);
        lds[2 * s] = k;
        lds[2 * s + 1] = c;
    }
}

}  // namespace dnagpu
