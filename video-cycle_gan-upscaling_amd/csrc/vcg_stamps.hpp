// In-kernel stamps for diagnostic builds (-DVCG_STAMPS; scripts/micro/stamps.py builds the whole library with it, in a directory of its
// own, and prints each family's report).  A kernel brackets its segments with VCG_STAMP, sums the differences per wave in scalar
// registers with VCG_STAMP_ADD (or under #ifdef VCG_STAMPS) and writes the sums to its family's buffer after its loop.  Without the
// define every macro here expands to nothing: no stamp executes in the shipped library.  Read the SHARES of a stamped build, not its
// run time.
#pragma once

#ifdef VCG_STAMPS
// t = s_memtime, waited for; the scheduling barriers keep the read where the source puts it
#define VCG_STAMP(t)                                                                  \
    do {                                                                              \
        __builtin_amdgcn_sched_barrier(0);                                            \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");     \
        __builtin_amdgcn_sched_barrier(0);                                            \
    } while (0)
#define VCG_STAMP_ADD(sum, a, b) sum += (b) - (a)
// A family's buffer of n sums and the export that copies it to the host after the device has drained.  (The export keeps its C name
// inside an anonymous namespace as well, where the kernels and the constants that size the buffer live: clang, which hipcc is, gives an
// extern "C" function external linkage there; under a compiler that does not, stamps.py run fails at once on the missing symbol.)
#define VCG_STAMP_SUMS(fam, n)                                                                                        \
    __device__ unsigned long long vcg_##fam##_stamp_sums[n];                                                          \
    extern "C" int vcg_debug_##fam##_stamps(unsigned long long* host_out) {                                           \
        if (hipDeviceSynchronize() != hipSuccess) return -1;                                                          \
        return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(vcg_##fam##_stamp_sums), sizeof(unsigned long long) * (n)); \
    }
#else
#define VCG_STAMP(t) do { } while (0)
#define VCG_STAMP_ADD(sum, a, b) do { } while (0)
#define VCG_STAMP_SUMS(fam, n)
#endif
