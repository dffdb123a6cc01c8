// What the multi-tensor kernels over a device job table share (wc_optim.hip, wc_ema.hip): the chunk
// geometry, the global-memory pointer types and the bisect that takes a workgroup from its chunk to
// its job.  A job row is any struct with an int64_t chunk0 column numbered through the table.
#pragma once
#include "wc_common.hpp"

namespace wcjobs {

constexpr int OPT_THREADS = 256;
constexpr int OPT_VEC = 4;                                 // f32x4 per thread and operand in a full chunk
constexpr int OPT_CHUNK = OPT_THREADS * OPT_VEC * 4;       // 4096 elements == wc_optim_chunk_elems()

// The tensors' addresses come out of the job table, so the compiler knows no address space for them and
// would issue flat loads and stores; they are device global memory, and these types say so.
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) const float gcf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
typedef __attribute__((address_space(1))) const f32x4 gcf32x4;

// The last job of the table slice whose first chunk is <= c (the slice's first job has chunk0 <= c).
template <typename Job>
WC_DEVICE int find_job(const Job* __restrict__ jobs, int njobs, int64_t c) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].chunk0 <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace wcjobs
