// Stable ray compaction without atomics, shared by cull.hip (background culling) and objects.hip (object render): the bodies of
// the two launches over workgroups of 256 rays (4 waves).  The kernels themselves - their keep predicate, their arguments and
// their LDS arrays - stay with their file; these bodies are inlined into them.
//   totals : keep mask -> wave ballot + popcount -> one total per workgroup
//   emit   : every workgroup sums the totals in front of it (fixed order), recomputes its ballots and writes
//            map[k] = ray, slot[ray] = k or -1; the last workgroup writes the count
// Survivors come out in ascending ray order, identically on every run.  The count stays on the device.
#pragma once
#include "common.h"

namespace neo {
namespace compact {

constexpr int BLOCK = 256;

// keep(ray): the caller's predicate (false beyond its R); s_wave: int[BLOCK / 64] of LDS
template <class Keep>
__device__ __forceinline__ void totals_body(Keep keep, int* s_wave, int* __restrict__ totals) {
    const int ray = blockIdx.x * BLOCK + threadIdx.x;
    const unsigned long long ballot = __ballot(keep(ray));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) totals[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// s_part, s_wave: int[BLOCK / 64] of LDS each
template <class Keep>
__device__ __forceinline__ void emit_body(Keep keep_of, int R, const int* __restrict__ totals, int* s_part, int* s_wave,
                                          int* __restrict__ map, int* __restrict__ slot, int* __restrict__ count,
                                          int* __restrict__ count_out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // survivors in front of this workgroup: integer sums, any order gives the same value
    int part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += BLOCK) part += totals[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    const int ray = blockIdx.x * BLOCK + threadIdx.x;
    const bool keep = keep_of(ray);
    const unsigned long long ballot = __ballot(keep);
    if (lane == 0) { s_part[wv] = part; s_wave[wv] = __popcll(ballot); }
    __syncthreads();
    int base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    for (int w = 0; w < wv; ++w) base += s_wave[w];
    if (ray < R) {
        const int k = base + __popcll(ballot & ((1ull << lane) - 1ull));
        if (keep) map[k] = ray;
        slot[ray] = keep ? k : -1;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const int n = s_part[0] + s_part[1] + s_part[2] + s_part[3] + s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        *count = n;
        if (count_out) *count_out = n;
    }
}

inline int blocks(int R) { return (R + BLOCK - 1) / BLOCK; }

}  // namespace compact
}  // namespace neo
