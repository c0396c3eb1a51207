// The KEEP RULE of one point over an occupancy grid and the compaction of kept points (point_list.hip builds the point rows of the
// NeO-360 and the vanilla frames with them, vanilla_train_march.hip its training rows): the rule, the host helpers that fill a grid
// descriptor, the per-workgroup totals and the rank of a kept point among the kept points in front of it.  The descriptor itself,
// OccGrid with its OCC_* outside policies, is declared in kernels.h, because the context (ctx.h) holds one per installed grid and
// the launch wrappers take it.  Everything here has internal linkage.
#pragma once
#include <cmath>

#include "common.h"
#include "kernels.h"      // OccGrid

namespace neo {

namespace {

constexpr int OCC_BLOCK = 256;
constexpr int OCC_ROUNDS = 4;
constexpr int OCC_POINTS = OCC_BLOCK * OCC_ROUNDS;      // points per workgroup
constexpr int OCC_SEGS = OCC_POINTS / 64;               // 64-point segments per workgroup, in point order

// KEEP RULE of the point x = o + t d (mul then add, as the evaluators).  In this order: a non-finite coordinate is kept (the
// negation of `<`, as cull_keep: a NaN survives to the caller); no grid keeps; then the cell floorf((x - lo) scale) per axis - for
// the unit cube (x + 1) (G / 2) bit for bit - decides: outside [0, G) (an overflow to inf included) OCC_CLAMP takes the edge cell,
// clamped before the conversion to int, OCC_KEEP keeps and OCC_SKIP skips; inside, the cell's bit.
__device__ __forceinline__ bool occ_keep(const OccGrid& g, const float* __restrict__ o, const float* __restrict__ d, float tv) {
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = o[a] + tv * d[a];
    if (!(fabsf(x[0]) < __builtin_inff()) || !(fabsf(x[1]) < __builtin_inff()) || !(fabsf(x[2]) < __builtin_inff())) return true;
    if (!g.bits) return true;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float cf = floorf((x[a] - g.lo[a]) * g.scale[a]);
        if (g.outside == OCC_CLAMP) {
            cf = cf > 0.0f ? cf : 0.0f;
            cf = cf < (float)(g.G - 1) ? cf : (float)(g.G - 1);
        } else if (!(cf >= 0.0f && cf < (float)g.G)) {
            return g.outside == OCC_KEEP;
        }
        c[a] = (int)cf;
    }
    const int lin = (c[0] * g.G + c[1]) * g.G + c[2];
    return (g.bits[lin >> 5] >> (lin & 31)) & 1u;
}

inline bool occ_resolution_ok(int G) { return G == 8 || G == 16 || (G >= 32 && G <= 256 && G % 32 == 0); }
constexpr const char* OCC_RESOLUTION_MSG = "occupancy resolution must be 8, 16 or a multiple of 32 in [32, 256]";

// the unit cube [-1, 1]^3: lo = -1, scale = G / 2, the edge cell outside
inline OccGrid occ_grid_unit(const uint32_t* bits, int G) {
    const float h = 0.5f * static_cast<float>(G);
    return {bits, G, {-1.0f, -1.0f, -1.0f}, {h, h, h}, OCC_CLAMP};
}

// a caller's box: lo < hi, both finite, and a finite positive scale (float)G / (hi - lo) per axis; fills G, lo, scale and the
// policy of `clip` (bits stay the caller's).  Returns the message of the failing check, or NULL.
inline const char* occ_grid_box(int G, const float* lo, const float* hi, int clip, OccGrid& out) {
    for (int a = 0; a < 3; ++a) {
        if (!(std::fabs(lo[a]) < INFINITY) || !(std::fabs(hi[a]) < INFINITY) || !(lo[a] < hi[a])) return "the box needs finite lo < hi on every axis";
        const float scale = static_cast<float>(G) / (hi[a] - lo[a]);
        if (!(scale > 0.0f && scale < INFINITY)) return "the box is too thin or too wide for fp32 cell arithmetic";
        out.lo[a] = lo[a];
        out.scale[a] = scale;
    }
    out.G = G;
    out.outside = clip ? OCC_SKIP : OCC_KEEP;
    return nullptr;
}

// The first launch of the compaction: totals[workgroup] = the kept points of this workgroup, from the keep flag of this thread's
// point of every round (false beyond the launch's points).  s_seg: int[OCC_SEGS] of LDS.  Called by the whole workgroup.
__device__ __forceinline__ void occ_total(const bool (&k)[OCC_ROUNDS], int* s_seg, int* __restrict__ totals) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        const unsigned long long ballot = __ballot(k[it]);
        if (lane == 0) s_seg[it * 4 + wv] = __popcll(ballot);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
#pragma unroll
        for (int g = 0; g < OCC_SEGS; ++g) n += s_seg[g];
        totals[blockIdx.x] = n;
    }
}

// The compact index of this thread's point of every round (k[it], valid where kept[it]) and the kept points up to and including
// this workgroup (`upto`): the sums of compact.h's emit over this file's segments.  Integer sums: any order gives the same value.
// Every workgroup of the launch must have a total, also one that owns no point (P may be smaller than the launch: then 0).
struct OccRank {
    bool kept[OCC_ROUNDS];
    int k[OCC_ROUNDS];
    int upto;
};
__device__ __forceinline__ OccRank occ_rank(const uint8_t* __restrict__ keep, int P, const int* __restrict__ totals, int* s_part,
                                            int* s_seg) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int part = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += OCC_BLOCK) part += totals[b];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    OccRank rk;
    int below[OCC_ROUNDS];
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        rk.kept[it] = p < P && keep[p] != 0;
        const unsigned long long ballot = __ballot(rk.kept[it]);
        below[it] = __popcll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) s_seg[it * 4 + wv] = __popcll(ballot);
    }
    if (lane == 0) s_part[wv] = part;
    __syncthreads();
    int run = s_part[0] + s_part[1] + s_part[2] + s_part[3];
#pragma unroll
    for (int g = 0; g < OCC_SEGS; ++g) {
        if ((g & 3) == wv) rk.k[g >> 2] = run + below[g >> 2];
        run += s_seg[g];
    }
    rk.upto = run;
    return rk;
}

inline int occ_blocks(long P) { return (int)((P + OCC_POINTS - 1) / OCC_POINTS); }

}  // namespace

}  // namespace neo
