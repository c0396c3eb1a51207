// What the point compactions of occupancy.hip (k_occ_keep / k_occ_emit / k_occ_scatter), accelerate.hip (k_acc_keep / k_acc_emit) and
// vanilla_march.hip (k_vm_keep / k_vm_emit) share: the KEEP RULE of one point over the unit cube, the per-workgroup totals and the
// rank of a kept point among the kept points in front of it - and, for the two vanilla files (vanilla_march.hip and the training row
// builder of vanilla_train_march.hip), the BOX GRID's cell rule.  Included by those files only; everything here has internal linkage.
#pragma once
#include <cmath>

#include "common.h"

namespace neo {

namespace {

constexpr int OCC_BLOCK = 256;
constexpr int OCC_ROUNDS = 4;
constexpr int OCC_POINTS = OCC_BLOCK * OCC_ROUNDS;      // points per workgroup
constexpr int OCC_SEGS = OCC_POINTS / 64;               // 64-point segments per workgroup, in point order

// i = min(max((int)floorf((x + 1) (G / 2)), 0), G - 1), clamped before the conversion (the same value for every finite x)
__device__ __forceinline__ int occ_cell(float x, int G) {
    float c = floorf((x + 1.0f) * (0.5f * (float)G));
    c = c > 0.0f ? c : 0.0f;
    c = c < (float)(G - 1) ? c : (float)(G - 1);
    return (int)c;
}

// KEEP RULE: a set cell, a non-finite coordinate (the negation of `<`, as cull_keep: a NaN survives to the caller) or no grid
__device__ __forceinline__ bool occ_keep_point(const uint32_t* __restrict__ bits, int G, const float* __restrict__ o,
                                               const float* __restrict__ d, float tv) {
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = o[a] + tv * d[a];
    if (!(fabsf(x[0]) < __builtin_inff()) || !(fabsf(x[1]) < __builtin_inff()) || !(fabsf(x[2]) < __builtin_inff())) return true;
    if (!bits) return true;
    const int lin = (occ_cell(x[0], G) * G + occ_cell(x[1], G)) * G + occ_cell(x[2], G);
    return (bits[lin >> 5] >> (lin & 31)) & 1u;
}

// BOX GRID (include/neo360_hip.h): bits (GRID LAYOUT of occupancy.hip) or NULL for "no grid"; scale_a = (float)G / (hi_a - lo_a),
// host fp32
struct VmBox {
    const uint32_t* bits;
    int G, clip;
    float lo[3], scale[3];
};

// BOX KEEP RULE: a non-finite coordinate (the negation of `<`: a NaN survives), no grid, outside the box without clip, or a set cell
__device__ __forceinline__ bool vm_keep_point(const VmBox& b, const float* __restrict__ o, const float* __restrict__ d, float tv) {
    float x[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) x[a] = o[a] + tv * d[a];      // mul then add, as the evaluators
    if (!(fabsf(x[0]) < __builtin_inff()) || !(fabsf(x[1]) < __builtin_inff()) || !(fabsf(x[2]) < __builtin_inff())) return true;
    if (!b.bits) return true;
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float cf = floorf((x[a] - b.lo[a]) * b.scale[a]);
        if (!(cf >= 0.0f && cf < (float)b.G)) return b.clip == 0;      // outside (an overflow to inf included)
        c[a] = (int)cf;
    }
    const int lin = (c[0] * b.G + c[1]) * b.G + c[2];
    return (b.bits[lin >> 5] >> (lin & 31)) & 1u;
}

inline bool vm_resolution_ok(int G) { return G == 8 || G == 16 || (G >= 32 && G <= 256 && G % 32 == 0); }

// lo < hi, both finite, and a finite positive scale per axis; fills box.lo / box.scale
inline const char* vm_box_from(int G, const float* lo, const float* hi, VmBox& box) {
    for (int a = 0; a < 3; ++a) {
        if (!(std::fabs(lo[a]) < INFINITY) || !(std::fabs(hi[a]) < INFINITY) || !(lo[a] < hi[a])) return "the box needs finite lo < hi on every axis";
        const float scale = static_cast<float>(G) / (hi[a] - lo[a]);
        if (!(scale > 0.0f && scale < INFINITY)) return "the box is too thin or too wide for fp32 cell arithmetic";
        box.lo[a] = lo[a];
        box.scale[a] = scale;
    }
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
