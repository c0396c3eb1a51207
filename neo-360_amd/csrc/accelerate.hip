// Occupancy skipping and early ray termination TOGETHER (neo_tp_render_accelerated): the point list of one segment of a terminating
// march holds only the samples that the installed occupancy grid keeps.  This file holds the one device-side piece that neither
// parent has - a fused classify + compact over the CANDIDATES of a segment launch; the driver is tp_eval_march with a grid (api_tp.hip),
// and everything else of a segment (k_march_scatter, k_march_advance on rows in which a skipped sample is a zero row) is march.hip's.
//
// CANDIDATES.  One window (rays r0 .. of the frame's R), one segment (samples b0 .. b0 + len - 1 of the level's N).  The alive rays
// come from launch_cull_compact on the running transmittance: map[k], k < *alive (a device word), ascending.  Candidate
// p < *alive len is sample j = b0 + p % len of ray r0 + map[p / len] - k_march_emit's row order.
//
//   k_acc_keep   the totals launch of compact.h on candidates: a workgroup owns 1024 consecutive candidates in the 4 x 256 layout
//                of k_occ_keep, applies occ_keep_point (the KEEP RULE) to x = o + t d of each, writes the keep byte and its kept count;
//   k_acc_emit   ranks each kept candidate by the fixed-order sum of the totals in front of it (occ_rank) and writes its point row -
//                origin, direction, the view direction of the quirk-Q1 ray c0 + ((r - c0) N + j) mod bc of the DENSE launch of the
//                level's full N, t, dst = r N + j - at that rank: ascending candidate order, identically on every run.
//
// The launches are sized on the host for rays x len while the candidate count lives on the device: a workgroup past the count
// classifies nothing and still writes a total of 0, so every prefix sum may run over all workgroups in front; the count is written
// by thread 0 of the LAST workgroup of the launch, whose `upto` covers every candidate.  With nobody alive, or nothing kept, all
// totals are 0 and so is the count.  No atomics, no spinning: the int64 counter is bumped by that one thread, behind the previous
// segment in stream order.
#include "common.h"
#include "march.h"
#include "occ_points.h"
#include "tp_frame.h"

using namespace neo_host;

namespace neo {

namespace {

__global__ __launch_bounds__(OCC_BLOCK) void k_acc_keep(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                        const float* __restrict__ t, const int* __restrict__ map,
                                                        const int* __restrict__ alive, int r0, int N, int b0, int len,
                                                        const uint32_t* __restrict__ bits, int G, uint8_t* __restrict__ keep,
                                                        int* __restrict__ totals) {
    __shared__ int s_seg[OCC_SEGS];
    const int cand = *alive * len;      // at most rays x len, which the driver holds below 2^31 / 3
    bool k[OCC_ROUNDS];
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        k[it] = false;
        if (p < cand) {
            const int kk = p / len, j = b0 + (p - kk * len);
            const int ray = r0 + map[kk];
            k[it] = occ_keep_point(bits, G, rays_o + (long)ray * 3, rays_d + (long)ray * 3, t[(long)ray * N + j]);
            keep[p] = k[it] ? 1 : 0;
        }
    }
    occ_total(k, s_seg, totals);
}

__global__ __launch_bounds__(OCC_BLOCK) void k_acc_emit(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                        const float* __restrict__ viewdirs, const float* __restrict__ t,
                                                        const int* __restrict__ map, const int* __restrict__ alive,
                                                        const uint8_t* __restrict__ keep, int r0, int R, int N, int b0, int len,
                                                        int chunk, const int* __restrict__ totals, float* __restrict__ c_o,
                                                        float* __restrict__ c_d, float* __restrict__ c_v, float* __restrict__ c_t,
                                                        int* __restrict__ dst, int* __restrict__ rows,
                                                        long long* __restrict__ kept_sum) {
    __shared__ int s_part[OCC_BLOCK / 64];
    __shared__ int s_seg[OCC_SEGS];
    const int cand = *alive * len;
    const OccRank rk = occ_rank(keep, cand, totals, s_part, s_seg);
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        if (!rk.kept[it]) continue;
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        const int k = rk.k[it];
        const int kk = p / len, j = b0 + (p - kk * len);
        const int ray = r0 + map[kk];
        const int c0 = (ray / chunk) * chunk;
        const int bc = min(chunk, R - c0);
        const int dray = c0 + (int)(((long)(ray - c0) * N + j) % bc);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c_o[(long)k * 3 + a] = rays_o[(long)ray * 3 + a];
            c_d[(long)k * 3 + a] = rays_d[(long)ray * 3 + a];
            c_v[(long)k * 3 + a] = viewdirs[(long)dray * 3 + a];
        }
        c_t[k] = t[(long)ray * N + j];
        dst[k] = ray * N + j;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *rows = rk.upto;
        if (kept_sum) *kept_sum = *kept_sum + (long long)rk.upto;
    }
}

}  // namespace

void launch_acc_compact(const float* rays_o, const float* rays_d, const float* viewdirs, const float* t, const int* map, const int* alive,
                        int r0, int rays, int R, int N, int b0, int len, int chunk, const uint32_t* bits, int G, uint8_t* keep,
                        const OccRows& w, long long* kept_sum, hipStream_t s) {
    const long P = (long)rays * len;
    if (P <= 0) return;
    const int nb = occ_blocks(P);
    hipLaunchKernelGGL(k_acc_keep, dim3(nb), dim3(OCC_BLOCK), 0, s, rays_o, rays_d, t, map, alive, r0, N, b0, len, bits, G, keep,
                       w.totals);
    hipLaunchKernelGGL(k_acc_emit, dim3(nb), dim3(OCC_BLOCK), 0, s, rays_o, rays_d, viewdirs, t, map, alive, (const uint8_t*)keep, r0, R,
                       N, b0, len, chunk, (const int*)w.totals, w.o, w.d, w.v, w.t, w.dst, w.count, kept_sum);
}

}  // namespace neo
