// THE POINT LIST: the single-point rows (OccRows) that an evaluator's compact launch reads, for every frame that evaluates less
// than its dense rows - the skipping, terminating, accelerated and marching frames of NeO-360 and the vanilla marching frame
// (driver: march_level, march.h) - and the keep mask alone for the pure functions neo_tp_occupancy_keep /
// neo_vanilla_occupancy_keep, the mask outputs of the frames and the training row builder (vanilla_train_march.hip).
//
// CANDIDATES (march.h: PointSource).  One window of rows, one segment of samples: candidate p < n len is sample j = b0 + p % len of
// row first + map_w[p / len], n = *count_w alive rows - or all `rows` rows of the window.  The launches are sized on the host for
// rows x len while the candidate count may live on the device: a workgroup behind the count classifies nothing and still writes a
// total of 0, so every prefix sum may run over all workgroups in front.
//
//   k_point_keep       a workgroup owns OCC_POINTS consecutive candidates (4 rounds of 256 threads), applies the KEEP RULE
//                      (occ_points.h: occ_keep) to each, writes the keep byte and, when asked, its kept count: the totals launch of
//                      compact.h on candidates;
//   k_point_emit       ranks each kept candidate by the fixed-order sum of the totals in front of it (occ_rank) and writes its
//                      point row at that rank: ascending candidate order, identically on every run; thread 0 of the LAST workgroup,
//                      whose `upto` covers every candidate, writes the count;
//   k_point_emit_all   no grid: the row of candidate p is row p, no mask and no ranking; thread 0 writes the count.
//
// That sum of totals is linear in the workgroups of ONE launch, and the drivers keep launches small: at the default window a
// level-1 launch of the 129 + 385 skipping frame is 1540 workgroups, 1.2 M integer reads for all of them together - no
// hierarchical scan is needed at that size.  No atomics, no spinning: the int64 counter is bumped by the one thread
// that writes the count, behind the previous launch in stream order.
//
// A point row is ONE point: the evaluator's compact launch with N = 1 and the identity map forms x = o[row] + t[row] d[row] and
// takes the view direction of row `row` itself (point_setup_row: c0 + ((row - c0) 1 + 0) mod bc = row), so point_row writes the view
// direction of the quirk-Q1 ray of the DENSE launch of the level's full N and - point_setup_row reads far[row] - outside the
// sphere the ray's far.  The evaluator sources are not touched.
#include "common.h"
#include "march.h"
#include "occ_points.h"

namespace neo {

namespace {

// candidates of the launch: at most rows x len, which the drivers hold below 2^31 / 3
__device__ __forceinline__ int point_candidates(const PointSource& s) {
    return (s.count_w ? min(*s.count_w, s.rows) : s.rows) * s.len;
}

// row, ray and sample of candidate p
__device__ __forceinline__ void point_candidate(const PointSource& s, int p, int& row, int& ray, int& j) {
    const int kk = p / s.len;
    j = s.b0 + (p - kk * s.len);
    row = s.first + (s.map_w ? s.map_w[kk] : kk);
    ray = s.map ? s.map[row] : row;
}

// THE POINT ROW of candidate p at row k of the list
__device__ __forceinline__ void point_row(const PointSource& s, int p, const OccRows& w, long k) {
    int row, ray, j;
    point_candidate(s, p, row, ray, j);
    // every load in front of the first store: the columns are plain pointers, so a load behind a store would have to wait for it
    float o[3], d[3], v[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        o[a] = s.rays_o[(long)ray * 3 + a];
        d[a] = s.dirs[(long)ray * 3 + a];
    }
    if (s.viewdirs) {
        const int c0 = (ray / s.chunk) * s.chunk;
        const int bc = min(s.chunk, s.R - c0);
        const int dray = c0 + (int)(((long)(ray - c0) * s.N + j) % bc);
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = s.viewdirs[(long)dray * 3 + a];
    }
    const float t = s.pos[(long)row * s.stride + j];
    const float far = s.far ? s.far[ray] : 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        w.o[k * 3 + a] = o[a];
        w.d[k * 3 + a] = d[a];
        if (s.viewdirs) w.v[k * 3 + a] = v[a];
    }
    w.t[k] = t;
    if (s.far) w.far[k] = far;
    w.dst[k] = (row - s.first) * s.N + j;      // within the window: at most win x N, whatever the frame's size
}

__device__ __forceinline__ void point_count(const OccRows& w, int n, long long* __restrict__ kept_sum) {
    *w.count = n;
    if (kept_sum) *kept_sum = *kept_sum + (long long)n;
}

__global__ __launch_bounds__(OCC_BLOCK) void k_point_keep(PointSource src, OccGrid grid, uint8_t* __restrict__ keep,
                                                          int* __restrict__ totals) {
    __shared__ int s_seg[OCC_SEGS];
    const int cand = point_candidates(src);
    bool k[OCC_ROUNDS];
    // all four rounds' loads in front of the first store: the source columns are plain pointers, so a load behind a keep byte
    // would have to wait for it
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        k[it] = false;
        if (p < cand) {
            int row, ray, j;
            point_candidate(src, p, row, ray, j);
            k[it] = occ_keep(grid, src.rays_o + (long)ray * 3, src.dirs + (long)ray * 3, src.pos[(long)row * src.stride + j]);
        }
    }
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        if (p < cand) keep[p] = k[it] ? 1 : 0;
    }
    if (totals) occ_total(k, s_seg, totals);
}

__global__ __launch_bounds__(OCC_BLOCK) void k_point_emit(PointSource src, const uint8_t* __restrict__ keep, OccRows w,
                                                          long long* __restrict__ kept_sum) {
    __shared__ int s_part[OCC_BLOCK / 64];
    __shared__ int s_seg[OCC_SEGS];
    const OccRank rk = occ_rank(keep, point_candidates(src), w.totals, s_part, s_seg);
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it)
        if (rk.kept[it]) point_row(src, blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x, w, rk.k[it]);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) point_count(w, rk.upto, kept_sum);
}

__global__ __launch_bounds__(256) void k_point_emit_all(PointSource src, OccRows w, long long* __restrict__ kept_sum) {
    const int cand = point_candidates(src);
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0) point_count(w, cand, kept_sum);
    if (p < cand) point_row(src, p, w, p);
}

}  // namespace

void launch_point_keep(const PointSource& src, const OccGrid& grid, uint8_t* keep, int* totals, hipStream_t s) {
    const long P = (long)src.rows * src.len;
    if (P > 0) hipLaunchKernelGGL(k_point_keep, dim3(occ_blocks(P)), dim3(OCC_BLOCK), 0, s, src, grid, keep, totals);
}

void launch_point_list(const PointSource& src, const OccGrid* grid, uint8_t* keep, const OccRows& w, long long* kept_sum, hipStream_t s) {
    const long P = (long)src.rows * src.len;
    if (P <= 0) return;
    if (!grid || !grid->bits) {
        hipLaunchKernelGGL(k_point_emit_all, dim3((int)((P + 255) / 256)), dim3(256), 0, s, src, w, kept_sum);
        return;
    }
    launch_point_keep(src, *grid, keep, w.totals, s);
    hipLaunchKernelGGL(k_point_emit, dim3(occ_blocks(P)), dim3(OCC_BLOCK), 0, s, src, (const uint8_t*)keep, w, kept_sum);
}

}  // namespace neo
