// Empty-space skipping of the NeO-360 frame (neo_tp_render_skipping): a per-scene occupancy grid over the world cube [-1, 1]^3
// decides, SAMPLE by sample, which inside-sphere points the evaluators see.  This file holds everything but the driver
// (tp_eval_skipping, api_tp.hip):
//
//   k_occ_keep          the classifier: x = o + t d (point_setup_row's expression, this library's -ffp-contract=off), the cell of x,
//                       one bit of the grid -> a uint8 keep mask over dense (R, N) rows; with `totals` also the kept points of every
//                       workgroup (the first launch of the compaction);
//   k_occ_emit          the second launch of the compaction: the compact rows of the kept points of one WINDOW of rays;
//   k_occ_scatter       compact (rgb, sigma) rows back to their dense place, zeros where a sample was skipped;
//   k_occ_from_sigma    a lattice of activated densities -> the bits of a grid (threshold, dilation, unit-sphere clip).
//
// GRID LAYOUT (include/neo360_hip.h: OCCUPANCY GRID).  Cell (ix, iy, iz) is bit lin & 31 of the 32-bit word lin >> 5,
// lin = (ix G + iy) G + iz: G^3 / 32 words, iz fastest, the order of a contiguous bool (G, G, G) tensor.
//
// COMPACTION.  The totals / emit scheme of compact.h on POINTS: no atomics, no spinning on other workgroups, survivors in ascending
// point order p = r N + j of the window, identically on every run.  A workgroup owns 1024 consecutive points (4 rounds of 256
// threads, one ballot per wave and round: 16 segments of 64 points in LDS), and emit sums the totals of the workgroups in front of
// it as compact.h does.  That sum is linear in the workgroups of ONE window, and the driver keeps windows small: at its default of
// 4096 rays a level-1 window of the 129 + 385 frame is 1540 workgroups, 1.2 M integer reads per window for all of them together -
// no hierarchical scan is needed at that size.
//
// A compact row is ONE point: the evaluator's compact launch with N = 1 and the identity map forms x = o[row] + t[row] d[row] and
// takes the view direction of row `row` itself (point_setup_row: c0 + ((row - c0) 1 + 0) mod bc = row), so emit writes, per kept
// point, the origin and direction of its ray, its t, and the view direction of the quirk-Q1 ray of the DENSE launch,
// c0 + ((r - c0) N + j) mod bc.  The evaluator sources are not touched.
#include "common.h"
#include "occ_points.h"
#include "tp_frame.h"

using namespace neo_host;

namespace neo {

namespace {

// the workgroup layout, occ_cell, occ_keep_point (the KEEP RULE) and occ_rank: occ_points.h, shared with accelerate.hip

// rays_o / rays_d: row 0 is the ray of point 0; t, keep: P = rays x N points.  totals (may be null): kept points per workgroup.
__global__ __launch_bounds__(OCC_BLOCK) void k_occ_keep(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                        const float* __restrict__ t, int P, int N,
                                                        const uint32_t* __restrict__ bits, int G, uint8_t* __restrict__ keep,
                                                        int* __restrict__ totals) {
    __shared__ int s_seg[OCC_SEGS];
    bool k[OCC_ROUNDS];
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        k[it] = false;
        if (p < P) {
            const int r = p / N;
            k[it] = occ_keep_point(bits, G, rays_o + (long)r * 3, rays_d + (long)r * 3, t[p]);
            keep[p] = k[it] ? 1 : 0;
        }
    }
    if (totals) occ_total(k, s_seg, totals);
}

// One window: rays r0 .. r0 + P / N - 1 of the frame's R rays; t and keep are the window's rows.  Per kept point p = r_w N + j:
// c_o, c_d = the ray's origin and direction, c_v = the view direction of ray c0 + ((r - c0) N + j) mod bc (r = r0 + r_w, c0 and bc
// the reference chunk of r: the `chunk` arithmetic of point_setup_row), c_t = t, dst = p.  The last workgroup writes the count and
// adds it to *kept_sum (one thread, behind the previous window in stream order: no atomic).
__global__ __launch_bounds__(OCC_BLOCK) void k_occ_emit(const float* __restrict__ rays_o, const float* __restrict__ rays_d,
                                                        const float* __restrict__ viewdirs, const float* __restrict__ t,
                                                        const uint8_t* __restrict__ keep, int r0, int R, int P, int N, int chunk,
                                                        const int* __restrict__ totals, float* __restrict__ c_o,
                                                        float* __restrict__ c_d, float* __restrict__ c_v, float* __restrict__ c_t,
                                                        int* __restrict__ dst, int* __restrict__ count,
                                                        long long* __restrict__ kept_sum) {
    __shared__ int s_part[OCC_BLOCK / 64];
    __shared__ int s_seg[OCC_SEGS];
    const OccRank rk = occ_rank(keep, P, totals, s_part, s_seg);
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        if (!rk.kept[it]) continue;
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        const int k = rk.k[it];
        const int rw = p / N, j = p - rw * N;
        const int ray = r0 + rw;
        const int c0 = (ray / chunk) * chunk;
        const int bc = min(chunk, R - c0);
        const int dray = c0 + ((ray - c0) * N + j) % bc;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            c_o[(long)k * 3 + a] = rays_o[(long)ray * 3 + a];
            c_d[(long)k * 3 + a] = rays_d[(long)ray * 3 + a];
            c_v[(long)k * 3 + a] = viewdirs[(long)dray * 3 + a];
        }
        c_t[k] = t[p];
        dst[k] = p;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *count = rk.upto;
        if (kept_sum) *kept_sum = *kept_sum + (long long)rk.upto;
    }
}

// dense row p of the window: the compact row of its rank where kept, (0, 0, 0, 0) where skipped
__global__ __launch_bounds__(OCC_BLOCK) void k_occ_scatter(const uint8_t* __restrict__ keep, int P, const int* __restrict__ totals,
                                                           const float4* __restrict__ c_out, float4* __restrict__ out) {
    __shared__ int s_part[OCC_BLOCK / 64];
    __shared__ int s_seg[OCC_SEGS];
    const OccRank rk = occ_rank(keep, P, totals, s_part, s_seg);
#pragma unroll
    for (int it = 0; it < OCC_ROUNDS; ++it) {
        const int p = blockIdx.x * OCC_POINTS + it * OCC_BLOCK + threadIdx.x;
        if (p >= P) continue;
        out[p] = rk.kept[it] ? c_out[rk.k[it]] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__global__ void k_occ_iota(int* __restrict__ map, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) map[i] = i;
}

// One thread per cell, 64 consecutive cells (one wave) = two words of the grid.  sigma: (M, M, M), M = G probes, the lattice of
// cell sub-centres in the index order of the grid.  A cell is RAW-occupied iff one of its probes^3 densities is not <= threshold (a
// NaN density counts as occupied, so that it reaches the caller); occupied iff a cell within `dilate` cells of it in every axis (the 26-neighbourhood, `dilate` times) is raw-occupied;
// and cleared when no point of it lies inside the closed unit sphere: with h = G / 2 and n_a = the distance of the cell from the
// origin along axis a in whole cells (i - h for i >= h, h - 1 - i below), iff n_x^2 + n_y^2 + n_z^2 > h^2 - integers, no rounding.
// SPHERE = false (neo_occupancy_from_sigma_box: a grid over a caller's box, which has no unit sphere) leaves that last step out.
template <bool SPHERE>
__global__ __launch_bounds__(OCC_BLOCK) void k_occ_from_sigma(const float* __restrict__ sigma, int G, int probes, float threshold,
                                                              int dilate, uint32_t* __restrict__ bits) {
    const int idx = blockIdx.x * OCC_BLOCK + threadIdx.x;         // G^3 is a multiple of 256
    const int iz = idx % G, iy = (idx / G) % G, ix = idx / (G * G);
    const int h = G / 2;
    const int nx = ix >= h ? ix - h : h - 1 - ix, ny = iy >= h ? iy - h : h - 1 - iy, nz = iz >= h ? iz - h : h - 1 - iz;
    bool occ = false;
    if (!SPHERE || nx * nx + ny * ny + nz * nz <= h * h) {
        const long M = (long)G * probes;
        for (int cx = max(ix - dilate, 0); cx <= min(ix + dilate, G - 1) && !occ; ++cx)
            for (int cy = max(iy - dilate, 0); cy <= min(iy + dilate, G - 1) && !occ; ++cy)
                for (int cz = max(iz - dilate, 0); cz <= min(iz + dilate, G - 1) && !occ; ++cz)
                    for (int a = 0; a < probes; ++a)
                        for (int b = 0; b < probes; ++b)
                            for (int c = 0; c < probes; ++c)
                                occ = occ || !(sigma[(((long)cx * probes + a) * M + ((long)cy * probes + b)) * M + (long)cz * probes + c] <= threshold);
    }
    const unsigned long long ballot = __ballot(occ);
    if ((threadIdx.x & 63) == 0) {
        bits[idx >> 5] = (uint32_t)ballot;
        bits[(idx >> 5) + 1] = (uint32_t)(ballot >> 32);
    }
}

}  // namespace

void OccRows::carve(void* base, size_t cap) {
    float* f = static_cast<float*>(base);
    out = f, o = f + cap * 4, d = f + cap * 7, v = f + cap * 10, t = f + cap * 13;      // the float4 rows first: 16-byte aligned
    far = f + cap * 14;
    int* i = reinterpret_cast<int*>(f + cap * 15);
    dst = i, iota = i + cap, count = i + 2 * cap, totals = count + 1;
}
size_t occ_rows_bytes(size_t cap) { return cap * 68 + (1 + (size_t)occ_blocks((long)cap)) * sizeof(int); }

void launch_occ_keep(const float* rays_o, const float* rays_d, const float* t, int R, int N, const uint32_t* bits, int G, uint8_t* keep,
                     hipStream_t s) {
    if (R <= 0 || N <= 0) return;
    const int P = R * N;
    hipLaunchKernelGGL(k_occ_keep, dim3(occ_blocks(P)), dim3(OCC_BLOCK), 0, s, rays_o, rays_d, t, P, N, bits, G, keep, (int*)nullptr);
}

void launch_occ_iota(int* map, int n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_occ_iota, dim3((n + 255) / 256), dim3(256), 0, s, map, n);
}

void launch_occ_compact(const float* rays_o, const float* rays_d, const float* viewdirs, const float* t_win, int r0, int rays, int R,
                        int N, int chunk, const uint32_t* bits, int G, uint8_t* keep_win, const OccRows& w, long long* kept_sum,
                        hipStream_t s) {
    if (rays <= 0) return;
    const int P = rays * N, nb = occ_blocks(P);
    hipLaunchKernelGGL(k_occ_keep, dim3(nb), dim3(OCC_BLOCK), 0, s, rays_o + (size_t)r0 * 3, rays_d + (size_t)r0 * 3, t_win, P, N, bits,
                       G, keep_win, w.totals);
    hipLaunchKernelGGL(k_occ_emit, dim3(nb), dim3(OCC_BLOCK), 0, s, rays_o, rays_d, viewdirs, t_win, (const uint8_t*)keep_win, r0, R, P,
                       N, chunk, (const int*)w.totals, w.o, w.d, w.v, w.t, w.dst, w.count, kept_sum);
}

void launch_occ_scatter(const uint8_t* keep_win, int P, const OccRows& w, float* out_win, hipStream_t s) {
    if (P <= 0) return;
    hipLaunchKernelGGL(k_occ_scatter, dim3(occ_blocks(P)), dim3(OCC_BLOCK), 0, s, keep_win, P, (const int*)w.totals,
                       (const float4*)w.out, (float4*)out_win);
}

void launch_occ_from_sigma(const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits, hipStream_t s,
                           bool sphere) {
    const long cells = (long)G * G * G;
    hipLaunchKernelGGL(sphere ? k_occ_from_sigma<true> : k_occ_from_sigma<false>, dim3((int)(cells / OCC_BLOCK)), dim3(OCC_BLOCK), 0, s, sigma, G, probes, threshold, dilate, bits);
}

}  // namespace neo

namespace {

bool occ_resolution_ok(int G) { return G == 8 || G == 16 || (G >= 32 && G <= 256 && G % 32 == 0); }

}  // namespace

extern "C" {

// copies into context-owned memory that the frame calls read: an exclusive call, ordered across streams
int neo_tp_set_occupancy(neo_ctx* ctx, const uint32_t* bits, int G, void* stream) {
    ENTER(ctx);
    hipStream_t s = static_cast<hipStream_t>(stream);
    ORDERED(ctx, s);
    if (!bits) {
        ctx->occ_G = 0;
        return NEO_OK;
    }
    REQUIRE(occ_resolution_ok(G), "occupancy resolution must be 8, 16 or a multiple of 32 in [32, 256]");
    const size_t bytes = static_cast<size_t>(G) * G * G / 8;
    ctx->occ_G = 0;
    if (ctx->occ_bits.reserve(bytes)) return NEO_ERR_NOMEM;
    HIP_TRY(hipMemcpyAsync(ctx->occ_bits.p, bits, bytes, hipMemcpyDeviceToDevice, s));
    ctx->occ_G = G;
    return NEO_OK;
}

int neo_tp_set_skip_window(neo_ctx* ctx, int rays) {
    ENTER(ctx);
    REQUIRE(rays >= 0 && rays <= 65536, "skip window must be 0 (the default) or 1 .. 65536 rays");
    ctx->skip_window = rays;
    return NEO_OK;
}

// the pure function k_occ_keep on caller rows; touches no context-owned memory: no ordering scope (as neo_tp_edit_rows)
int neo_tp_occupancy_keep(neo_ctx* ctx, const uint32_t* bits, int G, const float* rays_o, const float* rays_d, const float* t, int R,
                          int N, uint8_t* keep, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(static_cast<long>(R) * N <= 2147483647L - 1024, "too many points for 32-bit indices");
    REQUIRE(!bits || occ_resolution_ok(G), "occupancy resolution must be 8, 16 or a multiple of 32 in [32, 256]");
    if (R == 0) return NEO_OK;
    REQUIRE(rays_o && rays_d && t && keep, "null pointer");
    neo::launch_occ_keep(rays_o, rays_d, t, R, N, bits, G, keep, static_cast<hipStream_t>(stream));
    return check_launch();
}

}  // extern "C"

namespace {

// the pure function k_occ_from_sigma; touches no context-owned memory
int occ_from_sigma(neo_ctx* ctx, const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits, bool sphere,
                   void* stream) {
    ENTER(ctx);
    REQUIRE(occ_resolution_ok(G), "occupancy resolution must be 8, 16 or a multiple of 32 in [32, 256]");
    REQUIRE(probes >= 1 && probes <= 4, "1 .. 4 probes per cell and axis");
    REQUIRE(dilate >= 0 && dilate <= 4, "dilation of 0 .. 4 cells");
    REQUIRE(!(threshold != threshold), "the density threshold is NaN");
    REQUIRE(sigma && bits, "null pointer");
    neo::launch_occ_from_sigma(sigma, G, probes, threshold, dilate, bits, static_cast<hipStream_t>(stream), sphere);
    return check_launch();
}

}  // namespace

extern "C" {

int neo_occupancy_from_sigma(neo_ctx* ctx, const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits,
                             void* stream) {
    return occ_from_sigma(ctx, sigma, G, probes, threshold, dilate, bits, true, stream);
}

int neo_occupancy_from_sigma_box(neo_ctx* ctx, const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits,
                                 void* stream) {
    return occ_from_sigma(ctx, sigma, G, probes, threshold, dilate, bits, false, stream);
}

}  // extern "C"
