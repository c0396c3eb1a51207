// The occupancy grids: a per-scene grid over the world cube [-1, 1]^3 (NeO-360, neo_tp_set_occupancy) or over a caller-given box
// (vanilla, neo_vanilla_set_occupancy) decides, SAMPLE by sample, which points the evaluators see.  The rule of one point and the
// compaction are occ_points.h's, the point rows point_list.hip's, the loop march_level's (march.h).  This file holds
//
//   the installation    one helper behind both set_occupancy entry points: the bits into context-owned memory, the descriptor beside;
//   the pure functions  neo_tp_occupancy_keep / neo_vanilla_occupancy_keep, the KEEP RULE on caller rows (launch_point_keep);
//   k_occ_from_sigma    a lattice of activated densities -> the bits of a grid (threshold, dilation, unit-sphere clip);
//   OccRows             the carving of one launch's point rows.
//
// GRID LAYOUT (include/neo360_hip.h: OCCUPANCY GRID).  Cell (ix, iy, iz) is bit lin & 31 of the 32-bit word lin >> 5,
// lin = (ix G + iy) G + iz: G^3 / 32 words, iz fastest, the order of a contiguous bool (G, G, G) tensor.
#include "common.h"
#include "march.h"
#include "occ_points.h"

using namespace neo_host;

namespace neo {

namespace {

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

void launch_occ_iota(int* map, int n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_occ_iota, dim3((n + 255) / 256), dim3(256), 0, s, map, n);
}

void launch_occ_from_sigma(const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits, hipStream_t s,
                           bool sphere) {
    const long cells = (long)G * G * G;
    hipLaunchKernelGGL(sphere ? k_occ_from_sigma<true> : k_occ_from_sigma<false>, dim3((int)(cells / OCC_BLOCK)), dim3(OCC_BLOCK), 0, s, sigma, G, probes, threshold, dilate, bits);
}

}  // namespace neo

namespace {

using neo::occ_resolution_ok;      // occ_points.h
using neo::OCC_RESOLUTION_MSG;

// copies into context-owned memory that the frame calls read: an exclusive call, ordered across streams.  bits NULL removes the
// grid; desc: the validated descriptor of the new one (its bits are replaced by the context's copy)
int set_occupancy(neo_ctx* ctx, neo_ctx::OccInstalled& to, const uint32_t* bits, const neo::OccGrid& desc, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    ORDERED(ctx, s);
    to.clear();
    if (!bits) return NEO_OK;
    const size_t bytes = static_cast<size_t>(desc.G) * desc.G * desc.G / 8;
    if (to.bits.reserve(bytes)) return NEO_ERR_NOMEM;
    HIP_TRY(hipMemcpyAsync(to.bits.p, bits, bytes, hipMemcpyDeviceToDevice, s));
    to.grid = desc;
    to.grid.bits = to.bits.as<uint32_t>();
    return NEO_OK;
}

// a BOX GRID (include/neo360_hip.h) into the slot `to`: validated, then installed; bits NULL removes the slot's grid
int set_box_occupancy(neo_ctx* ctx, neo_ctx::OccInstalled& to, const uint32_t* bits, int G, const float* lo, const float* hi, int clip,
                      void* stream) {
    neo::OccGrid box{};
    if (bits) {
        REQUIRE(occ_resolution_ok(G), OCC_RESOLUTION_MSG);
        REQUIRE(lo && hi, "null pointer");
        if (const char* msg = neo::occ_grid_box(G, lo, hi, clip, box)) return fail(NEO_ERR_INVALID, "%s", msg);
    }
    return set_occupancy(ctx, to, bits, box, stream);
}

// the KEEP RULE on caller rows (R,N): touches no context-owned memory, no ordering scope (as neo_tp_edit_rows)
int occupancy_keep(const neo::OccGrid& grid, const float* rays_o, const float* dirs, const float* t, int R, int N, uint8_t* keep,
                   void* stream) {
    if (R == 0) return NEO_OK;
    REQUIRE(rays_o && dirs && t && keep, "null pointer");
    neo::launch_point_keep(neo::point_source_dense(rays_o, dirs, t, N, R, N), grid, keep, nullptr, static_cast<hipStream_t>(stream));
    return check_launch();
}

}  // namespace

extern "C" {

int neo_tp_set_occupancy(neo_ctx* ctx, const uint32_t* bits, int G, void* stream) {
    ENTER(ctx);
    REQUIRE(!bits || occ_resolution_ok(G), OCC_RESOLUTION_MSG);
    return set_occupancy(ctx, ctx->occ, bits, neo::occ_grid_unit(bits, G), stream);
}

int neo_vanilla_set_occupancy(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip, void* stream) {
    ENTER(ctx);
    return set_box_occupancy(ctx, ctx->vocc, bits, G, lo, hi, clip, stream);
}

// the same BOX GRID in the PixelNeRF decoder's own slot (neo_pix_render_marching reads it)
int neo_pix_set_occupancy(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip, void* stream) {
    ENTER(ctx);
    return set_box_occupancy(ctx, ctx->pocc, bits, G, lo, hi, clip, stream);
}

int neo_tp_set_skip_window(neo_ctx* ctx, int rays) {
    ENTER(ctx);
    REQUIRE(rays >= 0 && rays <= 65536, "skip window must be 0 (the default) or 1 .. 65536 rays");
    ctx->skip_window = rays;
    return NEO_OK;
}

int neo_tp_occupancy_keep(neo_ctx* ctx, const uint32_t* bits, int G, const float* rays_o, const float* rays_d, const float* t, int R,
                          int N, uint8_t* keep, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(static_cast<long>(R) * N <= 2147483647L - 1024, "too many points for 32-bit indices");
    REQUIRE(!bits || occ_resolution_ok(G), OCC_RESOLUTION_MSG);
    return occupancy_keep(neo::occ_grid_unit(bits, G), rays_o, rays_d, t, R, N, keep, stream);
}

int neo_vanilla_occupancy_keep(neo_ctx* ctx, const uint32_t* bits, int G, const float* lo, const float* hi, int clip,
                               const float* rays_o, const float* dirs, const float* t, int R, int N, uint8_t* keep, void* stream) {
    ENTER(ctx);
    REQUIRE(R >= 0 && N >= 1, "bad shape");
    REQUIRE(static_cast<long>(R) * N <= 2147483647L - 1024, "too many points for 32-bit indices");
    neo::OccGrid box{};
    if (bits) {
        REQUIRE(occ_resolution_ok(G), OCC_RESOLUTION_MSG);
        REQUIRE(lo && hi, "null pointer");
        if (const char* msg = neo::occ_grid_box(G, lo, hi, clip, box)) return fail(NEO_ERR_INVALID, "%s", msg);
        box.bits = bits;
    }
    return occupancy_keep(box, rays_o, dirs, t, R, N, keep, stream);
}

}  // extern "C"

namespace {

// the pure function k_occ_from_sigma; touches no context-owned memory
int occ_from_sigma(neo_ctx* ctx, const float* sigma, int G, int probes, float threshold, int dilate, uint32_t* bits, bool sphere,
                   void* stream) {
    ENTER(ctx);
    REQUIRE(occ_resolution_ok(G), OCC_RESOLUTION_MSG);
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
