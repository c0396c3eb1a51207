// The windowed, segmented march of a level (include/neo360_hip.h: KEEP RULE, STOP RULE, OUTSIDE STOP RULE, VANILLA MARCHING FRAME):
// the point-list builder (point_list.hip), the march kernels (march.hip) and the one level loop, march_level below, that the
// NeO-360 frames (api_tp.hip), the vanilla frame (vanilla_march.hip) and the PixelNeRF frame (api_pix.hip) drive with their own
// evaluator.  One set of kernels serves every user:
//
//                     NeO-360 inside the sphere       NeO-360 outside the sphere        vanilla                                 PixelNeRF
//   rows              dense, row = ray                compact, row k of ray map[k]      dense, row = ray                        dense, row = ray
//   position rows     (R, N)                          stride given (level 0: one row)   stride given (level 0: one shared row)  as vanilla
//   direction column  rays_d                          rays_d                            viewdirs                                rays_d
//   view column       quirk-Q1 ray                    quirk-Q1 ray                      not written                             quirk-Q1 ray
//   far column        not written                     written (the evaluators read it)  not written                             not written
//   grid              unit cube, edge cell outside    none                              caller's box, keep or skip outside      as vanilla
//   composite mode    1                               2                                 0                                       0
//   running value     (float)carry                    lam_c x (float)carry              (float)carry                            (float)carry
//
// The arithmetic differences (mode, the multiply) are compile-time; map, far, viewdirs and lam are optional pointers.
#pragma once
#include <algorithm>

#include "ctx.h"
#include "kernels.h"

namespace neo {

// Where the CANDIDATES of one point list come from: one window (rows first .. first + rows - 1 of the level), one segment (samples
// b0 .. b0 + len - 1 of the level's N).  Candidate p < n len is sample j = b0 + p % len of row first + map_w[p / len], n = *count_w
// alive rows (launch_cull_compact on the running value: ascending, the count a device word); map_w and count_w NULL: all `rows`
// rows.  The row's ray is map[row] (map NULL: the row itself); its position is pos[row stride + j].  A plain struct: travels by
// value as a kernel argument.
struct PointSource {
    const float *rays_o, *dirs;      // by ray: the origin and direction columns
    const float* viewdirs;           // optional: the view column, of the quirk-Q1 ray of the DENSE launch of the level's full N,
                                     // c0 + ((ray - c0) N + j) mod bc on the dense ray index (`chunk`, R: its arithmetic)
    const float* far;                // optional: the far column, far[ray]
    const float* pos;
    long stride;
    const int *map, *map_w, *count_w;
    int first, rows, R, N, b0, len, chunk;
};

// every sample of dense (R,N) rows as the candidates of one launch, p = ray N + j: the source of a level's whole keep mask
inline PointSource point_source_dense(const float* rays_o, const float* dirs, const float* pos, long stride, int R, int N) {
    PointSource src{};
    src.rays_o = rays_o, src.dirs = dirs, src.pos = pos, src.stride = stride;
    src.rows = src.R = R, src.N = src.len = N;
    return src;
}

// keep[p] = the KEEP RULE (occ_points.h) at candidate p, for every candidate; totals (may be null: the mask alone) = the kept
// candidates of every workgroup of OCC_POINTS candidates, 0 for one behind the candidates
void launch_point_keep(const PointSource& src, const OccGrid& grid, uint8_t* keep, int* totals, hipStream_t s);
// The point rows (OccRows) of the candidates: origin, direction and t, optional view and far columns, dst = (row - first) N + j, the sample's
// place in the window's rows.  *w.count =
// their number, also added to *kept_sum when not null.  grid NULL or without bits: every candidate, in candidate order, one launch.
// Otherwise launch_point_keep into keep (rows x len bytes) and w.totals, then the kept candidates by rank: ascending candidate
// order, identically on every run.  No atomics, no spinning: the count is written by one thread behind its producers.
void launch_point_list(const PointSource& src, const OccGrid* grid, uint8_t* keep, const OccRows& w, long long* kept_sum, hipStream_t s);

// per row k < R, of which n = *count (count null: R) are live: lam_c = lam[map[k]], alive = 1 and stop = stop_value where live;
// alive = -1 (dead at every eps >= 0), stop = 0 and lam_c = 0 behind n; value = 0; *kept (may be null) = kept_per_row x n.
// lam_c / alive / value / stop may be null; lam and map are read only for lam_c.
void launch_march_init(const float* lam, const int* map, const int* count, int R, float* lam_c, float* alive, float* value, int* stop,
                       int stop_value, long long* kept, long long kept_per_row, hipStream_t s);
// out[w.dst[p]] = w.out[p] for p < *w.count; P: the host's bound of the row count
void launch_march_scatter(const OccRows& w, long P, float* out, hipStream_t s);
// The stop rule of composite mode `mode` (2: outside the sphere, lam_c by row; 1: inside, rays_d and t_far by row; 0: the vanilla
// renderer's, rays_d by row, t_far and lam_c unread, stride 0 for a shared row of positions) over samples b0 .. b_end - 1 (whole
// segments) of rows first + map_w[kk], kk < *count_w (map_w / count_w null: rows 0 .. n_rows - 1).  carry: fp64 per row (may be null
// when b0 == 0 and nothing continues); v = the region's running value at the stop goes to value and to alive (either may be null);
// stop = samples marched.
void launch_march_advance(int mode, const float* rgbsigma, const float* pos, long stride, const float* rays_d, const float* t_far,
                          const float* lam_c, int N, int b0, int b_end, int segment, float eps, const int* map_w, const int* count_w,
                          int n_rows, int first, double* carry, float* value, float* alive, int* stop, hipStream_t s);
// dense by ray through the slot table: stop (R) / value (R) = the compact entry at slot[ray], 0 where slot[ray] < 0; either may be null
void launch_march_by_slot(const int* stop_c, const float* value_c, const int* slot, int R, int* stop, float* value, hipStream_t s);
// dst (R,N) = src_c row slot[ray], zeros where slot[ray] < 0
void launch_march_rows_by_slot(const float* src_c, const int* slot, int R, int N, float* dst, hipStream_t s);

}  // namespace neo

namespace neo_host {

// Per-row state of one level's march, carved from one buffer:
//   [carry fp64 R | with_lam: lam_c fp32 R | alive fp32 R | with_lam: value fp32 R | stop int R | the alive compaction of one
//    window | with a grid: one keep byte per candidate of one launch].
// alive is what the compaction reads: 1 in front of segment 0, then the running value; -1 behind a device row count.  with_lam: the
// outside-sphere rows, whose running value carries the row's lambda.  keep_dense: `keep` is a caller's (R,N) mask of a level that
// does not follow the stop rule - its candidates ARE the dense rows - and the loop writes window k0's bytes at keep + k0 N.
struct MarchState {
    double* carry;
    float *lam_c, *alive, *value;
    int *stop, *cws;
    uint8_t* keep;
    bool keep_dense = false;
    static size_t bytes(bool with_lam, size_t r, int win, size_t candidates = 0) {
        return r * (with_lam ? 24 : 16) + neo::cull_ws_ints(win) * sizeof(int) + candidates;
    }
    void carve(void* base, bool with_lam, size_t r, int win) {
        carry = static_cast<double*>(base);
        float* f = reinterpret_cast<float*>(carry + r);
        lam_c = with_lam ? f : nullptr;
        alive = with_lam ? f + r : f;
        value = with_lam ? f + 2 * r : nullptr;
        stop = reinterpret_cast<int*>(alive + (with_lam ? 2 : 1) * r);
        cws = stop + r;
        keep = reinterpret_cast<uint8_t*>(cws + neo::cull_ws_ints(win));
    }
};

// How a level stops.  follow: the level obeys the stop rule of composite mode `mode` at eps in segments of `segment`; otherwise it
// is ONE segment of N samples and stop = N (eps and segment unread).  rays_d, t_far: by row, what the rule of the mode reads; lam
// and count (outside the sphere only): the level's dense lambdas and the device count of live rows.
struct MarchRule {
    bool follow;
    float eps;
    int segment, mode;
    const float *rays_d, *t_far, *lam;
    const int* count;
};

// Point rows per launch of a level: what the caller reserves for march_level's `w` (occ_rows_bytes) and, with a grid, as keep bytes
inline size_t march_level_cap(const MarchRule& rule, int N, int win) {
    return static_cast<size_t>(win) * (rule.follow ? std::min(rule.segment, N) : N);
}

// THE LEVEL LOOP.  One level of src.R rows x src.N samples into `out` (R,N,4): zero rows, the state's init, then per window of
// `win` rows and per segment
//     [compact the alive rows, launch_cull_compact on the running value: !(alive < eps)]  ->  the point list of the segment
//     (launch_point_list: with a grid only the samples that the KEEP RULE keeps)  ->  eval(w, P), ONE compact evaluator launch on
//     single points under the device count *w.count <= P  ->  scatter into the window's zero rows  ->  [advance: the stop rule]
// with the bracketed steps only where the level follows the rule.  A sample that is skipped or lies behind its row's stop stays a
// zero row, which is what the advance and the composite read.  st.stop (may be null without `follow`): samples marched per row;
// *kept (may be null): the evaluated samples.  src: the level's columns; the loop fills first, rows, b0, len, map_w and count_w.
// Launches only: the caller checks.
template <class Eval>
int march_level(neo::PointSource src, const neo::OccGrid* grid, const MarchRule& rule, const MarchState& st, int win,
                const neo::OccRows& w, float* out, long long* kept, hipStream_t s, Eval&& eval) {
    const int R = src.R, N = src.N;
    const int seg = rule.follow ? std::min(rule.segment, N) : N;
    HIP_TRY(hipMemsetAsync(out, 0, static_cast<size_t>(R) * N * 16, s));
    neo::launch_march_init(rule.lam, src.map, rule.count, R, st.lam_c, st.alive, st.value, st.stop, rule.follow ? 0 : N, kept, 0, s);
    for (int k0 = 0; k0 < R; k0 += win) {
        src.first = k0;
        src.rows = std::min(win, R - k0);
        for (int b0 = 0; b0 < N; b0 += seg) {
            src.b0 = b0;
            src.len = std::min(seg, N - b0);
            const long P = static_cast<long>(src.rows) * src.len;
            src.map_w = src.count_w = nullptr;
            if (rule.follow) {
                neo::launch_cull_compact(st.alive + k0, st.alive + k0, src.rows, rule.eps, st.cws, nullptr, s);
                src.map_w = neo::cull_map_of(st.cws, src.rows);      // the workspace's layout follows the window's row count
                src.count_w = neo::cull_count_of(st.cws, src.rows);
            }
            neo::launch_point_list(src, grid, st.keep_dense ? st.keep + static_cast<size_t>(k0) * N : st.keep, w, kept, s);
            if (int rc = eval(w, P)) return rc;
            neo::launch_march_scatter(w, P, out + static_cast<size_t>(k0) * N * 4, s);
            if (rule.follow)
                neo::launch_march_advance(rule.mode, out, src.pos, src.stride, rule.rays_d, rule.t_far, st.lam_c, N, b0, b0 + src.len,
                                          rule.segment, rule.eps, src.map_w, src.count_w, src.rows, k0, st.carry, st.value, st.alive,
                                          st.stop, s);
        }
    }
    return NEO_OK;
}

// THE TWO-LEVEL MODE-0 FRAME (include/neo360_hip.h: VANILLA MARCHING FRAME, PIXELNERF MARCHING FRAME): a coarse + fine render whose
// levels are march_level in composite mode 0 - one shared row of level-0 positions, launch_resample between the levels.  What a
// renderer brings is data and its evaluator: the columns (dirs: what positions lie along; viewdirs / chunk: the optional view column of
// PointSource), its grid, its window, and two callbacks,
//     dense(level, src, out)     the renderer's dense launch of the level (src.pos / stride / R / N), taken when the level has neither
//                                a grid nor a rule to follow - the level of the plain render;
//     compact(level, rows, P)    its compact launch on the point rows (march_level's eval).
struct Mode0Frame {
    const float *rays_o, *dirs, *viewdirs, *rays_d;
    int R, chunk;
    float near, far;
    int n_coarse, n_fine, white_bkgd;
    float eps;
    int segment, coarse;
    float *rgb0, *acc0, *depth0, *rgb1, *acc1, *depth1;
    const neo_vanilla_march_samples *samples0, *samples1;      // per level: t, w, keep, stop, rows; any pointer may be null
    long long* kept;
};

template <class Dense, class Compact>
int march_frame_mode0(neo_ctx* ctx, const Mode0Frame& f, const neo::OccGrid* grid, int window, hipStream_t s, Dense&& dense,
                      Compact&& compact) {
    const int R = f.R;
    REQUIRE(R >= 0, "negative ray count");
    REQUIRE(f.n_coarse >= 3 && f.n_coarse <= 256 && f.n_fine >= 1 && f.n_coarse + 1 + f.n_fine <= 1024, "unsupported sample counts");
    REQUIRE(f.eps >= 0.0f && f.eps < 1.0f, "eps must lie in [0, 1)");
    REQUIRE(f.segment >= 64 && f.segment % 64 == 0, "segment must be a positive multiple of 64");
    if (R == 0) {
        if (f.kept) HIP_TRY(hipMemsetAsync(f.kept, 0, 2 * sizeof(long long), s));
        return NEO_OK;
    }
    REQUIRE(f.rays_o && f.dirs && f.rays_d, "null pointer");
    const int N0 = f.n_coarse + 1, N1 = N0 + f.n_fine;
    REQUIRE(static_cast<long>(R) * N1 <= 2147483647L - 1024, "too many points for 32-bit indices");
    const float* t0 = ctx->get_edges(f.n_coarse, f.near, f.far, s);
    const float* u = ctx->get_quantiles(f.n_fine, s);
    if (!t0 || !u) return fail(NEO_ERR_HIP, "constant table upload failed");
    ORDERED_LANE(ctx, s);      // writes this lane's workspaces only, reads the packed weights and the grid
    const int win = std::min(window, R);
    const size_t r = static_cast<size_t>(R);
    // eps == 0 stops nothing (a transmittance is >= 0 or NaN): no level follows the rule, stop = N
    const bool follow[2] = {f.coarse != 0 && f.eps > 0.0f, f.eps > 0.0f};
    const size_t candidates = grid ? static_cast<size_t>(win) * N1 : 0;
    if (ctx->ws[0].reserve(r * N0 * 16) || ctx->ws[1].reserve(r * N0 * 4) || ctx->ws[2].reserve(r * N1 * 4) ||
        ctx->ws[3].reserve(r * N1 * 16) || ctx->ws[4].reserve(MarchState::bytes(false, r, win, candidates)))
        return NEO_ERR_NOMEM;
    const neo_vanilla_march_samples *s0 = f.samples0, *s1 = f.samples1;
    MarchState st[2];
    st[0].carve(ctx->ws[4].p, false, r, win);
    st[1] = st[0];
    if (s0 && s0->stop) st[0].stop = s0->stop;
    if (s1 && s1->stop) st[1].stop = s1->stop;
    float* out0 = s0 && s0->rows ? s0->rows : ctx->ws[0].as<float>();
    float* w0 = s0 && s0->w ? s0->w : ctx->ws[1].as<float>();
    float* t1 = s1 && s1->t ? s1->t : ctx->ws[2].as<float>();
    float* out1 = s1 && s1->rows ? s1->rows : ctx->ws[3].as<float>();
    neo::PointSource src{};
    src.rays_o = f.rays_o, src.dirs = f.dirs, src.viewdirs = f.viewdirs, src.R = R, src.chunk = f.chunk;
    // one level into `out` (R,N,4) with its stops in the state: the dense launch, or march_level with the point rows in W[5]
    const auto level = [&](int lv, float* out, long long* kept) -> int {
        const MarchRule rule{follow[lv], f.eps, f.segment, 0, f.rays_d, nullptr, nullptr, nullptr};
        if (!rule.follow && !grid) {
            neo::launch_march_init(nullptr, nullptr, nullptr, R, nullptr, nullptr, nullptr, st[lv].stop, src.N, kept, src.N, s);
            return dense(lv, src, out);
        }
        const size_t cap = march_level_cap(rule, src.N, win);
        if (ctx->ws[5].reserve(neo::occ_rows_bytes(cap))) return NEO_ERR_NOMEM;
        neo::OccRows w;
        w.carve(ctx->ws[5].p, cap);
        return march_level(src, grid, rule, st[lv], win, w, out, kept, s,
                           [&](const neo::OccRows& rows, long P) { return compact(lv, rows, P); });
    };
    // level 0: one shared row of positions (stride 0)
    src.pos = t0, src.stride = 0, src.N = N0;
    if (int rc = level(0, out0, f.kept)) return rc;
    neo::launch_composite(0, out0, t0, 0, f.rays_d, nullptr, R, N0, f.white_bkgd, f.rgb0, f.acc0, f.depth0, w0, nullptr, s);
    if (neo::launch_resample(t0, 0, w0, u, 0, R, N0, f.n_fine, 0, t1, s)) return fail(NEO_ERR_INVALID, "unsupported sample counts");
    src.pos = t1, src.stride = N1, src.N = N1;
    if (int rc = level(1, out1, f.kept ? f.kept + 1 : nullptr)) return rc;
    neo::launch_composite(0, out1, t1, N1, f.rays_d, nullptr, R, N1, f.white_bkgd, f.rgb1, f.acc1, f.depth1, s1 ? s1->w : nullptr, nullptr, s);
    if (s0 && s0->t) HIP_TRY(hipMemcpyAsync(s0->t, t0, static_cast<size_t>(N0) * sizeof(float), hipMemcpyDeviceToDevice, s));
    // the keep masks of the whole rows, behind the stops as well (no grid: all ones)
    const neo::OccGrid mask_grid = grid ? *grid : neo::OccGrid{};
    if (s0 && s0->keep) neo::launch_point_keep(neo::point_source_dense(f.rays_o, f.dirs, t0, 0, R, N0), mask_grid, s0->keep, nullptr, s);
    if (s1 && s1->keep) neo::launch_point_keep(neo::point_source_dense(f.rays_o, f.dirs, t1, N1, R, N1), mask_grid, s1->keep, nullptr, s);
    return check_launch();
}

}  // namespace neo_host
