// The segmented march of the NeO-360 frame (march.hip, accelerate.hip; driver: tp_eval_march / tp_render_marching in api_tp.hip;
// include/neo360_hip.h: STOP RULE, OUTSIDE STOP RULE, ACCELERATED FRAME).  One set of kernels serves both regions:
//
//                     inside the sphere               outside the sphere
//   rows              dense, row = ray                compact, row k of ray map[k]
//   position rows     (R, N)                          stride given (level 0: one shared row)
//   far column        not written                     written (the outside evaluators read it)
//   composite mode    1                               2
//   running value     (float)carry                    lam_c x (float)carry
//
// The arithmetic differences (mode, the multiply) are compile-time; map, far and lam are optional pointers.
#pragma once
#include "kernels.h"

namespace neo {

// per row k < R, of which n = *count (count null: R) are live: lam_c = lam[map[k]], alive = 1 and stop = stop_value where live;
// alive = -1 (dead at every eps >= 0), stop = 0 and lam_c = 0 behind n; value = 0; *kept (may be null) = kept_per_row x n.
// lam_c / alive / value may be null; lam and map are read only for lam_c.
void launch_march_init(const float* lam, const int* map, const int* count, int R, float* lam_c, float* alive, float* value, int* stop,
                       int stop_value, long long* kept, long long kept_per_row, hipStream_t s);
// the point rows (OccRows, as launch_occ_compact leaves them) of samples b0 .. b0 + len - 1 of rows first + map_w[kk],
// kk < *count_w <= rows: origin and direction of the row's ray (map[row]; map null: the row itself), t = pos[row stride + j], the view
// direction of the quirk-Q1 ray of the dense launch of the level's full N on the DENSE ray index, dst = row N + j; with far also
// w.far = far[ray].  *w.count = *count_w len, also added to *kept_sum when not null
void launch_march_emit(const float* rays_o, const float* rays_d, const float* viewdirs, const float* far, const float* pos, long stride,
                       const int* map, const int* map_w, const int* count_w, int first, int rows, int R, int N, int b0, int len, int chunk,
                       const OccRows& w, long long* kept_sum, hipStream_t s);
// out[w.dst[p]] = w.out[p] for p < *w.count; P: the host's bound of the row count
void launch_march_scatter(const OccRows& w, long P, float* out, hipStream_t s);
// the stop rule of the region over samples b0 .. b_end - 1 (whole segments) of rows first + map_w[kk], kk < *count_w (map_w / count_w
// null: rows 0 .. n_rows - 1).  carry: fp64 per row (may be null when b0 == 0 and nothing continues); v = the region's running value
// at the stop goes to value and to alive (either may be null); stop = samples marched.  Inside: rays_d and t_far by row; outside: lam_c.
void launch_march_advance(bool outside, const float* rgbsigma, const float* pos, long stride, const float* rays_d, const float* t_far,
                          const float* lam_c, int N, int b0, int b_end, int segment, float eps, const int* map_w, const int* count_w,
                          int n_rows, int first, double* carry, float* value, float* alive, int* stop, hipStream_t s);
// the same kernel by composite mode: 2 and 1 are the two calls above; 0 is the vanilla renderer's rule (rays_d by row, t_far and lam_c
// unread, stride 0 for a shared row of positions).  launch_march_advance(outside, ...) is this with mode = outside ? 2 : 1.
void launch_march_advance_mode(int mode, const float* rgbsigma, const float* pos, long stride, const float* rays_d, const float* t_far,
                               const float* lam_c, int N, int b0, int b_end, int segment, float eps, const int* map_w,
                               const int* count_w, int n_rows, int first, double* carry, float* value, float* alive, int* stop,
                               hipStream_t s);
// dense by ray through the slot table: stop (R) / value (R) = the compact entry at slot[ray], 0 where slot[ray] < 0; either may be null
void launch_march_by_slot(const int* stop_c, const float* value_c, const int* slot, int R, int* stop, float* value, hipStream_t s);
// dst (R,N) = src_c row slot[ray], zeros where slot[ray] < 0
void launch_march_rows_by_slot(const float* src_c, const int* slot, int R, int N, float* dst, hipStream_t s);

// accelerate.hip - the inside emit restricted to the samples that the KEEP RULE keeps.  The candidates are launch_march_emit's rows
// (sample b0 + p % len of ray r0 + map[p / len], p < *alive len); keep (rays x len bytes) receives their keep bytes, w.totals the
// per-workgroup sums, and the kept ones leave point rows as launch_march_emit's, in ascending candidate order; *w.count = their
// number, also added to *kept_sum when not null.  Two launches, no atomics.
void launch_acc_compact(const float* rays_o, const float* rays_d, const float* viewdirs, const float* t, const int* map, const int* alive,
                        int r0, int rays, int R, int N, int b0, int len, int chunk, const uint32_t* bits, int G, uint8_t* keep,
                        const OccRows& w, long long* kept_sum, hipStream_t s);

}  // namespace neo
