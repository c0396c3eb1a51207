// Point order of a NeO-360 evaluator launch: which (ray, sample) pair the tile-order ("virtual") point index gv stands for.
// Plain integer arithmetic, usable from host code (tests/test_point_order_cpu.py builds it into a stand-alone program) and
// from the kernels (tp_common.h).  Two maps, applied one after the other by launch_point:
//   quad_point   samples of four (or 8, 16) consecutive launch-order rays interleaved (TpScene::quad), then
//   patch_point  launch-order ray -> the pixel it stands for under the pixel-grid hint (TpScene::grid_w).
// Both are bijections on the launch's points [0, R * N); results of a launch do not depend on either.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEO_PO_HD __host__ __device__ __forceinline__
#else
#define NEO_PO_HD inline
#endif

namespace neo {
namespace tp {

// Virtual point index (tile order) -> the point it stands for: identity unless the launch carries a pixel-grid hint
// (TpScene::grid_w), then the rays of every WHOLE band of 2^ph image rows inside the launch are visited patch by patch
// (2^pw x 2^ph pixels, row-major inside a patch, patches left to right).  A bijection on the launch's points; rays outside whole
// bands (a shard's ragged ends) keep their place.
NEO_PO_HD long patch_point(long gv, int N, int R, int grid_w, long grid_first, int pw = 3, int ph = 3) {
    if (grid_w <= 0) return gv;
    const long rayv = gv / N;
    const int s = (int)(gv - rayv * N);
    const long band = (long)grid_w << ph;
    const long G = grid_first + rayv;
    const long b = G / band;
    if (b * band < grid_first || (b + 1) * band > grid_first + R) return gv;
    const int k = (int)(G - b * band), r = k & ((1 << (pw + ph)) - 1);
    const long Gt = b * band + (long)(r >> pw) * grid_w + ((long)(k >> (pw + ph)) << pw) + (r & ((1 << pw) - 1));
    return (Gt - grid_first) * N + s;
}

// Quad order.  Ray-major order puts 64 consecutive samples of one ray into a tile, and the four rows one gather instruction
// covers (tile rows 4 k .. 4 k + 3) are four adjacent samples of that ray.  With quad = G != 0 (rays per group: 4 = a quad, or 8, 16,
// .. - a multiple of 4) the launch-order rays 0 .. G * (R / G) - 1 are taken in groups of G consecutive rays, and inside a group the
// G N points go sample by sample: virtual index group * G N + G s + r stands for sample s of ray G * group + r.  A tile then holds
// 64 / G samples of G neighbouring rays (G = 4: 16 samples of a quad; G = 16: 4 samples of 16 rays) and the four rows of an
// instruction are four consecutive rays of the group at ONE sample index, whose taps fall on almost the same texels.  The last
// R % G rays keep ray-major order.  Returns the ray-major virtual index; identity for quad == 0.
NEO_PO_HD long quad_point(long gv, int N, int R, int quad) {
    if (!quad) return gv;
    const long span = (long)quad * N;
    const long q = gv / span;
    if (quad * q + quad > (long)R) return gv;
    const long within = gv - q * span;
    return (quad * q + within % quad) * N + within / quad;
}

// the two maps in the order the kernels apply them
NEO_PO_HD long launch_point(long gv, int N, int R, int quad, int grid_w, long grid_first, int pw = 3, int ph = 3) {
    return patch_point(quad_point(gv, N, R, quad), N, R, grid_w, grid_first, pw, ph);
}

}  // namespace tp
}  // namespace neo
