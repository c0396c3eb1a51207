// Backward of the scene encoder's pillar stage (pillar.hip; models/neo360/encoder_tp_fusion_conv.py:472-578 under autograd).
// The forward under autograd is pillar.hip's launch_pillar, unchanged, writing h1, h2, L and the scores to a caller-owned tape
// instead of the context workspace (bitwise the floor-plans of neo_enc_floorplans).  Everything here is EXACT fp32
// (v_mfma_f32_32x32x2_f32), like every other training operator: gradients span many decades and fp16's range would drop the
// small ones.
//
// Per cell-view row m (M = nv G0 G1 G2 rows, view-major, x slowest) and axis a with softmax weight w_a, floor-plan gradient
// row g_a of the pillar the cell lies in:
//   1. aggregate:  t_a = g_a . L,   g_s_a = w_a (t_a - sum_pillar w t_a)  (= w_a (g_a . L - g_a . fp_a)),   g_L = sum_a w_a g_a
//                  k_agg_dot (t), k_agg_stats (per pillar: max, denominator and sum w t, in the forward's order), k_agg_bwd
//                  (g_s, g_L written once per row, no atomics)
//   2. scorers:    k_pt_gemm<false, 0> recomputes z = L W0_a[:, :512]^T + b0_a + coord_a W0_a[:, 512] and writes
//                  g_z = g_s_a head_a 1[z > 0] in its epilogue, with per-tile partials of sum g_s relu(z) (head weight) and
//                  sum g_z coord_a (W0_a's coordinate column), reduced in a fixed order (k_tile_reduce); the 512 x 512 part of
//                  dW0_a and db0_a go through launch_weight_grad (k_dw, split-K, ordered partial tiles) on the materialised
//                  g_z; g_L += g_z W0_a[:, :512] (k_pt_gemm<true, 1>, accumulating)
//   3. depth_fc:   g_h2 = (g_L W2) 1[h2 > 0], g_h1 = (g_h2 W1) 1[h1 > 0] (masks in the GEMM epilogue), weight gradients by
//                  launch_weight_grad; the first layer's input x = [latent 512 | cam xyz | masked dir] is re-gathered
//                  (k_gather_x: 3 floats of tape per row saved for 518 of recompute reads)
//   4. latent:     g_x_lat = g_h1 W0[:, :512], scattered through the transpose of the bilinear lookup (same taps as the
//                  forward) into a channels-last accumulator (atomics), then added into the NCHW gradient (k_cl_add_nchw)
// No gradient reaches poses, focal or the principal point (the decoder's operators do the same).
#include <hip/hip_runtime.h>

#include "mfma_tile.h"
#include "pillar_train.h"
#include "tp_common.h"
#include "train_kernels.h"

namespace neo {

namespace {

constexpr int W5 = 512;        // layer width
constexpr int BM = 128;        // GEMM tile rows
constexpr int BN = 128;        // GEMM tile columns (4 tiles span the 512 outputs)
constexpr int BK = 32;         // K step
constexpr int AP = BK + 4;     // pitch of a K-fastest LDS tile [rows][k]
constexpr int BPT = BN + 4;    // pitch of an N-fastest LDS tile [k][n]
constexpr int LDX = 518;       // row pitch of the re-gathered first-layer input

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // 16-B global access at 4-B alignment (pitches 513, 518)

// axis index of row m's cell along `axis` (0: x = i, 1: y = j, 2: z = k)
__device__ __forceinline__ int cell_index(long m, int G0, int G1, int G2, int axis) {
    const long NC = (long)G0 * G1 * G2;
    const long cell = m % NC;
    if (axis == 0) return (int)(cell / ((long)G1 * G2));
    if (axis == 1) return (int)((cell / G2) % G1);
    return (int)(cell % G2);
}

// pillar of row m for scorer a (0: xz plan, softmax along y; 1: yz plan, along x; 2: xy plan, along z) = the floor-plan row
__device__ __forceinline__ long pillar_of(long m, int G0, int G1, int G2, int a) {
    const long NC = (long)G0 * G1 * G2;
    const long v = m / NC, cell = m - v * NC;
    const long i = cell / ((long)G1 * G2), j = (cell / G2) % G1, k = cell % G2;
    if (a == 0) return (v * G0 + i) * G2 + k;
    if (a == 1) return (v * G1 + j) * G2 + k;
    return (v * G0 + i) * G1 + j;
}

// row m's view, bilinear taps and [cam xyz | masked dir]: k_pillar_dense<0, *>'s per-row set-up, operation for operation
struct RowGeo {
    int v;
    tp::TapSet t;
    float ex[6];
};
__device__ __forceinline__ RowGeo row_geo(const PillarGeom& gm, long m) {
    RowGeo r;
    const long NC = (long)gm.G0 * gm.G1 * gm.G2;
    const int v = (int)(m / NC);
    const long cell = m - (long)v * NC;
    const int i = (int)(cell / ((long)gm.G1 * gm.G2)), j = (int)((cell / gm.G2) % gm.G1), k = (int)(cell % gm.G2);
    const float w3[3] = {gm.axes[i], gm.axes[256 + j], gm.axes[512 + k]};
    const float* rot = gm.rot[v];
    const float* trn = gm.trans[v];
    const float cxp = (rot[0] * w3[0] + rot[1] * w3[1] + rot[2] * w3[2]) + trn[0];
    const float cyp = (rot[3] * w3[0] + rot[4] * w3[1] + rot[5] * w3[2]) + trn[1];
    const float czp = (rot[6] * w3[0] + rot[7] * w3[1] + rot[8] * w3[2]) + trn[2];
    const float mask = czp < 1e-3f ? 1.0f : 0.0f;
    float d[3], n2 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) { d[a] = w3[a] - gm.cpos[v][a]; const float e = d[a] + 1e-9f; n2 += e * e; }
    const float nrm = sqrtf(n2);
    const float den = czp + 1e-9f;
    const float u = (-cxp / den) * gm.focal + gm.cx;
    const float w_ = (-cyp / den) * (-gm.focal) + gm.cy;
    r.v = v;
    r.t = tp::bilinear_taps(u * gm.sx - 1.0f, w_ * gm.sy - 1.0f, gm.Wf, gm.Hf);
    r.ex[0] = cxp; r.ex[1] = cyp; r.ex[2] = czp;
#pragma unroll
    for (int a = 0; a < 3; ++a) r.ex[3 + a] = (d[a] / nrm) * mask;
    return r;
}

// |z| below which the scorer recompute re-evaluates z in fp64 (fp32 accumulation error of a 513-term row: ~1e-7 .. 1e-6;
// 1e-4 cost 12 ms of the 64^3 backward, 1e-5 about a tenth of that)
constexpr float KINK = 1e-5f;

// z = x . w[:512] + coord w[512] + bias in fp64 (rare: only entries within KINK of the ReLU's kink)
__device__ __attribute__((noinline)) double z_exact(const float* __restrict__ x, const float* __restrict__ w, float bias, float coord) {
    double z = (double)bias + (double)coord * (double)w[512];
    for (int k = 0; k < W5; k += 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + k);
        const f4u b = *reinterpret_cast<const f4u*>(w + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) z += (double)a[e] * (double)b[e];
    }
    return z;
}

struct PtEpi {
    // EPI 0 (scorer recompute): z = acc + bias[n] + coord(m) wc[n * ldb]; C = g_z; part[tile][0 / 1][n] = sum g_s relu(z) / sum g_z coord
    const float* bias;
    const float* wc;
    const float* axes;
    int G0, G1, G2, coord_axis;
    const float* gs;
    const float* head;
    float* part;
    // EPI 1 (input gradient): C = (accumulate ? C : 0) + acc, zeroed where mask (ld 512) <= 0
    const float* mask;
    int accumulate;
};

// C[M][512] = A[M][512] . op(B): BT = false: B stored [n][k] (a weight (out, in) read as W^T: z = x W^T);
// BT = true: B stored [k][n] (dX = dY W).  128 x 128 tiles, 4 waves of 64 x 64, K stepped by 32 through one LDS tile pair with
// the next step's operands in registers.  Rows beyond M are clamped on load and not stored.
template <bool BT, int EPI>
__global__ __launch_bounds__(256, 2) void k_pt_gemm(long M, const float* __restrict__ A, const float* __restrict__ B, long ldb,
                                                    float* __restrict__ C, PtEpi ep) {
    __shared__ __attribute__((aligned(16))) float As[BM * AP];
    __shared__ __attribute__((aligned(16))) float Bs[BT ? BK * BPT : BN * AP];
    LaneCtx L;
    L.init();
    const int tid = threadIdx.x;
    const int n0 = blockIdx.x * BN;
    const long m0 = (long)blockIdx.y * BM;
    const int wm = L.wv & 1, wn = L.wv >> 1;
    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][nt][r] = 0.0f;
    // this thread's four 16-B pieces of each operand tile
    const float* pa[4];
    const float* pb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int idx4 = tid + 256 * j;
        long r = m0 + (idx4 >> 3);
        if (r >= M) r = M - 1;
        pa[j] = A + r * W5 + (idx4 & 7) * 4;
        pb[j] = BT ? B + (long)(idx4 >> 5) * ldb + n0 + (idx4 & 31) * 4 : B + (long)(n0 + (idx4 >> 3)) * ldb + (idx4 & 7) * 4;
    }
    f32x4 qa[4], qb[4];
    auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            qa[j] = *reinterpret_cast<const f4u*>(pa[j] + k0);
            qb[j] = *reinterpret_cast<const f4u*>(pb[j] + (BT ? (long)k0 * ldb : (long)k0));
        }
    };
    auto stage = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx4 = tid + 256 * j;
            *reinterpret_cast<f32x4*>(As + (idx4 >> 3) * AP + (idx4 & 7) * 4) = qa[j];
            if (BT) *reinterpret_cast<f32x4*>(Bs + (idx4 >> 5) * BPT + (idx4 & 31) * 4) = qb[j];
            else *reinterpret_cast<f32x4*>(Bs + (idx4 >> 3) * AP + (idx4 & 7) * 4) = qb[j];
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < W5; k0 += BK) {
        stage();
        __syncthreads();
        if (k0 + BK < W5) fetch(k0 + BK);
#pragma unroll
        for (int c = 0; c < BK / 8; ++c) {
            f32x4 a[2], bb[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int n = wn * 64 + 32 * nt + L.l31;
                if (BT) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[nt][e] = Bs[(8 * c + 4 * L.half + e) * BPT + n];
                } else {
                    a[nt] = *reinterpret_cast<const f32x4*>(Bs + n * AP + 8 * c + 4 * L.half);
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) bb[t] = *reinterpret_cast<const f32x4*>(As + (wm * 64 + 32 * t + L.l31) * AP + 8 * c + 4 * L.half);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[t][nt] = NEO_MFMA(a[nt][e], bb[t][e], acc[t][nt]);   // D rows = n, cols = m
        }
        __syncthreads();
    }
    // ---- epilogue: lane = row m (l31), register 4 g + e = column n = 8 g + 4 half + e of the 32-column block ----
    if (EPI == 0) {
        float ph[2][16], pc[2][16];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { ph[nt][r] = 0.0f; pc[nt][r] = 0.0f; }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long m = m0 + wm * 64 + 32 * t + L.l31;
            const bool valid = m < M;
            const long mc = valid ? m : M - 1;
            const float co = ep.axes[256 * ep.coord_axis + cell_index(mc, ep.G0, ep.G1, ep.G2, ep.coord_axis)];
            const float gsm = valid ? ep.gs[m] : 0.0f;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = n0 + wn * 64 + 32 * nt + 8 * g + 4 * L.half;
                    const f32x4 bs = *reinterpret_cast<const f32x4*>(ep.bias + n);
                    const f32x4 hw = *reinterpret_cast<const f32x4*>(ep.head + n);
                    f32x4 out;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float z = acc[t][nt][4 * g + e] + bs[e] + co * ep.wc[(long)(n + e) * ldb];
                        // the ReLU's kink: an fp32 sum of 513 products can land on the wrong side of zero, and that one
                        // entry then moves a whole g_s head weight into (or out of) the gradient - decide the sign exactly
                        if (fabsf(z) < KINK) z = (float)z_exact(A + mc * W5, B + (long)(n + e) * ldb, ep.bias[n + e], co);
                        const float gz = z > 0.0f ? gsm * hw[e] : 0.0f;
                        out[e] = gz;
                        ph[nt][4 * g + e] += gsm * fmaxf(z, 0.0f);
                        pc[nt][4 * g + e] += gz * co;
                    }
                    if (valid) *reinterpret_cast<f32x4*>(C + m * W5 + n) = out;
                }
        }
        // column sums over this wave's 32 rows of each half (lanes l31), then over the two waves sharing the columns
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) {
                    ph[nt][r] += __shfl_xor(ph[nt][r], o, 64);
                    pc[nt][r] += __shfl_xor(pc[nt][r], o, 64);
                }
        float* red = As;                          // [2 wm][2 kinds][128 columns]; every wave is past the last barrier's reads
        if (L.l31 == 0) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int col = wn * 64 + 32 * nt + 8 * g + 4 * L.half + e;
                        red[(wm * 2 + 0) * BN + col] = ph[nt][4 * g + e];
                        red[(wm * 2 + 1) * BN + col] = pc[nt][4 * g + e];
                    }
        }
        __syncthreads();
        {
            const int kind = tid >> 7, col = tid & 127;
            ep.part[(long)blockIdx.y * (2 * W5) + kind * W5 + n0 + col] = red[kind * BN + col] + red[(2 + kind) * BN + col];
        }
    } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const long m = m0 + wm * 64 + 32 * t + L.l31;
            if (m >= M) continue;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int n = n0 + wn * 64 + 32 * nt + 8 * g + 4 * L.half;
                    float* dst = C + m * W5 + n;
                    f32x4 old = {0.0f, 0.0f, 0.0f, 0.0f}, mk = {1.0f, 1.0f, 1.0f, 1.0f};
                    if (ep.accumulate) old = *reinterpret_cast<const f32x4*>(dst);
                    if (ep.mask) mk = *reinterpret_cast<const f32x4*>(ep.mask + m * W5 + n);
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x = old[e] + acc[t][nt][4 * g + e];
                        v[e] = mk[e] > 0.0f ? x : 0.0f;
                    }
                    *reinterpret_cast<f32x4*>(dst) = v;
                }
        }
    }
}

// t[a][m] = g_a[pillar_a(m)] . L[m] for the three scorers: one wave per row, 8 channels per lane
__global__ __launch_bounds__(256) void k_agg_dot(long M, int G0, int G1, int G2, const float* __restrict__ Lf,
                                                 const float* __restrict__ g_xz, const float* __restrict__ g_yz,
                                                 const float* __restrict__ g_xy, float* __restrict__ t) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const f32x4 l0 = *reinterpret_cast<const f32x4*>(Lf + m * W5 + lane * 8);
    const f32x4 l1 = *reinterpret_cast<const f32x4*>(Lf + m * W5 + lane * 8 + 4);
    const float* gp[3] = {g_xz, g_yz, g_xy};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float* g = gp[a] + pillar_of(m, G0, G1, G2, a) * W5 + lane * 8;
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(g);
        const f32x4 g1 = *reinterpret_cast<const f32x4*>(g + 4);
        float s = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s += g0[e] * l0[e] + g1[e] * l1[e];
        s = wave_sum(s);
        if (lane == 0) t[a * M + m] = s;
    }
}

// per pillar of each scorer (pillars of xz, then yz, then xy): max and denominator of the softmax exactly as k_pillar_aggregate
// forms them, and sum_p w_p t_p (= g . fp)
__global__ void k_agg_stats(int nv, int G0, int G1, int G2, const float* __restrict__ score, const float* __restrict__ t,
                            float* __restrict__ st) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n_xz = (long)nv * G0 * G2, n_yz = (long)nv * G1 * G2, n_xy = (long)nv * G0 * G1;
    if (q >= n_xz + n_yz + n_xy) return;
    const long M = (long)nv * G0 * G1 * G2, NC = (long)G0 * G1 * G2;
    int a;
    long cellab;
    if (q < n_xz) { a = 0; cellab = q; }
    else if (q < n_xz + n_yz) { a = 1; cellab = q - n_xz; }
    else { a = 2; cellab = q - n_xz - n_yz; }
    const int AXIS = a == 0 ? 1 : a == 1 ? 0 : 2;            // axis the softmax runs along
    const int GA = AXIS == 0 ? G0 : AXIS == 1 ? G1 : G2;
    const int A_ = AXIS == 0 ? G1 : G0, B_ = AXIS == 2 ? G1 : G2;
    const int v = (int)(cellab / ((long)A_ * B_));
    const int ai = (int)((cellab / B_) % A_), bi = (int)(cellab % B_);
    auto cell = [&](int p) -> long {
        const int i = AXIS == 0 ? p : ai, j = AXIS == 1 ? p : (AXIS == 0 ? ai : bi), k = AXIS == 2 ? p : bi;
        return (long)v * NC + ((long)i * G1 + j) * G2 + k;
    };
    const float* sc = score + (long)a * M;
    const float* ta = t + (long)a * M;
    float mx = -__builtin_inff();
    for (int p = 0; p < GA; ++p) mx = fmaxf(mx, sc[cell(p)]);
    float den = 0.f;
    for (int p = 0; p < GA; ++p) den += expf(sc[cell(p)] - mx);
    float dot = 0.f;
    for (int p = 0; p < GA; ++p) {
        const long c = cell(p);
        dot += (expf(sc[c] - mx) / den) * ta[c];
    }
    st[3 * q + 0] = mx;
    st[3 * q + 1] = den;
    st[3 * q + 2] = dot;
}

// g_s[a][m] = w_a (t_a - dot_a), g_L[m] = sum_a w_a g_a[pillar_a(m)]: one wave per row
__global__ __launch_bounds__(256) void k_agg_bwd(long M, int nv, int G0, int G1, int G2, const float* __restrict__ score,
                                                 const float* __restrict__ t, const float* __restrict__ st,
                                                 const float* __restrict__ g_xz, const float* __restrict__ g_yz,
                                                 const float* __restrict__ g_xy, float* __restrict__ gs, float* __restrict__ gL) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const long base[3] = {0, (long)nv * G0 * G2, (long)nv * G0 * G2 + (long)nv * G1 * G2};
    const float* gp[3] = {g_xz, g_yz, g_xy};
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long pl = pillar_of(m, G0, G1, G2, a);
        const float* sp = st + 3 * (base[a] + pl);
        const float w = expf(score[a * M + m] - sp[0]) / sp[1];
        if (lane == 0) gs[a * M + m] = w * (t[a * M + m] - sp[2]);
        const float* g = gp[a] + pl * W5 + lane * 8;
        s0 = s0 + *reinterpret_cast<const f32x4*>(g) * w;
        s1 = s1 + *reinterpret_cast<const f32x4*>(g + 4) * w;
    }
    *reinterpret_cast<f32x4*>(gL + m * W5 + lane * 8) = s0;
    *reinterpret_cast<f32x4*>(gL + m * W5 + lane * 8 + 4) = s1;
}

// partial column sums of the scorer epilogue, [tiles][2][512] -> head weight gradient (kind 0) and W0's coordinate column
// (kind 1, pitch 513), in a fixed order: 16 row groups per column, combined in order
__global__ __launch_bounds__(1024) void k_tile_reduce(long tiles, const float* __restrict__ part, float* __restrict__ g_head,
                                                      float* __restrict__ g_w0) {
    __shared__ float red[16][64];
    const int col = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;     // col in [0, 1024)
    float s = 0.0f;
    for (long r = grp; r < tiles; r += 16) s += part[r * (2 * W5) + col];
    red[grp][threadIdx.x & 63] = s;
    __syncthreads();
    if (grp == 0) {
        float tot = 0.0f;
        for (int g = 0; g < 16; ++g) tot += red[g][threadIdx.x & 63];
        if (col < W5) g_head[col] += tot;
        else g_w0[(long)(col - W5) * 513 + 512] += tot;
    }
}

// out[0] += sum x[0..n) in a fixed order (one workgroup), accumulated in fp64.  What it sums are the g_s of one scorer, whose
// exact sum is zero pillar by pillar (softmax shift invariance): in fp32 the partial sums over equal positions of ALL pillars
// (~1e-3) cancelled only in the last additions, so the result was a small multiple of THEIR ulp (2^-35 on the z axis) and every
// tenth call or so it came out as exactly 0.0 by chance; in fp64 it is the sum of the fp32 terms themselves - what their own
// rounding left, ~1e-12 - and still the same bits on every run.
__global__ __launch_bounds__(1024) void k_sum_fixed(long n, const float* __restrict__ x, float* __restrict__ out) {
    __shared__ double red[1024];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) s += (double)x[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] += (float)red[0];
}

// x[m] = [bilinear latent (512) | cam xyz | masked dir] (pitch 518): the first layer's input as k_pillar_dense<0, *> forms it
__global__ __launch_bounds__(256) void k_gather_x(PillarGeom gm, long M, const float* __restrict__ latent, float* __restrict__ x) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const RowGeo r = row_geo(gm, m);
    const long tex0 = (long)r.v * gm.Hf * gm.Wf;
    const f32x4 w = {r.t.w[0], r.t.w[1], r.t.w[2], r.t.w[3]};
    float* dst = x + m * LDX;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x4 tap[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) tap[q] = *reinterpret_cast<const f32x4*>(latent + (tex0 + r.t.off[q]) * W5 + lane * 8 + 4 * h);
        *reinterpret_cast<f4u*>(dst + lane * 8 + 4 * h) = tp::blend4(tap, w);
    }
    if (lane < 6) dst[W5 + lane] = r.ex[lane];
}

// transpose of the bilinear lookup: g_cl[v][texel][c] += w_q g_x[m][c] over the row's four taps (zero-weight taps skipped)
__global__ __launch_bounds__(256) void k_scatter_latent(PillarGeom gm, long M, const float* __restrict__ gx, float* __restrict__ g_cl) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (m >= M) return;
    const RowGeo r = row_geo(gm, m);
    const long tex0 = (long)r.v * gm.Hf * gm.Wf;
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gx + m * W5 + lane * 8);
    const f32x4 g1 = *reinterpret_cast<const f32x4*>(gx + m * W5 + lane * 8 + 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float w = r.t.w[q];
        if (w == 0.0f) continue;
        float* dst = g_cl + (tex0 + r.t.off[q]) * W5 + lane * 8;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            atomicAdd(dst + e, w * g0[e]);
            atomicAdd(dst + 4 + e, w * g1[e]);
        }
    }
}

// g[v][c][p] += g_cl[v][p][c] (p < HW, c < 512): 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void k_cl_add_nchw(long HW, const float* __restrict__ g_cl, float* __restrict__ g) {
    __shared__ float tile[32][33];
    const long p0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32, v = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const long p = p0 + r;
        tile[r][tx] = p < HW ? g_cl[((long)v * HW + p) * W5 + c0 + tx] : 0.0f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const long p = p0 + tx;
        if (p < HW) g[((long)v * W5 + c0 + r) * HW + p] += tile[tx][r];
    }
}

__global__ void k_zero(float* __restrict__ x, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = 0.0f;
}

inline unsigned row_waves(long M) { return (unsigned)((M + 3) / 4); }

void gemm_fwd_scorer(long M, const float* L, const float* w0, const float* b0, int coord_axis, const PillarGeom& gm, const float* gs,
                     const float* head, float* gz, float* part, hipStream_t s) {
    PtEpi ep{};
    ep.bias = b0; ep.wc = w0 + 512; ep.axes = gm.axes; ep.G0 = gm.G0; ep.G1 = gm.G1; ep.G2 = gm.G2; ep.coord_axis = coord_axis;
    ep.gs = gs; ep.head = head; ep.part = part;
    hipLaunchKernelGGL((k_pt_gemm<false, 0>), dim3(W5 / BN, (unsigned)((M + BM - 1) / BM)), dim3(256), 0, s, M, L, w0, 513L, gz, ep);
}

// gx (M x 512) = (accumulate ? gx : 0) + gy W[:, :512], zeroed where mask <= 0 (mask may be null); W (512 out x ldw)
void gemm_input_grad(long M, const float* gy, const float* w, long ldw, const float* mask, int accumulate, float* gx, hipStream_t s) {
    PtEpi ep{};
    ep.mask = mask; ep.accumulate = accumulate;
    hipLaunchKernelGGL((k_pt_gemm<true, 1>), dim3(W5 / BN, (unsigned)((M + BM - 1) / BM)), dim3(256), 0, s, M, gy, w, ldw, gx, ep);
}

struct Scratch {
    float *S0, *S1, *X, *t, *gs, *st, *part, *dw, *gcl;
};
Scratch carve(float* base, int nv, int G0, int G1, int G2, int Hf, int Wf) {
    const long M = (long)nv * G0 * G1 * G2;
    const long tiles = (M + BM - 1) / BM;
    const long pillars = (long)nv * ((long)G0 * G2 + (long)G1 * G2 + (long)G0 * G1);
    Scratch s;
    auto take = [&](long n) { float* p = base; base += (n + 63) / 64 * 64; return p; };
    s.S0 = take(M * W5);
    s.S1 = take(M * W5);
    s.X = take(M * LDX);
    s.t = take(3 * M);
    s.gs = take(3 * M);
    s.st = take(3 * pillars);
    s.part = take(tiles * 2 * W5);
    s.dw = take((long)weight_grad_scratch_floats());
    s.gcl = take((long)nv * Hf * Wf * W5);
    return s;
}

}  // namespace

size_t pillar_train_tape_floats(int nv, int G0, int G1, int G2) {
    const long M = (long)nv * G0 * G1 * G2;
    return (size_t)(M * (3 * W5 + 3));
}

size_t pillar_train_scratch_floats(int nv, int G0, int G1, int G2, int Hf, int Wf, int with_latent) {
    const long M = (long)nv * G0 * G1 * G2;
    const long tiles = (M + BM - 1) / BM;
    const long pillars = (long)nv * ((long)G0 * G2 + (long)G1 * G2 + (long)G0 * G1);
    auto r = [](long n) { return (n + 63) / 64 * 64; };
    long n = r(M * W5) * 2 + r(M * LDX) + r(3 * M) * 2 + r(3 * pillars) + r(tiles * 2 * W5) + r((long)weight_grad_scratch_floats());
    if (with_latent) n += r((long)nv * Hf * Wf * W5);
    return (size_t)n;
}

void launch_pillar_backward(const PillarGeom& gm, const float* const* w, const float* const* b, const float* latent_cl,
                            const float* tape, const float* g_yz, const float* g_xz, const float* g_xy, float* const* gw,
                            float* const* gb, float* g_latent, float* scratch, hipStream_t s) {
    const long M = (long)gm.nv * gm.G0 * gm.G1 * gm.G2;
    const float* h1 = tape;
    const float* h2 = tape + M * W5;
    const float* Lf = tape + 2 * M * W5;
    const float* score = tape + 3 * M * W5;
    const Scratch sc = carve(scratch, gm.nv, gm.G0, gm.G1, gm.G2, gm.Hf, gm.Wf);
    const long tiles = (M + BM - 1) / BM;
    const long pillars = (long)gm.nv * ((long)gm.G0 * gm.G2 + (long)gm.G1 * gm.G2 + (long)gm.G0 * gm.G1);

    // 1. aggregate backward: g_s (3 x M) and g_L (S0)
    hipLaunchKernelGGL(k_agg_dot, dim3(row_waves(M)), dim3(256), 0, s, M, gm.G0, gm.G1, gm.G2, Lf, g_xz, g_yz, g_xy, sc.t);
    hipLaunchKernelGGL(k_agg_stats, dim3((unsigned)((pillars + 255) / 256)), dim3(256), 0, s, gm.nv, gm.G0, gm.G1, gm.G2, score, sc.t, sc.st);
    hipLaunchKernelGGL(k_agg_bwd, dim3(row_waves(M)), dim3(256), 0, s, M, gm.nv, gm.G0, gm.G1, gm.G2, score, sc.t, sc.st, g_xz, g_yz,
                       g_xy, sc.gs, sc.S0);

    // 2. scorers (score a: xz reads the y coordinate, yz x, xy z; layers 3 + 2a (513 -> 512) and 4 + 2a (512 -> 1))
    const int coord[3] = {1, 0, 2};
    for (int a = 0; a < 3; ++a) {
        const float* w0 = w[3 + 2 * a];
        gemm_fwd_scorer(M, Lf, w0, b[3 + 2 * a], coord[a], gm, sc.gs + a * M, w[4 + 2 * a], sc.S1, sc.part, s);
        launch_weight_grad(W5, W5, (int)M, sc.S1, W5, Lf, W5, gw[3 + 2 * a], 513, gb[3 + 2 * a], sc.dw, s);
        hipLaunchKernelGGL(k_tile_reduce, dim3(2 * W5 / 64), dim3(1024), 0, s, tiles, sc.part, gw[4 + 2 * a], gw[3 + 2 * a]);
        hipLaunchKernelGGL(k_sum_fixed, dim3(1), dim3(1024), 0, s, M, sc.gs + a * M, gb[4 + 2 * a]);
        gemm_input_grad(M, sc.S1, w0, 513, nullptr, 1, sc.S0, s);
    }

    // 3. depth_fc: L = W2 h2 + b2, h2 = relu(W1 h1 + b1), h1 = relu(W0 x + b0)
    launch_weight_grad(W5, W5, (int)M, sc.S0, W5, h2, W5, gw[2], W5, gb[2], sc.dw, s);
    gemm_input_grad(M, sc.S0, w[2], W5, h2, 0, sc.S1, s);                     // g_h2
    launch_weight_grad(W5, W5, (int)M, sc.S1, W5, h1, W5, gw[1], W5, gb[1], sc.dw, s);
    gemm_input_grad(M, sc.S1, w[1], W5, h1, 0, sc.S0, s);                     // g_h1
    hipLaunchKernelGGL(k_gather_x, dim3(row_waves(M)), dim3(256), 0, s, gm, M, latent_cl, sc.X);
    launch_weight_grad(W5, LDX, (int)M, sc.S0, W5, sc.X, LDX, gw[0], LDX, gb[0], sc.dw, s);

    // 4. latent: g_x_lat = g_h1 W0[:, :512], scattered back through the bilinear taps
    if (g_latent) {
        const long HW = (long)gm.Hf * gm.Wf, n_cl = (long)gm.nv * HW * W5;
        gemm_input_grad(M, sc.S0, w[0], LDX, nullptr, 0, sc.S1, s);
        hipLaunchKernelGGL(k_zero, dim3((unsigned)((n_cl + 255) / 256)), dim3(256), 0, s, sc.gcl, n_cl);
        hipLaunchKernelGGL(k_scatter_latent, dim3(row_waves(M)), dim3(256), 0, s, gm, M, sc.S1, sc.gcl);
        hipLaunchKernelGGL(k_cl_add_nchw, dim3((unsigned)((HW + 31) / 32), W5 / 32, (unsigned)gm.nv), dim3(256), 0, s, HW, sc.gcl, g_latent);
    }
}

}  // namespace neo
