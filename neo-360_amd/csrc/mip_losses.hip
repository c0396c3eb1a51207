// The two regularisers of Mip-NeRF 360's training step (mipnerf360/helper.py:108-148, called from model.py:725-741):
// lossfun_outer - the interlevel loss of a proposal histogram (t_env, w_env) against the final level's (t, w) - with its backward,
// and lossfun_distortion with its unit gradient.  The reference's forms are quadratic ((R, Ne+1, N+1) comparison tensors,
// (R, N, N) midpoint distances); both have linear-time forms on sorted edges.  One 64-lane wave per ray, four rays per block, like
// k_distloss (training.hip).  Inputs and outputs are fp32; every prefix sum, every difference taken from one and every quotient is
// fp64, and each output entry is rounded once.  No atomics: the summation order is fixed, results repeat bit for bit.
#include "common.h"
#include "kernels.h"

namespace neo {

namespace {

constexpr int RPB = 4;                  // rays (waves) per 256-thread block
constexpr int MAXE = 1024;              // intervals per histogram the per-wave LDS rows hold
constexpr int ROUNDS = MAXE / 64;
constexpr double EPS = 1.1920929e-07;   // helper.py:18

// entries of the non-decreasing row e[0, n) that are <= v / < v
__device__ __forceinline__ int count_le(const float* e, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int count_lt(const float* e, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// inclusive scan over the 64 lanes
__device__ __forceinline__ double wave_scan_add(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// ---- lossfun_outer (helper.py:108-137) ---------------------------------------------------------------------------------------------
// cy = exclusive prefix sum of w_env (Ne + 1 entries).  For a fine edge v, ub = #{envelope edges <= v}; the reference's searchsorted
// pair is lo = max(ub - 1, 0), hi = min(ub, Ne) (its defaults when no edge qualifies included).  Per fine interval i:
//   w_outer_i = cy[hi_{i+1}] - cy[lo_i],  d_i = max(w_i - w_outer_i, 0),  loss_i = d_i^2 / (w_i + eps).
// Backward (BWD), upstream g:  g_w_i = g_i (2 d_i (w_i + eps) - d_i^2) / (w_i + eps)^2, and with a_i = -2 g_i d_i / (w_i + eps) and A its
// exclusive prefix sum, g_w_env_k = sum of a_i over the fine intervals whose [lo_i, hi_{i+1}) covers bin k.  lo_i and hi_{i+1} do not
// decrease with i, so those intervals are the range [q, p) with
//   p = #{i : lo_i <= k} = #{i < N : t_i < t_env_{k+1}},   q = #{i : hi_{i+1} <= k} = #{i < N : t_{i+1} < t_env_k}
// (ub_i <= k + 1 exactly when envelope edge k + 1 lies beyond t_i): two binary searches in the fine edges and a gather, no scatter.
// lo / hi / d are recomputed here rather than saved by the forward.  The LDS rows hold the envelope (edges, cy) while the fine
// intervals are walked and the fine histogram (edges, A) afterwards; a_i waits in registers in between (ROUNDS values per lane).
// Surplus waves of the last block redo the last ray and write nothing: the barriers stay uniform (as k_mip_resample).
template <bool BWD>
__global__ __launch_bounds__(256) void k_mip_outer(const float* __restrict__ t, const float* __restrict__ w,
                                                    const float* __restrict__ t_env, const float* __restrict__ w_env,
                                                    const float* __restrict__ g, int R, int N, int Ne,
                                                    float* __restrict__ out /* loss | g_w */, float* __restrict__ g_w_env) {
    __shared__ float s_e[RPB][MAXE + 1];
    __shared__ double s_c[RPB][MAXE + 1];
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const int ray_raw = blockIdx.x * RPB + wv;
    const bool live = ray_raw < R;
    const int ray = live ? ray_raw : R - 1;
    float* E = s_e[wv];
    double* C = s_c[wv];
    const float* tr = t + (long)ray * (N + 1);
    const float* wr = w + (long)ray * N;
    const float* ter = t_env + (long)ray * (Ne + 1);
    const float* wer = w_env + (long)ray * Ne;
    for (int k = lane; k <= Ne; k += 64) E[k] = ter[k];
    double carry = 0.0;
    for (int base = 0; base < Ne; base += 64) {
        const int k = base + lane;
        const double incl = wave_scan_add(k < Ne ? (double)wer[k] : 0.0, lane);
        if (k < Ne) C[k + 1] = carry + incl;
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) C[0] = 0.0;
    __syncthreads();
    // one search per fine edge: lane l of a round searches the RIGHT edge of interval base + l and takes the left one from lane l - 1
    int ub_prev = count_le(E, Ne + 1, tr[0]);
    double a_reg[ROUNDS];
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        a_reg[rd] = 0.0;
        if (rd * 64 < N) {
            const int i = rd * 64 + lane;
            const bool valid = i < N;
            const int ub_r = count_le(E, Ne + 1, tr[valid ? i + 1 : N]);
            int ub_l = __shfl_up(ub_r, 1, 64);
            if (lane == 0) ub_l = ub_prev;
            ub_prev = __shfl(ub_r, 63, 64);
            const int lo = ub_l > 0 ? ub_l - 1 : 0, hi = ub_r < Ne ? ub_r : Ne;
            const double wi = valid ? (double)wr[i] : 0.0;
            const double w_outer = C[hi] - C[lo];
            const double d = fmax(wi - w_outer, 0.0), den = wi + EPS;
            if (!BWD) {
                if (valid && live) out[(long)ray * N + i] = (float)(d * d / den);
            } else {
                const double gi = valid ? (double)g[(long)ray * N + i] : 0.0;
                if (valid && live && out) out[(long)ray * N + i] = (float)(gi * (2.0 * d * den - d * d) / (den * den));
                a_reg[rd] = -2.0 * gi * d / den;
            }
        }
    }
    if (!BWD || g_w_env == nullptr) return;          // uniform over the block
    __syncthreads();                                 // every wave is done with the envelope rows
    for (int j = lane; j <= N; j += 64) E[j] = tr[j];
    carry = 0.0;
#pragma unroll
    for (int rd = 0; rd < ROUNDS; ++rd) {
        if (rd * 64 < N) {
            const int i = rd * 64 + lane;
            const double incl = wave_scan_add(a_reg[rd], lane);
            if (i < N) C[i + 1] = carry + incl;
            carry += __shfl(incl, 63, 64);
        }
    }
    if (lane == 0) C[0] = 0.0;
    __syncthreads();
    for (int k = lane; k < Ne; k += 64) {
        const int p = count_lt(E, N, ter[k + 1]);
        const int q = count_lt(E + 1, N, ter[k]);
        if (live) g_w_env[(long)ray * Ne + k] = p > q ? (float)(C[p] - C[q]) : 0.0f;
    }
}

// ---- lossfun_distortion (helper.py:140-148) ----------------------------------------------------------------------------------------
// u_i = (t_i + t_{i+1}) / 2, D_i = t_{i+1} - t_i, W / WU inclusive prefix sums of w / w u.  On non-decreasing edges
//   loss_ray = sum w_i^2 D_i / 3 + 2 sum (w_i u_i Wpre_i - w_i WUpre_i),
//   d loss_ray / d w_i = 2 w_i D_i / 3 + 2 (u_i (Wpre_i - Wsuf_i) + (WUsuf_i - WUpre_i)).
// k_distloss (training.hip) with a width and a midpoint per sample taken from the edges, and with the products w u and the two totals
// in fp64 as well (k_distloss forms them in fp32, and its results are pinned bit for bit: the two kernels stay apart).
__global__ __launch_bounds__(256) void k_mip_distortion(const float* __restrict__ t, const float* __restrict__ w, int R, int N,
                                                         float* __restrict__ loss_rays, float* __restrict__ grad_w) {
    const int wv = threadIdx.x >> 6, lane = lane_id();
    const int ray = blockIdx.x * RPB + wv;
    if (ray >= R) return;
    const float* tr = t + (long)ray * (N + 1);
    const float* wr = w + (long)ray * N;
    double W_total = 0.0, WU_total = 0.0;
    for (int i = lane; i < N; i += 64) {
        const double wi = (double)wr[i];
        W_total += wi;
        WU_total += wi * (((double)tr[i] + (double)tr[i + 1]) * 0.5);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        W_total += __shfl_xor(W_total, o, 64);
        WU_total += __shfl_xor(WU_total, o, 64);
    }
    double cw = 0.0, cwu = 0.0, loss = 0.0;
    for (int base = 0; base < N; base += 64) {
        const int i = base + lane;
        const bool valid = i < N;
        const double wi = valid ? (double)wr[i] : 0.0;
        const double t0 = valid ? (double)tr[i] : 0.0, t1 = valid ? (double)tr[i + 1] : 0.0;
        const double ui = (t0 + t1) * 0.5, di = t1 - t0, wu = wi * ui;
        const double iw = wave_scan_add(wi, lane), iwu = wave_scan_add(wu, lane);
        const double Wpre = cw + iw - wi, WUpre = cwu + iwu - wu;      // strictly before i
        cw += __shfl(iw, 63, 64);
        cwu += __shfl(iwu, 63, 64);
        if (valid) {
            const double Wsuf = W_total - Wpre - wi, WUsuf = WU_total - WUpre - wu;
            loss += wi * wi * di / 3.0 + 2.0 * (wu * Wpre - wi * WUpre);
            if (grad_w) grad_w[(long)ray * N + i] = (float)(2.0 * wi * di / 3.0 + 2.0 * (ui * (Wpre - Wsuf) + (WUsuf - WUpre)));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) loss += __shfl_xor(loss, o, 64);
    if (lane == 0) loss_rays[ray] = (float)loss;
}

}  // namespace

int launch_mip_lossfun_outer(const float* t, const float* w, const float* t_env, const float* w_env, int R, int N, int Ne, float* loss,
                             hipStream_t s) {
    if (N < 1 || N > MAXE || Ne < 1 || Ne > MAXE) return -1;
    if (R <= 0) return 0;
    hipLaunchKernelGGL(k_mip_outer<false>, dim3((R + RPB - 1) / RPB), dim3(256), 0, s, t, w, t_env, w_env, nullptr, R, N, Ne, loss, nullptr);
    return 0;
}

int launch_mip_lossfun_outer_bwd(const float* t, const float* w, const float* t_env, const float* w_env, const float* g_loss, int R, int N,
                                 int Ne, float* g_w, float* g_w_env, hipStream_t s) {
    if (N < 1 || N > MAXE || Ne < 1 || Ne > MAXE) return -1;
    if (R <= 0) return 0;
    hipLaunchKernelGGL(k_mip_outer<true>, dim3((R + RPB - 1) / RPB), dim3(256), 0, s, t, w, t_env, w_env, g_loss, R, N, Ne, g_w, g_w_env);
    return 0;
}

int launch_mip_lossfun_distortion(const float* t, const float* w, int R, int N, float* loss_rays, float* grad_w, hipStream_t s) {
    if (N < 1 || N > MAXE) return -1;
    if (R <= 0) return 0;
    hipLaunchKernelGGL(k_mip_distortion, dim3((R + RPB - 1) / RPB), dim3(256), 0, s, t, w, R, N, loss_rays, grad_w);
    return 0;
}

}  // namespace neo
