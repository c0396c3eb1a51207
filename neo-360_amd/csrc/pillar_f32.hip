// Pillar stage of the NeO-360 scene encoder in the reference's own arithmetic: the exact-fp32 twin of pillar.hip's
// k_pillar_dense (v_mfma_f32_32x32x2_f32 through mfma_tile.h instead of fp16 MFMA on hi/lo-split operands).  What it is for:
// precision "f32" end to end, and the retry of a call whose operands left the fp16 range (GridEncoder.on_range) - there is no
// range guard here, no flag is read or written.
//
// Same work decomposition as the split kernel (pillar.hip:26-34): one kernel per layer with the activations resident in HBM,
// workgroup = 64 rows x all 512 outputs, 8 waves (wave w: N-tiles 2w, 2w+1 x both 32-row M-tiles = 64 accumulator registers);
// the input is streamed 64 features at a time into a double-buffered swizzled LDS tile [64][64] fp32, the first layer's bilinear
// gather included (the M x 518 input is never written to memory), each stage produced in two 32-row halves so that only four
// taps (16 VGPRs) are in flight per lane; weights come from L2 in mfma_tile.h's fragment order (launch_pillar_pack_f32), one
// 16-B load per lane and k-chunk of 8, prefetched one chunk ahead.  The softmax aggregation is pillar.hip's
// (launch_pillar_aggregate: fp32 already).  Fixed accumulation order, no atomics: bitwise repeatable.
#include "pillar_f32.h"
#include "tp_common.h"

namespace neo {

namespace {

constexpr int PT = 64;                 // rows per tile
constexpr int PW = 512;                // layer width
constexpr int XLD = 64;                // streamed-input tile [64 rows][64 features], 16-B pieces XOR-swizzled with (row & 15)
constexpr int KC_MAIN = 64;            // k-chunks (8 features) of the 512 main features
constexpr int KC_ALL = 65;             // + one chunk of extras (camera xyz + direction, or the axis coordinate)

// IN: 0 = gathered latent + [cam xyz | dir] extras (first layer), 1 = rows of X (512), 2 = rows of X + axis coordinate
// EPI: 0 = bias + ReLU -> Y, 1 = bias -> Y, 2 = bias + ReLU -> dot with the 512 -> 1 head -> score
template <int IN, int EPI>
__global__ __launch_bounds__(512, 2) void k_pillar_dense_f32(PillarGeom gm, const float* __restrict__ latent, const float* __restrict__ X,
                                                            const f32x4* __restrict__ wp, const float* __restrict__ bias,
                                                            const float* __restrict__ head_w, float head_b, int coord_axis,
                                                            long M, float* __restrict__ Y, float* __restrict__ score) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    auto xbuf = [&](int b) { return smem + b * (PT * XLD); };    // 2 x 16 KB
    int* loc_off = reinterpret_cast<int*>(smem + 8192);          // [64][4]
    float* loc_w = smem + 8192 + 256;                            // [64][4]
    float* extra = smem + 8192 + 512;                            // [64][8]: extras of the 65th k-chunk
    float* sred = smem + 8192 + 1024;                            // [8][64] scorer partial sums
    LaneCtx L;
    L.init();
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * PT;
    constexpr int KC = IN == 1 ? KC_MAIN : KC_ALL;

    // ---- per-row set-up (threads 0..63): k_pillar_dense's, operation for operation ----
    if (IN != 1 && tid < PT) {
        long m = row0 + tid;
        if (m >= M) m = M - 1;
        const long NC = (long)gm.G0 * gm.G1 * gm.G2;
        const int v = (int)(m / NC);
        const long cell = m - (long)v * NC;
        const int i = (int)(cell / ((long)gm.G1 * gm.G2)), j = (int)((cell / gm.G2) % gm.G1), k = (int)(cell % gm.G2);
        const float w3[3] = {gm.axes[i], gm.axes[256 + j], gm.axes[512 + k]};
        if (IN == 0) {
            const float* rot = gm.rot[v];
            const float* trn = gm.trans[v];
            const float cxp = (rot[0] * w3[0] + rot[1] * w3[1] + rot[2] * w3[2]) + trn[0];
            const float cyp = (rot[3] * w3[0] + rot[4] * w3[1] + rot[5] * w3[2]) + trn[1];
            const float czp = (rot[6] * w3[0] + rot[7] * w3[1] + rot[8] * w3[2]) + trn[2];
            const float mask = czp < 1e-3f ? 1.0f : 0.0f;                       // :509
            float d[3], n2 = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) { d[a] = w3[a] - gm.cpos[v][a]; const float e = d[a] + 1e-9f; n2 += e * e; }
            const float nrm = sqrtf(n2);
            const float den = czp + 1e-9f;
            const float u = (-cxp / den) * gm.focal + gm.cx;
            const float w_ = (-cyp / den) * (-gm.focal) + gm.cy;
            const tp::TapSet t = tp::bilinear_taps(u * gm.sx - 1.0f, w_ * gm.sy - 1.0f, gm.Wf, gm.Hf);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                loc_off[tid * 4 + q] = (int)((uint32_t)(v * gm.Hf * gm.Wf + t.off[q]) * 2048u);
                loc_w[tid * 4 + q] = t.w[q];
            }
            extra[tid * 8 + 0] = cxp; extra[tid * 8 + 1] = cyp; extra[tid * 8 + 2] = czp;
#pragma unroll
            for (int a = 0; a < 3; ++a) extra[tid * 8 + 3 + a] = (d[a] / nrm) * mask;
            extra[tid * 8 + 6] = 0.f; extra[tid * 8 + 7] = 0.f;
        } else {
            extra[tid * 8] = w3[coord_axis];
#pragma unroll
            for (int a = 1; a < 8; ++a) extra[tid * 8 + a] = 0.f;
        }
    }
    __syncthreads();

    f32x16 acc[2][2];
    const int nts[2] = {2 * L.wv, 2 * L.wv + 1};
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        bias_tile(acc[nt][0], bias, nts[nt], L);
        acc[nt][1] = acc[nt][0];
    }
    // producer: 16 lanes per row (4 features each), 32 rows per half, 2 halves per 64-feature stage
    const int col4 = tid & 15, rg = tid >> 4;
    f32x4 tap[4];
    auto issue = [&](int s, int hf) __attribute__((always_inline)) {
        const int row = rg + 32 * hf;
        if (IN == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) tap[q] = tp::load_tap(latent, (uint32_t)loc_off[row * 4 + q] + 16u * col4 + 256u * s);
        } else {
            long m = row0 + row;
            if (m >= M) m = M - 1;
            tap[0] = *reinterpret_cast<const f32x4*>(X + m * PW + s * 64 + col4 * 4);
        }
    };
    auto finish = [&](float* buf, int hf) __attribute__((always_inline)) {
        const int row = rg + 32 * hf;
        f32x4 val;
        if (IN == 0) val = tp::blend4(tap, *reinterpret_cast<const f32x4*>(loc_w + row * 4));
        else val = tap[0];
        *reinterpret_cast<f32x4*>(buf + row * XLD + ((col4 ^ (row & 15)) << 2)) = val;
    };
    // the extras k-chunk: features 0..7 of a row = 16-B pieces 0 and 1
    auto finish_extra = [&](float* buf) __attribute__((always_inline)) {
        if (tid < 2 * PT) {
            const int row = tid >> 1, piece = tid & 1;
            *reinterpret_cast<f32x4*>(buf + row * XLD + ((piece ^ (row & 15)) << 2)) = *reinterpret_cast<const f32x4*>(extra + row * 8 + 4 * piece);
        }
    };
    // acc += W chunks [kc0, kc0 + n) x tile chunks [tc0, tc0 + n); `a` holds the fragments of chunk kc0 on entry and those of
    // chunk kc0 + n (clamped to the last one) on exit
    f32x4 a[2];
    auto load_w = [&](int kc) __attribute__((always_inline)) {
        const int c = kc < KC ? kc : KC - 1;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) a[nt] = load_a(wp, KC, nts[nt], c, L.lane);
    };
    auto mma = [&](const float* tile, int kc0, int tc0, int n) __attribute__((always_inline)) {
#pragma unroll
        for (int c = 0; c < n; ++c) {
            f32x4 an[2], b[2];
            const int nx = kc0 + c + 1 < KC ? kc0 + c + 1 : KC - 1;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) an[nt] = load_a(wp, KC, nts[nt], nx, L.lane);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) b[mt] = load_b<XLD, 15>(tile, mt, tc0 + c, L);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) acc[nt][mt] = NEO_MFMA(a[nt][e], b[mt][e], acc[nt][mt]);
            a[0] = an[0];
            a[1] = an[1];
        }
    };
    load_w(0);
    issue(0, 0);
    finish(xbuf(0), 0);
    issue(0, 1);
    finish(xbuf(0), 1);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 8; ++s) {
        const float* cur = xbuf(s & 1);
        float* nxt = xbuf((s + 1) & 1);
#pragma unroll 1
        for (int hf = 0; hf < 2; ++hf) {
            if (s < 7) issue(s + 1, hf);
            mma(cur, 8 * s + 4 * hf, 4 * hf, 4);
            if (s < 7) finish(nxt, hf);
        }
        if (IN != 1 && s == 7) finish_extra(xbuf(0));         // stage 8 lands in buffer 0 (stage 6's, consumed before the last barrier)
        __syncthreads();
    }
    if (IN != 1) mma(xbuf(0), KC_MAIN, 0, 1);

    // ---- epilogue ----
    if (EPI != 2) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const long m = row0 + mt * 32 + L.l31;
                if (m >= M) continue;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 val;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x = acc[nt][mt][4 * g + e];
                        val[e] = EPI == 0 ? fmaxf(x, 0.0f) : x;
                    }
                    *reinterpret_cast<f32x4*>(Y + m * PW + nts[nt] * 32 + 8 * g + 4 * L.half) = val;
                }
            }
    } else {
        // score = head_w . relu(hidden) + head_b: this wave's 64 outputs of each row, then across the 8 waves in a fixed order
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            float part = 0.f;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 hw = *reinterpret_cast<const f32x4*>(head_w + nts[nt] * 32 + 8 * g + 4 * L.half);
#pragma unroll
                    for (int e = 0; e < 4; ++e) part = __builtin_fmaf(fmaxf(acc[nt][mt][4 * g + e], 0.0f), hw[e], part);
                }
            part += __shfl_xor(part, 32, 64);
            if (L.half == 0) sred[L.wv * 64 + mt * 32 + L.l31] = part;
        }
        __syncthreads();
        if (tid < PT && row0 + tid < M) {
            float s = head_b;
#pragma unroll
            for (int w = 0; w < 8; ++w) s += sred[w * 64 + tid];
            score[row0 + tid] = s;
        }
    }
}

// f32x4 units per stage = 16 N-tiles x KC x 64 lanes; stages as in pillar.hip (0 = depth_fc.0, 1 = depth_fc.2, 2 = depth_encoder,
// 3..5 = scorer hidden layers xz, yz, xy)
size_t stage_off_f4(int st) {
    const int kc[6] = {KC_ALL, KC_MAIN, KC_MAIN, KC_ALL, KC_ALL, KC_ALL};
    size_t o = 0;
    for (int i = 0; i < st; ++i) o += (size_t)16 * kc[i] * 64;
    return o;
}

}  // namespace

size_t pillar_wpack_f32_bytes() { return stage_off_f4(6) * 16; }

void launch_pillar_pack_f32(const float* const* w, float* wpack, hipStream_t s) {
    // w: depth_fc.0 (512x518), depth_fc.2, depth_encoder, agg_xz.0 (512x513), agg_yz.0, agg_xy.0; k beyond the row is zero
    const PackSegs none = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    PackSegs s518 = none; s518.len[0] = 518;
    PackSegs s512 = none; s512.len[0] = 512;
    PackSegs s513 = none; s513.len[0] = 513;
    pack_block(w[0], 518, 512, KC_ALL, 0, s518, wpack + stage_off_f4(0) * 4, s);
    pack_block(w[1], 512, 512, KC_MAIN, 0, s512, wpack + stage_off_f4(1) * 4, s);
    pack_block(w[2], 512, 512, KC_MAIN, 0, s512, wpack + stage_off_f4(2) * 4, s);
    for (int a = 0; a < 3; ++a) pack_block(w[3 + a], 513, 512, KC_ALL, 0, s513, wpack + stage_off_f4(3 + a) * 4, s);
}

int launch_pillar_f32(const PillarGeom& gm, const float* latent_cl, const float* wpack, const float* bias /* 6 x 512 */,
                      const float* head_w /* 3 x 512 */, const float* head_b_host /* 3 */, float* h1, float* h2, float* Lf,
                      float* score /* 3 x M */, float* fp_yz, float* fp_xz, float* fp_xy, hipStream_t s) {
    if (gm.G0 > 256 || gm.G1 > 256 || gm.G2 > 256) return -1;
    const long M = (long)gm.nv * gm.G0 * gm.G1 * gm.G2;
    const unsigned tiles = (unsigned)((M + PT - 1) / PT);
    const size_t lds = (8192 + 1024 + 512) * sizeof(float);
    const f32x4* wp = reinterpret_cast<const f32x4*>(wpack);
    hipLaunchKernelGGL((k_pillar_dense_f32<0, 0>), dim3(tiles), dim3(512), lds, s, gm, latent_cl, nullptr, wp + stage_off_f4(0), bias,
                       nullptr, 0.f, 0, M, h1, nullptr);
    hipLaunchKernelGGL((k_pillar_dense_f32<1, 0>), dim3(tiles), dim3(512), lds, s, gm, nullptr, h1, wp + stage_off_f4(1), bias + 512,
                       nullptr, 0.f, 0, M, h2, nullptr);
    hipLaunchKernelGGL((k_pillar_dense_f32<1, 1>), dim3(tiles), dim3(512), lds, s, gm, nullptr, h2, wp + stage_off_f4(2), bias + 1024,
                       nullptr, 0.f, 0, M, Lf, nullptr);
    // scorers: xz uses the y coordinate, yz the x coordinate, xy the z coordinate (:556-574)
    const int coord[3] = {1, 0, 2};
    for (int a = 0; a < 3; ++a)
        hipLaunchKernelGGL((k_pillar_dense_f32<2, 2>), dim3(tiles), dim3(512), lds, s, gm, nullptr, Lf, wp + stage_off_f4(3 + a),
                           bias + 1536 + 512 * a, head_w + 512 * a, head_b_host[a], coord[a], M, nullptr, score + (long)a * M);
    launch_pillar_aggregate(gm, Lf, score, fp_yz, fp_xz, fp_xy, s);
    return 0;
}

}  // namespace neo
