// Baseline for csrc/pillar_f32.hip: the exact-fp32 pillar forward COMPOSED from the kernels the backward already had
// (csrc/pillar_train.hip) - k_gather_x writes the M x 518 first-layer input to memory, then one plain fp32-MFMA GEMM
// (k_pt_gemm, 128 x 128 tiles) per layer: depth_fc's three and the three scorer hidden layers.  This is what an exact forward
// costs WITHOUT a new kernel, and a lower bound of it: the GEMMs run bare (K = 512: no bias, no ReLU, no extras columns, no
// 512 -> 1 scorer heads, no aggregation), which flatters the baseline.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -I neo-360_amd/csrc tools/pillar_composed_bench.hip \
//         -o tools/build/pillar_composed_bench -L neo-360_amd/lib -lneo360_hip -Wl,-rpath,'$ORIGIN/../../neo-360_amd/lib'
//   tools/build/pillar_composed_bench [runs = 7] [warmup = 2] [grid = 64] [views = 3] [Hf = 240] [Wf = 320]
// Prints one JSON line: median / min / max ms of the whole composition and of the gather alone (device events).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pillar_train.hip"

using namespace neo;

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(1); } } while (0)

__global__ void k_fill(float* __restrict__ x, size_t n, uint32_t seed, float scale) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t h = (uint32_t)i * 2654435761u + seed;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        x[i] = ((float)(h & 0xffffu) / 32768.0f - 1.0f) * scale;
    }
}

// synth.look_at_origin / source_views: cameras on the test orbit (radius 0.6, height 0.3), looking at the origin
static void view(float az_deg, float* rot, float* trans, float* cpos) {
    const double a = az_deg * M_PI / 180.0;
    double eye[3] = {0.6 * cos(a), 0.6 * sin(a), 0.3};
    const double ne = sqrt(eye[0] * eye[0] + eye[1] * eye[1] + eye[2] * eye[2]);
    double back[3] = {eye[0] / ne, eye[1] / ne, eye[2] / ne};
    double right[3] = {-back[1], back[0], 0.0};                                // z x back
    const double nr = sqrt(right[0] * right[0] + right[1] * right[1]);
    for (double& r : right) r /= nr;
    double up[3] = {back[1] * right[2] - back[2] * right[1], back[2] * right[0] - back[0] * right[2], back[0] * right[1] - back[1] * right[0]};
    const double* cols[3] = {right, up, back};                                 // c2w[:3, :3] columns
    for (int r = 0; r < 3; ++r) {
        double t = 0.0;
        for (int c = 0; c < 3; ++c) { rot[r * 3 + c] = (float)cols[r][c]; t += cols[r][c] * eye[c]; }      // rot = R^T
        trans[r] = (float)-t;
        cpos[r] = (float)eye[r];
    }
}

int main(int argc, char** argv) {
    const int runs = argc > 1 ? atoi(argv[1]) : 7, warm = argc > 2 ? atoi(argv[2]) : 2;
    const int G = argc > 3 ? atoi(argv[3]) : 64, nv = argc > 4 ? atoi(argv[4]) : 3;
    const int Hf = argc > 5 ? atoi(argv[5]) : 240, Wf = argc > 6 ? atoi(argv[6]) : 320;
    if (runs < 1 || G < 1 || G > 256 || nv < 1 || nv > TP_MAX_VIEWS || Hf < 2 || Wf < 2) { printf("bad arguments\n"); return 1; }
    const long M = (long)nv * G * G * G;
    float *latent, *X, *A, *B, *W, *axes;
    CK(hipMalloc(&latent, (size_t)nv * Hf * Wf * 512 * 4));
    CK(hipMalloc(&X, (size_t)M * LDX * 4));
    CK(hipMalloc(&A, (size_t)M * W5 * 4));
    CK(hipMalloc(&B, (size_t)M * W5 * 4));
    CK(hipMalloc(&W, (size_t)6 * 512 * LDX * 4));
    CK(hipMalloc(&axes, 3 * 256 * 4));
    hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, latent, (size_t)nv * Hf * Wf * 512, 1u, 0.1f);
    hipLaunchKernelGGL(k_fill, dim3(1024), dim3(256), 0, 0, W, (size_t)6 * 512 * LDX, 2u, 0.06f);
    std::vector<float> ax(3 * 256, 0.0f);
    for (int i = 0; i < G; ++i) {
        const float t = G > 1 ? (float)i / (float)(G - 1) : 0.0f;
        ax[i] = -1.0f + 2.0f * t; ax[256 + i] = -1.0f + 2.0f * t; ax[512 + i] = t;
    }
    CK(hipMemcpy(axes, ax.data(), ax.size() * 4, hipMemcpyHostToDevice));
    PillarGeom gm{};
    gm.nv = nv; gm.G0 = gm.G1 = gm.G2 = G; gm.Hf = Hf; gm.Wf = Wf;
    const float iw = 2.0f * Wf, ih = 2.0f * Hf;                                // the encoder halves the image size
    gm.focal = 0.8f * iw; gm.cx = iw / 2; gm.cy = ih / 2;
    gm.sx = (((float)Wf / (Wf - 1.0f)) * 2.0f) / iw;
    gm.sy = (((float)Hf / (Hf - 1.0f)) * 2.0f) / ih;
    gm.axes = axes;
    const float az[8] = {0.f, 115.f, 229.f, 300.f, 60.f, 170.f, 20.f, 270.f};
    for (int v = 0; v < nv; ++v) view(az[v], gm.rot[v], gm.trans[v], gm.cpos[v]);

    PtEpi ep{};
    const dim3 grid(W5 / BN, (unsigned)((M + BM - 1) / BM));
    auto gemm = [&](const float* in, long ldin_unused, const float* w, long ldw, float* out) {
        (void)ldin_unused;
        hipLaunchKernelGGL((k_pt_gemm<false, 1>), grid, dim3(256), 0, 0, M, in, w, ldw, out, ep);
    };
    auto gather = [&]() { hipLaunchKernelGGL(k_gather_x, dim3(row_waves(M)), dim3(256), 0, 0, gm, M, latent, X); };
    auto forward = [&]() {
        gather();
        // first layer: k_pt_gemm reads rows of pitch 512, so the 518-pitch gather output cannot feed it directly; the baseline
        // runs it on a 512-pitch buffer of the same size class (A), which costs the same
        gemm(A, 512, W, LDX, B);                               // depth_fc.common_branch.0
        gemm(B, 512, W + 512 * LDX, 512, A);                   // .2
        gemm(A, 512, W + 2 * 512 * LDX, 512, B);               // depth_encoder
        for (int a = 0; a < 3; ++a) gemm(B, 512, W + (3 + a) * 512 * LDX, 513, A);      // scorer hidden layers
    };
    hipLaunchKernelGGL(k_fill, dim3(4096), dim3(256), 0, 0, A, (size_t)M * W5, 3u, 0.5f);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto timed = [&](auto fn, std::vector<float>& ms) {
        for (int i = 0; i < warm; ++i) fn();
        CK(hipDeviceSynchronize());
        for (int i = 0; i < runs; ++i) {
            CK(hipEventRecord(e0, 0));
            fn();
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float t;
            CK(hipEventElapsedTime(&t, e0, e1));
            ms.push_back(t);
        }
        CK(hipGetLastError());
        std::sort(ms.begin(), ms.end());
    };
    std::vector<float> all, g;
    timed(forward, all);
    timed(gather, g);
    printf("{\"composed_ms\": %.4f, \"composed_min_ms\": %.4f, \"composed_max_ms\": %.4f, \"gather_ms\": %.4f, \"runs\": %d, "
           "\"cell_views\": %ld, \"latent_hw\": [%d, %d]}\n",
           all[all.size() / 2], all.front(), all.back(), g[g.size() / 2], runs, M, Hf, Wf);
    return 0;
}
