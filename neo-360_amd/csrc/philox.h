// The library's counter-based generator (neo_rand_uniform): Philox4x32-10 (Salmon et al., SC'11), one 128-bit block per
// (row, col, stream).  Device code with internal linkage, shared by training.hip (the samplers' uniforms) and vanilla_train_march.hip
// (the probe points of the running occupancy grid).
#pragma once
#include "common.h"

namespace neo {

namespace {

__device__ __forceinline__ uint32_t philox_u32(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * x0, p1 = (uint64_t)0xCD9E8D57u * x2;
        const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1;
        const uint32_t y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1, y3 = (uint32_t)p0;
        x0 = y0; x1 = y1; x2 = y2; x3 = y3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return x0;
}
// uniform in [0, 1) with 24 random bits, as torch.rand produces fp32 (value = k 2^-24)
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint32_t row, uint32_t col, uint32_t stream) {
    return (float)(philox_u32(seed, row, col, stream) >> 8) * 5.9604644775390625e-08f;
}

}  // namespace

}  // namespace neo
