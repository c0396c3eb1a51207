// Launchers of pillar_f32.hip - the scene encoder's pillar stage on exact fp32 MFMA - and what it shares with the split path
// (pillar.hip's aggregation, a range check for per-call inputs).  Kept apart from kernels.h, like pillar_train.h, so that the
// evaluators' sources (the hashes bench.py stamps its counter profiles with) stay untouched.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "kernels.h"

namespace neo {

// pillar.hip: the softmax-weighted sums alone (fp32; both arithmetics end with it).  Lf (M,512), score (3,M) in the order xz, yz, xy
void launch_pillar_aggregate(const PillarGeom& gm, const float* Lf, const float* score, float* fp_yz, float* fp_xz, float* fp_xy,
                             hipStream_t s);

// fragments in mfma_tile.h's order (about 6 MB); w as for launch_pillar_pack
size_t pillar_wpack_f32_bytes();
void launch_pillar_pack_f32(const float* const* w, float* wpack, hipStream_t s);
// launch_pillar's arguments with the fp32 pack in place of the split one; no range guard, no flags
int launch_pillar_f32(const PillarGeom& gm, const float* latent_cl, const float* wpack, const float* bias, const float* head_w,
                      const float* head_b_host, float* h1, float* h2, float* Lf, float* score, float* fp_yz, float* fp_xz,
                      float* fp_xy, hipStream_t s);

// pack_h.hip: launch_f32_range_check for a PER-CALL input (the encoder's latent): raises flag bit 1 only, not the static bit
void launch_f32_input_range_check(const float* x, size_t n, float limit, uint32_t* flags, hipStream_t s);

}  // namespace neo
