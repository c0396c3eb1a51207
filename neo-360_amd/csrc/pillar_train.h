// Launchers of pillar_train.hip: the pillar stage of the scene encoder under autograd (forward with a caller-owned tape,
// backward on exact fp32 MFMA).  Kept apart from kernels.h / train_kernels.h so that the evaluators' and the decoder
// training's sources (the hashes bench.py stamps its counter profiles with) stay untouched.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels.h"

namespace neo {

// tape of one differentiable forward (floats): h1, h2, L (M x 512 each, M = nv G0 G1 G2 cell-views, view-major, x slowest)
// then the three score vectors (xz, yz, xy; M each).  The first-layer input is NOT taped: the backward re-gathers it.
size_t pillar_train_tape_floats(int nv, int G0, int G1, int G2);
// scratch of the backward (floats); with_latent: room for the channels-last latent gradient
size_t pillar_train_scratch_floats(int nv, int G0, int G1, int G2, int Hf, int Wf, int with_latent);

// w / b: the nine fp32 layers in neo_enc_upload order (depth_fc.common_branch.0, .2, depth_encoder, then aggregator .0 / .2 of
// xz, yz, xy).  latent_cl: channels-last latent (nv, Hf, Wf, 512) the forward read.  g_yz / g_xz / g_xy: floor-plan gradients,
// channels-last like the outputs.  gw / gb: accumulated (+=; zeroed by the caller).  g_latent (nv, 512, Hf, Wf) NCHW,
// accumulated, may be null.  The tape is only read.
void launch_pillar_backward(const PillarGeom& gm, const float* const* w, const float* const* b, const float* latent_cl,
                            const float* tape, const float* g_yz, const float* g_xz, const float* g_xy, float* const* gw,
                            float* const* gb, float* g_latent, float* scratch, hipStream_t s);

}  // namespace neo
