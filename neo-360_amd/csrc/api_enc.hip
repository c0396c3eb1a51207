// Scene-encoder entry points of the C ABI: the pillar stage of GridEncoder (SURVEY.md §8f row 1;
// models/neo360/encoder_tp_fusion_conv.py:472-578) between the ResNet latent and the floor-plan conv nets.
#include "ctx.h"
#include "pillar_f32.h"
#include "pillar_train.h"

using namespace neo_host;

namespace {

int enc_check(int NV, int Hf, int Wf, int G0, int G1, int G2) {
    REQUIRE(NV >= 1 && NV <= neo::TP_MAX_VIEWS, "1..8 source views supported");
    REQUIRE(Hf >= 2 && Wf >= 2, "latent must be at least 2x2");
    REQUIRE(G0 >= 1 && G1 >= 1 && G2 >= 1 && G0 <= 256 && G1 <= 256 && G2 <= 256, "grid sizes must be 1..256");
    REQUIRE(static_cast<long>(NV) * Hf * Wf * 2048 <= 4294967295L, "latent too large for 32-bit byte offsets");
    return NEO_OK;
}

// the set-up the pillar stage's forward entry points share: channels-last latent, world axes, geometry
int enc_prepare(neo_ctx* ctx, const float* latent, int NV, int Hf, int Wf, float image_w, float image_h, const float* src_poses,
                float focal, float cx, float cy, int G0, int G1, int G2, hipStream_t s, neo::PillarGeom& gm) {
    if (ctx->enc_latent.reserve(static_cast<size_t>(NV) * 512 * Hf * Wf * 4)) return NEO_ERR_NOMEM;
    neo::launch_channels_last(latent, NV, 512, Hf, Wf, ctx->enc_latent.as<float>(), s);
    // world grid axes: torch.linspace values, x / y in [-1, 1], z in [0, 1] (side_lengths = [1,1,1], :481-489)
    float axes[3 * 256] = {};
    neo_linspace_host(-1.0f, 1.0f, G0, axes);
    neo_linspace_host(-1.0f, 1.0f, G1, axes + 256);
    neo_linspace_host(0.0f, 1.0f, G2, axes + 512);
    if (ctx->enc_axes.reserve(sizeof axes)) return NEO_ERR_NOMEM;
    HIP_TRY(hipMemcpyAsync(ctx->enc_axes.p, axes, sizeof axes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));        // `axes` is on the host stack
    gm = neo::PillarGeom{};
    gm.nv = NV; gm.G0 = G0; gm.G1 = G1; gm.G2 = G2; gm.Hf = Hf; gm.Wf = Wf;
    gm.focal = focal; gm.cx = cx; gm.cy = cy;
    const float wf = static_cast<float>(Wf), hf = static_cast<float>(Hf);
    gm.sx = ((wf / (wf - 1.0f)) * 2.0f) / image_w;
    gm.sy = ((hf / (hf - 1.0f)) * 2.0f) / image_h;
    gm.axes = ctx->enc_axes.as<float>();
    for (int i = 0; i < NV; ++i) {           // rot = c2w[:3,:3]^T, trans = -rot c2w[:3,3] (neo360/util.py:64-66)
        const float* m = src_poses + i * 16;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) gm.rot[i][r * 3 + c] = m[c * 4 + r];
        for (int r = 0; r < 3; ++r) {
            float acc = gm.rot[i][r * 3 + 0] * m[0 * 4 + 3];
            acc = acc + gm.rot[i][r * 3 + 1] * m[1 * 4 + 3];
            acc = acc + gm.rot[i][r * 3 + 2] * m[2 * 4 + 3];
            gm.trans[i][r] = -acc;
            gm.cpos[i][r] = m[r * 4 + 3];
        }
    }
    return NEO_OK;
}

// the forward in the context's arithmetic, with the activations in h1 / h2 / Lf / score.  Split fp16 (precision 1): range guards,
// then launch_pillar; the latent is this call's input, not an uploaded map, so a trip on it does not carry the static bit.
// Exact fp32 (precision 0): launch_pillar_f32, no range check, no flag bit.
int enc_forward(neo_ctx* ctx, const neo::PillarGeom& gm, float* h1, float* h2, float* Lf, float* score, float* fp_yz, float* fp_xz,
                float* fp_xy, hipStream_t s) {
    const long M = static_cast<long>(gm.nv) * gm.G0 * gm.G1 * gm.G2;
    MlpSlot& sl = ctx->enc;
    int rc;
    if (ctx->precision == 1) {
        guard_split_weights(sl, sl.wpack_h.p, neo::pillar_wpack_bytes(), ctx->flags, s, neo::SPLIT_WEIGHT_LOW_ENC);
        neo::launch_f32_input_range_check(ctx->enc_latent.as<float>(), static_cast<size_t>(gm.nv) * 512 * gm.Hf * gm.Wf, 65504.0f, ctx->flags, s);
        {   // low end of the same per-call operand: a latent that is small everywhere (kernels.h SPLIT_LATENT_LOW_ENC)
            const float* lat = ctx->enc_latent.as<float>();
            if (int rc = guard_map_low(ctx, MAP_MAX_ENC_LATENT, &lat, 1, static_cast<size_t>(gm.nv) * 512 * gm.Hf * gm.Wf,
                                       neo::SPLIT_LATENT_LOW_ENC, false, s)) return rc;
        }
        ctx->span_begin(s);
        rc = neo::launch_pillar(gm, ctx->enc_latent.as<float>(), sl.wpack_h.p, sl.bias.as<float>(), sl.heads.as<float>(),
                                ctx->enc_head_b, h1, h2, Lf, score, ctx->flags, fp_yz, fp_xz, fp_xy, s);
    } else {
        ctx->span_begin(s);
        rc = neo::launch_pillar_f32(gm, ctx->enc_latent.as<float>(), sl.wpack.as<float>(), sl.bias.as<float>(), sl.heads.as<float>(),
                                    ctx->enc_head_b, h1, h2, Lf, score, fp_yz, fp_xz, fp_xy, s);
    }
    // algorithmic MACs per cell-view: 518*512 + 2*512^2 + 3*(513*512 + 512) (encoder_tp_fusion_conv.py:263-279, :364-373)
    ctx->span_end(s, static_cast<double>(M), 2.0 * (518.0 * 512 + 2.0 * 512 * 512 + 3.0 * (513.0 * 512 + 512)));
    if (rc) return fail(NEO_ERR_INVALID, "unsupported grid");
    return check_launch();
}

}  // namespace

extern "C" {

int neo_enc_upload(neo_ctx* ctx, const float* const* weights, const float* const* biases, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(weights && biases, "null pointer table");
    for (int i = 0; i < 9; ++i) REQUIRE(weights[i] && biases[i], "null layer pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MlpSlot& sl = ctx->enc;
    if (sl.wpack_h.reserve(neo::pillar_wpack_bytes())) return NEO_ERR_NOMEM;
    if (sl.wpack.reserve(neo::pillar_wpack_f32_bytes())) return NEO_ERR_NOMEM;       // the exact-fp32 twin's fragments
    if (sl.bias.reserve(6 * 512 * sizeof(float))) return NEO_ERR_NOMEM;
    if (sl.heads.reserve(3 * 512 * sizeof(float))) return NEO_ERR_NOMEM;
    // order: depth_fc.common_branch.0, .2, depth_fc.depth_encoder, then per axis (xz, yz, xy): aggregator .0, .2
    const float* hidden[6] = {weights[0], weights[1], weights[2], weights[3], weights[5], weights[7]};
    const float* hidden_b[6] = {biases[0], biases[1], biases[2], biases[3], biases[5], biases[7]};
    neo::launch_pillar_pack(hidden, sl.wpack_h.p, s);
    neo::launch_pillar_pack_f32(hidden, sl.wpack.as<float>(), s);
    for (int i = 0; i < 6; ++i) neo::copy_floats(hidden_b[i], 512, sl.bias.as<float>() + 512 * i, s);
    for (int a = 0; a < 3; ++a) {
        neo::copy_floats(weights[4 + 2 * a], 512, sl.heads.as<float>() + 512 * a, s);
        HIP_TRY(hipMemcpyAsync(&ctx->enc_head_b[a], biases[4 + 2 * a], sizeof(float), hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));        // the three scalar head biases are kernel arguments
    {   // element counts in upload order: common_branch.0, .2, depth_encoder, then per axis the aggregator's layer and its scorer head
        const size_t counts[9] = {512 * 518, 512 * 512, 512 * 512, 512 * 513, 512, 512 * 513, 512, 512 * 513, 512};
        if (int rc = record_weight_maxima(sl, weights, counts, 9, s)) return rc;
    }
    sl.weights_epoch += 1;
    sl.ready = true;
    return check_launch();
}


int neo_enc_floorplans(neo_ctx* ctx, const float* latent, int NV, int Hf, int Wf, float image_w, float image_h,
                       const float* src_poses, float focal, float cx, float cy, int G0, int G1, int G2, float* fp_yz,
                       float* fp_xz, float* fp_xy, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));      // touches context-owned memory: ordered across streams
    REQUIRE(latent && src_poses && fp_yz && fp_xz && fp_xy, "null pointer");
    if (const int rc = enc_check(NV, Hf, Wf, G0, G1, G2)) return rc;
    if (!ctx->enc.ready) return fail(NEO_ERR_STATE, "encoder weights not uploaded (neo_enc_upload)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    neo::PillarGeom gm;
    if (const int rc = enc_prepare(ctx, latent, NV, Hf, Wf, image_w, image_h, src_poses, focal, cx, cy, G0, G1, G2, s, gm)) return rc;
    const long M = static_cast<long>(NV) * G0 * G1 * G2;
    for (int i = 0; i < 3; ++i)
        if (ctx->enc_ws[i].reserve(static_cast<size_t>(M) * 512 * 4)) return NEO_ERR_NOMEM;
    if (ctx->enc_ws[3].reserve(static_cast<size_t>(M) * 3 * 4)) return NEO_ERR_NOMEM;
    return enc_forward(ctx, gm, ctx->enc_ws[0].as<float>(), ctx->enc_ws[1].as<float>(), ctx->enc_ws[2].as<float>(),
                       ctx->enc_ws[3].as<float>(), fp_yz, fp_xz, fp_xy, s);
}

long neo_enc_train_tape_floats(int NV, int G0, int G1, int G2) {
    if (NV < 1 || G0 < 1 || G1 < 1 || G2 < 1) return 0;
    return static_cast<long>(neo::pillar_train_tape_floats(NV, G0, G1, G2));
}

int neo_enc_floorplans_train(neo_ctx* ctx, const float* latent, int NV, int Hf, int Wf, float image_w, float image_h,
                             const float* src_poses, float focal, float cx, float cy, int G0, int G1, int G2, float* tape,
                             float* fp_yz, float* fp_xz, float* fp_xy, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));
    REQUIRE(latent && src_poses && tape && fp_yz && fp_xz && fp_xy, "null pointer");
    if (const int rc = enc_check(NV, Hf, Wf, G0, G1, G2)) return rc;
    REQUIRE(static_cast<long>(NV) * G0 * G1 * G2 <= 65535L * 128, "at most 8,388,480 cell-views per call");
    if (!ctx->enc.ready) return fail(NEO_ERR_STATE, "encoder weights not uploaded (neo_enc_upload)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    neo::PillarGeom gm;
    if (const int rc = enc_prepare(ctx, latent, NV, Hf, Wf, image_w, image_h, src_poses, focal, cx, cy, G0, G1, G2, s, gm)) return rc;
    const long M = static_cast<long>(NV) * G0 * G1 * G2;
    return enc_forward(ctx, gm, tape, tape + M * 512, tape + 2 * M * 512, tape + 3 * M * 512, fp_yz, fp_xz, fp_xy, s);
}

int neo_enc_floorplans_backward(neo_ctx* ctx, const float* const* w, const float* const* b, const float* latent, int NV, int Hf,
                                int Wf, float image_w, float image_h, const float* src_poses, float focal, float cx, float cy,
                                int G0, int G1, int G2, const float* tape, const float* g_yz, const float* g_xz, const float* g_xy,
                                float* const* gw, float* const* gb, float* g_latent, void* stream) {
    ENTER(ctx);
    ORDERED(ctx, static_cast<hipStream_t>(stream));
    REQUIRE(w && b && latent && src_poses && tape && g_yz && g_xz && g_xy && gw && gb, "null pointer");
    if (const int rc = enc_check(NV, Hf, Wf, G0, G1, G2)) return rc;
    for (int i = 0; i < 9; ++i) REQUIRE(w[i] && b[i] && gw[i] && gb[i], "null weight / gradient pointer");
    REQUIRE(static_cast<long>(NV) * G0 * G1 * G2 <= 65535L * 128, "at most 8,388,480 cell-views per call");
    hipStream_t s = static_cast<hipStream_t>(stream);
    neo::PillarGeom gm;
    if (const int rc = enc_prepare(ctx, latent, NV, Hf, Wf, image_w, image_h, src_poses, focal, cx, cy, G0, G1, G2, s, gm)) return rc;
    if (ctx->train_scratch.reserve(neo::pillar_train_scratch_floats(NV, G0, G1, G2, Hf, Wf, g_latent != nullptr) * sizeof(float)))
        return NEO_ERR_NOMEM;
    neo::launch_pillar_backward(gm, w, b, ctx->enc_latent.as<float>(), tape, g_yz, g_xz, g_xy, gw, gb, g_latent,
                                ctx->train_scratch.as<float>(), s);
    return check_launch();
}

}  // extern "C"
