// The NeRF_TP frame driver (host code only; defined in api_tp.hip beside tp_launch): what every frame entry point shares.
//
//   TpFrame::begin      the call preamble - argument, scene and slot checks, this call's scene descriptor, N0 / N1, the constant
//                       tables, the lane ordering scope;
//   tp_render_dense     the dense two-level launch list on all R rays, inside and outside the sphere (neo_tp_render,
//                       neo_tp_render_extras, neo_tp_render_edited, neo_tp_render_decomposed, neo_tp_render_skipping);
//   tp_march_compact    the two-level inside-sphere march on compact rows under a device count (neo_tp_render_objects, every
//                       window of neo_tp_render_instances).
//
// neo_tp_render_culled, neo_tp_render_terminating, neo_tp_render_accelerated and neo_tp_render_marching share one driver of their own,
// tp_render_marching in api_tp.hip, with a launch order of its own - the foreground of both levels first, then the background on the
// rays that still let light through; it takes the preamble and the dense row layout only.  Where a level marches, the driver calls
// tp_eval_march, a call of the one window x segment loop march_level (march.h, with the region table).
#pragma once
#include "ctx.h"

namespace neo_host {

// the arguments every frame entry point of the C ABI has
struct TpFrameArgs {
    const float *rays_o, *rays_d, *viewdirs;
    int R, chunk;
    const float* src_poses;
    int NV;
    float focal, cx, cy;
    int n_coarse, n_fine;
    void* stream;
};

struct TpFrame {
    // An entry point's OWN argument checks, by where their message ranks among the shared ones (the rank decides which of two bad
    // arguments a call reports): each is the message of its first failing check (NEO_ERR_INVALID) or NULL.
    struct Own {
        const char* after_rays = nullptr;      // reported behind "bad ray count / chunk"
        const char* after_counts = nullptr;    // ... behind "unsupported sample counts"
        bool empty = false;                    // nothing to render although R > 0: leave as for R == 0
        bool ptrs = true;                      // the entry point's further pointers of the "null pointer" check
        const char* after_ptrs = nullptr;      // ... behind "null pointer"
    };

    neo_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    bool empty = false;                        // R == 0 (or own.empty): begin() stopped behind the argument checks, nothing is set up
    neo::TpScene sc{};                         // this call's scene descriptor and views (call_scene)
    neo::TpViews views{};
    int N0 = 0, N1 = 0;                        // samples per ray of the two levels
    static constexpr float near = 1e-4f;       // model.py:277
    const float* edges = nullptr;              // linspace(0,1,n_coarse+1)
    const float* u = nullptr;                  // the resampling quantiles

    // outside: the outside-sphere slots 2, 3 are needed; use_grid: the dense calls take the ray-grid hint of the frame API.
    // Returns behind ORDERED_LANE: the scope ends with this object.  `empty` is left to the caller (it may have a device word to zero).
    int begin(neo_ctx* ctx, const TpFrameArgs& a, bool outside, bool use_grid, const Own& own);
    ~TpFrame() {
        if (ordered) {
            neo_order_scope end_{ctx, s};
        }
    }
    TpFrame() = default;
    TpFrame(const TpFrame&) = delete;
    TpFrame& operator=(const TpFrame&) = delete;

private:
    bool ordered = false;
};

// W[0..8] of the lane's workspaces as the dense frame lays them out (neo_tp_render_culled keeps compact rows in the bg_* ones);
// nine pointers and nothing else, so that a caller can bind them by name
struct TpDenseRows {
    float *far, *fg_t0, *bg_s0, *fg_out, *bg_out, *fg_w0, *bg_w0, *fg_t1, *bg_s1;
    int reserve(DevBuf* W, size_t r, int N0, int N1) {
        if (W[0].reserve(r * 4) || W[1].reserve(r * N0 * 4) || W[2].reserve(r * N0 * 4) || W[3].reserve(r * N1 * 16) ||
            W[4].reserve(r * N1 * 16) || W[5].reserve(r * N0 * 4) || W[6].reserve(r * N0 * 4) || W[7].reserve(r * N1 * 4) ||
            W[8].reserve(r * N1 * 4))
            return NEO_ERR_NOMEM;
        *this = {W[0].as<float>(), W[1].as<float>(), W[2].as<float>(), W[3].as<float>(), W[4].as<float>(),
                 W[5].as<float>(), W[6].as<float>(), W[7].as<float>(), W[8].as<float>()};
        return NEO_OK;
    }
};

// What a dense frame does beyond neo_tp_render's list, per level where it says so.  All zero: neo_tp_render with a full level 0.
struct TpDenseOptions {
    const neo_tp_level_out* level[2] = {nullptr, nullptr};
    bool level0_may_be_sigma_only = false;     // run level 0 density-only when nobody reads its colours or depth
    const float* u_extras = nullptr;           // extras (tp_extras.hip): one k_tp_extras behind the merge of a level that asks
    int n_u = 0;
    const neo_tp_extras_out* extras[2] = {nullptr, nullptr};
    const float *near_inst = nullptr, *far_inst = nullptr;      // the (K, R) intervals of the edit and of the decomposition
    const neo::TpEditTable* edit = nullptr;    // k_tp_edit on the inside-sphere rows before their composite
    int K_edit = 0;
    const neo_tp_layers* layers = nullptr;     // k_composite_layers as the inside-sphere composite
    int L = 0;
    const neo_tp_decomposed_out* decomposed[2] = {nullptr, nullptr};      // k_tp_decompose behind the inside-sphere composite
    int K_dec = 0;
    const neo_tp_edit_samples* samples[2] = {nullptr, nullptr};          // copies of the level's sample rows and scene weights
    // skipping (tp_eval_skipping: march_level without a stop rule): the inside-sphere launch of each level becomes, per window of
    // rays, the point list (classify + compact), one compact launch of single points, scatter; fg_keep / fg_rows (may be null): the level's keep mask (R,N) and rgb/sigma rows (R,N,4);
    // kept (may be null): int64[2] on the device, the kept points per level
    bool skip = false;
    uint8_t* fg_keep[2] = {nullptr, nullptr};
    float* fg_rows[2] = {nullptr, nullptr};
    long long* kept = nullptr;
};

// the caller has entered the context (ENTER) and checked its own counts
int tp_render_dense(neo_ctx* ctx, const TpFrameArgs& a, const TpDenseOptions& o);

// One window of compact rows (row k belongs to ray map[k]) in the lane's workspaces, sized for R rows: the level-0 rows the caller
// fills, the march's scratch and its per-level results.
struct TpCompactRows {
    float *far, *t0, *rays_d, *out, *w0, *t1;
    float *rgb[2], *acc[2], *depth[2];         // per level, 5 floats a row in W[9]
    int reserve(DevBuf* W, size_t r, int N0, int N1) {
        if (W[0].reserve(r * 4) || W[1].reserve(r * N0 * 4) || W[2].reserve(r * 3 * 4) || W[3].reserve(r * N1 * 16) ||
            W[5].reserve(r * N0 * 4) || W[7].reserve(r * N1 * 4) || W[9].reserve(r * 10 * 4))
            return NEO_ERR_NOMEM;
        far = W[0].as<float>(), t0 = W[1].as<float>(), rays_d = W[2].as<float>();
        out = W[3].as<float>(), w0 = W[5].as<float>(), t1 = W[7].as<float>();
        float* res = W[9].as<float>();
        for (int l = 0; l < 2; ++l) {
            rgb[l] = res + r * 5 * l;
            acc[l] = res + r * (5 * l + 3);
            depth[l] = res + r * (5 * l + 4);
        }
        return NEO_OK;
    }
};

// evaluate, composite, resample, evaluate, composite on the *count rows of `rows`; grids are sized for R, every kernel takes its
// row count from the device word
int tp_march_compact(const TpFrame& f, const TpFrameArgs& a, const TpCompactRows& rows, const int* map, const int* count, int white);

}  // namespace neo_host
