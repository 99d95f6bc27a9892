// post_check.hpp — what the calls on a render's buffers refuse (rt_denoise*, rt_denoise_dual*, rt_temporal*, rt_adaptive_*)
// and where the pieces of their workspaces lie. Pure arithmetic on the caller's words, no HIP: every refusal comes before the
// first device call, and tests/post_units.cpp holds all of it to literals as a stand-alone program.
// A *_params_fault says what is wrong with the parameters (null: nothing) — the family's *_workspace_bytes answers 0 to the
// same faults. A *_buffers_fault of a family with parameters is the whole check of a call: the params fault first, then what is
// wrong with the buffers. `device`: the pointers are device memory, with a workspace and alignment rules.
#ifndef RT2022_POST_CHECK_HPP
#define RT2022_POST_CHECK_HPP
#include <cmath>
#include <cstdint>

#include "../../../include/rt2022.h"

namespace rt2022 {

// Whether any of the pointers has a bit of `mask` set (null passes).
template <class... P>
inline bool misaligned(uintptr_t mask, P... ptrs) { return (((uintptr_t)ptrs | ...) & mask) != 0; }

// The device rules the two denoisers and the temporal accumulation share: a workspace, 16 bytes for it and the buffers, 4 for the rows.
template <class... P>
inline const char *device_buffers_fault(const void *workspace, const void *rows, P... buffers) {
    if (!workspace) return "null workspace";
    if (misaligned(15u, workspace, buffers...)) return "the buffers and the workspace must be 16-byte aligned";
    return misaligned(3u, rows) ? "row_ids must be 4-byte aligned" : nullptr;
}

// ---- the row map: what the row kernel (pt_rows.hip) leaves in every family's workspace ----------------------------------
struct RowMapLayout {
    uint64_t inv;                      // height x uint32: image row -> buffer row
    uint64_t bad;                      // one uint32 in a 16-byte piece: bad or repeated row ids of the call's list
};
inline uint64_t row_map_bytes(uint32_t height) { return ((uint64_t)height * sizeof(uint32_t) + 15u) / 16u * 16u; }
// The map at `at` with the count behind it: ends at bad + 16.
inline RowMapLayout row_map_then_count(uint64_t at, uint32_t height) { return RowMapLayout{at, at + row_map_bytes(height)}; }

// ---- rt_denoise* ---------------------------------------------------------------------------------------------------------
inline const char *denoise_params_fault(const rt_denoise_params *p) {
    if (!p) return "null params";
    if (p->width == 0 || p->height == 0) return "empty image (width or height is 0)";
    if (p->spp == 0) return "spp is 0";
    if (p->n_iter > RT_DENOISE_MAX_ITER) return "n_iter > RT_DENOISE_MAX_ITER";
    for (double s : {p->sigma_color, p->sigma_normal, p->sigma_depth, p->sigma_albedo})
        if (!(s > 0.0)) return "a sigma is <= 0 or NaN";
    if (!(p->albedo_floor > 0.0) || std::isinf(p->albedo_floor)) return "albedo_floor is <= 0, NaN or infinite";
    if (p->flags & ~RT_DENOISE_NO_DEMODULATE) return "flag bits other than RT_DENOISE_NO_DEMODULATE";
    if ((uint64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return "width * height > RT_DENOISE_MAX_PIXELS";
    return nullptr;
}

// The workspace (byte offsets, each a multiple of 16). A pixel's ten doubles are five 16-byte pieces, each a plane of its own.
struct DenoiseLayout {
    uint64_t guides;                   // 3 planes of n_pixels double2: {n0, n1} {n2, z} {a0, a1}, image order
    uint64_t colour[2];                // ping-pong, each 2 planes of n_pixels double2: {e0, e1} {e2, a2}
    RowMapLayout rows;
    uint64_t bytes;
};
inline DenoiseLayout denoise_layout(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)width * height;
    DenoiseLayout l;
    l.guides = 0;
    l.colour[0] = 3 * n * 16u;
    l.colour[1] = l.colour[0] + 2 * n * 16u;
    l.rows = row_map_then_count(l.colour[1] + 2 * n * 16u, height);
    l.bytes = l.rows.bad + 16u;
    return l;
}
inline uint64_t denoise_workspace_bytes(const rt_denoise_params *p) { return denoise_params_fault(p) ? 0 : denoise_layout(p->width, p->height).bytes; }

inline const char *denoise_buffers_fault(const void *sum, const void *feat, const void *rows, const rt_denoise_params *p, const void *out,
                                         const void *workspace, bool device) {
    if (const char *fault = denoise_params_fault(p)) return fault;
    if (!sum || !feat || !out) return "null sums, features or output";
    return device ? device_buffers_fault(workspace, rows, sum, feat, out) : nullptr;
}

// ---- rt_denoise_dual*: what rt_denoise* refuses, then the dual filter's own ------------------------------------------------
inline const char *denoise_dual_params_fault(const rt_denoise_dual_params *q) {
    if (!q) return "null dual params";
    if (q->var_iter > RT_DENOISE_MAX_VAR_ITER) return "var_iter > RT_DENOISE_MAX_VAR_ITER";
    if (!(q->var_floor > 0.0) || std::isinf(q->var_floor)) return "var_floor is <= 0, NaN or infinite";
    if (q->flags != 0) return "dual flags must be 0";
    return nullptr;
}

// The dual filter's workspace (byte offsets, each a multiple of 16). A pixel's eleven doubles are five 16-byte pieces and one
// 8-byte piece, each a plane of its own.
struct DenoiseDualLayout {
    uint64_t guides;                   // 3 planes of n_pixels double2: {n0, n1} {n2, z} {a0, a1}, image order
    uint64_t a2;                       // 1 plane of n_pixels double: the albedo's third component
    uint64_t colour[2];                // ping-pong, each 2 planes of n_pixels double2: {e0, e1} {e2, u}
    uint64_t var[2];                   // ping-pong of the prefilter, each 1 plane of n_pixels double: v
    RowMapLayout rows;
    uint64_t bytes;
};
inline DenoiseDualLayout denoise_dual_layout(uint32_t width, uint32_t height) {
    const uint64_t n = (uint64_t)width * height, n2 = (n + 1u) / 2u * 2u;   // (a plane of doubles ends on a 16-byte piece)
    DenoiseDualLayout l;
    l.guides = 0;
    l.a2 = 3 * n * 16u;
    l.colour[0] = l.a2 + n2 * 8u;
    l.colour[1] = l.colour[0] + 2 * n * 16u;
    l.var[0] = l.colour[1] + 2 * n * 16u;
    l.var[1] = l.var[0] + n2 * 8u;
    l.rows = row_map_then_count(l.var[1] + n2 * 8u, height);
    l.bytes = l.rows.bad + 16u;
    return l;
}
// (of the shared parameters alone: the size does not depend on `q`)
inline uint64_t denoise_dual_workspace_bytes(const rt_denoise_params *p) { return denoise_params_fault(p) ? 0 : denoise_dual_layout(p->width, p->height).bytes; }

// (the rules of `q` come where they always came: behind `p`'s, half A's buffers and half B's, before the device rules)
inline const char *denoise_dual_buffers_fault(const void *sum_a, const void *sum_b, const void *feat_a, const void *feat_b, const void *rows,
                                              const rt_denoise_params *p, const rt_denoise_dual_params *q, const void *out, const void *out_var,
                                              const void *workspace, bool device) {
    if (const char *fault = denoise_params_fault(p)) return fault;
    if (!sum_a || !feat_a || !out) return "null sums, features or output";
    if (q && (!sum_b || !feat_b)) return "null sums or features of the second half";
    if (const char *fault = denoise_dual_params_fault(q)) return fault;
    return device ? device_buffers_fault(workspace, rows, sum_a, sum_b, feat_a, feat_b, out, out_var) : nullptr;
}

// ---- rt_temporal* --------------------------------------------------------------------------------------------------------
inline const char *temporal_params_fault(const rt_temporal_params *p) {
    if (!p) return "null params";
    if (p->width == 0 || p->height == 0) return "empty image (width or height is 0)";
    if (p->spp == 0) return "spp is 0";
    if ((uint64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return "width * height > RT_DENOISE_MAX_PIXELS";
    if (!(p->tol_depth > 0.0) || !(p->tol_normal > 0.0)) return "a tolerance is <= 0 or NaN";
    if (!(p->n_max >= 1.0) || std::isinf(p->n_max)) return "n_max is < 1, NaN or infinite";
    if (!(p->w_min > 0.0) || !(p->w_min <= 1.0)) return "w_min is outside (0, 1]";
    if (!(p->albedo_floor > 0.0) || std::isinf(p->albedo_floor)) return "albedo_floor is <= 0, NaN or infinite";
    if (p->flags & ~(RT_TEMPORAL_NO_DEMODULATE | RT_TEMPORAL_FAR_MISSES)) return "flag bits other than RT_TEMPORAL_NO_DEMODULATE | RT_TEMPORAL_FAR_MISSES";
    return nullptr;
}

// The workspace holds nothing but the row map.
struct TemporalLayout { RowMapLayout rows; uint64_t bytes; };
inline TemporalLayout temporal_layout(uint32_t height) { return TemporalLayout{row_map_then_count(0, height), row_map_bytes(height) + 16u}; }
inline uint64_t temporal_workspace_bytes(const rt_temporal_params *p) { return temporal_params_fault(p) ? 0 : temporal_layout(p->height).bytes; }

// (the states' address ranges are compared in both forms)
inline const char *temporal_buffers_fault(const void *sum, const void *feat, const void *rows, const void *cam, const void *prev,
                                          const void *prev_cam, const rt_temporal_params *p, const void *state_out, const void *out,
                                          const void *workspace, bool device) {
    if (const char *fault = temporal_params_fault(p)) return fault;
    if (!sum || !feat || !out) return "null sums, features or output";
    if (!state_out) return "null output state";
    if (!cam) return "null camera";
    if (prev && !prev_cam) return "a previous state without its camera";
    if (const char *fault = device ? device_buffers_fault(workspace, rows, sum, feat, out, state_out, prev) : nullptr) return fault;
    if (prev) {
        const uint64_t bytes = (uint64_t)p->width * p->height * sizeof(rt_temporal_pixel);
        const uintptr_t a = (uintptr_t)prev, b = (uintptr_t)state_out;
        if (a < b ? b - a < bytes : a - b < bytes) return "the output state overlaps the previous state";
    }
    return nullptr;
}

// ---- rt_adaptive_* -------------------------------------------------------------------------------------------------------
inline const char *adaptive_params_fault(const rt_adaptive_params *p) {
    if (!p) return "null params";
    if (p->width == 0 || p->height == 0) return "empty image (width or height is 0)";
    if ((uint64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return "width * height > RT_DENOISE_MAX_PIXELS";
    if (p->max_units == 0) return "max_units is 0";
    if ((uint64_t)p->first_frame + p->max_units > 0xFFFFFFFFull) return "first_frame + max_units > 2^32 - 1";
    if (!(p->scale > 0.0) || std::isinf(p->scale)) return "scale is <= 0, NaN or infinite";
    if (p->flags != 0 || p->_pad != 0) return "flags must be 0";
    return nullptr;
}

// The planner's workspace (byte offsets, each a multiple of 16): here the count comes before the map.
constexpr uint32_t kAdaptiveTile = 1024;      // pixels a workgroup of the scan owns (pt_adaptive.hip)
struct AdaptiveLayout {
    uint64_t n_tiles;                  // workgroups of the scan
    uint64_t totals;                   // (n_tiles + 1) x uint64: the tiles' units, then their exclusive scan; the last word: the total
    RowMapLayout rows;
    uint64_t bytes;
};
inline AdaptiveLayout adaptive_layout(uint32_t width, uint32_t height) {
    AdaptiveLayout l;
    l.n_tiles = ((uint64_t)width * height + kAdaptiveTile - 1) / kAdaptiveTile;
    l.totals = 0;
    l.rows.bad = ((l.n_tiles + 1) * sizeof(uint64_t) + 15u) / 16u * 16u;
    l.rows.inv = l.rows.bad + 16u;
    l.bytes = l.rows.inv + row_map_bytes(height);
    return l;
}
inline uint64_t adaptive_workspace_bytes(const rt_adaptive_params *p) { return adaptive_params_fault(p) ? 0 : adaptive_layout(p->width, p->height).bytes; }

inline const char *adaptive_plan_buffers_fault(const void *err, const void *rows, const rt_adaptive_params *p, const void *units, const void *offsets,
                                               const void *entries, uint64_t capacity, const void *workspace, bool device) {
    if (const char *fault = adaptive_params_fault(p)) return fault;
    if (!err || !units || !offsets) return "null error map, units or offsets";
    if (!entries && capacity != 0) return "null entries with a capacity";
    return !device ? nullptr : !workspace ? "null workspace" : misaligned(15u, err, workspace) ? "the error map and the workspace must be 16-byte aligned"
         : misaligned(7u, offsets, entries) ? "offsets and entries must be 8-byte aligned" : misaligned(3u, units, rows) ? "units and row_ids must be 4-byte aligned" : nullptr;
}

// The merges and resolves exist in the device form only. Rule by rule: the pixel count; a call on no pixels passes whatever
// its pointers are; a null buffer; then `misaligned_fault`, the call's own verdict on its pointers' alignment (null: none).
inline const char *pixel_buffers_fault(uint64_t n_pixels, bool any_null, const char *misaligned_fault) {
    if (n_pixels > RT_DENOISE_MAX_PIXELS) return "n_pixels > RT_DENOISE_MAX_PIXELS";
    return n_pixels == 0 ? nullptr : any_null ? "null buffer" : misaligned_fault;
}

inline const char *adaptive_merge_buffers_fault(const void *entry_sums, const void *units, const void *offsets, uint64_t n_pixels,
                                                const void *acc_sum, const void *acc_n) {
    return pixel_buffers_fault(n_pixels, !entry_sums || !units || !offsets || !acc_sum || !acc_n,
                               misaligned(7u, entry_sums, offsets, acc_sum, acc_n) ? "sums, offsets and accumulators must be 8-byte aligned"
                               : misaligned(3u, units) ? "units must be 4-byte aligned" : nullptr);
}

inline const char *adaptive_resolve_buffers_fault(const void *acc_sum, const void *acc_n, uint64_t n_pixels, const void *out) {
    return pixel_buffers_fault(n_pixels, !acc_sum || !acc_n || !out, misaligned(7u, acc_sum, acc_n, out) ? "the buffers must be 8-byte aligned" : nullptr);
}

inline const char *adaptive_merge_features_buffers_fault(const void *entry_features, const void *units, const void *offsets, uint64_t n_pixels,
                                                         const void *acc) {
    return pixel_buffers_fault(n_pixels, !entry_features || !units || !offsets || !acc,
                               misaligned(15u, entry_features, acc) ? "the records must be 16-byte aligned"
                               : misaligned(7u, offsets) ? "offsets must be 8-byte aligned" : misaligned(3u, units) ? "units must be 4-byte aligned" : nullptr);
}

inline const char *adaptive_resolve_features_buffers_fault(const void *acc, const void *acc_n, uint64_t n_pixels, const void *out) {
    return pixel_buffers_fault(n_pixels, !acc || !acc_n || !out, misaligned(15u, acc, out) ? "the records must be 16-byte aligned"
                                                                  : misaligned(7u, acc_n) ? "the sample counts must be 8-byte aligned" : nullptr);
}

} // namespace rt2022
#endif
