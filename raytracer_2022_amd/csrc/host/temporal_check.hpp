// temporal_check.hpp — what rt_temporal* refuses and the size of its workspace. Pure arithmetic on the caller's words, no HIP:
// every refusal comes before the first device call.
#ifndef RT2022_TEMPORAL_CHECK_HPP
#define RT2022_TEMPORAL_CHECK_HPP
#include <cmath>
#include <cstdint>

#include "../../../include/rt2022.h"

namespace rt2022 {

// What is wrong with the parameters of rt_temporal* (null: nothing) — rt_temporal_workspace_bytes answers 0 to the same faults.
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

// The workspace (byte offsets, each a multiple of 16): the row kernel's inverse map and its count of bad ids.
struct TemporalLayout {
    uint64_t inv_rows;                 // height x uint32: image row -> buffer row
    uint64_t bad_rows;                 // one uint32: bad or repeated row ids of the call's list
    uint64_t bytes;
};
inline TemporalLayout temporal_layout(uint32_t height) {
    TemporalLayout l;
    l.inv_rows = 0;
    l.bad_rows = ((uint64_t)height * sizeof(uint32_t) + 15u) / 16u * 16u;
    l.bytes = l.bad_rows + 16u;
    return l;
}

// What is wrong with the buffers of a call whose parameters are sound (null: nothing). `device`: the pointers are device
// memory, with a workspace and alignment rules; the states' address ranges are compared either way.
inline const char *temporal_buffers_fault(const void *sum, const void *feat, const void *rows, const void *cam, const void *prev,
                                          const void *prev_cam, const rt_temporal_params *p, const void *state_out, const void *out,
                                          const void *workspace, bool device) {
    if (!sum || !feat || !out) return "null sums, features or output";
    if (!state_out) return "null output state";
    if (!cam) return "null camera";
    if (prev && !prev_cam) return "a previous state without its camera";
    if (device) {
        if (!workspace) return "null workspace";
        if (((uintptr_t)sum | (uintptr_t)feat | (uintptr_t)out | (uintptr_t)state_out | (uintptr_t)prev | (uintptr_t)workspace) & 15u)
            return "the buffers and the workspace must be 16-byte aligned";
        if ((uintptr_t)rows & 3u) return "row_ids must be 4-byte aligned";
    }
    if (prev) {
        const uint64_t bytes = (uint64_t)p->width * p->height * sizeof(rt_temporal_pixel);
        const uintptr_t a = (uintptr_t)prev, b = (uintptr_t)state_out;
        if (a < b ? b - a < bytes : a - b < bytes) return "the output state overlaps the previous state";
    }
    return nullptr;
}

} // namespace rt2022
#endif
