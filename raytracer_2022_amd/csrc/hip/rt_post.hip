// rt_post.hip — what works on a render's buffers and takes no scene: the denoisers (rt_denoise*, rt_denoise_dual*), the
// temporal accumulation (rt_temporal*) and the adaptive-sampling planner, merge and resolve (rt_adaptive_*).
#include <cmath>

#include "../host/temporal_check.hpp"
#include "rt_internal.hpp"

using namespace rt2022;

namespace {

// A host row list (null: none) must be a permutation of [0, height) — the device lists' twin is the row kernel (read_bad_rows).
void check_row_permutation(const uint32_t *row_ids, uint32_t height, const std::string &w) {
    if (!row_ids) return;
    std::vector<char> seen(height, 0);
    for (uint32_t i = 0; i < height; i++) {
        RT_REQUIRE(row_ids[i] < height && !seen[row_ids[i]], RT_ERR_INVALID, w + ": row_ids is not a permutation of the image's rows");
        seen[row_ids[i]] = 1;
    }
}

// The row kernel's verdict on a list from the caller's HBM: its count of bad or repeated ids, at `d_bad` in the workspace
// (null: no list), read behind ONE synchronisation of the stream — which also completes what the caller queued before it.
void read_bad_rows(const char *d_bad, hipStream_t stream, const std::string &w) {
    uint32_t bad = 0;
    if (d_bad) RT_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    RT_REQUIRE(bad == 0, RT_ERR_INVALID, w + ": row_ids is not a permutation of the image's rows");
}

// The device time of a host denoiser's call on the null stream: events around run(), waited for; report() once the results are back.
struct NullStreamTimer {
    Event ev0{hipEventDefault}, ev1{hipEventDefault};
    template <class Run>
    void run(Run run) {
        RT_HIP(hipEventRecord(ev0, nullptr));
        run();
        RT_HIP(hipEventRecord(ev1, nullptr));
        RT_HIP(hipStreamSynchronize(nullptr));
    }
    void report(double *ms) const {
        if (!ms) return;
        float t = 0.f;
        RT_HIP(hipEventElapsedTime(&t, ev0, ev1));
        *ms = (double)t;
    }
};

// What is wrong with the parameters of rt_adaptive_plan* (null: nothing) — rt_adaptive_workspace_bytes answers 0 to the same faults.
const char *adaptive_params_fault(const rt_adaptive_params *p) {
    if (!p) return "null params";
    if (p->width == 0 || p->height == 0) return "empty image (width or height is 0)";
    if ((uint64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return "width * height > RT_DENOISE_MAX_PIXELS";
    if (p->max_units == 0) return "max_units is 0";
    if ((uint64_t)p->first_frame + p->max_units > 0xFFFFFFFFull) return "first_frame + max_units > 2^32 - 1";
    if (!(p->scale > 0.0) || std::isinf(p->scale)) return "scale is <= 0, NaN or infinite";
    if (p->flags != 0 || p->_pad != 0) return "flags must be 0";
    return nullptr;
}

// One plan on `stream`: device buffers, the arguments checked. The kernels, then ONE synchronisation behind which the total
// and the row kernel's count are read together.
void run_adaptive_plan(const double *d_err, const uint32_t *d_rows, const rt_adaptive_params *p, uint32_t *d_units, uint64_t *d_offsets,
                       uint64_t *d_entries, uint64_t capacity, char *d_ws, hipStream_t stream, uint64_t *out_total, const std::string &w) {
    AdaptivePlanArgs a{};
    a.width = p->width; a.height = p->height; a.first_frame = p->first_frame; a.max_units = p->max_units; a.scale = p->scale;
    a.err = d_err; a.rows = d_rows; a.units = d_units; a.offsets = d_offsets; a.entries = d_entries; a.capacity = capacity; a.ws = d_ws;
    const AdaptiveLayout l = adaptive_layout(p->width, p->height);
    RT_HIP(launch_adaptive_plan(a, stream));
    unsigned long long total = 0;
    RT_HIP(hipMemcpyAsync(&total, d_ws + l.totals + l.n_tiles * sizeof(unsigned long long), sizeof total, hipMemcpyDeviceToHost, stream));
    read_bad_rows(d_rows ? d_ws + l.bad_rows : nullptr, stream, w);
    if (out_total) *out_total = total;
}

// What is wrong with the parameters of rt_denoise* (null: nothing) — rt_denoise_workspace_bytes answers 0 to the same faults.
const char *denoise_params_fault(const rt_denoise_params *p) {
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

void check_denoise(const double *sum, const rt_feature *feat, const rt_denoise_params *p, const double *out, const std::string &w) {
    const char *fault = denoise_params_fault(p);
    RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
    RT_REQUIRE(sum && feat && out, RT_ERR_INVALID, w + ": null sums, features or output");
}

// The filter's arguments as the kernels take them (pt_device.h), from the caller's parameters and device buffers.
DenoiseArgs denoise_args(const double *d_sum, const rt_feature *d_feat, const uint32_t *d_rows, const rt_denoise_params *p, double *d_out, char *d_ws) {
    DenoiseArgs a{};
    a.width = p->width; a.height = p->height;
    a.sp = (double)p->spp;
    a.inv_n = 1.0 / (p->sigma_normal * p->sigma_normal);
    a.inv_z = 1.0 / (p->sigma_depth * p->sigma_depth);
    a.inv_a = 1.0 / (p->sigma_albedo * p->sigma_albedo);
    a.albedo_floor = p->albedo_floor;
    a.demodulate = !(p->flags & RT_DENOISE_NO_DEMODULATE);
    a.sum = d_sum; a.feat = d_feat; a.rows = d_rows; a.out = d_out; a.ws = d_ws;
    return a;
}

// Enqueue one denoise on `stream`: device buffers, the arguments checked. `check_rows`: the row list came from the caller's
// HBM — its fault count is read behind one synchronisation of the stream before anything that writes the output is enqueued.
void run_denoise(const double *d_sum, const rt_feature *d_feat, const uint32_t *d_rows, const rt_denoise_params *p, double *d_out,
                 char *d_ws, hipStream_t stream, bool check_rows, const std::string &w) {
    const DenoiseArgs a = denoise_args(d_sum, d_feat, d_rows, p, d_out, d_ws);
    double inv_c[RT_DENOISE_MAX_ITER];
    for (uint32_t k = 0; k < p->n_iter; k++) {
        const double sigma_k = std::ldexp(p->sigma_color, -(int)k);
        inv_c[k] = 1.0 / (sigma_k * sigma_k);
    }
    if (d_rows) {
        RT_HIP(launch_denoise_rows(a, stream));
        if (check_rows) read_bad_rows(d_ws + denoise_layout(p->width, p->height).bad_rows, stream, w);
    }
    RT_HIP(launch_denoise(a, p->n_iter, inv_c, stream));
}

// The arguments of rt_denoise_dual*: what rt_denoise* refuses, then the dual filter's own.
void check_denoise_dual(const double *sum_a, const double *sum_b, const rt_feature *feat_a, const rt_feature *feat_b, const rt_denoise_params *p,
                        const rt_denoise_dual_params *q, const double *out, const std::string &w) {
    check_denoise(sum_a, feat_a, p, out, w);
    RT_REQUIRE(q, RT_ERR_INVALID, w + ": null dual params");
    RT_REQUIRE(sum_b && feat_b, RT_ERR_INVALID, w + ": null sums or features of the second half");
    RT_REQUIRE(q->var_iter <= RT_DENOISE_MAX_VAR_ITER, RT_ERR_INVALID, w + ": var_iter > RT_DENOISE_MAX_VAR_ITER");
    RT_REQUIRE(q->var_floor > 0.0 && !std::isinf(q->var_floor), RT_ERR_INVALID, w + ": var_floor is <= 0, NaN or infinite");
    RT_REQUIRE(q->flags == 0, RT_ERR_INVALID, w + ": dual flags must be 0");
}

// Enqueue one dual denoise on `stream`, like run_denoise.
void run_denoise_dual(const double *d_sum_a, const double *d_sum_b, const rt_feature *d_feat_a, const rt_feature *d_feat_b, const uint32_t *d_rows,
                      const rt_denoise_params *p, const rt_denoise_dual_params *q, double *d_out, double *d_out_var, char *d_ws,
                      hipStream_t stream, bool check_rows, const std::string &w) {
    DenoiseDualArgs d{};
    d.a = denoise_args(d_sum_a, d_feat_a, d_rows, p, d_out, d_ws);
    const DenoiseArgs &a = d.a;
    d.sum_b = d_sum_b; d.feat_b = d_feat_b; d.out_var = d_out_var;
    d.sp2 = a.sp + a.sp;
    d.inv_c = 1.0 / (p->sigma_color * p->sigma_color);
    d.var_floor = q->var_floor;
    if (d_rows) {
        RT_HIP(launch_denoise_dual_rows(d, stream));
        if (check_rows) read_bad_rows(d_ws + denoise_dual_layout(p->width, p->height).bad_rows, stream, w);
    }
    RT_HIP(launch_denoise_dual(d, q->var_iter, p->n_iter, stream));
}

// The arguments of rt_temporal* (host/temporal_check.hpp has the rules): the parameters, then the buffers.
void check_temporal(const double *sum, const rt_feature *feat, const uint32_t *rows, const rt_camera *cam, const rt_temporal_pixel *prev,
                    const rt_camera *prev_cam, const rt_temporal_params *p, const rt_temporal_pixel *state_out, const double *out,
                    const void *workspace, bool device, const std::string &w) {
    const char *fault = temporal_params_fault(p);
    if (!fault) fault = temporal_buffers_fault(sum, feat, rows, cam, prev, prev_cam, p, state_out, out, workspace, device);
    RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
}

// Enqueue one temporal accumulation on `stream`, like run_denoise: device buffers, the arguments checked.
void run_temporal(const double *d_sum, const rt_feature *d_feat, const uint32_t *d_rows, const rt_camera *cam, const rt_temporal_pixel *d_prev,
                  const rt_camera *prev_cam, const rt_temporal_params *p, rt_temporal_pixel *d_state, double *d_out, char *d_ws,
                  hipStream_t stream, bool check_rows, const std::string &w) {
    TemporalArgs a{};
    a.width = p->width; a.height = p->height;
    a.sp = (double)p->spp;
    a.wm1 = (double)(p->width - 1u); a.hm1 = (double)(p->height - 1u);
    a.wd = (double)p->width; a.hd = (double)p->height;
    a.tol_depth = p->tol_depth; a.tol_normal = p->tol_normal; a.n_max = p->n_max; a.w_min = p->w_min; a.albedo_floor = p->albedo_floor;
    a.demodulate = !(p->flags & RT_TEMPORAL_NO_DEMODULATE);
    a.depth_test = !std::isinf(p->tol_depth); a.normal_test = !std::isinf(p->tol_normal);
    a.far_misses = (p->flags & RT_TEMPORAL_FAR_MISSES) != 0;
    for (int k = 0; k < 3; k++) {
        a.o[k] = cam->origin[k]; a.llc[k] = cam->lower_left_corner[k]; a.hor[k] = cam->horizontal[k]; a.ver[k] = cam->vertical[k];
        if (d_prev) {
            a.po[k] = prev_cam->origin[k]; a.pr[k] = prev_cam->origin[k] - prev_cam->lower_left_corner[k];
            a.phor[k] = prev_cam->horizontal[k]; a.pver[k] = prev_cam->vertical[k];
        }
    }
    a.sum = d_sum; a.feat = d_feat; a.prev = d_prev; a.state = d_state; a.out = d_out;
    if (d_rows) {
        const TemporalLayout l = temporal_layout(p->height);
        uint32_t *const inv = reinterpret_cast<uint32_t *>(d_ws + l.inv_rows);
        RT_HIP(launch_row_list_check(d_rows, p->height, inv, reinterpret_cast<uint32_t *>(d_ws + l.bad_rows), stream));
        if (check_rows) read_bad_rows(d_ws + l.bad_rows, stream, w);
        a.inv = inv;
    }
    RT_HIP(launch_temporal(a, stream));
}

} // namespace

extern "C" {

uint64_t rt_adaptive_workspace_bytes(const rt_adaptive_params *p) {
    return adaptive_params_fault(p) ? 0 : adaptive_layout(p->width, p->height).bytes;
}

int rt_adaptive_plan_device(const double *d_err, const uint32_t *d_row_ids, const rt_adaptive_params *p, uint32_t *d_units, uint64_t *d_offsets,
                            uint64_t *d_entries, uint64_t capacity, void *d_workspace, void *hip_stream, uint64_t *out_total) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_plan_device");
        const char *fault = adaptive_params_fault(p);
        RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
        RT_REQUIRE(d_err && d_units && d_offsets, RT_ERR_INVALID, w + ": null error map, units or offsets");
        RT_REQUIRE(d_entries || capacity == 0, RT_ERR_INVALID, w + ": null entries with a capacity");
        RT_REQUIRE(d_workspace, RT_ERR_INVALID, w + ": null workspace");
        RT_REQUIRE(!(((uintptr_t)d_err | (uintptr_t)d_workspace) & 15u), RT_ERR_INVALID, w + ": the error map and the workspace must be 16-byte aligned");
        RT_REQUIRE(!(((uintptr_t)d_offsets | (uintptr_t)d_entries) & 7u), RT_ERR_INVALID, w + ": offsets and entries must be 8-byte aligned");
        RT_REQUIRE(!(((uintptr_t)d_units | (uintptr_t)d_row_ids) & 3u), RT_ERR_INVALID, w + ": units and row_ids must be 4-byte aligned");
        run_adaptive_plan(d_err, d_row_ids, p, d_units, d_offsets, d_entries, capacity, (char *)d_workspace, (hipStream_t)hip_stream, out_total, w);
        return RT_OK;
    });
}

int rt_adaptive_plan(const double *err, const uint32_t *row_ids, const rt_adaptive_params *p, uint32_t *units, uint64_t *offsets,
                     uint64_t *entries, uint64_t capacity, uint64_t *out_total) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_plan");
        const char *fault = adaptive_params_fault(p);
        RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
        RT_REQUIRE(err && units && offsets, RT_ERR_INVALID, w + ": null error map, units or offsets");
        RT_REQUIRE(entries || capacity == 0, RT_ERR_INVALID, w + ": null entries with a capacity");
        check_row_permutation(row_ids, p->height, w);
        const uint64_t n = (uint64_t)p->width * p->height;
        DeviceBuf<double> d_err(n);
        DeviceBuf<uint32_t> d_rows(row_ids ? p->height : 0), d_units(n);
        DeviceBuf<uint64_t> d_offsets(n + 1), d_entries(capacity);
        DeviceBuf<char> d_ws(adaptive_layout(p->width, p->height).bytes);
        RT_HIP(hipMemcpy(d_err, err, n * sizeof(double), hipMemcpyHostToDevice));
        if (row_ids) RT_HIP(hipMemcpy(d_rows, row_ids, p->height * sizeof(uint32_t), hipMemcpyHostToDevice));
        uint64_t total = 0;
        run_adaptive_plan(d_err, row_ids ? d_rows.p : nullptr, p, d_units, d_offsets, capacity ? d_entries.p : nullptr, capacity, d_ws, nullptr, &total, w);
        RT_HIP(hipMemcpy(units, d_units, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(offsets, d_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (total && total <= capacity) RT_HIP(hipMemcpy(entries, d_entries, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (out_total) *out_total = total;
        return RT_OK;
    });
}

int rt_adaptive_merge_device(const double *d_entry_sums, const uint32_t *d_units, const uint64_t *d_offsets, uint64_t n_pixels, uint32_t spp,
                             double *d_acc_sum, double *d_acc_n, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_merge_device");
        RT_REQUIRE(n_pixels <= RT_DENOISE_MAX_PIXELS, RT_ERR_INVALID, w + ": n_pixels > RT_DENOISE_MAX_PIXELS");
        if (n_pixels == 0) return RT_OK;
        RT_REQUIRE(d_entry_sums && d_units && d_offsets && d_acc_sum && d_acc_n, RT_ERR_INVALID, w + ": null buffer");
        RT_REQUIRE(!(((uintptr_t)d_entry_sums | (uintptr_t)d_offsets | (uintptr_t)d_acc_sum | (uintptr_t)d_acc_n) & 7u), RT_ERR_INVALID,
                   w + ": sums, offsets and accumulators must be 8-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_units & 3u), RT_ERR_INVALID, w + ": units must be 4-byte aligned");
        RT_HIP(launch_adaptive_merge(d_entry_sums, d_units, d_offsets, n_pixels, spp, d_acc_sum, d_acc_n, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

int rt_adaptive_resolve_device(const double *d_acc_sum, const double *d_acc_n, uint64_t n_pixels, uint32_t spp_out, double *d_out, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_resolve_device");
        RT_REQUIRE(n_pixels <= RT_DENOISE_MAX_PIXELS, RT_ERR_INVALID, w + ": n_pixels > RT_DENOISE_MAX_PIXELS");
        if (n_pixels == 0) return RT_OK;
        RT_REQUIRE(d_acc_sum && d_acc_n && d_out, RT_ERR_INVALID, w + ": null buffer");
        RT_REQUIRE(!(((uintptr_t)d_acc_sum | (uintptr_t)d_acc_n | (uintptr_t)d_out) & 7u), RT_ERR_INVALID, w + ": the buffers must be 8-byte aligned");
        RT_HIP(launch_adaptive_resolve(d_acc_sum, d_acc_n, n_pixels, spp_out, d_out, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

int rt_adaptive_merge_features_device(const rt_feature *d_entry_features, const uint32_t *d_units, const uint64_t *d_offsets, uint64_t n_pixels,
                                      rt_feature *d_acc, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_merge_features_device");
        RT_REQUIRE(n_pixels <= RT_DENOISE_MAX_PIXELS, RT_ERR_INVALID, w + ": n_pixels > RT_DENOISE_MAX_PIXELS");
        if (n_pixels == 0) return RT_OK;
        RT_REQUIRE(d_entry_features && d_units && d_offsets && d_acc, RT_ERR_INVALID, w + ": null buffer");
        RT_REQUIRE(!(((uintptr_t)d_entry_features | (uintptr_t)d_acc) & 15u), RT_ERR_INVALID, w + ": the records must be 16-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_offsets & 7u), RT_ERR_INVALID, w + ": offsets must be 8-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_units & 3u), RT_ERR_INVALID, w + ": units must be 4-byte aligned");
        RT_HIP(launch_adaptive_merge_features(d_entry_features, d_units, d_offsets, n_pixels, d_acc, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

int rt_adaptive_resolve_features_device(const rt_feature *d_acc, const double *d_acc_n, uint64_t n_pixels, uint32_t spp_out, rt_feature *d_out,
                                        void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_resolve_features_device");
        RT_REQUIRE(n_pixels <= RT_DENOISE_MAX_PIXELS, RT_ERR_INVALID, w + ": n_pixels > RT_DENOISE_MAX_PIXELS");
        if (n_pixels == 0) return RT_OK;
        RT_REQUIRE(d_acc && d_acc_n && d_out, RT_ERR_INVALID, w + ": null buffer");
        RT_REQUIRE(!(((uintptr_t)d_acc | (uintptr_t)d_out) & 15u), RT_ERR_INVALID, w + ": the records must be 16-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_acc_n & 7u), RT_ERR_INVALID, w + ": the sample counts must be 8-byte aligned");
        RT_HIP(launch_adaptive_resolve_features(d_acc, d_acc_n, n_pixels, spp_out, d_out, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

uint64_t rt_denoise_workspace_bytes(const rt_denoise_params *p) {
    return denoise_params_fault(p) ? 0 : denoise_layout(p->width, p->height).bytes;
}

int rt_denoise_device(const double *d_rgb_sum, const rt_feature *d_features, const uint32_t *d_row_ids, const rt_denoise_params *p,
                      double *d_out_rgb_sum, void *d_workspace, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_device");
        check_denoise(d_rgb_sum, d_features, p, d_out_rgb_sum, w);
        RT_REQUIRE(d_workspace, RT_ERR_INVALID, w + ": null workspace");
        RT_REQUIRE(!(((uintptr_t)d_rgb_sum | (uintptr_t)d_features | (uintptr_t)d_out_rgb_sum | (uintptr_t)d_workspace) & 15u), RT_ERR_INVALID,
                   w + ": the buffers and the workspace must be 16-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_row_ids & 3u), RT_ERR_INVALID, w + ": row_ids must be 4-byte aligned");
        run_denoise(d_rgb_sum, d_features, d_row_ids, p, d_out_rgb_sum, (char *)d_workspace, (hipStream_t)hip_stream, true, w);
        return RT_OK;
    });
}

int rt_denoise(const double *rgb_sum, const rt_feature *features, const uint32_t *row_ids, const rt_denoise_params *p,
               double *out_rgb_sum, double *ms) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise");
        check_denoise(rgb_sum, features, p, out_rgb_sum, w);
        check_row_permutation(row_ids, p->height, w);
        const uint64_t n = (uint64_t)p->width * p->height;
        DeviceBuf<double> d_sum(3 * n);                        // (filtered in place)
        DeviceBuf<rt_feature> d_feat(n);
        DeviceBuf<uint32_t> d_rows(row_ids ? p->height : 0);
        DeviceBuf<char> d_ws(denoise_layout(p->width, p->height).bytes);
        NullStreamTimer timer;
        RT_HIP(hipMemcpy(d_sum, rgb_sum, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_feat, features, n * sizeof(rt_feature), hipMemcpyHostToDevice));
        if (row_ids) RT_HIP(hipMemcpy(d_rows, row_ids, p->height * sizeof(uint32_t), hipMemcpyHostToDevice));
        timer.run([&] { run_denoise(d_sum, d_feat, row_ids ? d_rows.p : nullptr, p, d_sum, d_ws, nullptr, false, w); });
        RT_HIP(hipMemcpy(out_rgb_sum, d_sum, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        timer.report(ms);
        return RT_OK;
    });
}

uint64_t rt_denoise_dual_workspace_bytes(const rt_denoise_params *p) {
    return denoise_params_fault(p) ? 0 : denoise_dual_layout(p->width, p->height).bytes;
}

int rt_denoise_dual_device(const double *d_sum_a, const double *d_sum_b, const rt_feature *d_feat_a, const rt_feature *d_feat_b,
                           const uint32_t *d_row_ids, const rt_denoise_params *p, const rt_denoise_dual_params *q, double *d_out_rgb_sum,
                           double *d_out_variance, void *d_workspace, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_dual_device");
        check_denoise_dual(d_sum_a, d_sum_b, d_feat_a, d_feat_b, p, q, d_out_rgb_sum, w);
        RT_REQUIRE(d_workspace, RT_ERR_INVALID, w + ": null workspace");
        RT_REQUIRE(!(((uintptr_t)d_sum_a | (uintptr_t)d_sum_b | (uintptr_t)d_feat_a | (uintptr_t)d_feat_b | (uintptr_t)d_out_rgb_sum |
                      (uintptr_t)d_out_variance | (uintptr_t)d_workspace) & 15u),
                   RT_ERR_INVALID, w + ": the buffers and the workspace must be 16-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_row_ids & 3u), RT_ERR_INVALID, w + ": row_ids must be 4-byte aligned");
        run_denoise_dual(d_sum_a, d_sum_b, d_feat_a, d_feat_b, d_row_ids, p, q, d_out_rgb_sum, d_out_variance, (char *)d_workspace,
                         (hipStream_t)hip_stream, true, w);
        return RT_OK;
    });
}

int rt_denoise_dual(const double *sum_a, const double *sum_b, const rt_feature *feat_a, const rt_feature *feat_b, const uint32_t *row_ids,
                    const rt_denoise_params *p, const rt_denoise_dual_params *q, double *out_rgb_sum, double *out_variance, double *ms) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_dual");
        check_denoise_dual(sum_a, sum_b, feat_a, feat_b, p, q, out_rgb_sum, w);
        check_row_permutation(row_ids, p->height, w);
        const uint64_t n = (uint64_t)p->width * p->height;
        DeviceBuf<double> d_a(3 * n), d_b(3 * n);              // (A is filtered in place)
        DeviceBuf<rt_feature> d_fa(n), d_fb(n);
        DeviceBuf<double> d_var(out_variance ? n : 0);
        DeviceBuf<uint32_t> d_rows(row_ids ? p->height : 0);
        DeviceBuf<char> d_ws(denoise_dual_layout(p->width, p->height).bytes);
        NullStreamTimer timer;
        RT_HIP(hipMemcpy(d_a, sum_a, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_b, sum_b, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_fa, feat_a, n * sizeof(rt_feature), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_fb, feat_b, n * sizeof(rt_feature), hipMemcpyHostToDevice));
        if (row_ids) RT_HIP(hipMemcpy(d_rows, row_ids, p->height * sizeof(uint32_t), hipMemcpyHostToDevice));
        timer.run([&] { run_denoise_dual(d_a, d_b, d_fa, d_fb, row_ids ? d_rows.p : nullptr, p, q, d_a, out_variance ? d_var.p : nullptr, d_ws, nullptr, false, w); });
        RT_HIP(hipMemcpy(out_rgb_sum, d_a, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        if (out_variance) RT_HIP(hipMemcpy(out_variance, d_var, n * sizeof(double), hipMemcpyDeviceToHost));
        timer.report(ms);
        return RT_OK;
    });
}

uint64_t rt_temporal_workspace_bytes(const rt_temporal_params *p) {
    return temporal_params_fault(p) ? 0 : temporal_layout(p->height).bytes;
}

int rt_temporal_device(const double *d_rgb_sum, const rt_feature *d_features, const uint32_t *d_row_ids, const rt_camera *cam,
                       const rt_temporal_pixel *d_prev, const rt_camera *prev_cam, const rt_temporal_params *p, rt_temporal_pixel *d_state_out,
                       double *d_out_rgb_sum, void *d_workspace, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_temporal_device");
        check_temporal(d_rgb_sum, d_features, d_row_ids, cam, d_prev, prev_cam, p, d_state_out, d_out_rgb_sum, d_workspace, true, w);
        run_temporal(d_rgb_sum, d_features, d_row_ids, cam, d_prev, prev_cam, p, d_state_out, d_out_rgb_sum, (char *)d_workspace,
                     (hipStream_t)hip_stream, true, w);
        return RT_OK;
    });
}

int rt_temporal(const double *rgb_sum, const rt_feature *features, const uint32_t *row_ids, const rt_camera *cam, const rt_temporal_pixel *prev,
                const rt_camera *prev_cam, const rt_temporal_params *p, rt_temporal_pixel *state_out, double *out_rgb_sum, double *ms) {
    return guarded([&]() -> int {
        const std::string w("rt_temporal");
        check_temporal(rgb_sum, features, row_ids, cam, prev, prev_cam, p, state_out, out_rgb_sum, nullptr, false, w);
        check_row_permutation(row_ids, p->height, w);
        const uint64_t n = (uint64_t)p->width * p->height;
        DeviceBuf<double> d_sum(3 * n);                        // (accumulated in place)
        DeviceBuf<rt_feature> d_feat(n);
        DeviceBuf<rt_temporal_pixel> d_prev(prev ? n : 0), d_state(n);
        DeviceBuf<uint32_t> d_rows(row_ids ? p->height : 0);
        DeviceBuf<char> d_ws(temporal_layout(p->height).bytes);
        NullStreamTimer timer;
        RT_HIP(hipMemcpy(d_sum, rgb_sum, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_feat, features, n * sizeof(rt_feature), hipMemcpyHostToDevice));
        if (prev) RT_HIP(hipMemcpy(d_prev, prev, n * sizeof(rt_temporal_pixel), hipMemcpyHostToDevice));
        if (row_ids) RT_HIP(hipMemcpy(d_rows, row_ids, p->height * sizeof(uint32_t), hipMemcpyHostToDevice));
        timer.run([&] { run_temporal(d_sum, d_feat, row_ids ? d_rows.p : nullptr, cam, prev ? d_prev.p : nullptr, prev_cam, p, d_state, d_sum, d_ws, nullptr, false, w); });
        RT_HIP(hipMemcpy(out_rgb_sum, d_sum, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(state_out, d_state, n * sizeof(rt_temporal_pixel), hipMemcpyDeviceToHost));
        timer.report(ms);
        return RT_OK;
    });
}

} // extern "C"
