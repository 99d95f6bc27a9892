// rt_post.hip — what works on a render's buffers and takes no scene: the denoisers (rt_denoise*, rt_denoise_dual*), the
// temporal accumulation (rt_temporal*) and the adaptive-sampling planner, merge and resolve (rt_adaptive_*). What each call
// refuses and how its workspace is laid out is host/post_check.hpp's to say. A device form reads: check, run_* on the
// caller's stream. A host form: check, upload, timer.run(run_*) on the null stream, download, report.
#include <cmath>

#include "../host/post_check.hpp"
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

// The row stage of all four families: the row kernel on the call's list (null: none, nothing is enqueued) leaves its map and
// its count at `l` of the workspace. `read_count`: the list came from the caller's HBM — its count is read (read_bad_rows)
// before anything that writes an output is enqueued. Returns the map image row -> buffer row, or null.
const uint32_t *row_map(const uint32_t *d_rows, uint32_t height, char *d_ws, const RowMapLayout &l, hipStream_t stream, bool read_count,
                        const std::string &w) {
    if (!d_rows) return nullptr;
    uint32_t *const inv = reinterpret_cast<uint32_t *>(d_ws + l.inv);
    RT_HIP(launch_row_list_check(d_rows, height, inv, reinterpret_cast<uint32_t *>(d_ws + l.bad), stream));
    if (read_count) read_bad_rows(d_ws + l.bad, stream, w);
    return inv;
}

// The device time of a host form's call on the null stream: events around run(), waited for; report() once the results are back.
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

// One plan on `stream`: device buffers, the arguments checked. The kernels, then ONE synchronisation behind which the total
// and the row kernel's count are read together.
void run_adaptive_plan(const double *d_err, const uint32_t *d_rows, const rt_adaptive_params *p, uint32_t *d_units, uint64_t *d_offsets,
                       uint64_t *d_entries, uint64_t capacity, char *d_ws, hipStream_t stream, uint64_t *out_total, const std::string &w) {
    AdaptivePlanArgs a{};
    a.width = p->width; a.height = p->height; a.first_frame = p->first_frame; a.max_units = p->max_units; a.scale = p->scale;
    a.err = d_err; a.rows = d_rows; a.units = d_units; a.offsets = d_offsets; a.entries = d_entries; a.capacity = capacity; a.ws = d_ws;
    const AdaptiveLayout l = adaptive_layout(p->width, p->height);
    row_map(d_rows, p->height, d_ws, l.rows, stream, false, w);
    RT_HIP(launch_adaptive_plan(a, stream));
    unsigned long long total = 0;
    RT_HIP(hipMemcpyAsync(&total, d_ws + l.totals + l.n_tiles * sizeof(unsigned long long), sizeof total, hipMemcpyDeviceToHost, stream));
    read_bad_rows(d_rows ? d_ws + l.rows.bad : nullptr, stream, w);
    if (out_total) *out_total = total;
}

// The filter's arguments as the kernels take them (pt_device.h), from the caller's parameters and device buffers.
DenoiseArgs denoise_args(const double *d_sum, const rt_feature *d_feat, const uint32_t *d_inv, const rt_denoise_params *p, double *d_out, char *d_ws) {
    DenoiseArgs a{};
    a.width = p->width; a.height = p->height;
    a.sp = (double)p->spp;
    a.inv_n = 1.0 / (p->sigma_normal * p->sigma_normal);
    a.inv_z = 1.0 / (p->sigma_depth * p->sigma_depth);
    a.inv_a = 1.0 / (p->sigma_albedo * p->sigma_albedo);
    a.albedo_floor = p->albedo_floor;
    a.demodulate = !(p->flags & RT_DENOISE_NO_DEMODULATE);
    a.sum = d_sum; a.feat = d_feat; a.inv = d_inv; a.out = d_out; a.ws = d_ws;
    return a;
}

// Enqueue one denoise on `stream`: device buffers, the arguments checked. `check_rows`: the row list came from the caller's
// HBM (row_map's read_count).
void run_denoise(const double *d_sum, const rt_feature *d_feat, const uint32_t *d_rows, const rt_denoise_params *p, double *d_out,
                 char *d_ws, hipStream_t stream, bool check_rows, const std::string &w) {
    const uint32_t *const d_inv = row_map(d_rows, p->height, d_ws, denoise_layout(p->width, p->height).rows, stream, check_rows, w);
    const DenoiseArgs a = denoise_args(d_sum, d_feat, d_inv, p, d_out, d_ws);
    double inv_c[RT_DENOISE_MAX_ITER];
    for (uint32_t k = 0; k < p->n_iter; k++) {
        const double sigma_k = std::ldexp(p->sigma_color, -(int)k);
        inv_c[k] = 1.0 / (sigma_k * sigma_k);
    }
    RT_HIP(launch_denoise(a, p->n_iter, inv_c, stream));
}

// Enqueue one dual denoise on `stream`, like run_denoise.
void run_denoise_dual(const double *d_sum_a, const double *d_sum_b, const rt_feature *d_feat_a, const rt_feature *d_feat_b, const uint32_t *d_rows,
                      const rt_denoise_params *p, const rt_denoise_dual_params *q, double *d_out, double *d_out_var, char *d_ws,
                      hipStream_t stream, bool check_rows, const std::string &w) {
    const uint32_t *const d_inv = row_map(d_rows, p->height, d_ws, denoise_dual_layout(p->width, p->height).rows, stream, check_rows, w);
    DenoiseDualArgs d{};
    d.a = denoise_args(d_sum_a, d_feat_a, d_inv, p, d_out, d_ws);
    d.sum_b = d_sum_b; d.feat_b = d_feat_b; d.out_var = d_out_var;
    d.sp2 = d.a.sp + d.a.sp;
    d.inv_c = 1.0 / (p->sigma_color * p->sigma_color);
    d.var_floor = q->var_floor;
    RT_HIP(launch_denoise_dual(d, q->var_iter, p->n_iter, stream));
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
    a.inv = row_map(d_rows, p->height, d_ws, temporal_layout(p->height).rows, stream, check_rows, w);
    RT_HIP(launch_temporal(a, stream));
}

} // namespace

extern "C" {

uint64_t rt_adaptive_workspace_bytes(const rt_adaptive_params *p) { return adaptive_workspace_bytes(p); }

int rt_adaptive_plan_device(const double *d_err, const uint32_t *d_row_ids, const rt_adaptive_params *p, uint32_t *d_units, uint64_t *d_offsets,
                            uint64_t *d_entries, uint64_t capacity, void *d_workspace, void *hip_stream, uint64_t *out_total) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_plan_device");
        require_no_fault(adaptive_plan_buffers_fault(d_err, d_row_ids, p, d_units, d_offsets, d_entries, capacity, d_workspace, true), w);
        run_adaptive_plan(d_err, d_row_ids, p, d_units, d_offsets, d_entries, capacity, (char *)d_workspace, (hipStream_t)hip_stream, out_total, w);
        return RT_OK;
    });
}

int rt_adaptive_plan(const double *err, const uint32_t *row_ids, const rt_adaptive_params *p, uint32_t *units, uint64_t *offsets,
                     uint64_t *entries, uint64_t capacity, uint64_t *out_total) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_plan");
        require_no_fault(adaptive_plan_buffers_fault(err, row_ids, p, units, offsets, entries, capacity, nullptr, false), w);
        check_row_permutation(row_ids, p->height, w);
        const uint64_t n = (uint64_t)p->width * p->height;
        const DeviceBuf<double> d_err = uploaded(err, n);
        const DeviceBuf<uint32_t> d_rows = uploaded(row_ids, p->height), d_units(n);
        const DeviceBuf<uint64_t> d_offsets(n + 1), d_entries(capacity);
        const DeviceBuf<char> d_ws(adaptive_layout(p->width, p->height).bytes);
        uint64_t total = 0;
        run_adaptive_plan(d_err, d_rows, p, d_units, d_offsets, d_entries, capacity, d_ws, nullptr, &total, w);
        download(units, d_units, n);
        download(offsets, d_offsets, n + 1);
        if (total <= capacity) download(entries, d_entries, total);
        if (out_total) *out_total = total;
        return RT_OK;
    });
}

int rt_adaptive_merge_device(const double *d_entry_sums, const uint32_t *d_units, const uint64_t *d_offsets, uint64_t n_pixels, uint32_t spp,
                             double *d_acc_sum, double *d_acc_n, void *hip_stream) {
    return guarded([&]() -> int {
        require_no_fault(adaptive_merge_buffers_fault(d_entry_sums, d_units, d_offsets, n_pixels, d_acc_sum, d_acc_n), "rt_adaptive_merge_device");
        if (n_pixels) RT_HIP(launch_adaptive_merge(d_entry_sums, d_units, d_offsets, n_pixels, spp, d_acc_sum, d_acc_n, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

int rt_adaptive_resolve_device(const double *d_acc_sum, const double *d_acc_n, uint64_t n_pixels, uint32_t spp_out, double *d_out, void *hip_stream) {
    return guarded([&]() -> int {
        require_no_fault(adaptive_resolve_buffers_fault(d_acc_sum, d_acc_n, n_pixels, d_out), "rt_adaptive_resolve_device");
        if (n_pixels) RT_HIP(launch_adaptive_resolve(d_acc_sum, d_acc_n, n_pixels, spp_out, d_out, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

int rt_adaptive_merge_features_device(const rt_feature *d_entry_features, const uint32_t *d_units, const uint64_t *d_offsets, uint64_t n_pixels,
                                      rt_feature *d_acc, void *hip_stream) {
    return guarded([&]() -> int {
        require_no_fault(adaptive_merge_features_buffers_fault(d_entry_features, d_units, d_offsets, n_pixels, d_acc), "rt_adaptive_merge_features_device");
        if (n_pixels) RT_HIP(launch_adaptive_merge_features(d_entry_features, d_units, d_offsets, n_pixels, d_acc, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

int rt_adaptive_resolve_features_device(const rt_feature *d_acc, const double *d_acc_n, uint64_t n_pixels, uint32_t spp_out, rt_feature *d_out,
                                        void *hip_stream) {
    return guarded([&]() -> int {
        require_no_fault(adaptive_resolve_features_buffers_fault(d_acc, d_acc_n, n_pixels, d_out), "rt_adaptive_resolve_features_device");
        if (n_pixels) RT_HIP(launch_adaptive_resolve_features(d_acc, d_acc_n, n_pixels, spp_out, d_out, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

uint64_t rt_denoise_workspace_bytes(const rt_denoise_params *p) { return denoise_workspace_bytes(p); }

int rt_denoise_device(const double *d_rgb_sum, const rt_feature *d_features, const uint32_t *d_row_ids, const rt_denoise_params *p,
                      double *d_out_rgb_sum, void *d_workspace, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_device");
        require_no_fault(denoise_buffers_fault(d_rgb_sum, d_features, d_row_ids, p, d_out_rgb_sum, d_workspace, true), w);
        run_denoise(d_rgb_sum, d_features, d_row_ids, p, d_out_rgb_sum, (char *)d_workspace, (hipStream_t)hip_stream, true, w);
        return RT_OK;
    });
}

int rt_denoise(const double *rgb_sum, const rt_feature *features, const uint32_t *row_ids, const rt_denoise_params *p,
               double *out_rgb_sum, double *ms) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise");
        require_no_fault(denoise_buffers_fault(rgb_sum, features, row_ids, p, out_rgb_sum, nullptr, false), w);
        check_row_permutation(row_ids, p->height, w);
        const uint64_t n = (uint64_t)p->width * p->height;
        const DeviceBuf<double> d_sum = uploaded(rgb_sum, 3 * n);             // (filtered in place)
        const DeviceBuf<rt_feature> d_feat = uploaded(features, n);
        const DeviceBuf<uint32_t> d_rows = uploaded(row_ids, p->height);
        const DeviceBuf<char> d_ws(denoise_layout(p->width, p->height).bytes);
        NullStreamTimer timer;
        timer.run([&] { run_denoise(d_sum, d_feat, d_rows, p, d_sum, d_ws, nullptr, false, w); });
        download(out_rgb_sum, d_sum, 3 * n);
        timer.report(ms);
        return RT_OK;
    });
}

uint64_t rt_denoise_dual_workspace_bytes(const rt_denoise_params *p) { return denoise_dual_workspace_bytes(p); }

int rt_denoise_dual_device(const double *d_sum_a, const double *d_sum_b, const rt_feature *d_feat_a, const rt_feature *d_feat_b,
                           const uint32_t *d_row_ids, const rt_denoise_params *p, const rt_denoise_dual_params *q, double *d_out_rgb_sum,
                           double *d_out_variance, void *d_workspace, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_dual_device");
        require_no_fault(denoise_dual_buffers_fault(d_sum_a, d_sum_b, d_feat_a, d_feat_b, d_row_ids, p, q, d_out_rgb_sum, d_out_variance, d_workspace, true), w);
        run_denoise_dual(d_sum_a, d_sum_b, d_feat_a, d_feat_b, d_row_ids, p, q, d_out_rgb_sum, d_out_variance, (char *)d_workspace,
                         (hipStream_t)hip_stream, true, w);
        return RT_OK;
    });
}

int rt_denoise_dual(const double *sum_a, const double *sum_b, const rt_feature *feat_a, const rt_feature *feat_b, const uint32_t *row_ids,
                    const rt_denoise_params *p, const rt_denoise_dual_params *q, double *out_rgb_sum, double *out_variance, double *ms) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_dual");
        require_no_fault(denoise_dual_buffers_fault(sum_a, sum_b, feat_a, feat_b, row_ids, p, q, out_rgb_sum, out_variance, nullptr, false), w);
        check_row_permutation(row_ids, p->height, w);
        const uint64_t n = (uint64_t)p->width * p->height;
        const DeviceBuf<double> d_a = uploaded(sum_a, 3 * n), d_b = uploaded(sum_b, 3 * n);       // (A is filtered in place)
        const DeviceBuf<rt_feature> d_fa = uploaded(feat_a, n), d_fb = uploaded(feat_b, n);
        const DeviceBuf<double> d_var(out_variance ? n : 0);
        const DeviceBuf<uint32_t> d_rows = uploaded(row_ids, p->height);
        const DeviceBuf<char> d_ws(denoise_dual_layout(p->width, p->height).bytes);
        NullStreamTimer timer;
        timer.run([&] { run_denoise_dual(d_a, d_b, d_fa, d_fb, d_rows, p, q, d_a, d_var, d_ws, nullptr, false, w); });
        download(out_rgb_sum, d_a, 3 * n);
        download(out_variance, d_var, n);
        timer.report(ms);
        return RT_OK;
    });
}

uint64_t rt_temporal_workspace_bytes(const rt_temporal_params *p) { return temporal_workspace_bytes(p); }

int rt_temporal_device(const double *d_rgb_sum, const rt_feature *d_features, const uint32_t *d_row_ids, const rt_camera *cam,
                       const rt_temporal_pixel *d_prev, const rt_camera *prev_cam, const rt_temporal_params *p, rt_temporal_pixel *d_state_out,
                       double *d_out_rgb_sum, void *d_workspace, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_temporal_device");
        require_no_fault(temporal_buffers_fault(d_rgb_sum, d_features, d_row_ids, cam, d_prev, prev_cam, p, d_state_out, d_out_rgb_sum, d_workspace, true), w);
        run_temporal(d_rgb_sum, d_features, d_row_ids, cam, d_prev, prev_cam, p, d_state_out, d_out_rgb_sum, (char *)d_workspace,
                     (hipStream_t)hip_stream, true, w);
        return RT_OK;
    });
}

int rt_temporal(const double *rgb_sum, const rt_feature *features, const uint32_t *row_ids, const rt_camera *cam, const rt_temporal_pixel *prev,
                const rt_camera *prev_cam, const rt_temporal_params *p, rt_temporal_pixel *state_out, double *out_rgb_sum, double *ms) {
    return guarded([&]() -> int {
        const std::string w("rt_temporal");
        require_no_fault(temporal_buffers_fault(rgb_sum, features, row_ids, cam, prev, prev_cam, p, state_out, out_rgb_sum, nullptr, false), w);
        check_row_permutation(row_ids, p->height, w);
        const uint64_t n = (uint64_t)p->width * p->height;
        const DeviceBuf<double> d_sum = uploaded(rgb_sum, 3 * n);             // (accumulated in place)
        const DeviceBuf<rt_feature> d_feat = uploaded(features, n);
        const DeviceBuf<rt_temporal_pixel> d_prev = uploaded(prev, n), d_state(n);
        const DeviceBuf<uint32_t> d_rows = uploaded(row_ids, p->height);
        const DeviceBuf<char> d_ws(temporal_layout(p->height).bytes);
        NullStreamTimer timer;
        timer.run([&] { run_temporal(d_sum, d_feat, d_rows, cam, d_prev, prev_cam, p, d_state, d_sum, d_ws, nullptr, false, w); });
        download(out_rgb_sum, d_sum, 3 * n);
        download(state_out, d_state, n);
        timer.report(ms);
        return RT_OK;
    });
}

} // extern "C"
