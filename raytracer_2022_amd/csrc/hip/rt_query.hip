// rt_query.hip — the closest-hit calls on a device scene: ray queries (rt_intersect*, and rt_intersect_ordered*: the same
// launch between a gather and a scatter of pt_order.hip) and feature buffers (rt_features*,
// rt_features_pixels*, rt_features_rays*: first-hit records, and with RT_FLAG_SPECULAR the records behind glass and mirrors).
#include "pt_order.hpp"
#include "rt_internal.hpp"

using namespace rt2022;

namespace {

// The scratch of `stream` in sc->qs or sc->fs.
QueryScratch &scratch_for(rt_scene *sc, std::map<hipStream_t, std::unique_ptr<QueryScratch>> &of, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(sc->qmu);
    std::unique_ptr<QueryScratch> &q = of[stream];
    if (!q) q.reset(new QueryScratch());                   // (stored once it is complete, or not at all)
    return *q;
}

// One closest-hit call on `stream`, q locked: the counters reset, `launch()` — the kernel, on q.counter and, with `counters`,
// q.stats — and with stats the wait for it and what read_stats makes of it.
template <class Launch>
void run_counted(QueryScratch &q, bool counters, hipStream_t stream, rt_stats *stats, Launch launch) {
    RT_HIP(hipMemsetAsync(q.counter, 0, sizeof(unsigned long long), stream));
    if (counters) RT_HIP(hipMemsetAsync(q.stats, 0, sizeof(StatsDev), stream));
    if (stats) RT_HIP(hipEventRecord(q.ev0, stream));
    RT_HIP(launch());
    if (!stats) return;
    RT_HIP(hipEventRecord(q.ev1, stream));
    RT_HIP(hipStreamSynchronize(stream));
    StatsDev h;
    *stats = read_stats(q.ev0, q.ev1, counters ? q.stats.p : nullptr, h);
}

// The arguments of a query: what can be said without looking into the scene ...
void check_query_args(const rt_scene *scene, const void *rays, uint64_t n_rays, uint32_t flags, const void *hits, const char *who) {
    RT_REQUIRE(scene, RT_ERR_INVALID, std::string(who) + ": null scene");
    RT_REQUIRE(n_rays == 0 || (rays && hits), RT_ERR_INVALID, std::string(who) + ": null ray or hit buffer");
    RT_REQUIRE(!(flags & ~(RT_FLAG_COUNTERS | RT_FLAG_ANY_HIT)), RT_ERR_INVALID, std::string(who) + ": unknown flag bits");
}

// ... and what the scene has to say to the flags.
void check_query_scene(const rt_scene *scene, uint32_t flags, const char *who) {
    RT_REQUIRE(!(flags & RT_FLAG_ANY_HIT) || scene->dev.n_media == 0, RT_ERR_UNSUPPORTED,
               std::string(who) + ": RT_FLAG_ANY_HIT on a scene with a ConstantMedium (its verdict depends on the closest hit so far)");
}

void check_query(const rt_scene *scene, const void *rays, uint64_t n_rays, uint32_t flags, const void *hits, const char *who) {
    check_query_args(scene, rays, n_rays, flags, hits, who);
    check_query_scene(scene, flags, who);
}

// Enqueue one query on `stream` (the scene's device is current); with stats, wait for it and fill them.
void run_query(rt_scene *sc, const rt_query_ray *d_rays, uint64_t n_rays, uint32_t flags, rt_hit *d_hits, hipStream_t stream,
               rt_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_rays == 0) return;
    QueryScratch &q = scratch_for(sc, sc->qs, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    const bool counters = stats && (flags & RT_FLAG_COUNTERS);
    const QueryArgs a{d_rays, d_hits, n_rays, q.counter, counters ? q.stats.p : nullptr};
    run_counted(q, counters, stream, stats, [&] { return launch_query(sc->dev, a, sc->stack_need, counters, (flags & RT_FLAG_ANY_HIT) != 0, stream); });
    if (stats) stats->rays = n_rays;               // (a query counts no paths, rays or light tests of its own)
}

// The arguments of rt_intersect_ordered_device (host side only; the scene is looked into last, so that a bad argument is
// reported as such whatever the scene).
void check_ordered(const rt_scene *scene, const void *d_rays, const void *d_order, uint64_t n_rays, uint32_t flags, const void *d_hits,
                   const void *ws, uint64_t ws_bytes, const char *who) {
    check_query_args(scene, d_rays, n_rays, flags, d_hits, who);
    RT_REQUIRE(n_rays < kOrderMaxRays, RT_ERR_INVALID, std::string(who) + ": n_rays must be below 2^32 (an order entry is 32 bits)");
    const char *fault = n_rays ? order_buffers_fault(d_rays, d_order, d_hits, true, ws, ws_bytes, ordered_layout(n_rays).bytes) : nullptr;
    RT_REQUIRE(!fault, RT_ERR_INVALID, std::string(who) + ": " + (fault ? fault : ""));
    check_query_scene(scene, flags, who);
}

// run_query in the order of d_order (n_rays > 0): the rays gathered into the workspace, the query kernel on the gathered
// buffer, the records scattered back — all three between the call's two events.
void run_query_ordered(rt_scene *sc, const rt_query_ray *d_rays, const uint32_t *d_order, uint64_t n_rays, uint32_t flags, rt_hit *d_hits,
                       char *ws, hipStream_t stream, rt_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    const OrderedLayout l = ordered_layout(n_rays);
    rt_query_ray *g_rays = reinterpret_cast<rt_query_ray *>(ws + l.rays);
    rt_hit *g_hits = reinterpret_cast<rt_hit *>(ws + l.hits);
    unsigned long long *d_valid = stats ? reinterpret_cast<unsigned long long *>(ws + l.valid) : nullptr;
    QueryScratch &q = scratch_for(sc, sc->qs, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    const bool counters = stats && (flags & RT_FLAG_COUNTERS);
    const QueryArgs a{g_rays, g_hits, n_rays, q.counter, counters ? q.stats.p : nullptr};
    if (d_valid) RT_HIP(hipMemsetAsync(d_valid, 0, sizeof *d_valid, stream));
    run_counted(q, counters, stream, stats, [&] {
        hipError_t e = launch_order_gather(d_rays, d_order, n_rays, g_rays, d_valid, stream);
        if (e == hipSuccess) e = launch_query(sc->dev, a, sc->stack_need, counters, (flags & RT_FLAG_ANY_HIT) != 0, stream);
        if (e == hipSuccess) e = launch_order_scatter(g_hits, d_order, n_rays, d_hits, stream);
        return e;
    });
    if (stats) {                                   // (run_counted has synchronised the stream)
        unsigned long long valid = 0;
        RT_HIP(hipMemcpy(&valid, d_valid, sizeof valid, hipMemcpyDeviceToHost));
        stats->rays = valid;
    }
}

// The flag bits the six feature calls take, and the two checks they share.
constexpr uint32_t kFeatureFlags = RT_FLAG_COUNTERS | RT_FLAG_SURFACES | RT_FLAG_SPECULAR;

void require_feature_flags(uint32_t flags, const std::string &w) {
    RT_REQUIRE(!(flags & ~kFeatureFlags), RT_ERR_INVALID, w + ": flag bits other than RT_FLAG_COUNTERS | RT_FLAG_SURFACES | RT_FLAG_SPECULAR");
}

void require_feature_out_aligned(const void *d_out, const std::string &w) {
    RT_REQUIRE(!((uintptr_t)d_out & 15u), RT_ERR_INVALID, w + ": the output must be 16-byte aligned");
}

// paths and rays of a feature call of n samples. First-hit records: one camera path, one world.hit per sample; the kernel counts
// neither. RT_FLAG_SPECULAR: a sample has a segment per vertex it follows — rays is what the counter instance counted (read_stats
// put it there), 0 without counters.
void fill_feature_paths(rt_stats *stats, uint64_t n_samples, bool specular) {
    if (!stats) return;
    stats->paths = n_samples;
    if (!specular) stats->rays = n_samples;
}

// The arguments of rt_features* (host side only; the scene comes last so that a bad argument is reported as such whatever
// the scene). `device`: rows and output are rt_features_device's — the rows are range-checked on the device later.
void check_features(const rt_scene *scene, const rt_camera *cam, const rt_params *p, const void *out, bool device, const char *who) {
    const std::string w(who);
    RT_REQUIRE(p, RT_ERR_INVALID, w + ": null params");
    RT_REQUIRE(cam, RT_ERR_INVALID, w + ": null camera");
    require_feature_flags(p->flags, w);
    check_view(cam, p, w + ": ", " (width, height or n_frames is 0)");
    const bool need_rows = p->n_rows > 0 && p->spp > 0;
    RT_REQUIRE(p->n_rows == 0 || out, RT_ERR_INVALID, w + ": null output");
    RT_REQUIRE(!need_rows || p->row_ids, RT_ERR_INVALID, w + ": null row_ids");
    RT_REQUIRE((uint64_t)p->n_rows * p->width <= (1ull << 40), RT_ERR_INVALID, w + ": n_rows * width too large");
    if (device) {
        if (p->n_rows > 0) require_feature_out_aligned(out, w);
        RT_REQUIRE(!need_rows || !((uintptr_t)p->row_ids & 3u), RT_ERR_INVALID, w + ": row_ids must be 4-byte aligned");
    } else if (need_rows) {
        for (uint32_t i = 0; i < p->n_rows; i++)
            RT_REQUIRE(p->row_ids[i] < (uint64_t)p->height * p->n_frames, RT_ERR_INVALID, w + ": row id out of range");
    }
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
}

// Enqueue one feature call on `stream` (the scene's device is current, the arguments checked); with stats, wait for it and
// fill them. `check_rows`: the row ids came from the caller's HBM — range-check them first (one synchronisation of the stream).
void run_features(rt_scene *sc, const rt_camera *cam, const rt_params *p, const uint32_t *d_rows, rt_feature *d_out,
                  hipStream_t stream, rt_stats *stats, bool check_rows, const char *who) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    const uint64_t n_pixels = (uint64_t)p->n_rows * p->width;
    if (n_pixels == 0) return;
    if (p->spp == 0) {                                     // no sample: zeros, no kernel
        RT_HIP(hipMemsetAsync(d_out, 0, n_pixels * sizeof(rt_feature), stream));
        if (stats) RT_HIP(hipStreamSynchronize(stream));
        return;
    }
    QueryScratch &q = scratch_for(sc, sc->fs, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    if (check_rows) {
        q.rows.begin(d_rows, p->n_rows, (uint64_t)p->height * p->n_frames, stream);
        RT_HIP(hipStreamSynchronize(stream));
        q.rows.end(who, ": row id out of range");
    }
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    FeatureArgs a{};
    a.cam = *cam;
    a.width = p->width; a.height = p->height; a.spp = p->spp; a.n_rows = p->n_rows;
    std::memcpy(a.background, p->background, sizeof a.background);
    a.t_min = p->t_min;
    a.seed = p->seed;
    a.n_pixels = n_pixels;
    a.row_ids = d_rows;
    a.out = d_out;
    a.counter = q.counter;
    a.stats = counters ? q.stats.p : nullptr;
    const bool surfaces = (p->flags & RT_FLAG_SURFACES) != 0, specular = (p->flags & RT_FLAG_SPECULAR) != 0;
    run_counted(q, counters, stream, stats, [&] { return launch_features(sc->dev, a, sc->stack_need, counters, surfaces, specular, stream); });
    fill_feature_paths(stats, n_pixels * p->spp, specular);
}

// The arguments of rt_features_pixels* (host side only, the scene last, like check_features). `device`: ids and output are
// rt_features_pixels_device's — the ids are range-checked on the device later.
void check_features_pixels(const rt_scene *scene, const rt_camera *cam, const rt_params *p, const uint64_t *ids, uint64_t n_entries,
                           const void *out, bool device, const char *who) {
    const std::string w(who);
    RT_REQUIRE(p, RT_ERR_INVALID, w + ": null params");
    RT_REQUIRE(cam, RT_ERR_INVALID, w + ": null camera");
    require_feature_flags(p->flags, w);
    check_view(cam, p, w + ": ", " (width, height or n_frames is 0)");
    RT_REQUIRE(n_entries == 0 || (ids && out), RT_ERR_INVALID, w + ": null id or output buffer");
    RT_REQUIRE(n_entries <= (1ull << 40), RT_ERR_INVALID, w + ": n_entries too large");
    if (device) {
        RT_REQUIRE(n_entries == 0 || !((uintptr_t)ids & 7u), RT_ERR_INVALID, w + ": the id buffer must be 8-byte aligned");
        if (n_entries > 0) require_feature_out_aligned(out, w);
    } else {
        const uint64_t limit = (uint64_t)p->width * p->height * p->n_frames;      // (check_view: height * n_frames fits 32 bits)
        for (uint64_t i = 0; i < n_entries; i++)
            RT_REQUIRE(ids[i] < limit, RT_ERR_INVALID, w + ": pixel id out of range (>= width * height * n_frames)");
    }
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
}

// Enqueue one pixel-list feature call on `stream`, like run_features (n_entries > 0). `check_ids`: the ids came from the caller's
// HBM — range-check them first (one synchronisation of the stream), whatever becomes of the list: a refused call has enqueued
// nothing that writes the output.
void run_features_pixels(rt_scene *sc, const rt_camera *cam, const rt_params *p, const uint64_t *d_ids, uint64_t n_entries, rt_feature *d_out,
                         hipStream_t stream, rt_stats *stats, bool check_ids, const char *who) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    const uint64_t limit = (uint64_t)p->width * p->height * p->n_frames;
    QueryScratch &q = scratch_for(sc, sc->fs, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    if (check_ids) {
        q.pixels.begin(d_ids, n_entries, limit, stream);
        RT_HIP(hipStreamSynchronize(stream));
        q.pixels.end(who, ": pixel id out of range (>= width * height * n_frames)");
    }
    if (p->spp == 0) {                                     // no sample: zeros, no kernel
        RT_HIP(hipMemsetAsync(d_out, 0, n_entries * sizeof(rt_feature), stream));
        if (stats) RT_HIP(hipStreamSynchronize(stream));
        return;
    }
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    FeatureArgs a{};
    a.cam = *cam;
    a.width = p->width; a.height = p->height; a.spp = p->spp;
    a.ids32 = limit <= 0xFFFFFFFFull ? 1u : 0u;
    std::memcpy(a.background, p->background, sizeof a.background);
    a.t_min = p->t_min;
    a.seed = p->seed;
    a.n_pixels = n_entries;
    a.out = d_out;
    a.counter = q.counter;
    a.stats = counters ? q.stats.p : nullptr;
    const bool surfaces = (p->flags & RT_FLAG_SURFACES) != 0, specular = (p->flags & RT_FLAG_SPECULAR) != 0;
    a.pixel_ids = d_ids;
    run_counted(q, counters, stream, stats, [&] { return launch_features_pixels(sc->dev, a, sc->stack_need, counters, surfaces, specular, stream); });
    fill_feature_paths(stats, n_entries * p->spp, specular);
}

// The arguments of rt_features_rays* (host side only, the scene last, like check_features). `device`: rays and output are
// rt_features_rays_device's. Ray contents are never looked at.
void check_features_rays(const rt_scene *scene, const void *rays, uint64_t n_rays, const rt_radiance_params *p, const void *out, bool device,
                         const char *who) {
    const std::string w(who);
    RT_REQUIRE(p, RT_ERR_INVALID, w + ": null params");
    require_feature_flags(p->flags, w);
    RT_REQUIRE(n_rays == 0 || (rays && out), RT_ERR_INVALID, w + ": null ray or output buffer");
    RT_REQUIRE(n_rays <= (1ull << 40), RT_ERR_INVALID, w + ": n_rays too large");
    if (device && n_rays > 0) {
        RT_REQUIRE(!((uintptr_t)rays & 15u), RT_ERR_INVALID, w + ": the ray buffer must be 16-byte aligned");
        require_feature_out_aligned(out, w);
    }
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
}

// Enqueue one ray-list feature call on `stream`, like run_features (n_rays > 0). Nothing to check on the device: without stats
// nothing here waits for the stream.
void run_features_rays(rt_scene *sc, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *p, rt_feature *d_out,
                       hipStream_t stream, rt_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (p->spp == 0) {                                     // no sample: zeros, no kernel
        RT_HIP(hipMemsetAsync(d_out, 0, n_rays * sizeof(rt_feature), stream));
        if (stats) RT_HIP(hipStreamSynchronize(stream));
        return;
    }
    QueryScratch &q = scratch_for(sc, sc->fs, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    FeatureArgs a{};                                       // (cam, width, height and seed: unused by the ray source)
    a.spp = p->spp;
    std::memcpy(a.background, p->background, sizeof a.background);
    a.t_min = p->t_min;
    a.n_pixels = n_rays;
    a.rays = d_rays;
    a.out = d_out;
    a.counter = q.counter;
    a.stats = counters ? q.stats.p : nullptr;
    const bool surfaces = (p->flags & RT_FLAG_SURFACES) != 0, specular = (p->flags & RT_FLAG_SPECULAR) != 0;
    run_counted(q, counters, stream, stats, [&] { return launch_features_rays(sc->dev, a, sc->stack_need, counters, surfaces, specular, stream); });
    fill_feature_paths(stats, n_rays * p->spp, specular);
}

} // namespace

extern "C" {

int rt_intersect(rt_scene *scene, const rt_query_ray *rays, uint64_t n_rays, uint32_t flags, rt_hit *out_hits, rt_stats *stats) {
    return guarded([&]() -> int {
        check_query(scene, rays, n_rays, flags, out_hits, "rt_intersect");
        if (n_rays == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        RT_REQUIRE(n_rays <= (1ull << 40), RT_ERR_INVALID, "rt_intersect: n_rays too large");
        DeviceGuard guard(scene->device);
        DeviceBuf<rt_query_ray> d_rays(n_rays);                // (after the guard: freed with the scene's device current)
        DeviceBuf<rt_hit> d_hits(n_rays);
        RT_HIP(hipMemcpy(d_rays, rays, n_rays * sizeof(rt_query_ray), hipMemcpyHostToDevice));
        run_query(scene, d_rays, n_rays, flags, d_hits, nullptr, stats);
        RT_HIP(hipMemcpy(out_hits, d_hits, n_rays * sizeof(rt_hit), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_intersect_device(rt_scene *scene, const rt_query_ray *d_rays, uint64_t n_rays, uint32_t flags, rt_hit *d_out_hits,
                        void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_query(scene, d_rays, n_rays, flags, d_out_hits, "rt_intersect_device");
        RT_REQUIRE(n_rays == 0 || !(((uintptr_t)d_rays | (uintptr_t)d_out_hits) & 15u), RT_ERR_INVALID,
                   "rt_intersect_device: ray and hit buffers must be 16-byte aligned");
        if (n_rays == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        run_query(scene, d_rays, n_rays, flags, d_out_hits, (hipStream_t)hip_stream, stats);
        return RT_OK;
    });
}

uint64_t rt_intersect_ordered_workspace_bytes(uint64_t n_rays) {
    return ordered_layout(n_rays).bytes;
}

int rt_intersect_ordered_device(rt_scene *scene, const rt_query_ray *d_rays, const uint32_t *d_order, uint64_t n_rays, uint32_t flags,
                                rt_hit *d_out_hits, void *d_workspace, uint64_t workspace_bytes, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_ordered(scene, d_rays, d_order, n_rays, flags, d_out_hits, d_workspace, workspace_bytes, "rt_intersect_ordered_device");
        if (n_rays == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        run_query_ordered(scene, d_rays, d_order, n_rays, flags, d_out_hits, (char *)d_workspace, (hipStream_t)hip_stream, stats);
        return RT_OK;
    });
}

int rt_intersect_ordered(rt_scene *scene, const rt_query_ray *rays, const uint32_t *order, const rt_ray_order_params *p, uint64_t n_rays,
                         uint32_t flags, rt_hit *out_hits, rt_stats *stats) {
    return guarded([&]() -> int {
        const std::string w("rt_intersect_ordered");
        check_query_args(scene, rays, n_rays, flags, out_hits, w.c_str());
        RT_REQUIRE(n_rays < kOrderMaxRays, RT_ERR_INVALID, w + ": n_rays must be below 2^32 (an order entry is 32 bits)");
        if (!order) {
            const char *fault = order_params_fault(n_rays, p);
            if (!fault && p->ray_stride != sizeof(rt_query_ray)) fault = "ray_stride must be 80 (rt_query_ray)";
            RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
        }
        check_query_scene(scene, flags, w.c_str());
        if (n_rays == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        DeviceBuf<rt_query_ray> d_rays(n_rays);                // (after the guard: freed with the scene's device current)
        DeviceBuf<rt_hit> d_hits(n_rays);
        DeviceBuf<uint32_t> d_order(n_rays);
        DeviceBuf<char> d_ws(ordered_layout(n_rays).bytes);
        RT_HIP(hipMemcpy(d_rays, rays, n_rays * sizeof(rt_query_ray), hipMemcpyHostToDevice));
        // (the caller's records go up first: the record of a ray that no entry names comes back as it was)
        RT_HIP(hipMemcpy(d_hits, out_hits, n_rays * sizeof(rt_hit), hipMemcpyHostToDevice));
        if (order) {
            RT_HIP(hipMemcpy(d_order, order, n_rays * sizeof(uint32_t), hipMemcpyHostToDevice));
        } else {
            DeviceBuf<char> d_order_ws(order_layout(n_rays).bytes);
            launch_ray_order(OrderArgs{(const char *)d_rays.p, n_rays, *p, d_order, d_order_ws}, nullptr);
            RT_HIP(hipStreamSynchronize(nullptr));             // (the ordering's workspace dies here)
        }
        run_query_ordered(scene, d_rays, d_order, n_rays, flags, d_hits, d_ws, nullptr, stats);
        RT_HIP(hipMemcpy(out_hits, d_hits, n_rays * sizeof(rt_hit), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_features(rt_scene *scene, const rt_camera *cam, const rt_params *params, rt_feature *out_features, rt_stats *stats) {
    return guarded([&]() -> int {
        check_features(scene, cam, params, out_features, false, "rt_features");
        const uint64_t n_pixels = (uint64_t)params->n_rows * params->width;
        if (n_pixels == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        if (params->spp == 0) {                                // zeros, and nothing for the device to do
            if (stats) std::memset(stats, 0, sizeof *stats);
            std::memset(out_features, 0, n_pixels * sizeof(rt_feature));
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        DeviceBuf<uint32_t> d_rows(params->n_rows);            // (after the guard: freed with the scene's device current)
        DeviceBuf<rt_feature> d_out(n_pixels);
        RT_HIP(hipMemcpy(d_rows, params->row_ids, params->n_rows * sizeof(uint32_t), hipMemcpyHostToDevice));
        // Poison the output so an unwritten record cannot pass for a result.
        RT_HIP(hipMemset(d_out, 0xFF, n_pixels * sizeof(rt_feature)));
        run_features(scene, cam, params, d_rows, d_out, nullptr, stats, false, "rt_features");
        RT_HIP(hipMemcpy(out_features, d_out, n_pixels * sizeof(rt_feature), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_features_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, rt_feature *d_out_features, void *hip_stream,
                       rt_stats *stats) {
    return guarded([&]() -> int {
        check_features(scene, cam, params, d_out_features, true, "rt_features_device");
        if ((uint64_t)params->n_rows * params->width == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        run_features(scene, cam, params, params->row_ids, d_out_features, (hipStream_t)hip_stream, stats, true, "rt_features_device");
        return RT_OK;
    });
}

int rt_features_pixels(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *pixel_ids, uint64_t n_entries,
                       rt_feature *out_features, rt_stats *stats) {
    return guarded([&]() -> int {
        check_features_pixels(scene, cam, params, pixel_ids, n_entries, out_features, false, "rt_features_pixels");
        // (These early returns, here and in the device form, never read *scene: the checks above only compare the pointer with
        // null. tests/test_features_pixels_abi.py calls them with a handle that is no scene; keep it that way.)
        if (n_entries == 0 || params->spp == 0) {              // nothing, or zeros: nothing for the device to do
            if (stats) std::memset(stats, 0, sizeof *stats);
            if (n_entries) std::memset(out_features, 0, n_entries * sizeof(rt_feature));
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        DeviceBuf<uint64_t> d_ids(n_entries);                  // (after the guard: freed with the scene's device current)
        DeviceBuf<rt_feature> d_out(n_entries);
        RT_HIP(hipMemcpy(d_ids, pixel_ids, n_entries * sizeof(uint64_t), hipMemcpyHostToDevice));
        // Poison the output so an unwritten record cannot pass for a result.
        RT_HIP(hipMemset(d_out, 0xFF, n_entries * sizeof(rt_feature)));
        run_features_pixels(scene, cam, params, d_ids, n_entries, d_out, nullptr, stats, false, "rt_features_pixels");
        RT_HIP(hipMemcpy(out_features, d_out, n_entries * sizeof(rt_feature), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_features_pixels_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *d_pixel_ids, uint64_t n_entries,
                              rt_feature *d_out_features, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_features_pixels(scene, cam, params, d_pixel_ids, n_entries, d_out_features, true, "rt_features_pixels_device");
        if (n_entries == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        run_features_pixels(scene, cam, params, d_pixel_ids, n_entries, d_out_features, (hipStream_t)hip_stream, stats, true,
                            "rt_features_pixels_device");
        return RT_OK;
    });
}

int rt_features_rays(rt_scene *scene, const rt_radiance_ray *rays, uint64_t n_rays, const rt_radiance_params *p, rt_feature *out_features,
                     rt_stats *stats) {
    return guarded([&]() -> int {
        check_features_rays(scene, rays, n_rays, p, out_features, false, "rt_features_rays");
        // (These early returns never read *scene, like rt_features_pixels': tests/test_features_rays_abi.py calls them with a
        // handle that is no scene.)
        if (n_rays == 0 || p->spp == 0) {                      // nothing, or zeros: nothing for the device to do
            if (stats) std::memset(stats, 0, sizeof *stats);
            if (n_rays) std::memset(out_features, 0, n_rays * sizeof(rt_feature));
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        DeviceBuf<rt_radiance_ray> d_rays(n_rays);             // (after the guard: freed with the scene's device current)
        DeviceBuf<rt_feature> d_out(n_rays);
        RT_HIP(hipMemcpy(d_rays, rays, n_rays * sizeof(rt_radiance_ray), hipMemcpyHostToDevice));
        // Poison the output so an unwritten record cannot pass for a result.
        RT_HIP(hipMemset(d_out, 0xFF, n_rays * sizeof(rt_feature)));
        run_features_rays(scene, d_rays, n_rays, p, d_out, nullptr, stats);
        RT_HIP(hipMemcpy(out_features, d_out, n_rays * sizeof(rt_feature), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_features_rays_device(rt_scene *scene, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *p,
                            rt_feature *d_out_features, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_features_rays(scene, d_rays, n_rays, p, d_out_features, true, "rt_features_rays_device");
        if (n_rays == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        run_features_rays(scene, d_rays, n_rays, p, d_out_features, (hipStream_t)hip_stream, stats);
        return RT_OK;
    });
}

} // extern "C"
