// rt_query.hip — the closest-hit calls on a device scene: ray queries (rt_intersect*, and rt_intersect_ordered*: the same
// launch between a gather and a scatter of pt_order.hip) and feature buffers (rt_features*,
// rt_features_pixels*, rt_features_rays*: first-hit records, and with RT_FLAG_SPECULAR the records behind glass and mirrors).
// The six feature calls are one call with three sources of work items: one description of it (FeatureJob), one check of the
// arguments (check_features), one enqueue (run_features) and one staged host form (features_staged), as rt_render.hip has one
// RenderJob for its renders. Beside them the scatter step on the records of a query (rt_scatter*, pt_scatter.hip), with the same
// scratch, counting and staging.
#include <type_traits>

#include "../host/scatter_check.hpp"
#include "pt_order.hpp"
#include "pt_scatter.hpp"
#include "rt_internal.hpp"

using namespace rt2022;

namespace {

// The scratch of `stream` in sc->qs, sc->fs or sc->ss.
QueryScratch &scratch_for(rt_scene *sc, std::map<hipStream_t, std::unique_ptr<QueryScratch>> &of, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(sc->qmu);
    std::unique_ptr<QueryScratch> &q = of[stream];
    if (!q) q.reset(new QueryScratch());                   // (stored once it is complete, or not at all)
    return *q;
}

// One closest-hit or scatter call on `stream`, q locked: the counters reset, `launch()` — the kernel, on q.counter and, with
// `counters`, q.stats — and with stats the wait for it and what read_stats makes of it. `work_counter`: the kernel is a
// persistent grid that claims its work from q.counter (false: the scatter step, whose grid is sized to the batch).
template <class Launch>
void run_counted(QueryScratch &q, bool counters, hipStream_t stream, rt_stats *stats, Launch launch, bool work_counter = true) {
    if (work_counter) RT_HIP(hipMemsetAsync(q.counter, 0, sizeof(unsigned long long), stream));
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

// ---- feature buffers: one job, one check, one enqueue, one staged host form for the six calls ----

// One feature call: where its samples start — the rows of a view (kFeatRows), a list of (frame, pixel) ids of one (kFeatPixels) or
// the caller's rays (kFeatRays): `src`, with at most one of the three device pointers, that source's, and `count` rows, ids or
// rays — the view (which the ray source does not use: it stays zero), the sampling, and where the records and the stats go.
// The row and the pixel source differ at spp == 0, where the call writes zeros and launches nothing. The row call, the older
// one, then looks at nothing else: its row ids may be null or out of range. The pixel call took rt_render_pixels' rule that a
// list of ids is checked whatever becomes of it: device ids are range-checked first, and a refused call has enqueued nothing
// that writes the output. Nobody chose the difference; both are behaviour by now, and run_features keeps both.
struct FeatureJob {
    int src = kFeatRows;
    const uint32_t *d_rows = nullptr;
    const uint64_t *d_pixel_ids = nullptr;
    const rt_radiance_ray *d_rays = nullptr;
    uint64_t count = 0;
    bool check_ids = false;           // the row or pixel ids came from the caller's HBM: range-check them (IdCheck)
    const char *who = "";             // the entry point, for that check's message
    rt_camera cam{};
    uint32_t width = 0, height = 0, n_frames = 0;
    uint64_t seed = 0;
    uint32_t spp = 0, flags = 0;
    double background[3] = {0.0, 0.0, 0.0}, t_min = 0.0;
    rt_feature *d_out = nullptr;      // device: one record per pixel of the rows, per id or per ray
    rt_stats *stats = nullptr;        // host: filled by run_features (null: not wanted)
    uint64_t records() const { return src == kFeatRows ? count * width : count; }
};

// The job of a call on a view, rows or pixels (the caller adds the source's device pointer) ...
FeatureJob view_job(int src, const rt_camera *cam, const rt_params *p, uint64_t count, rt_feature *d_out, rt_stats *stats, bool check_ids,
                    const char *who) {
    FeatureJob j;
    j.src = src; j.count = count; j.check_ids = check_ids; j.who = who;
    j.cam = *cam;
    j.width = p->width; j.height = p->height; j.n_frames = p->n_frames; j.seed = p->seed;
    j.spp = p->spp; j.flags = p->flags;
    std::memcpy(j.background, p->background, sizeof j.background);
    j.t_min = p->t_min;
    j.d_out = d_out; j.stats = stats;
    return j;
}

// ... and of a call on the caller's rays: no view, and nothing to check on the device.
FeatureJob rays_job(const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *p, rt_feature *d_out, rt_stats *stats, const char *who) {
    FeatureJob j;
    j.src = kFeatRays; j.d_rays = d_rays; j.count = n_rays; j.who = who;
    j.spp = p->spp; j.flags = p->flags;
    std::memcpy(j.background, p->background, sizeof j.background);
    j.t_min = p->t_min;
    j.d_out = d_out; j.stats = stats;
    return j;
}

// FeatureArgs of `job` as the kernels take them: the one place that fills them.
FeatureArgs feature_args(const FeatureJob &job, QueryScratch &q, bool counters) {
    FeatureArgs a{};
    a.cam = job.cam;
    a.width = job.width; a.height = job.height; a.spp = job.spp;
    std::memcpy(a.background, job.background, sizeof a.background);
    a.t_min = job.t_min;
    a.seed = job.seed;
    a.n_pixels = job.records();
    switch (job.src) {                                     // (n_rows and ids32 share a word, the three pointers another)
        case kFeatRows: a.n_rows = (uint32_t)job.count; a.row_ids = job.d_rows; break;
        case kFeatPixels:
            a.ids32 = id_limit(job.d_pixel_ids, job.width, job.height, job.n_frames) <= 0xFFFFFFFFull ? 1u : 0u;
            a.pixel_ids = job.d_pixel_ids;
            break;
        default: a.rays = job.d_rays; break;
    }
    a.out = job.d_out;
    a.counter = q.counter;
    a.stats = counters ? q.stats.p : nullptr;
    return a;
}

// What the sources say where they share a rule of check_features but not its words (by src), and how their list is aligned.
struct SourceWords {
    const char *null_out, *null_in, *too_large, *in_misaligned;
    uintptr_t in_mask;
};
constexpr SourceWords kSourceWords[3] = {
    {": null output", ": null row_ids", ": n_rows * width too large", ": row_ids must be 4-byte aligned", 3u},
    {": null id or output buffer", ": null id or output buffer", ": n_entries too large", ": the id buffer must be 8-byte aligned", 7u},
    {": null ray or output buffer", ": null ray or output buffer", ": n_rays too large", ": the ray buffer must be 16-byte aligned", 15u},
};

// The arguments of the six feature calls (host side only; the scene comes last so that a bad argument is reported as such
// whatever the scene). P: rt_params — a view, with a camera, for rows (whose list and length are p's own: `in` and `count` are
// not looked at) and pixels — or rt_radiance_params for rays. `in`: the ids or rays, never read here but for host ids.
// `device`: `in` and `out` are a *_device call's — read and written in aligned pieces, the ids range-checked on the device later.
// The order of the rules is behaviour: of two faults, the one named is the one that comes first here.
template <class P>
void check_features(const rt_scene *scene, int src, const rt_camera *cam, const P *p, const void *in, uint64_t count, const void *out,
                    bool device, const char *who) {
    constexpr bool view = std::is_same<P, rt_params>::value;
    const std::string w(who);
    const SourceWords &words = kSourceWords[src];
    const bool rows = src == kFeatRows;
    RT_REQUIRE(p, RT_ERR_INVALID, w + ": null params");
    if constexpr (view) RT_REQUIRE(cam, RT_ERR_INVALID, w + ": null camera");
    RT_REQUIRE(!(p->flags & ~(RT_FLAG_COUNTERS | RT_FLAG_SURFACES | RT_FLAG_SPECULAR)), RT_ERR_INVALID,
               w + ": flag bits other than RT_FLAG_COUNTERS | RT_FLAG_SURFACES | RT_FLAG_SPECULAR");
    uint64_t records = count;
    if constexpr (view) {
        check_view(cam, p, w + ": ", " (width, height or n_frames is 0)");
        if (rows) { in = p->row_ids; count = p->n_rows; records = count * p->width; }
    }
    // (a row list is wanted only by a call that takes samples; a list of ids or rays by every call that has one)
    const bool need_in = count > 0 && (!rows || p->spp > 0);
    RT_REQUIRE(count == 0 || out, RT_ERR_INVALID, w + words.null_out);
    RT_REQUIRE(!need_in || in, RT_ERR_INVALID, w + words.null_in);
    RT_REQUIRE(records <= (1ull << 40), RT_ERR_INVALID, w + words.too_large);
    const auto out_aligned = [&] { RT_REQUIRE(count == 0 || !((uintptr_t)out & 15u), RT_ERR_INVALID, w + ": the output must be 16-byte aligned"); };
    if (device) {                                          // (the row call looks at its output first, the list calls at their list)
        if (rows) out_aligned();
        RT_REQUIRE(!need_in || !((uintptr_t)in & words.in_mask), RT_ERR_INVALID, w + words.in_misaligned);
        if (!rows) out_aligned();
    } else if constexpr (view) {
        if (need_in && rows) check_host_ids(static_cast<const uint32_t *>(in), count, p, w);
        if (need_in && !rows) check_host_ids(static_cast<const uint64_t *>(in), count, p, w);
    }
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
}

// Enqueue one feature call on `stream` (the scene's device is current, the arguments checked, there are records to write and the
// stats are zeroed); with stats, wait for it and fill them. No samples: zeros and no kernel — behind the range check of a pixel
// list, not of a row list (see FeatureJob). The ray source has nothing to check: without stats nothing here waits for the stream.
void run_features(rt_scene *sc, const FeatureJob &job, hipStream_t stream) {
    rt_stats *const stats = job.stats;
    const uint64_t n = job.records();
    const auto zeros = [&] {
        RT_HIP(hipMemsetAsync(job.d_out, 0, n * sizeof(rt_feature), stream));
        if (stats) RT_HIP(hipStreamSynchronize(stream));
    };
    if (job.spp == 0 && job.src != kFeatPixels) { zeros(); return; }
    QueryScratch &q = scratch_for(sc, sc->fs, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    q.ids.sync_and_check(job, stream, false);              // (ids from the caller's HBM: one synchronisation of the stream)
    if (job.spp == 0) { zeros(); return; }
    const bool counters = stats && (job.flags & RT_FLAG_COUNTERS);
    const bool surfaces = (job.flags & RT_FLAG_SURFACES) != 0, specular = (job.flags & RT_FLAG_SPECULAR) != 0;
    const FeatureArgs a = feature_args(job, q, counters);
    run_counted(q, counters, stream, stats, [&] { return launch_features(sc->dev, a, sc->stack_need, job.src, counters, surfaces, specular, stream); });
    // paths and rays of the call's n * spp samples. First-hit records: one camera path, one world.hit per sample; the kernel counts
    // neither. RT_FLAG_SPECULAR: a sample has a segment per vertex it follows — rays is what the counter instance counted
    // (read_stats put it there), 0 without counters.
    if (stats) {
        stats->paths = n * job.spp;
        if (!specular) stats->rays = n * job.spp;
    }
}

// A *_device call once its arguments are checked. Without records it returns before the scene is looked into (the ABI tests pass
// a handle that is no scene).
int features_device(rt_scene *scene, const FeatureJob &job, void *hip_stream) {
    if (job.stats) std::memset(job.stats, 0, sizeof *job.stats);
    if (job.records() == 0) return RT_OK;
    DeviceGuard guard(scene->device);
    run_features(scene, job, (hipStream_t)hip_stream);
    return RT_OK;
}

// The host form of a call: nothing, or zeros, with nothing for the device to do and the scene not looked into (as above); else
// `in` — job.count row ids, pixel ids or rays — goes up to where job.*source then points, run_features fills a device copy of
// the output — poisoned, so that an unwritten record cannot pass for a result — and that comes back.
template <class T>
int features_staged(rt_scene *scene, FeatureJob job, const T *FeatureJob::*source, const T *in, rt_feature *out) {
    const uint64_t n = job.records();
    if (job.stats) std::memset(job.stats, 0, sizeof *job.stats);
    if (n == 0 || job.spp == 0) {
        if (n) std::memset(out, 0, n * sizeof(rt_feature));
        return RT_OK;
    }
    DeviceGuard guard(scene->device);
    DeviceBuf<T> d_in(job.count);                              // (after the guard: freed with the scene's device current)
    DeviceBuf<rt_feature> d_out(n);
    RT_HIP(hipMemcpy(d_in, in, job.count * sizeof(T), hipMemcpyHostToDevice));
    RT_HIP(hipMemset(d_out, 0xFF, n * sizeof(rt_feature)));
    job.*source = d_in;
    job.d_out = d_out;
    run_features(scene, job, nullptr);
    RT_HIP(hipMemcpy(out, d_out, n * sizeof(rt_feature), hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- scatter: one step of ray_color on a batch of hit records ----

void check_scatter(const rt_scene *scene, const rt_scatter_params *p, const void *rays, const void *hits, const void *prev, uint64_t n,
                   const void *out_recs, const void *out_next, bool device, const char *who) {
    const char *fault = scatter_fault(scene, p, rays, hits, prev, n, out_recs, out_next, device);
    RT_REQUIRE(!fault, RT_ERR_INVALID, std::string(who) + ": " + (fault ? fault : ""));
}

// Enqueue one scatter step on `stream` (the scene's device is current, n > 0); with stats, wait for it and fill them.
void run_scatter(rt_scene *sc, const rt_query_ray *d_rays, const rt_hit *d_hits, const rt_scatter_rec *d_prev, uint64_t n,
                 const rt_scatter_params *p, rt_scatter_rec *d_recs, rt_query_ray *d_next, hipStream_t stream, rt_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    QueryScratch &q = scratch_for(sc, sc->ss, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    ScatterArgs a{};
    a.rays = d_rays; a.hits = d_hits; a.prev = d_prev; a.n = n;
    std::memcpy(a.background, p->background, sizeof a.background);
    a.t_min = p->t_min;
    a.out_recs = d_recs; a.out_next = d_next;
    a.n_materials = sc->n_materials;
    a.stats = counters ? q.stats.p : nullptr;
    run_counted(q, counters, stream, stats, [&] { return launch_scatter(sc->dev, a, counters, stream); }, false);      // (no persistent grid)
}

} // namespace

extern "C" {

int rt_scatter(rt_scene *scene, const rt_query_ray *rays, const rt_hit *hits, const rt_scatter_rec *prev, uint64_t n,
               const rt_scatter_params *p, rt_scatter_rec *out_recs, rt_query_ray *out_next_rays, rt_stats *stats) {
    return guarded([&]() -> int {
        check_scatter(scene, p, rays, hits, prev, n, out_recs, out_next_rays, false, "rt_scatter");
        if (n == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        DeviceBuf<rt_query_ray> d_rays(n), d_next(n);          // (after the guard: freed with the scene's device current)
        DeviceBuf<rt_hit> d_hits(n);
        DeviceBuf<rt_scatter_rec> d_prev(prev ? n : 1), d_recs(n);
        RT_HIP(hipMemcpy(d_rays, rays, n * sizeof(rt_query_ray), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_hits, hits, n * sizeof(rt_hit), hipMemcpyHostToDevice));
        if (prev) RT_HIP(hipMemcpy(d_prev, prev, n * sizeof(rt_scatter_rec), hipMemcpyHostToDevice));
        // (poisoned: an unwritten record cannot pass for a result)
        RT_HIP(hipMemset(d_recs, 0xFF, n * sizeof(rt_scatter_rec)));
        RT_HIP(hipMemset(d_next, 0xFF, n * sizeof(rt_query_ray)));
        run_scatter(scene, d_rays, d_hits, prev ? d_prev.p : nullptr, n, p, d_recs, d_next, nullptr, stats);
        RT_HIP(hipMemcpy(out_recs, d_recs, n * sizeof(rt_scatter_rec), hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(out_next_rays, d_next, n * sizeof(rt_query_ray), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_scatter_device(rt_scene *scene, const rt_query_ray *d_rays, const rt_hit *d_hits, const rt_scatter_rec *d_prev, uint64_t n,
                      const rt_scatter_params *p, rt_scatter_rec *d_out_recs, rt_query_ray *d_out_next_rays, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_scatter(scene, p, d_rays, d_hits, d_prev, n, d_out_recs, d_out_next_rays, true, "rt_scatter_device");
        if (n == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        run_scatter(scene, d_rays, d_hits, d_prev, n, p, d_out_recs, d_out_next_rays, (hipStream_t)hip_stream, stats);
        return RT_OK;
    });
}

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
        const char *who = "rt_features";
        check_features(scene, kFeatRows, cam, params, nullptr, 0, out_features, false, who);
        return features_staged(scene, view_job(kFeatRows, cam, params, params->n_rows, nullptr, stats, false, who), &FeatureJob::d_rows,
                               params->row_ids, out_features);
    });
}

int rt_features_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, rt_feature *d_out_features, void *hip_stream,
                       rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_features_device";
        check_features(scene, kFeatRows, cam, params, nullptr, 0, d_out_features, true, who);
        FeatureJob job = view_job(kFeatRows, cam, params, params->n_rows, d_out_features, stats, true, who);
        job.d_rows = params->row_ids;
        return features_device(scene, job, hip_stream);
    });
}

int rt_features_pixels(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *pixel_ids, uint64_t n_entries,
                       rt_feature *out_features, rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_features_pixels";
        check_features(scene, kFeatPixels, cam, params, pixel_ids, n_entries, out_features, false, who);
        return features_staged(scene, view_job(kFeatPixels, cam, params, n_entries, nullptr, stats, false, who), &FeatureJob::d_pixel_ids,
                               pixel_ids, out_features);
    });
}

int rt_features_pixels_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *d_pixel_ids, uint64_t n_entries,
                              rt_feature *d_out_features, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_features_pixels_device";
        check_features(scene, kFeatPixels, cam, params, d_pixel_ids, n_entries, d_out_features, true, who);
        FeatureJob job = view_job(kFeatPixels, cam, params, n_entries, d_out_features, stats, true, who);
        job.d_pixel_ids = d_pixel_ids;
        return features_device(scene, job, hip_stream);
    });
}

int rt_features_rays(rt_scene *scene, const rt_radiance_ray *rays, uint64_t n_rays, const rt_radiance_params *p, rt_feature *out_features,
                     rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_features_rays";
        check_features(scene, kFeatRays, nullptr, p, rays, n_rays, out_features, false, who);
        return features_staged(scene, rays_job(nullptr, n_rays, p, nullptr, stats, who), &FeatureJob::d_rays, rays, out_features);
    });
}

int rt_features_rays_device(rt_scene *scene, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *p,
                            rt_feature *d_out_features, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_features_rays_device";
        check_features(scene, kFeatRays, nullptr, p, d_rays, n_rays, d_out_features, true, who);
        return features_device(scene, rays_job(d_rays, n_rays, p, d_out_features, stats, who), hip_stream);
    });
}

} // extern "C"
