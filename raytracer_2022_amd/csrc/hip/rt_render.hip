// rt_render.hip — the calls that trace paths on a device scene: renders of image rows (rt_render, rt_render_device /
// rt_render_wait, rt_render_multi), of caller rays (rt_radiance*) and of pixel lists (rt_render_pixels*), all through one
// description of a render job and one enqueue; and rt_tonemap_device. No CPU fallback exists.
#include <algorithm>
#include <cstddef>

#include "../host/plan.hpp"
#include "rt_internal.hpp"

using namespace rt2022;

namespace {

Workspace &workspace_for(rt_scene *sc, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(sc->mu);
    return sc->ws.try_emplace(stream).first->second;      // (a new one is in the map once it is complete, or not at all)
}

void check_params(const rt_scene *scene, const rt_camera *cam, const rt_params *p) {
    RT_REQUIRE(scene && cam && p, RT_ERR_INVALID, "null argument");
    RT_REQUIRE(!(p->flags & RT_FLAG_SPECULAR), RT_ERR_INVALID, "flag bits: RT_FLAG_SPECULAR is for rt_features* / rt_features_pixels* only");
    check_view(cam, p, "", "");
    RT_REQUIRE(p->n_rows == 0 || p->row_ids, RT_ERR_INVALID, "row_ids is null");
}

template <class T>
T *pool_alloc(Workspace &w, uint64_t count) {
    w.pool_owned.emplace_back((count ? count : 1) * sizeof(T));
    return (T *)w.pool_owned.back().p;
}

// (Re)allocate the wavefront pool for `blocks` workgroups and `depth` tape records.
void ensure_pool(Workspace &w, uint32_t blocks, uint32_t depth, hipStream_t stream) {
    uint32_t slots = blocks * (uint32_t)kSlotsPerBlock;
    if (depth == 0) depth = 1;
    if (!w.fx) w.fx.reset(new EngineFixed());              // (stored once it is complete, or not at all)
    if (slots <= w.pool_slots && depth <= w.pool_depth) { w.pool.n_blocks = blocks; w.pool.n_slots = w.pool_slots; return; }
    // The pool is replaced as a whole — more slots may come with a shorter tape — behind everything that may still use it.
    RT_HIP(hipStreamSynchronize(stream));
    for (int g = 0; g < kMaxGroups; g++) RT_HIP(hipStreamSynchronize(w.fx->gs.stream[g]));    // (passes of an earlier call that failed half-way)
    w.pool_owned.clear();
    w.pool_slots = 0; w.pool_depth = 0;
    if (slots < w.pool.n_slots) slots = w.pool.n_slots;
    uint64_t tape_bytes = (uint64_t)slots * depth * 4 * sizeof(double);
    RT_REQUIRE(tape_bytes <= (64ull << 30), RT_ERR_UNSUPPORTED, "max_depth too large for the bounce tape");
    uint64_t P = slots;
    WfPool &q = w.pool;
    q.n_slots = slots;
    q.n_blocks = blocks;
    q.kind = pool_alloc<uint8_t>(w, P);
    q.ray = pool_alloc<double>(w, kRecDoubles * P);                       // the 128-byte slot records: ray | hit | state
    q.hit = reinterpret_cast<uint32_t *>(q.ray) + 16;
    q.state = reinterpret_cast<uint32_t *>(q.ray) + 24;
    q.pixel_sum = pool_alloc<double>(w, 4 * P);
    q.tape = pool_alloc<double>(w, (uint64_t)depth * 4 * P);
    q.tape_cap = depth;
    q.list = pool_alloc<uint16_t>(w, P);
    q.list_n = pool_alloc<uint32_t>(w, P / (uint64_t)kSlotsPerBlock);
    q.n_active = pool_alloc<uint32_t>(w, 2 * kMaxGroups);
    q.next_chunk = pool_alloc<uint32_t>(w, kMaxGroups);
    q.max_list = pool_alloc<uint32_t>(w, 2 * kMaxGroups);
    q.fault = pool_alloc<uint32_t>(w, 1);
    q.oldest = pool_alloc<unsigned long long>(w, 2);
    q.starved_n = pool_alloc<uint32_t>(w, P / (uint64_t)kSlotsPerBlock);
    w.pool_dbg = pool_alloc<unsigned long long>(w, 8 + 2 * 65536);
    w.pool_slots = slots;
    w.pool_depth = depth;
}

// One render job: where its paths start — the rows of an image, the caller's rays (rt_radiance*) or a list of (frame, pixel) ids
// (rt_render_pixels*): at most one of the three device pointers, `count` of them — the view and the sampling the engine needs,
// and where the sums and the stats go. Everything by value: an asynchronous call's host thread keeps a copy.
struct RenderJob {
    const uint32_t *d_rows = nullptr;          // row ids of the image
    const rt_radiance_ray *d_rays = nullptr;   // one "pixel" per ray: no image (width = height = n_frames = 1), no camera, seed 0;
                                               // wavefront engine only
    const uint64_t *d_pixel_ids = nullptr;     // entries of the image's width x height x n_frames; wavefront engine only
    uint64_t count = 0;
    bool check_ids = false;           // the row or pixel ids came from the caller's HBM: range-check them (IdCheck)
    const char *who = "";             // the entry point, for that check's message
    rt_camera cam{};
    uint32_t width = 1, height = 1, n_frames = 1;
    uint32_t spp = 0, spp_chunk = 0, max_depth = 0, flags = 0;
    double background[3] = {0.0, 0.0, 0.0}, t_min = 0.0;
    uint64_t seed = 0;
    Progress progress;                // cb and user of rt_params (rows only; the engine fills in the rest)
    double *d_out = nullptr;          // device: three sums per pixel, ray or entry
    rt_stats *stats = nullptr;        // host: filled by finish (null: not wanted)
};
static_assert(sizeof(rt_radiance_ray) == 64 && offsetof(rt_radiance_ray, time) == 48 && offsetof(rt_radiance_ray, rng_state) == 56,
              "rt_radiance_ray is the path slot's ray record {ox, oy, oz, dx, dy, dz, tm, rng}: wf_shade reads it in four 16-byte pieces");

// The job of an image call, its view and sampling from `p`; its paths start from p's rows, whose ids are at `d_rows`, and report
// to p's progress callback (a pixel-list call puts its own source in their place).
RenderJob image_job(const rt_camera *cam, const rt_params *p, const uint32_t *d_rows, double *d_out, rt_stats *stats, bool check_ids, const char *who) {
    RenderJob j;
    j.cam = *cam;
    j.width = p->width; j.height = p->height; j.n_frames = p->n_frames;
    j.spp = p->spp; j.spp_chunk = p->spp_chunk; j.max_depth = p->max_depth; j.flags = p->flags;
    std::memcpy(j.background, p->background, sizeof j.background);
    j.t_min = p->t_min; j.seed = p->seed;
    j.d_out = d_out; j.stats = stats; j.check_ids = check_ids; j.who = who;
    j.d_rows = d_rows; j.count = p->n_rows; j.progress.cb = p->progress_cb; j.progress.user = p->progress_user;
    return j;
}

// The one synchronisation of `stream` a call makes before its first pass (`sync_anyway`; false: only if there is something to
// check), with the two halves of the range check of the job's device ids (IdCheck) around it: no synchronisation of their own.
void sync_and_check_ids(Workspace &w, const RenderJob &job, hipStream_t stream, bool sync_anyway) {
    w.ids.sync_and_check(job, stream, sync_anyway);
}

// RenderArgs of `job` as the kernels take them — the one place that fills them, but for the two pointers that belong to an
// engine (`tape`, `claim_limit`: its half of the enqueue sets its own). Plans the ring and makes room for the partial sums;
// *partial_bytes: their size (left alone, at 0, with one work item per pixel: the sums go straight to the output).
RenderArgs render_args(const rt_scene *sc, Workspace &w, const RenderJob &job, bool counters, hipStream_t stream, uint64_t *partial_bytes) {
    RenderArgs a{};
    a.cam = job.cam;
    a.width = job.width; a.height = job.height; a.spp = job.spp; a.max_depth = job.max_depth;
    a.n_frames = job.n_frames; a.n_rows = job.d_rows ? (uint32_t)job.count : 0u;
    const Chunks ch = plan_chunks(job.spp, job.spp_chunk);
    a.chunk = ch.chunk; a.n_chunks = ch.n_chunks;
    std::memcpy(a.background, job.background, sizeof a.background);
    a.t_min = job.t_min; a.seed = job.seed;
    a.n_pixels = job.d_rows ? job.count * job.width : job.count;
    a.n_items = a.n_pixels * a.n_chunks;
    // The partial sums' byte counts below (24 B per work item) must not wrap: a wrapped size would allocate too little and the
    // shade pass would write past it. (rt_radiance*'s own limit, RT_RADIANCE_MAX_ITEMS, keeps its calls far below this.)
    RT_REQUIRE(a.n_pixels == 0 || (a.n_items / a.n_pixels == a.n_chunks && a.n_items <= (~0ull >> 1) / (3 * sizeof(double))),
               RT_ERR_INVALID, "work items of the call overflow the partial sums' 64-bit byte counts");
    a.row_ids = job.d_rows; a.rays = job.d_rays; a.pixel_ids = job.d_pixel_ids;
    const RingPlan rp = sc->engine == 1 ? plan_ring(a.chunk, a.n_chunks, a.n_pixels, a.n_items, sc->partial_ring, sc->partial_ring_group, sc->ring_threshold_bytes)
                                        : RingPlan{};
    a.ring = rp.planes; a.ring_group = rp.group;
    a.partial = job.d_out;
    if (a.n_chunks > 1) {
        *partial_bytes = (a.ring ? (uint64_t)a.ring * a.n_pixels : a.n_items) * 3 * sizeof(double);
        w.partial.reserve(*partial_bytes / sizeof(double), &stream, 1);     // (an earlier call on the stream may still be summing the old ones)
        a.partial = w.partial;
    }
    a.tuning = tune::for_kernels(sc->tuning, sc->boxes_plain);       // (see wf_trace's fast path)
    a.vote_weights = sc->vote_weights ? sc->vote_weights : kWfVoteWeights;      // (read by the wavefront engine only)
    a.work_counter = w.work_counter;
    a.stats = counters ? w.stats.p : nullptr;
    return a;
}

// Wavefront engine: pool of path slots, shade / trace passes until it drains. Blocks until every pass has been issued and observed.
void enqueue_wavefront(rt_scene *sc, Workspace &w, const RenderJob &job, RenderArgs &a, bool counters, hipStream_t stream, CallStats &used) {
    const PoolPlan pp = plan_pool(a.n_items, (uint32_t)sc->n_cus, job.max_depth, tune::segments(sc->tuning), sc->max_pool_blocks, w.pool_slots, [] {
        size_t free_b = 0, total_b = 0;
        return hipMemGetInfo(&free_b, &total_b) == hipSuccess ? (uint64_t)free_b : ~0ull;
    });
    ensure_pool(w, pp.blocks, job.max_depth, stream);
    EngineFixed &fx = *w.fx;
    a.claim_limit = fx.d_limit;                               // (no tape of its own: the pool's)
    w.pool.segs = pp.segs;
    w.pool.n_cus = (uint32_t)sc->n_cus;
    const bool timing = tune::pass_timing(sc->tuning);
    const bool want_kt = job.stats && (job.flags & RT_FLAG_KERNEL_TIMES);
    // Groups of pool segments passing independently, each on a stream of its own: one group's shade pass then runs beside another's
    // traversal pass and fills what its stragglers leave idle. 0 in the tuning word = the library's choice: two — measured
    // (profiles/r3ze_groups.log, bench.py --groups): 1e5 random spheres +18 %, Cornell box +3 %, random spheres +1 %, book-2 final
    // +0.4 % — except for meshes (wwscene: -3 % at two, -7 % at three), which keep one.
    fx.gs.n = (int)tune::groups(sc->tuning);
    if (fx.gs.n < 1) fx.gs.n = (sc->features & kFeatMisc) ? 1 : 2;
    if (fx.gs.n > kMaxGroups) fx.gs.n = kMaxGroups;
    w.pool.dbg = timing ? w.pool_dbg : nullptr;
#if defined(RT2022_SHADE_PROBE) || defined(RT2022_TRACE_PROBE)
    w.pool.dbg = w.pool_dbg;                                  // (diagnostic builds: the section clocks of the shade / traversal kernels)
    RT_HIP(hipMemsetAsync(w.pool_dbg + 64, 0, 48 * sizeof(unsigned long long), stream));
#endif
    if (timing) for (double &t : sc->pass_timing) t = 0.0;
    RT_HIP(hipMemsetAsync(w.work_counter, 0, sizeof(unsigned long long), stream));
    if (counters) RT_HIP(hipMemsetAsync(w.stats, 0, sizeof(StatsDev), stream));
    RT_HIP(hipMemcpyAsync(fx.d_args, &a, sizeof(RenderArgs), hipMemcpyHostToDevice, stream));
    sync_and_check_ids(w, job, stream, true);          // (`a` lives on the caller's stack)
    RT_HIP(hipEventRecord(w.ev0, stream));
    WfRender r;
    r.scene = &sc->dev; r.args = &a; r.d_args = fx.d_args; r.pool = &w.pool;
    r.stack_need = sc->stack_need; r.features = sc->features; r.counters = counters;
    r.gs = &fx.gs; r.stream = stream;
    r.progress = job.progress;
    r.progress.total = a.n_pixels * job.spp; r.progress.per_item = a.chunk;
    r.ring.planes = a.ring; r.ring.out = job.d_out; r.ring.d_limit = fx.d_limit;
    // (watchdog of the ring's pass loop: a frame needs about items / slots pool fills of at most max_depth + 1 passes each)
    // (... plus one drain per ring-full of planes when the ring is small)
    r.ring.max_passes = (uint32_t)std::min<uint64_t>(1u << 26, 64 + 8 * (a.n_items / ((uint64_t)w.pool.n_blocks * kSlotsPerBlock) + 2 + (a.ring ? a.n_chunks / a.ring : 0)) *
                                                                   ((uint64_t)job.max_depth + 2));
    r.timing = timing ? sc->pass_timing : nullptr;
    r.kt = want_kt ? &w.kt : nullptr;
    if (a.n_items > 0) {
        RT_HIP(launch_render_wavefront(r));
        w.iterations = r.passes;
        RT_REQUIRE(r.fault == 0, RT_ERR_DEVICE, "wavefront engine: a path slot reached the shade pass without having been traced (internal error; the frame is incomplete)");
        if (a.n_chunks > 1 && !a.ring) RT_HIP(launch_chunk_sum(a.partial, job.d_out, a.n_pixels * 3, a.n_chunks, stream));
    }
    used.passes = w.iterations; used.slots = (uint64_t)w.pool.n_blocks * kSlotsPerBlock;
    used.kt = want_kt && a.n_items > 0;
}

// Megakernel engine (A/B): one launch of a persistent grid. Bounce tape: max_depth records of 4 doubles for every lane of it.
void enqueue_megakernel(rt_scene *sc, Workspace &w, const RenderJob &job, RenderArgs &a, bool counters, hipStream_t stream) {
    int blocks = render_grid_blocks(sc->stack_need, counters);
    uint64_t want_blocks = (a.n_items + kBlock - 1) / kBlock;
    if ((uint64_t)blocks > want_blocks) blocks = (int)(want_blocks ? want_blocks : 1);
    uint64_t tape_bytes = (uint64_t)blocks * kBlock * (uint64_t)(job.max_depth ? job.max_depth : 1) * 4 * sizeof(double);
    RT_REQUIRE(tape_bytes <= (32ull << 30), RT_ERR_UNSUPPORTED, "max_depth too large for the bounce tape");
    w.tape.reserve(tape_bytes / sizeof(double), &stream, 1);
    a.tape = w.tape;
    sync_and_check_ids(w, job, stream, false);         // (this engine enqueues without a synchronisation of its own)
    RT_HIP(hipMemsetAsync(w.work_counter, 0, sizeof(unsigned long long), stream));
    if (counters) RT_HIP(hipMemsetAsync(w.stats, 0, sizeof(StatsDev), stream));
    RT_HIP(hipEventRecord(w.ev0, stream));
    if (a.n_items > 0) {
        RT_HIP(launch_render(sc->dev, a, sc->stack_need, counters, blocks, stream));
        if (a.n_chunks > 1) RT_HIP(launch_chunk_sum(a.partial, job.d_out, a.n_pixels * 3, a.n_chunks, stream));
    }
}

// Enqueue one render job on `stream` (the scene's device is current): the job's RenderArgs, the engine's half, and what finish
// will report of the call.
void enqueue(rt_scene *sc, const RenderJob &job, hipStream_t stream) {
    Workspace &w = workspace_for(sc, stream);
    CallStats used;
    used.out = job.stats; used.counters = job.stats && (job.flags & RT_FLAG_COUNTERS);
    RenderArgs a = render_args(sc, w, job, used.counters, stream, &used.partial_bytes);
    used.chunk = a.chunk;
    if (sc->engine == 1) enqueue_wavefront(sc, w, job, a, used.counters, stream, used);
    else enqueue_megakernel(sc, w, job, a, used.counters, stream);
    RT_HIP(hipEventRecord(w.ev1, stream));
    w.pending = used;
    if (job.progress.cb) {
        // (wavefront: every pass of the frame has been issued and observed — the render is complete up to the chunk sums queued
        // behind it; the megakernel is one launch with nothing to report in between: wait for it)
        if (sc->engine != 1) RT_HIP(hipStreamSynchronize(stream));
        job.progress.cb(job.progress.user, 0u, a.n_pixels * job.spp, a.n_pixels * job.spp);
    }
}

// The arguments of rt_radiance* (host side only, before the scene is looked at: the scene comes last so that a bad argument
// is reported as such whatever the scene). `device`: the buffers are rt_radiance_device's, read and written in 16-byte pieces.
void check_radiance(const rt_scene *scene, const void *rays, uint64_t n_rays, const rt_radiance_params *p, const void *out,
                    bool device, const char *who) {
    const std::string w(who);
    RT_REQUIRE(p, RT_ERR_INVALID, w + ": null params");
    RT_REQUIRE(!(p->flags & ~(RT_FLAG_COUNTERS | RT_FLAG_KERNEL_TIMES)), RT_ERR_INVALID,
               w + ": flag bits other than RT_FLAG_COUNTERS / RT_FLAG_KERNEL_TIMES");
    RT_REQUIRE(n_rays == 0 || (rays && out), RT_ERR_INVALID, w + ": null ray or output buffer");
    RT_REQUIRE(!device || n_rays == 0 || !(((uintptr_t)rays | (uintptr_t)out) & 15u), RT_ERR_INVALID,
               w + ": ray and output buffers must be 16-byte aligned");
    RT_REQUIRE(n_rays <= RT_RADIANCE_MAX_RAYS, RT_ERR_INVALID, w + ": n_rays > RT_RADIANCE_MAX_RAYS");
    // (a division, not a product: n_rays * spp itself may not fit 64 bits)
    RT_REQUIRE(p->spp == 0 || n_rays <= RT_RADIANCE_MAX_ITEMS / p->spp, RT_ERR_INVALID, w + ": n_rays * spp > RT_RADIANCE_MAX_ITEMS");
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
    RT_REQUIRE(scene->engine == 1, RT_ERR_UNSUPPORTED, w + ": only the wavefront engine traces caller rays (rt_debug_set_engine)");
}

// The arguments of rt_render_pixels* (host side only, the scene last, like check_radiance). `device`: the buffers are
// rt_render_pixels_device's — ids read as 8-byte words, sums written in 16-byte pieces.
void check_render_pixels(const rt_scene *scene, const rt_camera *cam, const rt_params *p, const void *ids, uint64_t n_entries, const void *out,
                         bool device, const char *who) {
    const std::string w(who);
    RT_REQUIRE(cam && p, RT_ERR_INVALID, w + ": null camera or params");
    check_view(cam, p, w + ": ", "");
    RT_REQUIRE(!(p->flags & ~(RT_FLAG_COUNTERS | RT_FLAG_KERNEL_TIMES)), RT_ERR_INVALID,
               w + ": flag bits other than RT_FLAG_COUNTERS / RT_FLAG_KERNEL_TIMES");
    RT_REQUIRE(n_entries == 0 || (ids && out), RT_ERR_INVALID, w + ": null id or output buffer");
    RT_REQUIRE(!device || n_entries == 0 || !((uintptr_t)ids & 7u), RT_ERR_INVALID, w + ": the id buffer must be 8-byte aligned");
    RT_REQUIRE(!device || n_entries == 0 || !((uintptr_t)out & 15u), RT_ERR_INVALID, w + ": the output buffer must be 16-byte aligned");
    RT_REQUIRE(n_entries <= RT_RADIANCE_MAX_RAYS, RT_ERR_INVALID, w + ": n_entries > RT_RADIANCE_MAX_RAYS");
    const uint64_t n_chunks = plan_chunks(p->spp, p->spp_chunk).n_chunks;
    // (a division, not a product: n_entries * n_chunks itself may not fit 64 bits)
    RT_REQUIRE(n_entries <= RT_RADIANCE_MAX_ITEMS / n_chunks, RT_ERR_INVALID, w + ": n_entries * ceil(spp / spp_chunk) > RT_RADIANCE_MAX_ITEMS");
    if (!device) check_host_ids(static_cast<const uint64_t *>(ids), n_entries, p, w);      // (device ids: the counting kernel, IdCheck)
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
    RT_REQUIRE(scene->engine == 1, RT_ERR_UNSUPPORTED, w + ": only the wavefront engine renders pixel lists (rt_debug_set_engine)");
}

void finish(rt_scene *sc, hipStream_t stream) {
    Workspace &w = workspace_for(sc, stream);
    RT_HIP(hipStreamSynchronize(stream));
    if (w.pending.out) {
        const CallStats &c = w.pending;
        StatsDev h;
        rt_stats out = read_stats(w.ev0, w.ev1, c.counters ? w.stats.p : nullptr, h);
        if (c.counters) {
            std::lock_guard<std::mutex> lock(sc->mu);
            for (int o = 0; o < 9; o++) { sc->census_rounds[o] = h.op_rounds[o]; sc->census_lanes[o] = h.op_lanes[o]; }
        }
        out.spp_chunk = c.chunk; out.passes = c.passes; out.pool_slots = c.slots;
        out.partial_bytes = c.partial_bytes;
        if (c.kt) { out.trace_ms = w.kt.trace_ms; out.shade_ms = w.kt.shade_ms; }
        *c.out = out;
        w.pending.out = nullptr;
    }
}

// Joins the worker of an RT_FLAG_ASYNC call in flight on (scene, stream), if any; returns what it ended with.
int join_async(rt_scene *scene, hipStream_t stream, std::string *err) {
    Workspace &w = workspace_for(scene, stream);
    if (!w.async_worker.joinable()) return RT_OK;
    w.async_worker.join();
    const int rc = w.async_rc;
    if (err) *err = w.async_err;
    w.async_rc = RT_OK; w.async_err.clear();
    return rc;
}

// One call at a time per (scene, stream): an asynchronous one still in flight there is joined and finished first — its rt_stats,
// as rt_render_wait would have filled them — and its failure is the failure of `who`, the call that found it.
void finish_previous_async(rt_scene *sc, hipStream_t stream, const char *who) {
    std::string err;
    const bool joined = workspace_for(sc, stream).async_worker.joinable();
    const int rc = join_async(sc, stream, &err);
    RT_REQUIRE(rc == RT_OK, rc, std::string(who) + ": the previous asynchronous call on this stream failed: " + err);
    if (joined) finish(sc, stream);
}

// One rt_radiance* / rt_render_pixels* call on `stream` (the scene's device is current, the arguments checked, finish_previous_async
// done; host ids already range-checked, device ids checked here or by the enqueue): the passes, and stats.
void run_list(rt_scene *sc, const RenderJob &job, hipStream_t stream) {
    rt_stats *const stats = job.stats;
    const uint32_t chunk = plan_chunks(job.spp, job.spp_chunk).chunk;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (job.count == 0) {
        if (stats) stats->spp_chunk = chunk;
        return;
    }
    if (job.spp == 0 || job.max_depth == 0) {                 // no sample is black, ray_color at depth 0 is black: zeros, no pass
        if (job.d_pixel_ids) sync_and_check_ids(workspace_for(sc, stream), job, stream, true);      // (a list of ids is checked whatever becomes of it)
        RT_HIP(hipMemsetAsync(job.d_out, 0, job.count * 3 * sizeof(double), stream));
        RT_HIP(hipStreamSynchronize(stream));
        if (stats) { stats->paths = job.count * job.spp; stats->spp_chunk = chunk; }
        return;
    }
    enqueue(sc, job, stream);
    finish(sc, stream);
    if (stats) stats->paths = job.count * job.spp;            // (the counter block's own count, also without RT_FLAG_COUNTERS)
}

// An rt_radiance* call runs in the render's workspace of (scene, stream): an asynchronous render still in flight there (its host
// thread drives passes on that workspace) is joined and finished first (finish_previous_async), as rt_render_device does. Each
// entry point does so once, before it touches the workspace in any way — rt_radiance before its staging buffers, which live in
// the workspace too.
void run_radiance(rt_scene *sc, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *rp, double *d_out,
                  hipStream_t stream, rt_stats *stats) {
    RenderJob job;                                             // (no image, no camera: the rays carry their own times and keys)
    job.d_rays = d_rays; job.count = n_rays;
    job.spp = rp->spp; job.max_depth = rp->max_depth; job.flags = rp->flags;
    job.spp_chunk = 1;                                         // one sample per work item: the sum is 0 + L_0 + L_1 + ... in order
    std::memcpy(job.background, rp->background, sizeof job.background);
    job.t_min = rp->t_min;
    job.d_out = d_out; job.stats = stats;
    run_list(sc, job, stream);
}

void run_render_pixels(rt_scene *sc, const rt_camera *cam, const rt_params *params, const uint64_t *d_ids, uint64_t n_entries,
                       double *d_out, hipStream_t stream, rt_stats *stats, bool check_ids, const char *who) {
    RenderJob job = image_job(cam, params, nullptr, d_out, stats, check_ids, who);
    job.d_pixel_ids = d_ids; job.count = n_entries; job.progress = Progress{};       // (p's n_rows, row_ids and callback are ignored)
    run_list(sc, job, stream);
}

// The host form of a list call: `in` goes to a staging buffer of the workspace (kept for the next call; the calls that used
// them were synchronous: nothing is in flight), run() fills the sums' staging buffer — poisoned, so that an unwritten sum cannot
// pass for a result — and they come back.
template <class T, class Run>
void run_staged(Workspace &w, DeviceBuf<T> &d_in, const T *in, uint64_t n, double *out, Run run) {
    d_in.reserve(n);
    w.rad_out.reserve(n * 3);
    if (n) {
        RT_HIP(hipMemcpy(d_in, in, n * sizeof(T), hipMemcpyHostToDevice));
        RT_HIP(hipMemset(w.rad_out, 0xFF, n * 3 * sizeof(double)));
    }
    run();
    if (n) RT_HIP(hipMemcpy(out, w.rad_out, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
}

} // namespace

extern "C" {

int rt_render_device(rt_scene *scene, const rt_camera *cam, const rt_params *params,
                     double *d_out_rgb_sum, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_params(scene, cam, params);
        RT_REQUIRE(d_out_rgb_sum || params->n_rows == 0, RT_ERR_INVALID, "rt_render_device: output is null");
        DeviceGuard guard(scene->device);
        const hipStream_t stream = (hipStream_t)hip_stream;
        finish_previous_async(scene, stream, "rt_render_device");
        const RenderJob job = image_job(cam, params, params->row_ids, d_out_rgb_sum, stats, true, "rt_render_device");
        if (!(params->flags & RT_FLAG_ASYNC)) {
            enqueue(scene, job, stream);
            return RT_OK;
        }
        // RT_FLAG_ASYNC: the engine drives its passes from a host thread (it polls one word per batch) — here a thread of the
        // library's own instead of the caller's. The job is copied; the device buffers are the caller's until the wait.
        Workspace &w = workspace_for(scene, stream);
        w.async_rc = RT_OK; w.async_err.clear();
        w.async_worker = std::thread([scene, job, stream, &w]() {
            w.async_rc = guarded([&]() -> int {
                DeviceGuard worker_guard(scene->device);
                enqueue(scene, job, stream);
                return RT_OK;
            });
            if (w.async_rc != RT_OK) w.async_err = rt_last_error();      // (this thread's own: guarded left it there)
        });
        return RT_OK;
    });
}

int rt_render_wait(rt_scene *scene, void *hip_stream) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene, RT_ERR_INVALID, "rt_render_wait: null scene");
        DeviceGuard guard(scene->device);
        std::string err;
        const int rc = join_async(scene, (hipStream_t)hip_stream, &err);
        RT_REQUIRE(rc == RT_OK, rc, err);
        finish(scene, (hipStream_t)hip_stream);
        return RT_OK;
    });
}

int rt_radiance(rt_scene *scene, const rt_radiance_ray *rays, uint64_t n_rays, const rt_radiance_params *p, double *out_rgb_sum,
                rt_stats *stats) {
    return guarded([&]() -> int {
        check_radiance(scene, rays, n_rays, p, out_rgb_sum, false, "rt_radiance");
        DeviceGuard guard(scene->device);
        finish_previous_async(scene, nullptr, "rt_radiance");       // (first: the staging buffers below belong to the workspace)
        Workspace &w = workspace_for(scene, nullptr);
        run_staged(w, w.rad_rays, rays, n_rays, out_rgb_sum, [&] { run_radiance(scene, w.rad_rays, n_rays, p, w.rad_out, nullptr, stats); });
        return RT_OK;
    });
}

int rt_radiance_device(rt_scene *scene, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *p,
                       double *d_out_rgb_sum, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_radiance(scene, d_rays, n_rays, p, d_out_rgb_sum, true, "rt_radiance_device");
        DeviceGuard guard(scene->device);
        finish_previous_async(scene, (hipStream_t)hip_stream, "rt_radiance_device");
        run_radiance(scene, d_rays, n_rays, p, d_out_rgb_sum, (hipStream_t)hip_stream, stats);
        return RT_OK;
    });
}

int rt_render_pixels(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *pixel_ids, uint64_t n_entries,
                     double *out_rgb_sum, rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_render_pixels";
        check_render_pixels(scene, cam, params, pixel_ids, n_entries, out_rgb_sum, false, who);
        DeviceGuard guard(scene->device);
        finish_previous_async(scene, nullptr, who);             // (first: the staging buffers below belong to the workspace)
        Workspace &w = workspace_for(scene, nullptr);
        run_staged(w, w.pix_ids, pixel_ids, n_entries, out_rgb_sum,
                   [&] { run_render_pixels(scene, cam, params, w.pix_ids, n_entries, w.rad_out, nullptr, stats, false, who); });
        return RT_OK;
    });
}

int rt_render_pixels_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *d_pixel_ids, uint64_t n_entries,
                            double *d_out_rgb_sum, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_render_pixels_device";
        check_render_pixels(scene, cam, params, d_pixel_ids, n_entries, d_out_rgb_sum, true, who);
        DeviceGuard guard(scene->device);
        finish_previous_async(scene, (hipStream_t)hip_stream, who);
        run_render_pixels(scene, cam, params, d_pixel_ids, n_entries, d_out_rgb_sum, (hipStream_t)hip_stream, stats, true, who);
        return RT_OK;
    });
}

int rt_render(rt_scene *scene, const rt_camera *cam, const rt_params *params, double *out_rgb_sum, rt_stats *stats) {
    return guarded([&]() -> int {
        check_params(scene, cam, params);
        RT_REQUIRE(out_rgb_sum || params->n_rows == 0, RT_ERR_INVALID, "rt_render: output is null");
        check_host_ids(params->row_ids, params->n_rows, params, "rt_render");
        uint64_t n_values = (uint64_t)params->n_rows * params->width * 3;
        DeviceGuard guard(scene->device);
        DeviceBuf<uint32_t> d_rows(params->n_rows ? params->n_rows : 1);     // (after the guard: freed with the scene's device current)
        DeviceBuf<double> d_out(n_values ? n_values : 1);
        if (params->n_rows) RT_HIP(hipMemcpy(d_rows, params->row_ids, params->n_rows * sizeof(uint32_t), hipMemcpyHostToDevice));
        // Poison the output so an unwritten pixel cannot pass for a result.
        RT_HIP(hipMemset(d_out, 0xFF, (n_values ? n_values : 1) * sizeof(double)));
        enqueue(scene, image_job(cam, params, d_rows, d_out, stats, false, "rt_render"), nullptr);
        finish(scene, nullptr);
        if (n_values) RT_HIP(hipMemcpy(out_rgb_sum, d_out, n_values * sizeof(double), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_render_multi(rt_scene_set *set, const rt_camera *cam, const rt_params *params, double *out_rgb_sum, rt_stats *stats) {
    return guarded([&]() -> int {
        RT_REQUIRE(set && !set->scenes.empty() && cam && params, RT_ERR_INVALID, "rt_render_multi: null argument");
        RT_REQUIRE(params->n_rows == 0 || (params->row_ids && out_rgb_sum), RT_ERR_INVALID, "rt_render_multi: null rows or output");
        const size_t n = set->scenes.size();
        const size_t row_doubles = (size_t)params->width * 3;
        struct Share {
            std::vector<uint32_t> rows;
            std::vector<double> out;
            rt_stats st;
            int rc = RT_OK;
            std::string err;
        };
        std::vector<Share> shares(n);
        for (uint32_t i = 0; i < params->n_rows; i++) shares[i % n].rows.push_back(params->row_ids[i]);
        std::vector<std::thread> workers;
        for (size_t k = 0; k < n; k++) {
            workers.emplace_back([&, k]() {
                Share &sh = shares[k];
                std::memset(&sh.st, 0, sizeof sh.st);
                rt_params p = *params;
                p.n_rows = (uint32_t)sh.rows.size();
                p.row_ids = sh.rows.data();
                // per-worker progress: this device's share under its place in the set (main.rs:124-127: one bar per thread)
                struct Relay { void (*cb)(void *, uint32_t, uint64_t, uint64_t); void *user; uint32_t worker; } relay{params->progress_cb, params->progress_user, (uint32_t)k};
                if (params->progress_cb) {
                    p.progress_user = &relay;
                    p.progress_cb = [](void *u, uint32_t, uint64_t done, uint64_t total) { const Relay *r = static_cast<const Relay *>(u); r->cb(r->user, r->worker, done, total); };
                }
                sh.out.resize(sh.rows.size() * row_doubles);
                // (rt_render makes the scene's device current for this thread and leaves the caller's alone)
                sh.rc = rt_render(set->scenes[k], cam, &p, sh.out.data(), &sh.st);
                if (sh.rc != RT_OK) sh.err = rt_last_error();
            });
        }
        for (std::thread &t : workers) t.join();
        for (size_t k = 0; k < n; k++)
            if (shares[k].rc != RT_OK) throw Fail{shares[k].rc, "rt_render_multi: device " + std::to_string(set->devices[k]) + ": " + shares[k].err};
        std::vector<size_t> taken(n, 0);
        for (uint32_t i = 0; i < params->n_rows; i++) {
            Share &sh = shares[i % n];
            std::memcpy(out_rgb_sum + (size_t)i * row_doubles, sh.out.data() + taken[i % n]++ * row_doubles, row_doubles * sizeof(double));
        }
        if (stats) {
            rt_stats tot;
            std::memset(&tot, 0, sizeof tot);
            for (const Share &sh : shares) {
                tot.paths += sh.st.paths; tot.rays += sh.st.rays; tot.node_visits += sh.st.node_visits;
                for (int k = 0; k < RT_KIND_COUNT; k++) tot.prim_tests[k] += sh.st.prim_tests[k];
                tot.light_pdf_tests += sh.st.light_pdf_tests; tot.rng_draws += sh.st.rng_draws;
                tot.ms = sh.st.ms > tot.ms ? sh.st.ms : tot.ms;
                tot.trace_ms = sh.st.trace_ms > tot.trace_ms ? sh.st.trace_ms : tot.trace_ms;
                tot.shade_ms = sh.st.shade_ms > tot.shade_ms ? sh.st.shade_ms : tot.shade_ms;
                tot.spp_chunk = sh.st.spp_chunk; tot.passes = sh.st.passes > tot.passes ? sh.st.passes : tot.passes;
                tot.pool_slots += sh.st.pool_slots;
            }
            *stats = tot;
        }
        return RT_OK;
    });
}

int rt_tonemap_device(const double *d_rgb_sum, uint64_t n_pixels, int32_t spp, uint8_t *d_rgb8, void *hip_stream) {
    return guarded([&]() -> int {
        RT_REQUIRE((d_rgb_sum && d_rgb8) || n_pixels == 0, RT_ERR_INVALID, "rt_tonemap_device: null argument");
        if (n_pixels) RT_HIP(launch_tonemap(d_rgb_sum, n_pixels, spp, d_rgb8, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

} // extern "C"
