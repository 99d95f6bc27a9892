// pt_wavefront.hip — the wavefront engine: the same per-path algorithm as the megakernel
// (pt_kernel.hip), cut at the one point where its register needs change character.
//
// Why two kernels: measured on MI355X, the single megakernel needs 256 VGPRs + scratch
// (traversal state and the shading temporaries — Perlin turbulence, ONB, light pdfs — are
// live together), which caps it at 2 waves/SIMD, and its spills land in the node loop
// (profiles/r1_megakernel_*.txt). Split at "closest hit found", the traversal kernel is
// lean and the shading kernel is wide, and each gets the occupancy it can use.
//
// Paths live in a pool of slots in HBM (WfPool, one record per slot and field). The pool is cut
// into segments of 4096 slots; a segment belongs to one shade workgroup for the whole frame; the trace
// pass is a persistent grid whose waves draw chunks of the segments' ray lists — so the only global
// atomics on the data path are the work counter (items) and the chunk counter (ray lists):
//   wf_shade  counting-sorts its slots by what they wait for (miss / light / lambertian by
//             texture / metal / dielectric / isotropic / fresh) in LDS and shades them in that
//             order — material dispatch by sorted type id, wave-uniform except at bin boundaries;
//             finished paths are unwound from the bounce tape, added to their pixel, and
//             replaced by the next sample / work item at once; last, it writes the segment's
//             ray list for the trace pass, longest expected traversal first;
//   wf_trace  runs the in-wave scheduled traversal over the lists: a wave claims 256 entries at a
//             time, its lanes pull the next ray as soon as theirs is done (__ballot / __popcll
//             refill), and the wave executes the operation most lanes wait for (node step, sphere
//             test, box, medium, ...).
// The host alternates the two until no slot carries a ray any more.
//
// Per-lane semantics never change: every path consumes its RNG stream and visits nodes
// in the reference's order, so results stay bit-identical to the oracle.
//
// This file is the driver: the pool's first state, the ring kernels, the groups and their passes. The two kernels, each with
// its launcher, are units of their own — pt_wavefront_shade.hip, pt_wavefront_trace.hip — and pt_wavefront.hpp is what the three share.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pt_wavefront.hpp"

namespace rt2022 {

// Marks the first `used` slots of every workgroup FRESH and the rest IDLE: a small job is spread
// over all workgroups (a few slots each) instead of filling a few workgroups to the brim.
__global__ void __launch_bounds__(256) wf_init(uint8_t *kind, uint16_t *list, uint32_t *list_n, uint32_t n_slots, uint32_t used) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots) {                                            // the first "ray list" of a segment: its slots in use, all FRESH
        const uint32_t local = i % (uint32_t)S;
        kind[i] = local < used ? (uint8_t)SK_FRESH : (uint8_t)SK_IDLE;
        list[i] = (uint16_t)local;
        if (local == 0) list_n[i / (uint32_t)S] = used;
    }
}

// Ring mode: out[i] = (first plane of the frame ? 0 : out[i]) + partial[first mod R][i] + ... in sample order — pixel_color += ...,
// main.rs:150, continued where the last call of this kernel left off (chunk_sum_kernel's sum, taken a few planes at a time).
__global__ void __launch_bounds__(256) ring_accumulate_kernel(const double *partial, double *out, uint64_t n_values, uint32_t first, uint32_t count, uint32_t ring) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < n_values; i += stride) {
        double acc = first == 0 ? 0.0 : out[i];
        for (uint32_t c = first; c < first + count; c++) acc += partial[(uint64_t)(c % ring) * n_values + i];
        out[i] = acc;
    }
}
__global__ void ring_set_limit_kernel(unsigned long long *limit, unsigned long long value) { *limit = value; }

static void launch_pass(const TraceChoice &c, const WfLaunch &w, uint32_t parity, hipEvent_t between = nullptr) {
    launch_shade(w, c.stats, parity);
    if (between) (void)hipEventRecord(between, w.stream);
    launch_trace(c, w, parity);
}

// ---- the pass driver ----
namespace {
// The pool is cut into groups of segments, each on a stream of its own and alternating shade / trace passes
// at its own pace: nothing couples the groups but the work counter, so while the last long rays of one
// group's trace pass keep a few waves busy, the other groups' kernels fill the rest of the chip. (Measured
// with one group: the mean wave lives 0.41 of a trace pass — rt_debug_pass_timing.)
struct PassDriver {
    struct Group {
        WfLaunch w;
        uint32_t iter = 0;      // passes enqueued
        uint32_t batches = 0;   // batches enqueued
        uint32_t waited = 0;    // batches whose answer has been read
        bool drained = false;
    };
    WfRender &r;
    const RenderArgs &args;
    const WfPool &pool;
    const WfStreams &gs;
    double *const timing;
    KernelTimes *const kt;
    const bool report;
    // Ring of partial-sum planes (RenderArgs::ring): planes consumed so far, and the claim limit that follows them.
    const bool ringed;
    uint32_t consumed = 0;      // planes added to the output so far (a multiple of the sample group)
    const uint64_t n_values, per_group;         // doubles of a plane; work items of one sample group
    unsigned long long reported = 0;
    TraceChoice choice{};
    int G = 1;
    Group grp[kMaxGroups];
    uint32_t poll_every = 4, iterations = 0;

    explicit PassDriver(WfRender &r_)
        : r(r_), args(*r_.args), pool(*r_.pool), gs(*r_.gs), timing(r_.timing), kt(r_.kt), report(r_.progress.cb && gs.h_work),
          ringed(r_.ring.planes > 0 && args.ring == r_.ring.planes && gs.h_work && gs.h_oldest && args.ring_group > 0 &&
                 args.ring % args.ring_group == 0 && args.n_chunks % args.ring_group == 0),
          n_values(args.n_pixels * 3), per_group(ringed ? args.n_pixels * args.ring_group : 1) {}
    hipError_t run();
    hipError_t init_pool();
    hipError_t cut_groups();
    hipError_t enqueue_batch(int g);
    void report_progress(unsigned long long items);
    hipError_t read_pass_timing(const Group &q, uint32_t rays);
    void log_pass(const Group &q, const unsigned long long h[5], uint32_t rays);
    unsigned long long ring_limit(uint32_t done) const;
    hipError_t ring_consume(uint32_t upto, hipStream_t st);
    hipError_t ring_advance(const Group &q, unsigned long long work, unsigned long long oldest);
    hipError_t sum_kernel_times();
};
hipError_t PassDriver::run() {
    if (r.stack_need > (uint32_t)kStackLarge) return hipErrorInvalidValue;
    if (r.ring.planes > 0 && !ringed) return hipErrorInvalidValue;
    choice = choose_trace(*r.scene, r.stack_need, args.tuning, r.features, r.counters, timing != nullptr);
    hipError_t e;
    if ((e = init_pool()) != hipSuccess) return e;
    if ((e = cut_groups()) != hipSuccess) return e;
    poll_every = timing ? 1 : 4;
    // One batch = poll_every passes + a read-back of the group's "rays handed on" counter. Two batches per group
    // are kept in flight so that a group's stream never runs empty while the host looks at the previous answer.
    for (int g = 0; g < G; g++) {
        if ((e = enqueue_batch(g)) != hipSuccess) return e;
        if (!timing && (e = enqueue_batch(g)) != hipSuccess) return e;
    }
    int live = G;
    while (live > 0) {
        for (int g = 0; g < G; g++) {
            Group &q = grp[g];
            if (q.drained) continue;
            const uint32_t at = 2 * g + (q.waited & 1u);            // the batch's words in the pinned arrays
            if ((e = hipEventSynchronize(gs.ev[g][q.waited & 1u])) != hipSuccess) return e;
            q.waited++;
            if (report) report_progress(gs.h_work[at]);
            if (timing && (e = read_pass_timing(q, gs.h_active[at])) != hipSuccess) return e;
            if (ringed && (e = ring_advance(q, gs.h_work[at], gs.h_oldest[at])) != hipSuccess) return e;
            if (gs.h_active[at] == 0) {         // the batch's last shade pass handed no ray on: the group has drained
                q.drained = true;
                live--;
                continue;
            }
            if (q.iter > (1u << 26)) return hipErrorUnknown;
            if ((e = enqueue_batch(g)) != hipSuccess) return e;
        }
    }
    if (ringed && (e = ring_consume(args.n_chunks, grp[0].w.stream)) != hipSuccess) return e;      // (nothing is in flight any more)
    for (int g = 0; g < G; g++)                 // (a drained group may still have an idle batch queued)
        if ((e = hipStreamSynchronize(grp[g].w.stream)) != hipSuccess) return e;
    if (kt && (e = sum_kernel_times()) != hipSuccess) return e;
    r.passes = iterations;
    return hipSuccess;
}
// Slots in use start FRESH (at most one work item per slot is ever needed at a time).
hipError_t PassDriver::init_pool() {
    const uint32_t blocks = pool.n_blocks;
    hipError_t e;
    uint64_t per_block = (args.n_items + blocks - 1) / blocks;
    uint32_t used = (uint32_t)(per_block > (uint64_t)S ? (uint64_t)S : (per_block + 63) / 64 * 64);
    if (used < 64) used = 64;
    uint32_t n = blocks * (uint32_t)S;
    hipLaunchKernelGGL(wf_init, dim3((n + 255) / 256), dim3(256), 0, r.stream, pool.kind, pool.list, pool.list_n, n, used);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemsetAsync(pool.n_active, 0, 2 * kMaxGroups * sizeof(uint32_t), r.stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(pool.max_list, 0, 2 * kMaxGroups * sizeof(uint32_t), r.stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(pool.fault, 0, sizeof(uint32_t), r.stream)) != hipSuccess) return e;
    if (ringed) {
        if ((e = hipMemsetAsync(pool.oldest, 0xFF, 2 * sizeof(unsigned long long), r.stream)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(pool.starved_n, 0, blocks * sizeof(uint32_t), r.stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(ring_set_limit_kernel, dim3(1), dim3(1), 0, r.stream, r.ring.d_limit, ring_limit(0));
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}
// Every group's view of the pool, and its stream behind the caller's.
hipError_t PassDriver::cut_groups() {
    const uint32_t trace_blocks = pool.n_blocks / pool.segs;
    G = (timing || kt || ringed) ? 1 : gs.n;    // (per-kernel times: one group, so that a launch's duration is its own; with several, launches of different groups overlap)
    if (G < 1) G = 1;
    if ((uint32_t)G > trace_blocks) G = (int)trace_blocks;
    for (int g = 0; g < G; g++) {
        const uint32_t tb0 = (uint32_t)((uint64_t)trace_blocks * g / G), tb1 = (uint32_t)((uint64_t)trace_blocks * (g + 1) / G);
        const uint32_t seg_begin = tb0 * pool.segs, n_segs = (tb1 - tb0) * pool.segs;
        const uint64_t off = (uint64_t)seg_begin * S;
        WfPool v = pool;
        v.n_blocks = n_segs; v.n_slots = n_segs * (uint32_t)S;
        v.kind += off; v.ray += off * kRecDoubles; v.hit += off * kRecWords; v.state += off * kRecWords; v.pixel_sum += off * 4;
        v.tape += off * pool.tape_cap * 4; v.list += off; v.list_n += seg_begin;
        v.n_active = pool.n_active + 2 * g;
        v.next_chunk = pool.next_chunk + g;
        v.max_list = pool.max_list + 2 * g;
        grp[g].w = WfLaunch{*r.scene, v, r.d_args, args.t_min, args.tuning, args.vote_weights, args.stats, n_segs,
                            G == 1 ? r.stream : gs.stream[g], ringed, args.rays != nullptr, args.pixel_ids != nullptr};
    }
    hipError_t e;
    if (G > 1) {                                // the groups start after what the caller's stream holds so far
        if ((e = hipEventRecord(gs.ev[0][0], r.stream)) != hipSuccess) return e;
        for (int g = 0; g < G; g++)
            if ((e = hipStreamWaitEvent(gs.stream[g], gs.ev[0][0], 0)) != hipSuccess) return e;
        if ((e = hipEventSynchronize(gs.ev[0][0])) != hipSuccess) return e;     // (the event is reused below)
    }
    return hipSuccess;
}
hipError_t PassDriver::enqueue_batch(int g) {
    Group &q = grp[g];
    const hipStream_t st = q.w.stream;
    hipError_t e;
    for (uint32_t k = 0; k < poll_every; k++) {
        if (timing) {
            if ((e = hipMemsetAsync(pool.dbg, 0xFF, sizeof(unsigned long long), st)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(pool.dbg + 1, 0, 4 * sizeof(unsigned long long), st)) != hipSuccess) return e;
        }
        // (kernel times: three events per pass pair k, on the stream of its group — 3k before its shade pass, 3k+1 between its shade
        // and trace pass, 3k+2 after: with several groups the pairs of different groups overlap, each launch's own duration is what
        // is summed)
        hipEvent_t mid = nullptr;
        if (kt) {
            while (kt->ev.size() < 3 * (size_t)iterations + 3) kt->ev.emplace_back(hipEventDefault);     // (throws Fail)
            if ((e = hipEventRecord(kt->ev[3 * iterations], st)) != hipSuccess) return e;
            mid = kt->ev[3 * iterations + 1];
        }
        launch_pass(choice, q.w, q.iter & 1u, mid);
        if (kt && (e = hipEventRecord(kt->ev[3 * iterations + 2], st)) != hipSuccess) return e;
        q.iter++;
        iterations++;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t b = q.batches++ & 1u, at = 2 * g + b;     // ring of two: batches of a group complete in order
    const uint32_t parity = (q.iter - 1) & 1u;  // (of the batch's last pass)
    if ((e = hipMemcpyAsync(gs.h_active + at, q.w.pool.n_active + parity, sizeof(uint32_t), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((report || ringed) && (e = hipMemcpyAsync(gs.h_work + at, args.work_counter, sizeof(unsigned long long),
                                                  hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if (ringed && (e = hipMemcpyAsync(gs.h_oldest + at, q.w.pool.oldest + parity, sizeof(unsigned long long),
                                      hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    return hipEventRecord(gs.ev[g][b], st);
}
// Work items handed out so far -> camera paths started (main.rs:154-155: the bar's inc).
void PassDriver::report_progress(unsigned long long items) {
    if (items > args.n_items) items = args.n_items;       // (the counter overshoots at the end of the work)
    unsigned long long paths = items * r.progress.per_item;
    if (paths > r.progress.total) paths = r.progress.total;
    if (paths > reported && paths < r.progress.total) { reported = paths; r.progress.cb(r.progress.user, 0u, paths, r.progress.total); }
}
// The probe's words of the pass just waited for (poll_every is 1), added to rt_debug_pass_timing's sums.
hipError_t PassDriver::read_pass_timing(const Group &q, uint32_t rays) {
    unsigned long long h[5];
    hipError_t e;
    if ((e = hipMemcpy(h, pool.dbg, sizeof h, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    if (!h[4]) return hipSuccess;
    timing[0] += (double)(h[1] - h[0]);                // span of the pass
    timing[1] += (double)h[2] / (double)h[4];          // mean wave lifetime
    timing[2] += (double)h[3] / (double)h[4];          // mean wave time after its list ran dry
    timing[3] += 1.0;
    timing[4] += (double)h[4];
    if (getenv("RT2022_PASS_LOG")) log_pass(q, h, rays);
    return hipSuccess;
}
// RT2022_PASS_LOG: one line per pass; for three passes also when wave 0 of every workgroup started and ended (RT2022_BLOCK_DUMP=
// file prefix: every workgroup's pair).
void PassDriver::log_pass(const Group &q, const unsigned long long h[5], uint32_t rays) {
    if (q.iter == 50 || q.iter == 51 || q.iter == 80) {
        const uint32_t nb = (uint32_t)(h[4] / 4);                 // (workgroups of the persistent grid that ran)
        std::vector<unsigned long long> bt(2 * nb);
        if (hipMemcpy(bt.data(), pool.dbg + 8, bt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
            std::vector<double> st_, en_;
            for (uint32_t b = 0; b < nb; b++) {
                st_.push_back((double)(bt[2 * b] - h[0]) / 100.0); en_.push_back((double)(bt[2 * b + 1] - h[0]) / 100.0);
            }
            if (const char *dump = getenv("RT2022_BLOCK_DUMP")) {
                char name[512];
                snprintf(name, sizeof name, "%s.%u", dump, q.iter);
                if (FILE *f = fopen(name, "w")) { for (uint32_t b = 0; b < nb; b++) fprintf(f, "%u %.1f %.1f\n", b, st_[b], en_[b]); fclose(f); }
            }
            std::sort(st_.begin(), st_.end()); std::sort(en_.begin(), en_.end());
            fprintf(stderr, "pass %u workgroups %u: start us p0 %.1f p50 %.1f p100 %.1f | end us p0 %.1f p10 %.1f p50 %.1f p90 %.1f p100 %.1f\n", q.iter, nb,
                    st_[0], st_[nb / 2], st_[nb - 1], en_[0], en_[nb / 10], en_[nb / 2], en_[nb * 9 / 10], en_[nb - 1]);
        }
    }
    fprintf(stderr, "pass %u span_us %.1f life/span %.3f dry/life %.3f waves %llu rays %u\n", q.iter, (double)(h[1] - h[0]) / 100.0,
            (double)h[2] / (double)h[4] / (double)(h[1] - h[0]), (double)h[3] / (double)(h[2] ? h[2] : 1), h[4], rays);
}
// The groups whose planes are free: those consumed, and R planes' worth beyond them.
unsigned long long PassDriver::ring_limit(uint32_t done) const {
    const unsigned long long lim = ((unsigned long long)done + r.ring.planes) / args.ring_group * per_group;
    return lim < args.n_items ? lim : (unsigned long long)args.n_items;
}
// Planes [consumed, upto) are complete: add them to the output and raise the claim limit behind them.
hipError_t PassDriver::ring_consume(uint32_t upto, hipStream_t st) {
    if (upto <= consumed) return hipSuccess;
    const uint64_t want = (n_values + 255) / 256;
    hipLaunchKernelGGL(ring_accumulate_kernel, dim3((unsigned)(want > 2048 ? 2048 : (want ? want : 1))), dim3(256), 0, st,
                       args.partial, r.ring.out, n_values, consumed, upto - consumed, r.ring.planes);
    consumed = upto;
    hipLaunchKernelGGL(ring_set_limit_kernel, dim3(1), dim3(1), 0, st, r.ring.d_limit, ring_limit(consumed));
    return hipGetLastError();
}
// Everything below the oldest item in flight (and below the counter: items not handed out yet are not in flight
// either) is finished: whole planes under that frontier go to the output, and the limit follows them. (The words
// were copied behind the batch's last shade pass; the kernels launched here run behind the batches already queued,
// whose claims still obey the old limit.)
hipError_t PassDriver::ring_advance(const Group &q, unsigned long long work, unsigned long long oldest) {
    unsigned long long groups_done = (work < args.n_items ? work : (unsigned long long)args.n_items) / per_group;
    if (oldest < groups_done) groups_done = oldest;
    hipError_t e;
    if ((e = ring_consume((uint32_t)groups_done * args.ring_group, q.w.stream)) != hipSuccess) return e;
    if (r.ring.max_passes && iterations > r.ring.max_passes) return hipErrorUnknown;     // (a frame cannot take this long: never spin)
    return hipSuccess;
}
// Device time of the shade passes and of the trace passes.
hipError_t PassDriver::sum_kernel_times() {
    hipError_t e;
    kt->shade_ms = kt->trace_ms = 0.0;
    for (uint32_t k = 0; k < iterations; k++) {
        float a = 0.f, b = 0.f;
        if ((e = hipEventElapsedTime(&a, kt->ev[3 * k], kt->ev[3 * k + 1])) != hipSuccess) return e;
        if ((e = hipEventElapsedTime(&b, kt->ev[3 * k + 1], kt->ev[3 * k + 2])) != hipSuccess) return e;
        kt->shade_ms += (double)a;
        kt->trace_ms += (double)b;
    }
    return hipSuccess;
}
} // namespace

hipError_t launch_render_wavefront(WfRender &r) {
    // Passes may still be queued or running against the pool on the group streams: let them finish (best
    // effort) before the caller sees the error and possibly frees or reuses the pool.
    const auto drain = [&r] {
        for (int g = 0; g < kMaxGroups; g++)
            if (r.gs->stream[g]) (void)hipStreamSynchronize(r.gs->stream[g]);
        (void)hipStreamSynchronize(r.stream);
    };
    hipError_t e;
    try { e = PassDriver(r).run(); } catch (...) { drain(); throw; }       // (a kernel-time event that could not be created)
    if (e != hipSuccess) { drain(); return e; }
#ifdef RT2022_TRACE_PROBE
    if (r.pool->dbg) print_trace_probe(*r.pool);
#endif
#ifdef RT2022_SHADE_PROBE
    if (r.pool->dbg) print_shade_probe(*r.pool);
#endif
    return hipMemcpy(&r.fault, r.pool->fault, sizeof r.fault, hipMemcpyDeviceToHost);
}

} // namespace rt2022
