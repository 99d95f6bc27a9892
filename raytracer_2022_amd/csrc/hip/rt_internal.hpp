// rt_internal.hpp — what the entry-point files (rt_scene.hip, rt_render.hip, rt_query.hip, rt_post.hip, rt_debug.hip) share:
// the scene behind the C ABI's handle, what it keeps per stream, and the small helpers every entry point uses.
#ifndef RT2022_RT_INTERNAL_HPP
#define RT2022_RT_INTERNAL_HPP
#include <cstring>
#include <exception>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "../host/scene_check.hpp"
#include "pt_device.h"                 // (with it: include/rt2022.h, hip_owned.hpp and host/rt_error.hpp, <string>, <vector>)

namespace rt2022 {

template <class F>
int guarded(F &&f) {
    try {
        return f();
    } catch (const Fail &e) {
        set_error(e.msg);
        return e.code;
    } catch (const std::exception &e) {
        set_error(e.what());
        return RT_ERR_INVALID;
    }
}

// A *_fault function's verdict (host/*_check.hpp; null: nothing wrong) as the call's refusal: "<who>: <fault>".
inline void require_no_fault(const char *fault, const std::string &who) { if (fault) throw Fail{RT_ERR_INVALID, who + ": " + fault}; }

// The shells of the host-buffer forms: `count` elements of host memory on the device (null or 0: an empty buffer, whose
// pointer is null), and back (null or 0: nothing is copied). Blocking copies on the null stream.
template <class T>
DeviceBuf<T> uploaded(const T *host, uint64_t count) {
    DeviceBuf<T> d(host ? count : 0);
    if (d.n) RT_HIP(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <class T>
void download(T *host, const DeviceBuf<T> &d, uint64_t count) { if (host && count) RT_HIP(hipMemcpy(host, d, count * sizeof(T), hipMemcpyDeviceToHost)); }

// The scene's buffers, pools and streams live on the device that was current at rt_scene_create. Every entry
// point that touches them makes that device current for the call and puts the caller's back afterwards, so one
// process may hold scenes on several GPUs (one host thread per scene and stream) whatever its current device is.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int want) {
        RT_HIP(hipGetDevice(&prev));
        if (prev != want) { RT_HIP(hipSetDevice(want)); switched = true; }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// What the wavefront engine needs whatever the size of its pool; all of it is created when one is constructed.
struct EngineFixed {
    DeviceBuf<SceneDev> d_scene{1};
    DeviceBuf<RenderArgs> d_args{1};
    DeviceBuf<WfPool> d_pool{1};
    DeviceBuf<unsigned long long> d_limit{1};   // ring mode: RenderArgs::claim_limit
    WfStreams gs;                     // group streams / events / pinned words
};

// Ids of n device-resident entries (row ids, pixel ids) that are >= limit.
template <class Id>
__global__ void __launch_bounds__(256) ids_bad_kernel(const Id *ids, uint64_t n, uint64_t limit, uint32_t *out) {
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) bad += ids[i] >= limit ? 1u : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bad += (uint32_t)__shfl_xor((int)bad, d);
    if ((threadIdx.x & 63u) == 0 && bad) atomicAdd(out, bad);
}
// The two kinds of id a call may list, told apart by the pointer's type: row ids, each < height * n_frames (check_view: that fits
// 32 bits), and pixel ids, each < width * height * n_frames — the limit in a view, and what the call says of an id beyond it.
inline uint64_t id_limit(const uint32_t *, uint32_t, uint32_t height, uint32_t n_frames) { return (uint64_t)height * n_frames; }
inline uint64_t id_limit(const uint64_t *, uint32_t width, uint32_t height, uint32_t n_frames) { return (uint64_t)width * height * n_frames; }
inline const char *id_message(const uint32_t *) { return ": row id out of range"; }
inline const char *id_message(const uint64_t *) { return ": pixel id out of range (>= width * height * n_frames)"; }

// The range check of ids in host memory, against the view of `p`.
template <class Id>
void check_host_ids(const Id *ids, uint64_t n, const rt_params *p, const std::string &who) {
    const uint64_t limit = id_limit(ids, p->width, p->height, p->n_frames);
    for (uint64_t i = 0; i < n; i++) RT_REQUIRE(ids[i] < limit, RT_ERR_INVALID, who + id_message(ids));
}

// The range check of ids that came from the caller's HBM (the twin of check_host_ids): how many are out of range is counted on
// the device and copied to a pinned word. Two halves, so that the check costs a call no synchronisation of its own:
// begin() is enqueued with the call's other preparations, and end() looks at the answer behind the synchronisation the call makes
// anyway before its first pass. (An id out of range cannot fault a kernel — it only mis-keys a frame or a path — so nothing is
// lost by finding out a moment later.) Every begin() starts from zero: a call that fails at either half leaves nothing the next
// call on the stream would trip over. Any nonzero count refuses the call.
// `job`: a RenderJob or a FeatureJob — check_ids, d_rows or d_pixel_ids (at most one), count, the view, and `who` for the message.
// (Templates: only the files that check ids compile the counting kernel.)
struct IdCheck {
    DeviceBuf<uint32_t> d_bad;        // device word: ids out of range in the call being checked (created on first use)
    PinnedBuf<uint32_t> h_bad;        // ... and the pinned word it is copied to
    template <class Id>
    void count(const Id *d_ids, uint64_t n, uint64_t limit, hipStream_t stream) {      // n > 0
        if (!h_bad) {                                  // (keyed on the one created last: a failure half-way is made good by the next call)
            d_bad = DeviceBuf<uint32_t>(1);
            h_bad = PinnedBuf<uint32_t>(1);
        }
        RT_HIP(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), stream));
        const uint64_t blocks = (n + 255u) / 256u;
        hipLaunchKernelGGL(ids_bad_kernel<Id>, dim3((unsigned)(blocks > 256 ? 256 : blocks)), dim3(256), 0, stream, d_ids, n, limit, d_bad.p);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpyAsync(h_bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    // Whether the job has ids to check; if so, the count of its bad ones is on its way.
    template <class Job>
    bool begin(const Job &job, hipStream_t stream) {
        if (!job.check_ids || job.count == 0 || !(job.d_rows || job.d_pixel_ids)) return false;
        if (job.d_rows) count(job.d_rows, job.count, id_limit(job.d_rows, job.width, job.height, job.n_frames), stream);
        else count(job.d_pixel_ids, job.count, id_limit(job.d_pixel_ids, job.width, job.height, job.n_frames), stream);
        return true;
    }
    template <class Job>
    void end(const Job &job) const {                   // (begin() said true, and the stream has been synchronised since)
        RT_REQUIRE(*h_bad.p == 0, RT_ERR_INVALID, std::string(job.who) + (job.d_rows ? id_message(job.d_rows) : id_message(job.d_pixel_ids)));
    }
    // The one synchronisation of `stream` a call makes before its first pass (`sync_anyway`; false: only if there is something
    // to check), with the two halves around it.
    template <class Job>
    void sync_and_check(const Job &job, hipStream_t stream, bool sync_anyway) {
        const bool check = begin(job, stream);
        if (check || sync_anyway) RT_HIP(hipStreamSynchronize(stream));
        if (check) end(job);
    }
};

// What rt_render_wait (finish) reports of the call last enqueued on a (scene, stream): assigned once, when the call has been enqueued.
struct CallStats {
    rt_stats *out = nullptr;          // host stats to fill (null: nothing pending)
    bool counters = false, kt = false;         // the counter block was run; RT_FLAG_KERNEL_TIMES: Workspace::kt holds the call's times
    uint32_t chunk = 0, passes = 0;
    uint64_t slots = 0, partial_bytes = 0;
};

// What one (scene, stream) keeps from render to render. Its members own their HIP resources; the ones every call needs —
// work counter, counter block, two events — are created when it is constructed.
struct Workspace {
    DeviceBuf<unsigned long long> work_counter{1};
    DeviceBuf<StatsDev> stats{1};
    DeviceBuf<double> partial, tape;  // partial sums (wavefront and megakernel), bounce tape (megakernel): grown as needed
    // wavefront engine
    WfPool pool{};
    std::vector<DeviceBuf<char>> pool_owned;
    uint32_t pool_slots = 0, pool_depth = 0;
    unsigned long long *pool_dbg = nullptr;    // (one of pool_owned)
    std::unique_ptr<EngineFixed> fx;  // (created on first use)
    uint32_t iterations = 0;
    Event ev0{hipEventDefault}, ev1{hipEventDefault};
    CallStats pending;                // of the call enqueued last, consumed by finish
    KernelTimes kt;                   // RT_FLAG_KERNEL_TIMES
    IdCheck ids;                      // rt_render_device's row ids, rt_render_pixels_device's pixel ids
    // rt_radiance (host buffers): the device copies of the caller's rays and of the sums, grown as needed
    DeviceBuf<rt_radiance_ray> rad_rays;
    DeviceBuf<double> rad_out;
    // rt_render_pixels' device copy of the caller's list (its sums go through rad_out)
    DeviceBuf<uint64_t> pix_ids;
    // RT_FLAG_ASYNC: the host thread that drives the passes of the call in flight on this (scene, stream), and what it ended with
    // (read by rt_render_wait after the join).
    std::thread async_worker;
    int async_rc = RT_OK;
    std::string async_err;
};

// Scratch of the closest-hit calls — queries (rt_intersect*) or feature buffers (rt_features*) — and of the scatter steps
// (rt_scatter*, which leave the work counter alone) on one (scene, stream): the work counter of the persistent grid, a counter block and two events, created when it is constructed. Nothing of a render's
// Workspace: such a call may run beside an asynchronous render of the same scene.
struct QueryScratch {
    std::mutex mu;                    // one call at a time enqueues — and, with stats, reads back — on this (scene, stream)
    DeviceBuf<unsigned long long> counter{1};
    DeviceBuf<StatsDev> stats{1};
    Event ev0{hipEventDefault}, ev1{hipEventDefault};
    IdCheck ids;                      // rt_features_device's row ids, rt_features_pixels_device's pixel ids
};

} // namespace rt2022

// The handles of the C ABI (include/rt2022.h).
struct rt_scene : rt2022::SceneFacts {               // (what check_scene found: stack_need, features, general_boundaries, boxes_plain)
    explicit rt_scene(const rt2022::SceneFacts &facts) : rt2022::SceneFacts(facts) {}
    rt2022::SceneDev dev{};
    std::vector<rt2022::DeviceBuf<char>> owned;        // the pools behind `dev`
    uint32_t tuning = rt2022::tune::kDefault;          // the tuning word (pt_device.h, namespace tune)
    uint32_t vote_weights = 0;                 // 0: the wavefront engine's default (kWfVoteWeights, pt_device.h)
    int engine = 1;                   // 0 = megakernel, 1 = wavefront (shade / trace passes)
    unsigned long long census_rounds[9] = {}, census_lanes[9] = {};   // of the last counter run
    int max_pool_blocks = 0;          // 0 = 5 x CUs x segments per trace workgroup
    int partial_ring = 0;             // planes of the partial-sum ring: 0 automatic, -1 never, > 0 this many (rt_debug_set_partial_ring)
    int partial_ring_group = 0;       // largest sample group of the ring (0: 25); env RT2022_RING_GROUP at rt_scene_create (A/B)
    uint64_t ring_threshold_bytes = 64ull << 30;   // partial sums above this switch the ring on: 40 % of the device's memory (rt_scene_create)
    double pass_timing[5] = {};       // of the last render with tuning bit 29 (rt_debug_pass_timing)
    int device = 0;
    int n_cus = 0;                    // compute units of `device`
    std::mutex mu;
    std::map<hipStream_t, rt2022::Workspace> ws;
    std::mutex qmu;                   // guards `qs`, `fs` and `ss`
    // (a map per family: a query, a feature call and a scatter step on one stream share no mutex and no counter, and run side by side)
    std::map<hipStream_t, std::unique_ptr<rt2022::QueryScratch>> qs, fs;    // of rt_intersect*, of rt_features*
    std::map<hipStream_t, std::unique_ptr<rt2022::QueryScratch>> ss;        // of rt_scatter*
    uint32_t n_materials = 0;         // records in dev.materials (rt_scatter* refuses a made-up record's index against it)
};

// One call, several GPUs: a scene per device of the mask.
struct rt_scene_set {
    std::vector<int> devices;
    std::vector<rt_scene *> scenes;
};

namespace rt2022 {

// The view of a render or a feature call: an image, a shutter interval, row ids that fit 32 bits. (`empty_note`: what the
// caller's message adds to "empty image".)
inline void check_view(const rt_camera *cam, const rt_params *p, const std::string &prefix, const char *empty_note) {
    RT_REQUIRE(p->width > 0 && p->height > 0 && p->n_frames > 0, RT_ERR_INVALID, prefix + "empty image" + empty_note);
    RT_REQUIRE(cam->time0 < cam->time1, RT_ERR_INVALID, prefix + "camera time0 >= time1 (gen_range panics in the reference, camera.rs:71)");
    RT_REQUIRE((uint64_t)p->height * p->n_frames <= 0xFFFFFFFFull, RT_ERR_INVALID, prefix + "height * n_frames overflows a row id");
}

// rt_stats of a finished call (its stream has been synchronised): the time between its two events and, with `d_stats`, the
// counter block of the run as rt_stats reports it (the whole block is left in `h` for the caller that wants more of it).
inline rt_stats read_stats(hipEvent_t ev0, hipEvent_t ev1, const StatsDev *d_stats, StatsDev &h) {
    rt_stats out;
    std::memset(&out, 0, sizeof out);
    if (d_stats) {
        RT_HIP(hipMemcpy(&h, d_stats, sizeof h, hipMemcpyDeviceToHost));
        out.paths = h.paths; out.rays = h.rays; out.node_visits = h.node_visits;
        for (int k = 0; k < RT_KIND_COUNT; k++) out.prim_tests[k] = h.prim_tests[k];
        out.light_pdf_tests = h.light_pdf_tests; out.rng_draws = h.rng_draws;
    }
    float ms = 0.f;
    RT_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    out.ms = (double)ms;
    return out;
}

} // namespace rt2022
#endif
