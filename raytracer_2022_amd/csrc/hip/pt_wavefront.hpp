// pt_wavefront.hpp — what the three units of the wavefront engine share (pt_wavefront.hip: the driver; pt_wavefront_shade.hip and
// pt_wavefront_trace.hip: its two kernels with their launchers): the pool's records as both kernels read and write them, what a
// launch is given, and the few functions the driver calls in the other two units.
#pragma once
#include "pt_common.hpp"

namespace rt2022 {

namespace {

constexpr int S = kSlotsPerBlock;
constexpr uint32_t kChunk = 256;           // list entries a wave claims at a time

// Records are fetched whole and at once — a few 16-byte loads issued back to back and waited for together — never
// field by field as the arithmetic gets to them: left to itself the compiler sinks each field's load into the branch
// that uses it, and an arm like Boxes::hit then waits for memory six to ten times in a row (seen in the ISA). The empty
// asm pins the value: the load cannot move below it, and everything pinned together shares one wait.
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x2_a8 __attribute__((ext_vector_type(2), aligned(8)));     // (records whose size is 8 mod 16)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <class T>
RT_DEV void t_pin(T &v) { asm volatile("" : "+v"(v)); }
// The wave's vote as the hardware gives it (a v_cmp into an SGPR pair); HIP's __ballot materialises the predicate as 0 / 1 first.
RT_DEV unsigned long long wballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

struct PoolView {
    const WfPool &p;
    // Ray + RNG state: one 64-byte line per slot.
    RT_DEV Ray load_ray(uint32_t slot, uint64_t &rng_state) const {
        const double2 *q = reinterpret_cast<const double2 *>(p.ray + (uint64_t)slot * kRecDoubles);
        double2 a = q[0], b = q[1], c = q[2], d = q[3];
        rng_state = rtm::d2u(d.y);
        return Ray(Vec3(a.x, a.y, b.x), Vec3(b.y, c.x, c.y), d.x);
    }
    RT_DEV Ray load_ray(uint32_t slot) const { uint64_t unused; return load_ray(slot, unused); }
    RT_DEV void store_ray(uint32_t slot, const Ray &r, uint64_t rng_state) const {
        double2 *q = reinterpret_cast<double2 *>(p.ray + (uint64_t)slot * kRecDoubles);
        q[0] = make_double2(r.orig.x, r.orig.y);
        q[1] = make_double2(r.orig.z, r.dir.x);
        q[2] = make_double2(r.dir.y, r.dir.z);
        q[3] = make_double2(r.tm, rtm::u2d(rng_state));
    }
    RT_DEV void store_rng(uint32_t slot, uint64_t rng_state) const { p.ray[(uint64_t)slot * kRecDoubles + 7] = rtm::u2d(rng_state); }
    // Winner of the traversal: one 32-byte record per slot.
    // meta = box face | movers << 4 | node steps of the traversal << 16 (the shade pass orders the next
    // trace pass by them); a miss stores nothing (its path ends).
    // Second half = the movers enclosing the leaf; its last word holds the leaf's material word instead whenever the
    // chain leaves it free (fewer than four movers): the shade pass then needs no look at the primitive for it.
    RT_DEV void store_hit(uint32_t slot, double t, uint32_t leaf, uint32_t meta, const Chain &ch, uint32_t mat_word) const {
        u32x4 *q = reinterpret_cast<u32x4 *>(p.hit + (uint64_t)slot * kRecWords);
        uint64_t tb = rtm::d2u(t);
        q[0] = (u32x4){(uint32_t)tb, (uint32_t)(tb >> 32), leaf, meta};
        q[1] = (u32x4){ch.c0, ch.c1, ch.c2, ch.n >= 4u ? ch.c3 : mat_word};
    }
    RT_DEV static void decode_hit(u32x4 a, u32x4 b, Winner &w, uint32_t &steps, uint32_t &mat_word, bool &have_mat) {
        w.t = rtm::u2d(((uint64_t)a.y << 32) | a.x);
        w.leaf = a.z;
        w.face = a.w & 0xFu;
        w.chain.n = (a.w >> 4) & 0xFu;
        steps = a.w >> 16;
        have_mat = w.chain.n < 4u;
        mat_word = b.w;
        w.chain.c0 = b.x; w.chain.c1 = b.y; w.chain.c2 = b.z; w.chain.c3 = have_mat ? 0u : b.w;
    }
};

} // namespace

// What a launch of either kernel is given (host side).
struct WfLaunch {
    SceneDev scene;
    WfPool pool;                // this group's view of the pool
    const RenderArgs *d_args;
    double t_min;
    uint32_t tuning;
    uint32_t vote_weights;
    StatsDev *stats;
    uint32_t blocks;            // segments of the group
    hipStream_t stream;
    bool ring = false;          // RenderArgs::ring in use: the shade pass's ring build
    bool rays = false;          // RenderArgs::rays in use: the shade pass's caller-ray build (rt_radiance*)
    bool pixels = false;        // RenderArgs::pixel_ids in use: the shade pass's pixel-list build (rt_render_pixels*)
};

// Which traversal kernel a call gets: one choice (choose_trace), one dispatch (launch_trace), both in pt_wavefront_trace.hip.
// The facts that pick a wf_trace instance, as that instance has them for template arguments.
enum TraceTable { kTablePlain, kTableWhole, kTablePartial, kTablePrims };
struct TraceChoice {
    // Node table in LDS (the 1024-thread variants, stacks of kStackTiny): none — the plain kernels; the whole table; its first
    // kNodeCache records; or a sphere-only scene whose node table and sphere pools all fit (the all-in-LDS instance).
    TraceTable table;
    int stack;                  // STACK
    unsigned feat;              // FEAT as instantiated (7 where the counters / the probe exist for the full kernel only)
    bool stats, probe;          // STATS, PROBE
    bool spheres;               // SPHERES: the scene is sphere-only and the instance exists in that flavour
};
// What the driver (pt_wavefront.hip) calls in the two kernels' units. (Hidden: they serve the engine's own units, the library
// exports none of them.)
#pragma GCC visibility push(hidden)
void launch_shade(const WfLaunch &w, bool stats, uint32_t parity);
TraceChoice choose_trace(const SceneDev &scene, uint32_t stack_need, uint32_t word, unsigned features, bool counters, bool probe);
void launch_trace(const TraceChoice &c, const WfLaunch &w, uint32_t parity);
// Diagnostic builds: what the section clocks of the traversal / shade kernels added up to over the render.
#ifdef RT2022_TRACE_PROBE
void print_trace_probe(const WfPool &pool);
#endif
#ifdef RT2022_SHADE_PROBE
void print_shade_probe(const WfPool &pool);
#endif
#pragma GCC visibility pop

} // namespace rt2022
