// pt_query.hip — batched closest-hit queries on a device scene (rt_intersect*, include/rt2022.h).
//
// `world.hit(r, t_min, t_max)` for caller-supplied rays, without rendering: the megakernel's traversal (pt_traverse.hpp)
// on its own, with each ray's own window, time and RNG state, and the winner's full HitRecord written back.
// The shell is pt_traverse.hpp's, shared with the feature kernel (pt_features.hip): a persistent wave64 grid sized by
// occupancy, one work item per lane, a lane that is done taking the next from a global counter with one atomic per wave
// for all the lanes that refill together — ray costs are ragged (a miss is a few node steps, a deep mesh ray hundreds), so
// a one-ray-per-thread launch would idle most lanes; the scheduler tuning (a node quorum of 8 and wf_trace's vote
// weights); the instance chosen from the scene's stack need, with the LDS node prefix where the stacks fit in 16 entries.
// What is the query kernel's own:
//   - the work item is one ray, with its own window, time and RNG state;
//   - whole-record I/O: an 80-byte ray is five 16-byte loads, a 96-byte hit six 16-byte stores; the world-frame ray is
//     read again from the caller's buffer where it is needed instead of being kept in registers;
//   - the ANY instances (RT_FLAG_ANY_HIT);
//   - the scheduler loop, written out here as in every kernel (pt_traverse.hpp says why).
// All arithmetic is f64 through rt_math.h with -ffp-contract=off, so every record is the CPU oracle's bit for bit.
#include "pt_traverse.hpp"

namespace rt2022 {

namespace {

constexpr uint32_t kQHasRay = 1u;      // lane flag: the lane carries a ray (its record is written when it is done)

struct QLane : TravLane {
    // (the world-frame ray is not kept: the few steps that need it — leaving a mover, the winner's record — read it
    // again from the caller's buffer, which saves the twelve registers that decide whether the plain instance spills)
    uint64_t ray;          // index of the ray the lane carries
};

RT_DEV Ray q_world(const QueryArgs &a, const QLane &L) {
    const double2 *q = reinterpret_cast<const double2 *>(a.rays + L.ray);
    const double2 w0 = q[0], w1 = q[1], w2 = q[2];
    return Ray(Vec3(w0.x, w0.y, w1.x), Vec3(w1.y, w2.x, w2.y), L.tm);
}

// The lane's answer, as six 16-byte stores: {t, u} {v, p.x} {p.y, p.z} {n.x, n.y} {n.z, hit | front_face} {mat | prim, draws | 0}.
RT_DEV void q_write(const SceneDev &s, const QueryArgs &a, const QLane &L) {
    double t = 0.0, u = 0.0, v = 0.0;
    Vec3 p(0.0, 0.0, 0.0), n(0.0, 0.0, 0.0);
    uint32_t hit = 0, front = 0, mat = 0, prim = RT_REF_NONE;
    if (L.flags & kFound) {
        HitRec rec;
        winner_record(s, q_world(a, L), L.win, rec, true);
        t = rec.t; u = rec.u; v = rec.v; p = rec.p; n = rec.normal;
        hit = 1; front = rec.front_face ? 1u : 0u; mat = rec.mat & kMatIndexMask; prim = L.win.leaf;
    }
    double2 *o = reinterpret_cast<double2 *>(a.hits + L.ray);
    o[0] = make_double2(t, u);
    o[1] = make_double2(v, p.x);
    o[2] = make_double2(p.y, p.z);
    o[3] = make_double2(n.x, n.y);
    o[4] = make_double2(n.z, rtm::u2d((uint64_t)hit | ((uint64_t)front << 32)));
    o[5] = make_double2(rtm::u2d((uint64_t)mat | ((uint64_t)prim << 32)), rtm::u2d((uint64_t)L.rng.draws));
}

// Done: write the finished ray's record, then take the next ray (one atomic per wave for every lane that refills).
template <bool STATS>
RT_DEV void q_refill(const SceneDev &s, const QueryArgs &a, QLane &L, unsigned lane, Counters<STATS> &cnt) {
    if (L.flags & kQHasRay) {
        q_write(s, a, L);
        cnt.draws(L.rng.draws);
        L.flags = 0;
    }
    const unsigned long long i = wave_claim(a.counter, __ballot(true), lane);
    const bool have = i < a.n_rays;
    // (every field of the lane is written on both paths: the finished ray's state is dead from here on, and the registers
    // it held serve the record above)
    double2 w0 = make_double2(0.0, 0.0), w1 = w0, w2 = w0, w3 = w0, w4 = w0;
    if (have) {
        const double2 *q = reinterpret_cast<const double2 *>(a.rays + i);     // one 80-byte ray = five 16-byte loads
        w0 = q[0]; w1 = q[1]; w2 = q[2]; w3 = q[3]; w4 = q[4];
    }
    trav_begin(s, L, have, XRay{Vec3(w0.x, w0.y, w1.x), Vec3(w1.y, w2.x, w2.y)}, w3.x, w3.y, w4.x, Rng(rtm::d2u(w4.y)));
    L.ray = i;
    if (have) L.flags = kQHasRay;
}

} // namespace

// STACK: traversal stack entries; WG: threads per workgroup; CACHE: node records kept in LDS (0: none);
// STATS: counter instance; ANY: RT_FLAG_ANY_HIT.
template <int STACK, int WG, int CACHE, bool STATS, bool ANY>
__global__ void __launch_bounds__(WG, (STACK > 32 ? 2 : STATS ? 3 : 4)) pt_query(const SceneDev s, const QueryArgs a) {
    __shared__ uint32_t stack_lds[STACK * WG];
    __shared__ double node_lds[CACHE > 0 ? CACHE * kTravNodeDoubles : 1];
    const uint32_t n_cached = trav_cache_nodes<WG, CACHE>(s, node_lds);      // (the top levels of the BVHs)
    TravStack<STACK, WG> st{stack_lds + threadIdx.x};
    const unsigned lane = threadIdx.x & 63u;
    Counters<STATS> cnt;

    QLane L;
    trav_lane_clear(L);
    L.ray = 0;

    const auto world = [&] { const Ray w = q_world(a, L); return XRay{w.orig, w.dir}; };
    for (;;) {
        // Fast path: keep stepping nodes while enough lanes want to.
        for (;;) {
            const bool isn = L.op == OP_NODE;
            if (__popcll(__ballot(isn)) < kQueryNodeQuorum) break;
            if (isn) trav_node<ANY, STACK, WG, CACHE, STATS>(s, node_lds, n_cached, L, st, cnt);
        }
        // Vote: the label with the largest lanes x weight (ties -> lowest id).
        int best = -1, best_n = 0;
#pragma unroll
        for (int o = 0; o < (int)OP_COUNT; o++) {
            const int n = __popcll(__ballot(L.op == (uint32_t)o)) * (int)((kQueryVoteWeights >> (4 * o)) & 0xFu);
            if (n > best_n) { best_n = n; best = o; }
        }
        if (best < 0) break;                               // every lane idle: no rays left
        if (L.op == (uint32_t)best) {
            switch (best) {
                case OP_NODE: trav_node<ANY, STACK, WG, CACHE, STATS>(s, node_lds, n_cached, L, st, cnt); break;
                case OP_SPHERE: trav_sphere<ANY>(s, L, st, cnt); break;
                case OP_RECT: trav_rect<ANY>(s, L, st, cnt); break;
                case OP_BOX: trav_box<ANY>(s, L, st, cnt); break;
                case OP_MEDIUM: trav_medium<ANY>(s, L, st, cnt); break;
                case OP_MISC: trav_misc<ANY>(s, L, st, cnt); break;
                case OP_CTX: trav_ctx<ANY>(s, L, st, cnt, world); break;
                default: q_refill<STATS>(s, a, L, lane, cnt); break;
            }
        }
    }
    if (STATS) cnt.flush_wave(a.stats);
}

hipError_t launch_query(const SceneDev &scene, const QueryArgs &args, uint32_t stack_need, bool counters, bool any_hit,
                        hipStream_t stream) {
    if (args.n_rays == 0) return hipSuccess;
    return trav_dispatch(stack_need, [&](auto shape) {
        using S = decltype(shape);
        void (*const kernel)(SceneDev, QueryArgs) =
            counters ? (any_hit ? pt_query<S::stack, S::wg, S::cache, true, true> : pt_query<S::stack, S::wg, S::cache, true, false>)
                     : (any_hit ? pt_query<S::stack, S::wg, S::cache, false, true> : pt_query<S::stack, S::wg, S::cache, false, false>);
        return launch_persistent(kernel, S::wg, args.n_rays, scene, args, stream);
    });
}

} // namespace rt2022
