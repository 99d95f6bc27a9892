// pt_query.hip — batched closest-hit queries on a device scene (rt_intersect*, include/rt2022.h).
//
// `world.hit(r, t_min, t_max)` for caller-supplied rays, without rendering: the megakernel's traversal (pt_traverse.hpp)
// on its own, with each ray's own window, time and RNG state, and the winner's full HitRecord written back. What is the
// query kernel's own:
//   - persistent grid, one ray per lane, wave64: a lane whose ray is done writes its record and takes the next one from
//     a global counter, one atomic per wave for all the lanes that refill together (__ballot / __popcll / __shfl) — ray
//     costs are ragged (a miss is a few node steps, a deep mesh ray hundreds), so a one-ray-per-thread launch would idle
//     most lanes;
//   - its scheduler tuning: a node quorum of 8 and wf_trace's vote weights (below);
//   - the traversal stack's depth chosen from the scene's stack need; where the stacks fit in 16 entries, one 1024-thread
//     workgroup per CU and the first kNodeCache node records in LDS (the nodes are numbered breadth-first at upload: a
//     prefix copy is the top levels of the BVHs);
//   - whole-record I/O: an 80-byte ray is five 16-byte loads, a 96-byte hit six 16-byte stores; the world-frame ray is
//     read again from the caller's buffer where it is needed instead of being kept in registers.
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
    const unsigned long long m = __ballot(true);
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(a.counter, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    const unsigned long long i = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    const bool have = i < a.n_rays;
    // (every field of the lane is written on both paths: the finished ray's state is dead from here on, and the registers
    // it held serve the record above)
    double2 w0 = make_double2(0.0, 0.0), w1 = w0, w2 = w0, w3 = w0, w4 = w0;
    if (have) {
        const double2 *q = reinterpret_cast<const double2 *>(a.rays + i);     // one 80-byte ray = five 16-byte loads
        w0 = q[0]; w1 = q[1]; w2 = q[2]; w3 = q[3]; w4 = q[4];
    }
    L.tm = w3.x;
    trav_set_cur(L, XRay{Vec3(w0.x, w0.y, w1.x), Vec3(w1.y, w2.x, w2.y)});
    L.t_min = w3.y;
    L.t_lo = w3.y;
    L.closest = w4.x;
    L.sub_closest = 0.0;
    L.med_t1 = 0.0;
    L.med_ref = 0;
    L.rng = Rng(rtm::d2u(w4.y));
    L.win.t = 0.0; L.win.leaf = 0; L.win.face = 0;
    L.ctx.c0 = L.ctx.c1 = L.ctx.c2 = L.ctx.c3 = 0; L.ctx.n = 0;
    L.win.chain = L.ctx;
    L.ray = i;
    L.sp = 0;
    L.flags = have ? kQHasRay : 0u;
    L.top = have ? s.root : REF_EMPTY;
    L.op = have ? classify(L.top) : (uint32_t)OP_IDLE;
}

} // namespace

// Lanes that must want a node step for the wave to keep taking the fast path. 8 rather than the render kernels' 18: measured
// with the weights below, +8 % on the headline's bounce rays and +9 % on C2's, -3 % on C5's (12: +2 %, +5 %, +-0).
constexpr int kQueryNodeQuorum = 8;
// Vote weights, four bits per label from the lowest nibble up (node, sphere, rect, box, medium, misc, ctx, done): the wave
// runs the label with the largest lanes x weight. Node steps and the refill yield to the leaf arms, like wf_trace's weights:
// measured against plain counts on the workloads of tools/query_bench.py, +20 % on the headline's bounce rays, +5-10 % on the
// others; a refill weighted up (done x 2) was 1-20 % slower.
constexpr uint32_t kQueryVoteWeights = 0x24444442u;

// STACK: traversal stack entries; WG: threads per workgroup; CACHE: node records kept in LDS (0: none);
// STATS: counter instance; ANY: RT_FLAG_ANY_HIT.
template <int STACK, int WG, int CACHE, bool STATS, bool ANY>
__global__ void __launch_bounds__(WG, (STACK > 32 ? 2 : STATS ? 3 : 4)) pt_query(const SceneDev s, const QueryArgs a) {
    __shared__ uint32_t stack_lds[STACK * WG];
    __shared__ double node_lds[CACHE > 0 ? CACHE * kTravNodeDoubles : 1];
    const uint32_t n_cached = CACHE > 0 ? (s.n_nodes < (uint32_t)CACHE ? s.n_nodes : (uint32_t)CACHE) : 0u;
    if (CACHE > 0) {                                       // prefix copy: the top levels of the BVHs (breadth-first numbering)
        for (uint32_t i = threadIdx.x; i < n_cached; i += WG) {
            const rt_bvh_node &q = s.nodes[i];
            double *d = node_lds + (size_t)i * kTravNodeDoubles;
            d[0] = q.bmin[0]; d[1] = q.bmin[1]; d[2] = q.bmin[2];
            d[3] = q.bmax[0]; d[4] = q.bmax[1]; d[5] = q.bmax[2];
            d[6] = rtm::u2d((uint64_t)q.left | ((uint64_t)q.right << 32));
        }
        __syncthreads();
    }
    TravStack<STACK, WG> st{stack_lds + threadIdx.x};
    const unsigned lane = threadIdx.x & 63u;
    Counters<STATS> cnt;

    QLane L;
    L.tm = 0.0;
    trav_set_cur(L, XRay{Vec3(0.0, 0.0, 0.0), Vec3(0.0, 0.0, 0.0)});
    L.t_min = L.t_lo = L.closest = L.sub_closest = L.med_t1 = 0.0;
    L.med_ref = 0;
    L.ctx.c0 = L.ctx.c1 = L.ctx.c2 = L.ctx.c3 = 0; L.ctx.n = 0;
    L.win.t = 0.0; L.win.leaf = 0; L.win.face = 0; L.win.chain = L.ctx;
    L.ray = 0; L.sp = 0; L.top = REF_EMPTY; L.op = OP_SHADE; L.flags = 0;

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

namespace {

template <int STACK, int WG, int CACHE, bool STATS, bool ANY>
hipError_t launch_one(const SceneDev &scene, const QueryArgs &args, hipStream_t stream) {
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, pt_query<STACK, WG, CACHE, STATS, ANY>, WG, 0);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    const uint64_t want = (args.n_rays + WG - 1) / WG;
    uint64_t blocks = (uint64_t)per_cu * (uint64_t)(cus > 0 ? cus : 1);
    if (blocks > want) blocks = want ? want : 1;
    hipLaunchKernelGGL((pt_query<STACK, WG, CACHE, STATS, ANY>), dim3((unsigned)blocks), dim3(WG), 0, stream, scene, args);
    return hipGetLastError();
}
template <int STACK, int WG, int CACHE>
hipError_t launch_flags(const SceneDev &scene, const QueryArgs &args, bool counters, bool any_hit, hipStream_t stream) {
    if (counters) return any_hit ? launch_one<STACK, WG, CACHE, true, true>(scene, args, stream) : launch_one<STACK, WG, CACHE, true, false>(scene, args, stream);
    return any_hit ? launch_one<STACK, WG, CACHE, false, true>(scene, args, stream) : launch_one<STACK, WG, CACHE, false, false>(scene, args, stream);
}

} // namespace

hipError_t launch_query(const SceneDev &scene, const QueryArgs &args, uint32_t stack_need, bool counters, bool any_hit,
                        hipStream_t stream) {
    if (args.n_rays == 0) return hipSuccess;
    if (stack_need > (uint32_t)kStackLarge) return hipErrorInvalidValue;
    if (stack_need <= (uint32_t)kStackTiny) return launch_flags<kStackTiny, kCacheBlock, kNodeCache>(scene, args, counters, any_hit, stream);
    if (stack_need <= (uint32_t)kStackSmall) return launch_flags<kStackSmall, kBlock, 0>(scene, args, counters, any_hit, stream);
    if (stack_need <= (uint32_t)kStackMid) return launch_flags<kStackMid, kBlock, 0>(scene, args, counters, any_hit, stream);
    return launch_flags<kStackLarge, kBlock, 0>(scene, args, counters, any_hit, stream);
}

} // namespace rt2022
