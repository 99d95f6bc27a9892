// pt_traverse.hpp — the f64 closest-hit traversal of the megakernel (pt_kernel.hip), the query kernel (pt_query.hip) and
// the feature kernel (pt_features.hip): the lane's traversal state, its LDS stack and the arms of the in-wave voted
// scheduler. The caller owns the world-frame ray, the done arm and the scheduler loop. (wf_trace, pt_wavefront.hip, has
// its own tuned copy.) At the end, the shell the two persistent closest-hit kernels share around their loops: the LDS
// node prefix, the lane's state before the loop and at the start of a ray, the one-atomic-per-wave claim of work (the
// megakernel's too), their scheduler tuning, and the launch side (occupancy-sized grid, instance by stack need). A helper
// is used where it leaves the kernel's register allocation as it was (tools/kernel_resources.py): the feature kernel,
// whose 1024-thread instance spills, keeps the node prefix and the lane's first state written out.
//
// The scheduler: every lane carries a label naming its next operation (node step, sphere, rect, box, medium, misc leaf,
// mover / list, done) and the wave runs the label that weighs most, with all the lanes that wait for it, and a fast path
// that keeps stepping nodes while enough lanes want to (a plain per-lane switch ran at 8 % lane utilisation). A lane's own
// sequence of operations — and so its RNG stream and hit order — never changes, only when it gets its turn. Each kernel
// writes that loop itself, around these arms: as a shared inline function it changed the query kernel's register
// allocation and made it slower.
// Per-lane semantics are the reference's: nodes in its order (left, then right against the closest hit so far,
// bvh/mod.rs:86-101), ConstantMedium's two boundary queries and its draw (constantmedium.rs:49-83), the record rebuilt
// for the winner only.
#ifndef RT2022_PT_TRAVERSE_HPP
#define RT2022_PT_TRAVERSE_HPP

#include "pt_common.hpp"

namespace rt2022 {

namespace {

// Lane flags, one vector register (a bool member would live as a lane mask in scalar registers and be merged at every
// join of the scheduler's control flow). Bit 0 is the caller's.
constexpr uint32_t kFound = 2u;        // the main query has accepted a candidate
constexpr uint32_t kSubFound = 4u;     // the medium boundary query in progress has found a hit

struct TravLane {
    // (the world-frame ray is the caller's: leaving a mover asks the caller for it)
    double tm;             // Ray::tm
    XRay cur;              // the ray inside the enclosing movers
    Vec3 inv;              // 1 / cur.d (aabb.rs:19, hoisted: same value at every node)
    double a_len;          // cur.d.length_sqr() (sphere.rs:41, hoisted likewise)
    double t_min;          // the ray's own lower bound
    // ConstantMedium::hit asks its boundary two closest-hit questions of its own (constantmedium.rs:50-51) when the
    // boundary is more than one plain sphere. They run through the same operations as the main query against
    // (t_lo, sub_closest) instead of (t_min, closest) and never touch the winner.
    double t_lo;           // lower bound in force: t_min, or the boundary query's
    double closest;        // upper bound of the main query: t_max, then the closest accepted t
    double sub_closest;
    double med_t1;         // the first boundary query's answer
    uint32_t med_ref;      // the medium whose boundary is being queried (0: none — a medium ref is never 0)
    Rng rng;
    Winner win;
    Chain ctx;
    int sp;
    uint32_t top, op, flags;
};

template <int STACK, int WG>
struct TravStack {
    uint32_t *col;         // this lane's column: entry d at col[d * WG]
    RT_DEV void push(TravLane &L, uint32_t ref) { if (L.sp < STACK) { col[L.sp * WG] = ref; L.sp++; } }
    RT_DEV uint32_t pop(TravLane &L) { if (L.sp > 0) { L.sp--; return col[L.sp * WG]; } return REF_EMPTY; }
};

RT_DEV void trav_set_cur(TravLane &L, const XRay &c) {
    L.cur = c;
    L.inv = Vec3(1.0 / c.d.x, 1.0 / c.d.y, 1.0 / c.d.z);
    L.a_len = c.d.length_sqr();
}
RT_DEV double trav_hi(const TravLane &L) { return L.med_ref ? L.sub_closest : L.closest; }
RT_DEV void trav_win(TravLane &L, double t, uint32_t leaf, uint32_t face) {
    L.closest = t;
    L.flags |= kFound;
    L.win.t = t; L.win.leaf = leaf; L.win.face = face; L.win.chain = L.ctx;
}
RT_DEV void trav_accept(TravLane &L, double t, uint32_t face) {
    if (L.med_ref) { L.sub_closest = t; L.flags |= kSubFound; return; }
    trav_win(L, t, L.top, face);
}
// The next entry of the stack — or, for an any-hit query that has accepted a candidate, the end of the ray.
template <bool ANY, int STACK, int WG>
RT_DEV void trav_next(TravLane &L, TravStack<STACK, WG> &st) {
    if (ANY && (L.flags & kFound)) { L.op = OP_SHADE; return; }
    L.top = st.pop(L);
    L.op = classify(L.top);
}

// A node record in LDS: bmin xyz, bmax xyz, then {left, right} in the seventh double (56 bytes).
constexpr int kTravNodeDoubles = 7;

// BvhNode::hit, bvh/mod.rs:86-101 + AABB::hit, aabb.rs:15-32. The left child is taken at once, the right one waits on
// the stack and is tested against the then-closest hit.
template <bool ANY, int STACK, int WG, int CACHE, bool STATS>
RT_DEV void trav_node(const SceneDev &s, const double *node_lds, uint32_t n_cached, TravLane &L, TravStack<STACK, WG> &st,
                      Counters<STATS> &cnt) {
    cnt.node();
    const uint32_t idx = RT_REF_INDEX(L.top);
    double b[6];
    uint64_t lr;
    if (CACHE > 0 && idx < n_cached) {
        const double *q = node_lds + (size_t)idx * kTravNodeDoubles;
#pragma unroll
        for (int i = 0; i < 6; i++) b[i] = q[i];
        lr = rtm::d2u(q[6]);
    } else {
        const double2 *q = reinterpret_cast<const double2 *>(s.nodes + idx);   // one 64-byte record = four 16-byte loads
        const double2 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
        b[0] = w0.x; b[1] = w0.y; b[2] = w1.x; b[3] = w1.y; b[4] = w2.x; b[5] = w2.y;
        lr = rtm::d2u(w3.x);
    }
    double tmn = L.t_lo, tmx = trav_hi(L);
    bool miss = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const double inv_d = L.inv[i];
        double t0 = (b[i] - L.cur.o[i]) * inv_d;
        double t1 = (b[3 + i] - L.cur.o[i]) * inv_d;
        if (inv_d < 0.0) { const double tmp = t0; t0 = t1; t1 = tmp; }
        tmn = t0 > tmn ? t0 : tmn;
        tmx = t1 < tmx ? t1 : tmx;
        miss = miss || (tmx <= tmn);
    }
    if (!miss) {
        st.push(L, (uint32_t)(lr >> 32));
        L.top = (uint32_t)lr;
        L.op = classify(L.top);
    } else {
        trav_next<ANY>(L, st);
    }
}

template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void trav_sphere(const SceneDev &s, TravLane &L, TravStack<STACK, WG> &st, Counters<STATS> &cnt) {
    const uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
    cnt.prim(kind);
    Vec3 center;
    double radius;
    if (kind == RT_KIND_SPHERE) { const rt_sphere &q = s.spheres[idx]; center = ld3(q.center); radius = q.radius; }
    else { const rt_moving_sphere &q = s.moving_spheres[idx]; center = moving_center(q, L.tm); radius = q.radius; }
    double t;
    if (sphere_t(center, radius, L.cur, L.a_len, L.t_lo, trav_hi(L), t)) trav_accept(L, t, 0);
    trav_next<ANY>(L, st);
}
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void trav_rect(const SceneDev &s, TravLane &L, TravStack<STACK, WG> &st, Counters<STATS> &cnt) {
    cnt.prim(RT_KIND_RECT);
    const rt_rect &q = s.rects[RT_REF_INDEX(L.top)];
    double t;
    if (rect_t(q.axis, q.a0, q.a1, q.b0, q.b1, q.k, L.cur, L.t_lo, trav_hi(L), t)) trav_accept(L, t, 0);
    trav_next<ANY>(L, st);
}
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void trav_box(const SceneDev &s, TravLane &L, TravStack<STACK, WG> &st, Counters<STATS> &cnt) {
    cnt.prim(RT_KIND_BOX);
    double t;
    uint32_t face = 0;
    if (box_t(s.boxes[RT_REF_INDEX(L.top)], L.cur, L.t_lo, trav_hi(L), t, face)) trav_accept(L, t, face);
    trav_next<ANY>(L, st);
}
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void trav_misc(const SceneDev &s, TravLane &L, TravStack<STACK, WG> &st, Counters<STATS> &cnt) {
    const uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
    cnt.prim(kind);
    double t;
    const bool h = kind == RT_KIND_TRIANGLE ? triangle_t(s.triangles[idx], L.cur, L.t_lo, trav_hi(L), t)
                                            : ring_t(s.rings[idx], L.cur, L.t_lo, trav_hi(L), t);
    if (h) trav_accept(L, t, 0);
    trav_next<ANY>(L, st);
}

// The end of ConstantMedium::hit once both boundary answers are in (constantmedium.rs:52-74).
RT_DEV void trav_medium_finish(TravLane &L, uint32_t med, double neg_inv_density, double t1, double t2) {
    t1 = rtm::fmax_(t1, L.t_min);
    t2 = rtm::fmin_(t2, L.closest);
    if (t1 >= t2) return;
    t1 = rtm::fmax_(t1, 0.0);
    const double ray_length = L.cur.d.length();
    const double distance_inside_boundary = (t2 - t1) * ray_length;
    const double rnd = L.rng.gen_f64();
    const double hit_distance = neg_inv_density * (rtm::log_(rnd) / rtm::log_(rtm::E_));
    if (hit_distance > distance_inside_boundary) return;
    trav_win(L, t1 + hit_distance / ray_length, med, 0);
}
// ConstantMedium::hit (constantmedium.rs:49-83). Three entries: the medium itself, and the two stack sentinels that
// mark the end of its first / second boundary query. A boundary that is one plain Sphere is answered on the spot, both
// queries from the medium's own record (the same sphere_t calls, counted the same way as a traversal would count them).
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void trav_medium(const SceneDev &s, TravLane &L, TravStack<STACK, WG> &st, Counters<STATS> &cnt) {
    const uint32_t top = L.top;
    if (RT_REF_KIND(top) == RT_KIND_MEDIUM) {
        cnt.prim(RT_KIND_MEDIUM);
        const MediumDev &m = s.media_dev[RT_REF_INDEX(top)];
        if (m.sphere_boundary) {
            const Vec3 center = ld3(m.center);
            double t1, t2;
            cnt.prim(RT_KIND_SPHERE);
            if (sphere_t(center, m.radius, L.cur, L.a_len, -rtm::INF, rtm::INF, t1)) {
                cnt.prim(RT_KIND_SPHERE);
                if (sphere_t(center, m.radius, L.cur, L.a_len, t1 + 0.0001, rtm::INF, t2)) trav_medium_finish(L, top, m.neg_inv_density, t1, t2);
            }
            trav_next<ANY>(L, st);
            return;
        }
        L.med_ref = top;                                   // boundary.hit(r, -inf, inf)
        L.t_lo = -rtm::INF;
        L.sub_closest = rtm::INF;
        L.flags &= ~kSubFound;
        st.push(L, REF_MED1);
        L.top = m.boundary;
        L.op = classify(L.top);
        return;
    }
    const MediumDev &m = s.media_dev[RT_REF_INDEX(L.med_ref)];
    const bool found = (L.flags & kSubFound) != 0;
    if (top == REF_MED1 && found) {                        // boundary.hit(r, rec1.t + 0.0001, inf)
        L.med_t1 = L.sub_closest;
        L.t_lo = L.med_t1 + 0.0001;
        L.sub_closest = rtm::INF;
        L.flags &= ~kSubFound;
        st.push(L, REF_MED2);
        L.top = m.boundary;
        L.op = classify(L.top);
        return;
    }
    const uint32_t med = L.med_ref;
    L.med_ref = 0;
    L.t_lo = L.t_min;
    if (top == REF_MED2 && found) trav_medium_finish(L, med, m.neg_inv_density, L.med_t1, L.sub_closest);
    trav_next<ANY>(L, st);
}

// Translate / RotateY / Zoom entry and exit; HittableList expansion (mod.rs:90-100). Leaving a mover rebuilds the ray
// from the world-frame one, which `world()` returns as an XRay.
template <bool ANY, int STACK, int WG, bool STATS, class World>
RT_DEV void trav_ctx(const SceneDev &s, TravLane &L, TravStack<STACK, WG> &st, Counters<STATS> &cnt, World world) {
    if (L.top == REF_POPCTX) {
        L.ctx.n--;
        trav_set_cur(L, ray_at_level(s, L.ctx, L.ctx.n, world()));
        trav_next<ANY>(L, st);
        return;
    }
    const uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
    cnt.prim(kind);
    if (kind == RT_KIND_LIST) {
        const rt_list &l = s.lists[idx];
        for (uint32_t i = l.count; i > 0; i--) st.push(L, s.list_items[l.first + i - 1]);
        trav_next<ANY>(L, st);
        return;
    }
    if (L.ctx.n < RT_MAX_XFORM_DEPTH) {
        L.ctx.push(L.top);
        trav_set_cur(L, xform_ray(s, L.top, L.cur));
        st.push(L, REF_POPCTX);
        L.top = s.xforms[idx].child;
        L.op = classify(L.top);
    } else {
        trav_next<ANY>(L, st);
    }
}

// ---- the shell of the persistent closest-hit kernels (pt_query, pt_features) --------------------------------------

// Lanes that must want a node step for the wave to keep taking the fast path. 8 rather than the render kernels' 18: measured
// with the weights below, +8 % on the headline's bounce rays and +9 % on C2's, -3 % on C5's (12: +2 %, +5 %, +-0).
constexpr int kQueryNodeQuorum = 8;
// Vote weights, four bits per label from the lowest nibble up (node, sphere, rect, box, medium, misc, ctx, done): the wave
// runs the label with the largest lanes x weight. Node steps and the refill yield to the leaf arms, like wf_trace's weights:
// measured against plain counts on the workloads of tools/query_bench.py, +20 % on the headline's bounce rays, +5-10 % on the
// others; a refill weighted up (done x 2) was 1-20 % slower.
// (Measured on the query kernel's caller rays. The feature kernel takes both as they are: camera rays of neighbouring
// pixels are more coherent than those, and nothing has been measured there that would justify other values.)
constexpr uint32_t kQueryVoteWeights = 0x24444442u;

// The first CACHE node records into LDS, by the whole workgroup (the nodes are numbered breadth-first at upload: a prefix
// copy is the top levels of the BVHs). Returns how many there are; CACHE 0: none, and nothing is done.
template <int WG, int CACHE>
RT_DEV uint32_t trav_cache_nodes(const SceneDev &s, double *node_lds) {
    const uint32_t n_cached = CACHE > 0 ? (s.n_nodes < (uint32_t)CACHE ? s.n_nodes : (uint32_t)CACHE) : 0u;
    if (CACHE > 0) {
        for (uint32_t i = threadIdx.x; i < n_cached; i += WG) {
            const rt_bvh_node &q = s.nodes[i];
            double *d = node_lds + (size_t)i * kTravNodeDoubles;
            d[0] = q.bmin[0]; d[1] = q.bmin[1]; d[2] = q.bmin[2];
            d[3] = q.bmax[0]; d[4] = q.bmax[1]; d[5] = q.bmax[2];
            d[6] = rtm::u2d((uint64_t)q.left | ((uint64_t)q.right << 32));
        }
        __syncthreads();
    }
    return n_cached;
}

// The lane before the loop: no ray, waiting for the done arm. (The kernel zeroes the fields it adds.)
RT_DEV void trav_lane_clear(TravLane &L) {
    L.tm = 0.0;
    trav_set_cur(L, XRay{Vec3(0.0, 0.0, 0.0), Vec3(0.0, 0.0, 0.0)});
    L.t_min = L.t_lo = L.closest = L.sub_closest = L.med_t1 = 0.0;
    L.med_ref = 0;
    L.ctx.c0 = L.ctx.c1 = L.ctx.c2 = L.ctx.c3 = 0; L.ctx.n = 0;
    L.win.t = 0.0; L.win.leaf = 0; L.win.face = 0; L.win.chain = L.ctx;
    L.sp = 0; L.top = REF_EMPTY; L.op = OP_SHADE; L.flags = 0;
}

// The start of world.hit(r, t_min, t_max) at the root, r = (cur, tm) with `rng` behind it — or, `have` false, nothing left:
// the lane idles. Every field of TravLane is written on both paths (the finished ray's state is dead from here on); flag
// bit 0 is the caller's to set afterwards.
RT_DEV void trav_begin(const SceneDev &s, TravLane &L, bool have, const XRay &cur, double tm, double t_min, double t_max,
                       const Rng &rng) {
    L.tm = tm;
    trav_set_cur(L, cur);
    L.t_min = t_min;
    L.t_lo = t_min;
    L.closest = t_max;
    L.sub_closest = 0.0;
    L.med_t1 = 0.0;
    L.med_ref = 0;
    L.rng = rng;
    L.win.t = 0.0; L.win.leaf = 0; L.win.face = 0;
    L.ctx.c0 = L.ctx.c1 = L.ctx.c2 = L.ctx.c3 = 0; L.ctx.n = 0;
    L.win.chain = L.ctx;
    L.sp = 0;
    L.flags = 0;
    L.top = have ? s.root : REF_EMPTY;
    L.op = have ? classify(L.top) : (uint32_t)OP_IDLE;
}

// One work item for every lane of the wave that wants one, by one atomic per wave: the first such lane adds their number to
// *counter, and each takes its place behind the base. `m`: their __ballot, not empty — the caller's, because where it
// is taken against the caller's branches is a matter of register allocation there. (The answer of a lane that wants none
// means nothing.)
RT_DEV unsigned long long wave_claim(unsigned long long *counter, unsigned long long m, unsigned lane) {
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    return base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
}

// A persistent grid of `kernel` (workgroups of `wg` threads): as many workgroups as the device holds at once, at most what
// n_work items at one per lane ask for.
template <class Args>
hipError_t launch_persistent(void (*kernel)(SceneDev, Args), int wg, uint64_t n_work, const SceneDev &scene, const Args &args,
                             hipStream_t stream) {
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, wg, 0);
    if (e != hipSuccess) return e;
    if (per_cu < 1) per_cu = 1;
    const uint64_t want = (n_work + wg - 1) / wg;
    uint64_t blocks = (uint64_t)per_cu * (uint64_t)(cus > 0 ? cus : 1);
    if (blocks > want) blocks = want ? want : 1;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(wg), 0, stream, scene, args);
    return hipGetLastError();
}

// The instance a scene's stack need selects: f(TravShape<STACK, WG, CACHE>) launches it. Where the stacks fit in kStackTiny
// entries, one kCacheBlock-thread workgroup per CU with the first kNodeCache node records in LDS.
template <int STACK, int WG, int CACHE>
struct TravShape { static constexpr int stack = STACK, wg = WG, cache = CACHE; };
template <class F>
hipError_t trav_dispatch(uint32_t stack_need, F f) {
    if (stack_need > (uint32_t)kStackLarge) return hipErrorInvalidValue;
    if (stack_need <= (uint32_t)kStackTiny) return f(TravShape<kStackTiny, kCacheBlock, kNodeCache>{});
    if (stack_need <= (uint32_t)kStackSmall) return f(TravShape<kStackSmall, kBlock, 0>{});
    if (stack_need <= (uint32_t)kStackMid) return f(TravShape<kStackMid, kBlock, 0>{});
    return f(TravShape<kStackLarge, kBlock, 0>{});
}

} // namespace

} // namespace rt2022
#endif
