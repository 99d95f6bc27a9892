// pt_query.hip — batched closest-hit queries on a device scene (rt_intersect*, include/rt2022.h).
//
// `world.hit(r, t_min, t_max)` for caller-supplied rays, without rendering: the traversal of the render kernels on its
// own, with each ray's own window, time and RNG state, and the winner's full HitRecord written back.
//
// Shape (what the render kernels measured on this chip):
//   - persistent grid, one ray per lane, wave64: a lane whose ray is done takes the next one from a global counter,
//     one atomic per wave for all the lanes that refill together (__ballot / __popcll / __shfl) — ray costs are ragged
//     (a miss is a few node steps, a deep mesh ray hundreds), so a one-ray-per-thread launch would idle most lanes;
//   - the in-wave voted scheduler: every lane carries a label naming its next operation (node step, sphere, rect, box,
//     medium, misc leaf, mover / list, done) and the wave runs the label most lanes wait for, with a fast path that
//     keeps stepping nodes while enough lanes want to (a plain per-lane switch ran at 8 % lane utilisation);
//   - the traversal stack in LDS as [depth][lane] (bank = lane); its depth chosen from the scene's stack need;
//   - where the stacks fit in 16 entries, one 1024-thread workgroup per CU and the first kNodeCache node records in
//     LDS (the nodes are numbered breadth-first at upload: a prefix copy is the top levels of the BVHs);
//   - whole-record I/O: an 80-byte ray is five 16-byte loads, a 96-byte hit six 16-byte stores.
// Per-lane semantics are the reference's: nodes in its order (left, then right against the closest hit so far,
// bvh/mod.rs:86-101), ConstantMedium's two boundary queries and its draw (constantmedium.rs:49-83), the record rebuilt
// for the winner only. All arithmetic is f64 through rt_math.h with -ffp-contract=off, so every record is the CPU
// oracle's bit for bit.
#include "pt_common.hpp"

namespace rt2022 {

namespace {

// Lane flags, one vector register (a bool member would live as a lane mask in scalar registers and be merged at every
// join of the scheduler's control flow).
constexpr uint32_t kQHasRay = 1u;      // the lane carries a ray (its record is written when it is done)
constexpr uint32_t kQFound = 2u;       // the main query has accepted a candidate
constexpr uint32_t kQSubFound = 4u;    // the medium boundary query in progress has found a hit

struct QLane {
    // (the world-frame ray is not kept: the few steps that need it — leaving a mover, the winner's record — read it
    // again from the caller's buffer, which saves the twelve registers that decide whether the plain instance spills)
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
    uint64_t ray;          // index of the ray the lane carries
    int sp;
    uint32_t top, op, flags;
};

template <int STACK, int WG>
struct QStack {
    uint32_t *col;         // this lane's column: entry d at col[d * WG]
    RT_DEV void push(QLane &L, uint32_t ref) { if (L.sp < STACK) { col[L.sp * WG] = ref; L.sp++; } }
    RT_DEV uint32_t pop(QLane &L) { if (L.sp > 0) { L.sp--; return col[L.sp * WG]; } return REF_EMPTY; }
};

RT_DEV void q_set_cur(QLane &L, const XRay &c) {
    L.cur = c;
    L.inv = Vec3(1.0 / c.d.x, 1.0 / c.d.y, 1.0 / c.d.z);
    L.a_len = c.d.length_sqr();
}
RT_DEV Ray q_world(const QueryArgs &a, const QLane &L) {
    const double2 *q = reinterpret_cast<const double2 *>(a.rays + L.ray);
    const double2 w0 = q[0], w1 = q[1], w2 = q[2];
    return Ray(Vec3(w0.x, w0.y, w1.x), Vec3(w1.y, w2.x, w2.y), L.tm);
}
RT_DEV double q_hi(const QLane &L) { return L.med_ref ? L.sub_closest : L.closest; }
RT_DEV void q_win(QLane &L, double t, uint32_t leaf, uint32_t face) {
    L.closest = t;
    L.flags |= kQFound;
    L.win.t = t; L.win.leaf = leaf; L.win.face = face; L.win.chain = L.ctx;
}
RT_DEV void q_accept(QLane &L, double t, uint32_t face) {
    if (L.med_ref) { L.sub_closest = t; L.flags |= kQSubFound; return; }
    q_win(L, t, L.top, face);
}
// The next entry of the stack — or, for an any-hit query that has accepted a candidate, the end of the ray.
template <bool ANY, int STACK, int WG>
RT_DEV void q_next(QLane &L, QStack<STACK, WG> &st) {
    if (ANY && (L.flags & kQFound)) { L.op = OP_SHADE; return; }
    L.top = st.pop(L);
    L.op = classify(L.top);
}

// A node record in LDS: bmin xyz, bmax xyz, then {left, right} in the seventh double (56 bytes).
constexpr int kQNodeDoubles = 7;

// BvhNode::hit, bvh/mod.rs:86-101 + AABB::hit, aabb.rs:15-32. The left child is taken at once, the right one waits on
// the stack and is tested against the then-closest hit.
template <bool ANY, int STACK, int WG, int CACHE, bool STATS>
RT_DEV void q_node(const SceneDev &s, const double *node_lds, uint32_t n_cached, QLane &L, QStack<STACK, WG> &st,
                   Counters<STATS> &cnt) {
    cnt.node();
    const uint32_t idx = RT_REF_INDEX(L.top);
    double b[6];
    uint64_t lr;
    if (CACHE > 0 && idx < n_cached) {
        const double *q = node_lds + (size_t)idx * kQNodeDoubles;
#pragma unroll
        for (int i = 0; i < 6; i++) b[i] = q[i];
        lr = rtm::d2u(q[6]);
    } else {
        const double2 *q = reinterpret_cast<const double2 *>(s.nodes + idx);   // one 64-byte record = four 16-byte loads
        const double2 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
        b[0] = w0.x; b[1] = w0.y; b[2] = w1.x; b[3] = w1.y; b[4] = w2.x; b[5] = w2.y;
        lr = rtm::d2u(w3.x);
    }
    double tmn = L.t_lo, tmx = q_hi(L);
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
        q_next<ANY>(L, st);
    }
}

template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void q_sphere(const SceneDev &s, QLane &L, QStack<STACK, WG> &st, Counters<STATS> &cnt) {
    const uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
    cnt.prim(kind);
    Vec3 center;
    double radius;
    if (kind == RT_KIND_SPHERE) { const rt_sphere &q = s.spheres[idx]; center = ld3(q.center); radius = q.radius; }
    else { const rt_moving_sphere &q = s.moving_spheres[idx]; center = moving_center(q, L.tm); radius = q.radius; }
    double t;
    if (sphere_t(center, radius, L.cur, L.a_len, L.t_lo, q_hi(L), t)) q_accept(L, t, 0);
    q_next<ANY>(L, st);
}
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void q_rect(const SceneDev &s, QLane &L, QStack<STACK, WG> &st, Counters<STATS> &cnt) {
    cnt.prim(RT_KIND_RECT);
    const rt_rect &q = s.rects[RT_REF_INDEX(L.top)];
    double t;
    if (rect_t(q.axis, q.a0, q.a1, q.b0, q.b1, q.k, L.cur, L.t_lo, q_hi(L), t)) q_accept(L, t, 0);
    q_next<ANY>(L, st);
}
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void q_box(const SceneDev &s, QLane &L, QStack<STACK, WG> &st, Counters<STATS> &cnt) {
    cnt.prim(RT_KIND_BOX);
    double t;
    uint32_t face = 0;
    if (box_t(s.boxes[RT_REF_INDEX(L.top)], L.cur, L.t_lo, q_hi(L), t, face)) q_accept(L, t, face);
    q_next<ANY>(L, st);
}
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void q_misc(const SceneDev &s, QLane &L, QStack<STACK, WG> &st, Counters<STATS> &cnt) {
    const uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
    cnt.prim(kind);
    double t;
    const bool h = kind == RT_KIND_TRIANGLE ? triangle_t(s.triangles[idx], L.cur, L.t_lo, q_hi(L), t)
                                            : ring_t(s.rings[idx], L.cur, L.t_lo, q_hi(L), t);
    if (h) q_accept(L, t, 0);
    q_next<ANY>(L, st);
}

// The end of ConstantMedium::hit once both boundary answers are in (constantmedium.rs:52-74).
RT_DEV void q_medium_finish(QLane &L, uint32_t med, double neg_inv_density, double t1, double t2) {
    t1 = rtm::fmax_(t1, L.t_min);
    t2 = rtm::fmin_(t2, L.closest);
    if (t1 >= t2) return;
    t1 = rtm::fmax_(t1, 0.0);
    const double ray_length = L.cur.d.length();
    const double distance_inside_boundary = (t2 - t1) * ray_length;
    const double rnd = L.rng.gen_f64();
    const double hit_distance = neg_inv_density * (rtm::log_(rnd) / rtm::log_(rtm::E_));
    if (hit_distance > distance_inside_boundary) return;
    q_win(L, t1 + hit_distance / ray_length, med, 0);
}
// ConstantMedium::hit (constantmedium.rs:49-83). Three entries: the medium itself, and the two stack sentinels that
// mark the end of its first / second boundary query. A boundary that is one plain Sphere is answered on the spot, both
// queries from the medium's own record (the same sphere_t calls, counted the same way as a traversal would count them).
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void q_medium(const SceneDev &s, QLane &L, QStack<STACK, WG> &st, Counters<STATS> &cnt) {
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
                if (sphere_t(center, m.radius, L.cur, L.a_len, t1 + 0.0001, rtm::INF, t2)) q_medium_finish(L, top, m.neg_inv_density, t1, t2);
            }
            q_next<ANY>(L, st);
            return;
        }
        L.med_ref = top;                                   // boundary.hit(r, -inf, inf)
        L.t_lo = -rtm::INF;
        L.sub_closest = rtm::INF;
        L.flags &= ~kQSubFound;
        st.push(L, REF_MED1);
        L.top = m.boundary;
        L.op = classify(L.top);
        return;
    }
    const MediumDev &m = s.media_dev[RT_REF_INDEX(L.med_ref)];
    const bool found = (L.flags & kQSubFound) != 0;
    if (top == REF_MED1 && found) {                        // boundary.hit(r, rec1.t + 0.0001, inf)
        L.med_t1 = L.sub_closest;
        L.t_lo = L.med_t1 + 0.0001;
        L.sub_closest = rtm::INF;
        L.flags &= ~kQSubFound;
        st.push(L, REF_MED2);
        L.top = m.boundary;
        L.op = classify(L.top);
        return;
    }
    const uint32_t med = L.med_ref;
    L.med_ref = 0;
    L.t_lo = L.t_min;
    if (top == REF_MED2 && found) q_medium_finish(L, med, m.neg_inv_density, L.med_t1, L.sub_closest);
    q_next<ANY>(L, st);
}

// Translate / RotateY / Zoom entry and exit; HittableList expansion (mod.rs:90-100).
template <bool ANY, int STACK, int WG, bool STATS>
RT_DEV void q_ctx(const SceneDev &s, const QueryArgs &a, QLane &L, QStack<STACK, WG> &st, Counters<STATS> &cnt) {
    if (L.top == REF_POPCTX) {
        L.ctx.n--;
        const Ray w = q_world(a, L);
        q_set_cur(L, ray_at_level(s, L.ctx, L.ctx.n, XRay{w.orig, w.dir}));
        q_next<ANY>(L, st);
        return;
    }
    const uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
    cnt.prim(kind);
    if (kind == RT_KIND_LIST) {
        const rt_list &l = s.lists[idx];
        for (uint32_t i = l.count; i > 0; i--) st.push(L, s.list_items[l.first + i - 1]);
        q_next<ANY>(L, st);
        return;
    }
    if (L.ctx.n < RT_MAX_XFORM_DEPTH) {
        L.ctx.push(L.top);
        q_set_cur(L, xform_ray(s, L.top, L.cur));
        st.push(L, REF_POPCTX);
        L.top = s.xforms[idx].child;
        L.op = classify(L.top);
    } else {
        q_next<ANY>(L, st);
    }
}

// The lane's answer, as six 16-byte stores: {t, u} {v, p.x} {p.y, p.z} {n.x, n.y} {n.z, hit | front_face} {mat | prim, draws | 0}.
RT_DEV void q_write(const SceneDev &s, const QueryArgs &a, const QLane &L) {
    double t = 0.0, u = 0.0, v = 0.0;
    Vec3 p(0.0, 0.0, 0.0), n(0.0, 0.0, 0.0);
    uint32_t hit = 0, front = 0, mat = 0, prim = RT_REF_NONE;
    if (L.flags & kQFound) {
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
    q_set_cur(L, XRay{Vec3(w0.x, w0.y, w1.x), Vec3(w1.y, w2.x, w2.y)});
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
#ifndef RT2022_QUERY_QUORUM
#define RT2022_QUERY_QUORUM 8
#endif
constexpr int kQueryNodeQuorum = RT2022_QUERY_QUORUM;
// Vote weights, four bits per label from the lowest nibble up (node, sphere, rect, box, medium, misc, ctx, done): the wave
// runs the label with the largest lanes x weight. Node steps and the refill yield to the leaf arms, like wf_trace's weights:
// measured against plain counts on the workloads of tools/query_bench.py, +20 % on the headline's bounce rays, +5-10 % on the
// others; a refill weighted up (done x 2) was 1-20 % slower.
#ifndef RT2022_QUERY_WEIGHTS
#define RT2022_QUERY_WEIGHTS 0x24444442u
#endif
constexpr uint32_t kQueryVoteWeights = RT2022_QUERY_WEIGHTS;

// STACK: traversal stack entries; WG: threads per workgroup; CACHE: node records kept in LDS (0: none);
// STATS: counter instance; ANY: RT_FLAG_ANY_HIT.
template <int STACK, int WG, int CACHE, bool STATS, bool ANY>
__global__ void __launch_bounds__(WG, (STACK > 32 ? 2 : STATS ? 3 : 4)) pt_query(const SceneDev s, const QueryArgs a) {
    __shared__ uint32_t stack_lds[STACK * WG];
    __shared__ double node_lds[CACHE > 0 ? CACHE * kQNodeDoubles : 1];
    const uint32_t n_cached = CACHE > 0 ? (s.n_nodes < (uint32_t)CACHE ? s.n_nodes : (uint32_t)CACHE) : 0u;
    if (CACHE > 0) {                                       // prefix copy: the top levels of the BVHs (breadth-first numbering)
        for (uint32_t i = threadIdx.x; i < n_cached; i += WG) {
            const rt_bvh_node &q = s.nodes[i];
            double *d = node_lds + (size_t)i * kQNodeDoubles;
            d[0] = q.bmin[0]; d[1] = q.bmin[1]; d[2] = q.bmin[2];
            d[3] = q.bmax[0]; d[4] = q.bmax[1]; d[5] = q.bmax[2];
            d[6] = rtm::u2d((uint64_t)q.left | ((uint64_t)q.right << 32));
        }
        __syncthreads();
    }
    QStack<STACK, WG> st{stack_lds + threadIdx.x};
    const unsigned lane = threadIdx.x & 63u;
    Counters<STATS> cnt;

    QLane L;
    L.tm = 0.0;
    q_set_cur(L, XRay{Vec3(0.0, 0.0, 0.0), Vec3(0.0, 0.0, 0.0)});
    L.t_min = L.t_lo = L.closest = L.sub_closest = L.med_t1 = 0.0;
    L.med_ref = 0;
    L.ctx.c0 = L.ctx.c1 = L.ctx.c2 = L.ctx.c3 = 0; L.ctx.n = 0;
    L.win.t = 0.0; L.win.leaf = 0; L.win.face = 0; L.win.chain = L.ctx;
    L.ray = 0; L.sp = 0; L.top = REF_EMPTY; L.op = OP_SHADE; L.flags = 0;

    for (;;) {
        // Fast path: keep stepping nodes while enough lanes want to.
        for (;;) {
            const bool isn = L.op == OP_NODE;
            if (__popcll(__ballot(isn)) < kQueryNodeQuorum) break;
            if (isn) q_node<ANY, STACK, WG, CACHE, STATS>(s, node_lds, n_cached, L, st, cnt);
        }
        // Vote: the label most lanes are waiting on (ties -> lowest id).
        int best = -1, best_n = 0;
#pragma unroll
        for (int o = 0; o < (int)OP_COUNT; o++) {
            const int n = __popcll(__ballot(L.op == (uint32_t)o)) * (int)((kQueryVoteWeights >> (4 * o)) & 0xFu);
            if (n > best_n) { best_n = n; best = o; }
        }
        if (best < 0) break;                               // every lane idle: no rays left
        if (L.op == (uint32_t)best) {
            switch (best) {
                case OP_NODE: q_node<ANY, STACK, WG, CACHE, STATS>(s, node_lds, n_cached, L, st, cnt); break;
                case OP_SPHERE: q_sphere<ANY>(s, L, st, cnt); break;
                case OP_RECT: q_rect<ANY>(s, L, st, cnt); break;
                case OP_BOX: q_box<ANY>(s, L, st, cnt); break;
                case OP_MEDIUM: q_medium<ANY>(s, L, st, cnt); break;
                case OP_MISC: q_misc<ANY>(s, L, st, cnt); break;
                case OP_CTX: q_ctx<ANY>(s, a, L, st, cnt); break;
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

#ifndef RT2022_QUERY_CACHE
#define RT2022_QUERY_CACHE 1
#endif
constexpr bool kQueryCache = RT2022_QUERY_CACHE;   // 0: no node-table instance (every scene takes the 256-thread kernels)

hipError_t launch_query(const SceneDev &scene, const QueryArgs &args, uint32_t stack_need, bool counters, bool any_hit,
                        hipStream_t stream) {
    if (args.n_rays == 0) return hipSuccess;
    if (stack_need > (uint32_t)kStackLarge) return hipErrorInvalidValue;
    if (kQueryCache && stack_need <= (uint32_t)kStackTiny) return launch_flags<kStackTiny, kCacheBlock, kNodeCache>(scene, args, counters, any_hit, stream);
    if (stack_need <= (uint32_t)kStackSmall) return launch_flags<kStackSmall, kBlock, 0>(scene, args, counters, any_hit, stream);
    if (stack_need <= (uint32_t)kStackMid) return launch_flags<kStackMid, kBlock, 0>(scene, args, counters, any_hit, stream);
    return launch_flags<kStackLarge, kBlock, 0>(scene, args, counters, any_hit, stream);
}

} // namespace rt2022
