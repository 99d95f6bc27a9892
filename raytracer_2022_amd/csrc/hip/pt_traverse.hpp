// pt_traverse.hpp — the f64 closest-hit traversal of the megakernel (pt_kernel.hip) and the query kernel (pt_query.hip):
// the lane's traversal state, its LDS stack and the arms of the in-wave voted scheduler. The caller owns the world-frame
// ray, the done arm and the scheduler loop. (wf_trace, pt_wavefront.hip, has its own tuned copy.)
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

} // namespace

} // namespace rt2022
#endif
