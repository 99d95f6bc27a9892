// pt_wavefront_trace.hip — the trace pass of the wavefront engine (pt_wavefront.hip): wf_trace, which of its instances a scene
// gets (choose_trace) and its launcher.
#include <algorithm>
#include <cstdio>
#include <type_traits>

#include "pt_wavefront.hpp"

namespace rt2022 {

// =====================================================================================
// Trace pass: closest hit of every pending ray, in-wave scheduled.
// =====================================================================================
namespace {

constexpr int kLeanBlocks = 5;             // resident traversal workgroups per CU of the sphere-only kernels (FEAT = 0, 256 threads)
// Operations of one kind a wf_trace lane takes in one turn of a voted arm, where its next entry is of the same kind again:
// the sphere and box arms take a span-2 leaf pair (three spheres: -1.6 % on the headline, -3 % on C2 in one A/B call).
constexpr int kSphereReps = 2, kNodeReps = 1, kBoxReps = 2, kMiscReps = 2;

struct TLane {
    XRay cur;              // ray inside the enclosing movers
    Vec3 inv;              // 1 / cur.d   (aabb.rs:19, hoisted: same value at every node)
    double a_len;          // cur.d.length_sqr()  (sphere.rs:41, hoisted likewise)
    double tm;
    double closest;
    // ConstantMedium::hit asks its boundary two closest-hit questions of its own
    // (constantmedium.rs:50-51). They run through the same operations as the main query,
    // against (t_lo, sub_closest) instead of (t_min, closest), and never touch the winner.
    double t_lo;           // lower bound in force: a.t_min, or the sub-query's
    double sub_closest;
    double med_t1;
    uint32_t med_ref;      // the medium being evaluated (0 = none: main query)
    Rng rng;
    Chain ctx;
    Chain win_chain;
    uint32_t win_leaf, win_face;
    uint32_t win_mat;      // material word of the winning leaf (index | slot kind << kMatKindShift), taken from the record at hand
    double stash_ix, stash_iz;   // 1/d.x, 1/d.z of the frame a RotateY was entered from (they change only there) ...
    uint32_t stash_level;        // ... and that frame's mover depth (0xFFFFFFFF: nothing stashed)
    // (node table in LDS, kSlabs) byte addresses, within the table's record 0, of the box coordinate the ray meets
    // first / last on each axis: bmin / bmax by the sign of 1/d — set wherever inv is (t_slabs)
    uint32_t near_at[3], far_at[3];
    // (single-precision slab test, kF32 / kF32G) per axis {(float)(1/d), (float)(-o/d)} — one operand pair of the packed
    // multiply-add that gives the axis' two slab distances — and the ray's share of the test's error bound; set with near_at
    f32x2 p32[3];
    float e_ray;
    uint32_t slot;
    uint32_t entry;        // where on the ray list the slot was found (its kind goes back to the same place)
    uint32_t steps;        // node steps of this ray
    int sp;
    uint32_t top, op;
    // Per-lane flags in ONE register rather than three bools: a bool member lives as a lane mask in a scalar register
    // pair, and every join of the scheduler's control flow then merges each of them with three scalar instructions
    // (seen in the ISA: ~30 per round of the outer loop); a vector register needs no merging.
    //   kPlain     the fast node step applies to this ray (see there)
    //   kHasRay    the lane carries a ray
    //   kSubFound  the medium sub-query in progress has found a boundary hit
    //   kNeed64    the single-precision slab test could not decide the node step at hand: the voted node arm takes it in double precision
    //   bits 25-30 (kOrderMask) the ray's side of the child order: bit 31 - k is set where a node of order k has its right child
    //              nearer to this ray (k = 1 + 2 * axis + sense, host/scene_check.hpp) — flags << k then has it in the sign bit,
    //              and a node of order 0 never does (bit 31 stays clear); set wherever inv is (t_flags)
    //   kNaN       this ray has accepted a NaN distance (t_accept): for the rest of it kPlain and the order bits stay clear
    //   kAgain     ... and had been visiting nodes in its own order until then: the ray is traversed once more (OP_SHADE)
    uint32_t flags;
};

template <int STACK, int WG = kBlock>
struct TStack {
    uint32_t *col;
    RT_DEV void push(TLane &L, uint32_t ref) { if (L.sp < STACK) { col[L.sp * WG] = ref; L.sp++; } }
    RT_DEV uint32_t pop(TLane &L) { if (L.sp > 0) { L.sp--; return col[L.sp * WG]; } return REF_EMPTY; }
};

constexpr uint32_t kPlain = 1u, kHasRay = 2u, kSubFound = 4u, kNeed64 = 8u, kNaN = 16u, kAgain = 32u, kOrderMask = 0x7E000000u;
RT_DEV void t_flag(TLane &L, uint32_t bit, bool on) { L.flags = on ? (L.flags | bit) : (L.flags & ~bit); asm volatile("" : "+v"(L.flags)); }
RT_DEV bool t_finite(double x) { return (rtm::d2u(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
// The fast node step applies (see there): every 1/d finite and non-zero, origin finite, boxes plain — and no NaN accepted so far.
// ... and the order bits (`order`: kOrderMask where the instance orders children and the tuning word lets it, else 0). As long
// as no accepted distance is a NaN any choice is a valid one — the closest hit does not depend on the order of the visits inside
// a subtree without media, ties go by rank (t_accept) — so a zero or NaN component simply counts as pointing up its axis. A ray
// that has accepted a NaN (kNaN) has no order bits: from then on the LAST leaf visited wins (see t_accept).
RT_DEV void t_flags(TLane &L, bool boxes_plain, uint32_t order) {
    const uint32_t sane = ((L.flags / kNaN) & 1u) - 1u;             // (all ones while no NaN has been accepted)
    const bool plain = boxes_plain && sane != 0u && t_finite(L.inv.x) && t_finite(L.inv.y) && t_finite(L.inv.z) && L.inv.x != 0.0 && L.inv.y != 0.0 &&
              L.inv.z != 0.0 && t_finite(L.cur.o.x) && t_finite(L.cur.o.y) && t_finite(L.cur.o.z);
    uint32_t m = 0;
    if (order) {                                                  // (kOrderMask or 0: one scalar register, known 0 where nothing is ordered)
#pragma unroll
        for (int i = 0; i < 3; i++) m |= (L.inv[i] < 0.0 ? 0x40000000u : 0x20000000u) >> (2 * i);
    }
    L.flags = (L.flags & ~kOrderMask) | (m & order & sane);
    t_flag(L, kPlain, plain);
}
// A node's children as a kernel takes them from the last 16 bytes of its record {left, right, push ref, left}: the last two
// words carry the order bits of the nodes they name (rt_scene_create) — the ordering kernels read those; the others the plain
// left child, and the plain push ref: the right child, or "nothing" where the record's push ref says so.
template <bool TAGGED>
RT_DEV void t_children(const u32x4 rw, uint32_t &left, uint32_t &push) {
    if (TAGGED) { left = rw.w; push = rw.z; }
    else { left = rw.x; push = rw.z == REF_EMPTY ? REF_EMPTY : rw.y; }
}
// For a plain ray the slab test's min(t0, t1) / max(t0, t1) per axis IS the choice of bmin or bmax by the sign of 1/d (the
// products are ordered by it: see the fast path) — made here once per direction instead of twice per axis and node step.
RT_DEV void t_slabs(TLane &L, uint32_t table_at) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const bool neg = L.inv[i] < 0.0;
        L.near_at[i] = table_at + (neg ? 24u : 0u) + 8u * (uint32_t)i;          // record: bmin x y z at +0 +8 +16, bmax at +24 +32 +40
        L.far_at[i] = table_at + (neg ? 0u : 24u) + 8u * (uint32_t)i;
    }
}
// The single-precision slab test of the node table in LDS (kF32; see the fast path). A node record there is eleven
// words: per axis {(float)bmin, (float)bmax, (float)bmin} — so that ONE two-word read at `base` or at `base + 4` delivers the
// pair in the order (first met, last met) for either sign of 1/d — then the left child and the push ref.
constexpr uint32_t kNode32Words = 11, kNode32Bytes = 4 * kNode32Words;
// Error bound (u = 2^-24). With b32 = (float)b, i32 = (float)(1/d), n32 = (float)(-o * (1/d)) the kernel computes
// t32 = fma(b32, i32, n32) where the double-precision step computes T = (b - o) * (1/d), rounded twice. Against the real
// number R = b/d - o/d (1/d being the f64 value both use):
//   |b32 i32 - b/d| <= |b/d| (2u + u^2),   |n32 + o/d| <= |o/d| (u + 2^-52),   the fma rounds once: u (1 + u) |t32|,   |T - R| <= 2^-52 |R|,
// and with |b/d| <= |R| + |o/d|, |R| <= |t32| + error, |o/d| <= |n32| (1 + u):
//   |t32 - T| <= 3.000001 u (|t32| + |n32|)
// — an error relative to the VALUE plus a constant of the ray, k = 3.000001 u max |n32|; nothing in it depends on how large the
// scene's other coordinates are. (A bound from the largest box coordinate instead was tried first: with 0.2-unit spheres on
// a 2000-unit ground it left a few per cent of the node steps undecided, and the kernel 10 % slower than the double-precision
// one.) The window's two ends, converted to float, are off by u of their value: the same form. x -> x + c|x| and x -> x - c|x|
// are increasing, so the max / min of such values is off by at most c |max| + k, and the rounded difference of the two by
//   (3.000001 u + u) (|tmx32| + |tmn32|) + 6.000002 u max |n32|   <   4.5 u (|tmx32| + |tmn32|) + e_ray,   e_ray = 6.5 u max |n32| + 2e-8
// (2e-8 for box coordinates below the float normal range, see t_slabs32; the eighths of slack cover the three roundings of the bound's own arithmetic, 3 u each at most).
// It has to be this tight: a ray that leaves a surface tests the boxes that surface lies on the face of, where the verdict hangs
// on t_min = 0.001 against a distance of zero — with coordinates in the hundreds the bound is a few 1e-4 of that.
// Any overflow on the way (1/d beyond f32) makes a value or the bound infinite or NaN: the test then decides nothing and
// the lane takes the double-precision step.
constexpr float kF32RelBound = 4.5f * 0x1p-24f, kF32RayBound = 6.5f * 0x1p-24f;
// The test's verdict from the window's two ends: a hit where they leave a gap, and undecided — left to the double-precision test —
// where the gap is within the error bound.
struct Verdict32 { bool hit, undecided; };
RT_DEV Verdict32 t_verdict32(float tmn32, float tmx32, float e_ray) {
    const float gap = tmx32 - tmn32;
    const float e_tot = __builtin_fmaf(__builtin_fabsf(tmx32) + __builtin_fabsf(tmn32), kF32RelBound, e_ray);
    return {gap > 0.0f, !(__builtin_fabsf(gap) > e_tot)};                          // (a NaN anywhere lands in `undecided` too)
}
// LDS: the records are those of the node table in LDS (kF32); otherwise the kernel fetches its single-precision records from HBM
// (kF32G): no per-lane table addresses, the record's {min, max} pairs are ordered after the multiply-adds instead.
template <bool LDS>
RT_DEV void t_slabs32(TLane &L, uint32_t table_at = 0) {
    float e = 0.0f;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (LDS) L.near_at[i] = table_at + 12u * (uint32_t)i + (L.inv[i] < 0.0 ? 4u : 0u);
        const float i32 = (float)L.inv[i], n32 = (float)(-(L.cur.o[i] * L.inv[i]));
        L.p32[i] = (f32x2){i32, n32};
        e = __builtin_fmaxf(e, __builtin_fabsf(n32));           // (n32 is no NaN for a plain ray — finite origin, finite non-zero 1/d — and only those take the test)
        // The analysis above takes i32 to be 1/d within u, and a float box coordinate within u of the double — or within 1.2e-38
        // of it, for a coordinate below the normal range: 1/d between 1e-30 and 1e30 makes the first true and keeps what the
        // second adds below the 2e-8 of e_ray; directions outside that range leave every step to the double-precision test.
        const float ai = __builtin_fabsf(i32);
        ok = ok && ai >= 1e-30f && ai <= 1e30f;
    }
    L.e_ray = ok ? __builtin_fmaf(e, kF32RayBound, 2e-8f) : __builtin_inff();
}
RT_DEV void t_set_cur(TLane &L, const XRay &c, bool boxes_plain, uint32_t order) {
    L.cur = c;
    L.inv = Vec3(1.0 / c.d.x, 1.0 / c.d.y, 1.0 / c.d.z);
    L.a_len = c.d.length_sqr();
    t_flags(L, boxes_plain, order);
}
RT_DEV double t_hi(const TLane &L) { return L.med_ref ? L.sub_closest : L.closest; }
// ORDER (the kernels that may visit a node's right child first): the reference accepts t == t_max, so among candidates of exactly
// equal t the one it visits LAST wins. Visited in another order, the same one wins when a tie between two different primitives
// goes to the higher rank in the reference's depth-first order (SceneDev::prim_rank; read here only, in a branch next to never taken).
//
// A NaN distance. sphere_t, rect_t and the box's faces accept one: `root < t_min || t_max < root` is false for it (inf - inf under
// the root of a sphere 1e200 away, 0 / 0 for a ray lying in a rect's plane or a MovingSphere with time0 == time1, any NaN
// component of the ray). With a NaN for its upper end the window rejects nothing any more and AABB::hit culls nothing
// (`t1 < t_max` and `t_max <= t_min` are false): every sphere and rect VISITED from then on accepts, and the one visited last
// wins — the result depends on the order of the visits, and on entering every node. So from the first NaN on the lane takes the
// reference's own steps only: no fast node step (its v_min_f64 drops a NaN operand where the reference keeps it), no order bits
// (kNaN clears both, for good). A lane that had order bits until then may have visited other leaves than the reference up to
// this point: it drops its stack and is traversed once more from the root (kAgain; OP_SHADE), in the reference's order and with
// its steps from the start. A medium's sub-query is treated alike. Costs an accepted hit one compare; rays that meet no NaN
// nothing else.
// `tainted` (the box arm): a box's own closest-so-far may have been a NaN between two of its faces — a face in whose plane the ray
// lies, 0 / 0 — and the face accepted after it then ignored the window: a finite t, possibly beyond the closest hit, which wins
// all the same. Whether it does depends on what was visited before, like a NaN itself: a lane with order bits is taken again.
// Only a ray that is not plain can meet it (finite o, finite non-zero d and finite corners — check_scene — give finite or
// infinite face distances), so the arm passes `not plain`, and no box test pays for it.
template <bool ORDER>
RT_DEV void t_accept(const SceneDev &s, TLane &L, double t, uint32_t face, uint32_t mat_word, bool tainted = false) {
    const bool nan = t != t;
    if (nan || tainted) {
        const bool again = ORDER && (L.flags & kOrderMask) != 0u;
        if (nan || again) L.flags = (L.flags & ~(kPlain | kOrderMask)) | kNaN | (again ? kAgain : 0u);
        if (again) { L.sp = 0; return; }                              // (the arm's T_NEXT finds the stack empty: OP_SHADE)
    }
    if (L.med_ref) { L.sub_closest = t; t_flag(L, kSubFound, true); return; }
    if (ORDER && t == L.closest && L.win_leaf != REF_EMPTY && ((L.win_leaf ^ L.top) << 1) != 0u && s.prim_rank) {
        const uint32_t mine = s.prim_rank[s.prim_rank[RT_REF_KIND(L.top) & 7u] + RT_REF_INDEX(L.top)];
        const uint32_t theirs = s.prim_rank[s.prim_rank[RT_REF_KIND(L.win_leaf) & 7u] + RT_REF_INDEX(L.win_leaf)];
        if (mine < theirs) return;
    }
    L.closest = t;
    L.win_leaf = L.top; L.win_face = face; L.win_chain = L.ctx; L.win_mat = mat_word;
}
// The two boundary queries of ConstantMedium::hit on ONE sphere (constantmedium.rs:50-51):
//     sphere_t(center, radius, r, a, -inf, +inf, t1)  and then  sphere_t(center, radius, r, a, t1 + 0.0001, +inf, t2)
// with what they share — oc, half_b, c, the discriminant, its square root and the near root — computed once. Every
// expression and comparison is sphere_t's own (pt_common.hpp, sphere.rs:39-58), so the values are the same bit for bit;
// `first` says whether the first query found a hit (the second is only made, and counted, then).
RT_DEV bool sphere_t_twice(Vec3 center, double radius, const XRay &r, double a, double &t1, double &t2, bool &first) {
    first = false;
    Vec3 oc = r.o - center;
    double half_b = rtm::dot(oc, r.d);
    double c = oc.length_sqr() - radius * radius;
    double discriminant = half_b * half_b - a * c;
    if (discriminant < 0.0) return false;
    double sqrtd = rtm::sqrt_(discriminant);
    const double near_root = (-half_b - sqrtd) / a;
    double root = near_root;
    if (root < -rtm::INF || rtm::INF < root) {
        root = (-half_b + sqrtd) / a;
        if (root < -rtm::INF || rtm::INF < root) return false;
    }
    t1 = root;
    first = true;
    const double t_min2 = t1 + 0.0001;
    root = near_root;
    if (root < t_min2 || rtm::INF < root) {
        root = (-half_b + sqrtd) / a;
        if (root < t_min2 || rtm::INF < root) return false;
    }
    t2 = root;
    return true;
}
// Boxes::hit over six sides given by value (boxes.rs:24-66,80-82 + mod.rs:90-100): box_t of pt_common.hpp, fed from
// registers.
RT_DEV bool t_box(double p0x, double p0y, double p0z, double p1x, double p1y, double p1z, const XRay &r, double t_min, double t_max,
                  double &t, uint32_t &face) {
    bool any = false;
    double closest = t_max, tt;
    if (rect_t(RT_RECT_XY, p0x, p1x, p0y, p1y, p1z, r, t_min, closest, tt)) { closest = tt; face = 0; any = true; }
    if (rect_t(RT_RECT_XY, p0x, p1x, p0y, p1y, p0z, r, t_min, closest, tt)) { closest = tt; face = 1; any = true; }
    if (rect_t(RT_RECT_XZ, p0x, p1x, p0z, p1z, p1y, r, t_min, closest, tt)) { closest = tt; face = 2; any = true; }
    if (rect_t(RT_RECT_XZ, p0x, p1x, p0z, p1z, p0y, r, t_min, closest, tt)) { closest = tt; face = 3; any = true; }
    if (rect_t(RT_RECT_YZ, p0y, p1y, p0z, p1z, p1x, r, t_min, closest, tt)) { closest = tt; face = 4; any = true; }
    if (rect_t(RT_RECT_YZ, p0y, p1y, p0z, p1z, p0x, r, t_min, closest, tt)) { closest = tt; face = 5; any = true; }
    t = closest;
    return any;
}
// L.top has just been set: label it. The two cheap steps of ConstantMedium::hit — start the first
// boundary query, turn the first into the second (constantmedium.rs:50-51) — are taken on the spot
// instead of costing the wave a scheduling round each; only the finish (RNG, log) is an operation.
template <int STACK, bool STATS, unsigned FEAT, int WG>
RT_DEV void t_settle(const SceneDev &s, TLane &L, TStack<STACK, WG> &st, double t_min, Counters<STATS> &cnt) {
    if (FEAT & kFeatVolumes) {
        for (int guard = 0; guard < 6; guard++) {
            if (RT_REF_KIND(L.top) == RT_KIND_MEDIUM) {               // a medium leaf: boundary.hit(r, -inf, inf)
                // (a boundary that is one plain sphere — the fog and the subsurface ball of the final scene —
                // is not traversed at all: the medium arm does both queries and the finish in one turn)
                if (s.media_mode == 1u || (s.media_mode == 2u && s.media_dev[RT_REF_INDEX(L.top)].sphere_boundary)) break;
                cnt.prim(RT_KIND_MEDIUM);
                L.med_ref = L.top;
                L.t_lo = -rtm::INF;
                L.sub_closest = rtm::INF; t_flag(L, kSubFound, false);
                st.push(L, REF_MED1);
                L.top = s.media_dev[RT_REF_INDEX(L.top)].boundary;
            } else if (L.top == REF_MED1) {
                if (L.flags & kSubFound) {                            // boundary.hit(r, rec1.t + 0.0001, inf)
                    L.med_t1 = L.sub_closest;
                    L.t_lo = L.med_t1 + 0.0001;
                    L.sub_closest = rtm::INF; t_flag(L, kSubFound, false);
                    st.push(L, REF_MED2);
                    L.top = s.media_dev[RT_REF_INDEX(L.med_ref)].boundary;
                } else {
                    L.med_ref = 0; L.t_lo = t_min;
                    L.top = st.pop(L);
                }
            } else {
                break;
            }
        }
    }
    L.op = classify(L.top);
}
#define T_NEXT() do { L.top = st.pop(L); t_settle<STACK, STATS, FEAT, WG>(s, L, st, t_min, cnt); } while (0)
#define T_SETTLE() t_settle<STACK, STATS, FEAT, WG>(s, L, st, t_min, cnt)
// L.inv has just been set: what the instance's slab test takes from it (kSlabs, kF32, kF32G: wf_trace).
#define T_SLABS() do { if (kSlabs) t_slabs(L, table_at); if (kF32) t_slabs32<true>(L, table_at); if (kF32G) t_slabs32<false>(L); } while (0)

} // namespace

// Census of the single-precision slab test (diagnostic build -DRT2022_F32_CENSUS only): node steps of the fast path that took
// it, how many of them it left to the double-precision test, and how many of its verdicts differed from that test's (the census
// build makes both): read and cleared by f32_slab_census (rt_debug_f32_slabs).
__device__ unsigned long long g_f32_census[3];

// ... counted at every step of the fast path that takes the test, and every verdict taken checked against the double-precision test on
// the node's record in HBM (hit, undecided, nidx, tlo_c, thi_c: the fast path's names; a macro, not a function: the census has to count the
// kernels as they are otherwise compiled, and as a function, by value or by reference, it changed their register allocation).
#ifdef RT2022_F32_CENSUS
#define T_CENSUS32() do { \
        f32_steps++; if (undecided) f32_undecided++; \
        if (!undecided) { \
            const f64x2 *np = reinterpret_cast<const f64x2 *>(s.nodes + nidx); \
            const f64x2 n0 = np[0], n1 = np[1], n2 = np[2]; \
            const double lo3[3] = {n0.x, n0.y, n1.x}, hi3[3] = {n1.y, n2.x, n2.y}; \
            double tmn = tlo_c, tmx = thi_c; \
            for (int i = 0; i < 3; i++) { \
                const double t0 = (lo3[i] - L.cur.o[i]) * L.inv[i], t1 = (hi3[i] - L.cur.o[i]) * L.inv[i]; \
                tmn = __builtin_fmax(tmn, __builtin_fmin(t0, t1)); \
                tmx = __builtin_fmin(tmx, __builtin_fmax(t0, t1)); \
            } \
            if (hit != !(tmx <= tmn)) f32_wrong++; \
        } \
    } while (0)
#else
#define T_CENSUS32() do {} while (0)
#endif

// Phase clock of the traversal kernel (diagnostic build -DRT2022_TRACE_PROBE only): every wave adds the shader-clock
// ticks it spent in each phase of the scheduler — [0] node fast path, [1] vote, [2..9] the voted arms by label (node,
// sphere, rect, box, medium, misc, ctx, done), [10] the rest — to pool.dbg[96 + phase]; printed after the render.
#ifdef RT2022_TRACE_PROBE
#define TP_DECL __shared__ unsigned long long tp_lds[WG / 64][12]; unsigned long long tp_t = __builtin_readcyclecounter(); \
    if (lane < 12) tp_lds[tid >> 6][lane] = 0
#define TP_MARK(i) do { const unsigned long long tp_n = __builtin_readcyclecounter(); const unsigned long long tp_m = wballot(true); \
    if ((int)lane == __ffsll((long long)tp_m) - 1) tp_lds[tid >> 6][(i)] += tp_n - tp_t; tp_t = tp_n; } while (0)
#define TP_FLUSH() do { if (lane < 12 && pool.dbg) atomicAdd(&pool.dbg[96 + lane], tp_lds[tid >> 6][lane]); } while (0)
#else
#define TP_DECL do {} while (0)
#define TP_MARK(i) do {} while (0)
#define TP_FLUSH() do {} while (0)
#endif

// Resident traversal workgroups per CU a variant is built and launched for (= waves per SIMD = its VGPR budget):
// the sphere-only kernel needs 82 VGPRs and runs five (C2: +4 % over four; six would spill), the full kernels four.
constexpr int trace_blocks_per_cu(int stack, bool stats, unsigned feat) {
    return stack > 32 ? 2 : stats ? 3 : (stack > kStackSmall || (feat & kFeatMisc)) ? 4 : feat == 0 ? kLeanBlocks : kTraceBlocksPerCU;
}
// The node-cache variants (TABLE other than kTablePlain: WG = kCacheBlock threads, one workgroup per CU, CACHE = kNodeCache records): the BVH's first
// CACHE node records live in LDS — 48 bytes of box and 8 of child refs each — beside the traversal stacks of the
// workgroup's 16 waves. A node step on a cached node is an LDS round trip instead of an L1 / L2 one; the 160 KiB of a
// CU belong to ONE workgroup, so the table exists once per CU rather than once per four waves. Two instances: the
// whole node table of a small scene (PARTIAL = false: no HBM path for nodes at all), and the first kNodeCache records
// of a larger one whose stacks still fit 16 entries (PARTIAL = true) — rt_scene_create numbers the nodes of the
// device copy breadth-first from the root, so the first records are the top levels of the BVHs, the ones every ray
// goes through. Same records, same arithmetic, same results. Measured (tools/scaling_scenes.py, 1200x800x160): 549
// nodes +21 %, 12 213 nodes (1740 of them in LDS) +8.5 %. A third instance — 700 records beside stacks of 30 entries
// for the deep BVHs of 131 K / 1 M / the 1.7 M-node mesh of C5 — measured -2 % / -4.5 % / +-0 and was dropped: the top
// levels of a big BVH are L1-resident anyway, and what the table saves on a small one is the L2 latency of the levels below.
constexpr int trace_wg(TraceTable table) { return table == kTablePlain ? kBlock : kCacheBlock; }
constexpr int trace_waves_per_simd(int stack, bool stats, unsigned feat, int wg) {
    return wg == kBlock ? trace_blocks_per_cu(stack, stats, feat) : wg / 256;
}
// Which wf_trace instances test node boxes in single precision, from the instance's template facts: wf_trace takes kF32 and
// kF32G from these two, trace_variant asks them the same at run time.
// f32_lds (kF32): the single-precision records of t_slabs32 in the node table in LDS — the all-in-LDS instance of sphere-only
// scenes, and the whole-table instance of the sphere-only scenes too large for it (601 to 1 740 nodes). Why sphere-only scenes:
// what the float test cannot decide is a ray leaving a surface against a box that surface lies on the face of (the verdict hangs
// on t_min = 0.001 against a distance of zero); a sphere touches its box in six points, a rect or a box lies in its faces: one
// node step in 96 000 on the random spheres, one in 194 on the book-2 final scene, one in 27 in the Cornell box
// (tools/f32_census.py) — measured, the random spheres' traversal kernel 6-7 % faster, the final scene's 1 % and the Cornell
// box's 6 % slower, whether the undecided lanes fetch the double-precision box on the spot or hand the step to the voted arm
// (profiles/r3q_ab_f32_slabs.log). A census build (-DRT2022_F32_CENSUS) puts the test into every whole-table instance without
// meshes instead, to count what it leaves undecided there.
constexpr bool f32_lds(unsigned feat, TraceTable table, bool spheres) {
#ifdef RT2022_F32_CENSUS
    return (table == kTableWhole || table == kTablePrims) && !(feat & kFeatMisc);
#else
    return table == kTablePrims || (spheres && feat == 0 && table == kTableWhole);
#endif
}
// f32_hbm (kF32G): the same test in the plain kernels, for sphere scenes too large for those instances: 32-byte single-precision
// records {min.x, max.x, min.y, max.y | min.z, max.z, left, push ref} — SceneDev::nodes32 — fetched as two 16-byte loads from
// L2 / HBM: half the bytes of the double-precision record per node step. (These scenes take the plain kernels even where the
// partial-table instance would apply: with the first 3 045 of these records in LDS that instance — four waves per SIMD against
// the plain kernel's five — measured 10 % slower on the 1e4-sphere scene, choose_trace.)
// ... and for the triangle meshes (kFeatMisc, no boxes or media): a triangle touches its box in its corners, one node step in
// 1 348 of wwscene is left undecided (its rings lie in the faces of theirs); C5's traversal kernel -3.2 % — once the ten VGPRs
// the test needs were found: the RotateY stash is dropped in these instances (two divisions at a RotateY's exit instead;
// measured alone: no cost).
constexpr bool f32_hbm(unsigned feat, TraceTable table, bool spheres, bool stats = false, bool probe = false) {
    return ((feat == 0 && spheres) || ((feat & kFeatMisc) && !(feat & kFeatVolumes))) && table == kTablePlain && !stats && !probe;
}
// Which wf_trace instances may visit a node's nearer child first (kOrder): the timed ones. The counting instances
// keep the reference's order — their node_visits and prim_tests are the oracle's, which follow it. Not the FEAT 7 ones either: they
// are at 128 VGPRs with spills as it is, and the step's extra scalar registers cost them one more spilled VGPR (kernel_resources).
constexpr bool trace_orders(bool stats, unsigned feat) { return !stats && (feat & 7u) != 7u; }
// FEAT: which arms the scene can reach (kFeat* bits); the others are compiled out, which is
// worth 20-60 VGPRs — the difference between 3 and 4-5 resident waves per SIMD.
// SPHERES: every primitive of the scene is a sphere (sphere_only) — the scenes whose node boxes are tested in single precision
// (a rect lies in the faces of its box, where that test decides nothing: see f32_lds).
// TABLE: what of the scene lives in LDS (TraceChoice::table) — the workgroup's size, the table's length and kind follow from it.
template <int STACK, bool STATS, unsigned FEAT, bool PROBE = false, TraceTable TABLE = kTablePlain, bool SPHERES = false>
__global__ void __launch_bounds__(trace_wg(TABLE), trace_waves_per_simd(STACK, STATS, FEAT, trace_wg(TABLE))) wf_trace(const SceneDev s, const WfPool pool,
                                                   const double t_min, const uint32_t tuning, const uint32_t parity, StatsDev *stats,
                                                   const uint32_t vote_weights) {
    static_assert(TABLE == kTablePlain || STACK == kStackTiny, "beside a node table in LDS there is room for stacks of kStackTiny entries");
    constexpr int WG = trace_wg(TABLE), CACHE = TABLE == kTablePlain ? 0 : TABLE == kTablePrims ? kPrimNodes : kNodeCache;
    constexpr bool PARTIAL = TABLE == kTablePartial, PRIMS = TABLE == kTablePrims;
    // (Scene and pool by value: pointer members of kernel arguments are known to be global
    // memory, so node / ray fetches compile to global_load instead of flat_load, and none of
    // them is re-read from a descriptor in memory inside the traversal loop.)
    __shared__ uint32_t stack_lds[STACK * WG];
    // The world ray of every lane's current path, [component][lane] (12 KiB where the scene has movers, 48 bytes
    // otherwise): leaving a mover restarts from it (a ray_at_level of the enclosing frame) without going back to HBM.
    // (The deeper-stack variants have no LDS to spare at four workgroups per CU: they fetch it from the pool again.)
    constexpr bool kStash = (FEAT & kFeatMovers) != 0 && STACK <= kStackSmall && CACHE == 0;
    __shared__ double wray_lds[kStash ? 6 * WG : 6];
    // Node cache (CACHE > 0): boxes as three 16-byte words per node, child refs as one 8-byte word per node — or (kF32) the
    // single-precision records of t_slabs32, 44 bytes per node; the double-precision boxes then stay in L2 for the few node steps
    // the single-precision test cannot decide. (kF32G: the plain kernels' test on SceneDev::nodes32; see f32_lds / f32_hbm.)
    constexpr bool kF32 = f32_lds(FEAT, TABLE, SPHERES);
    constexpr bool kF32G = f32_hbm(FEAT, TABLE, SPHERES, STATS, PROBE);
    constexpr bool kStashInv = !(kF32G && (FEAT & kFeatMovers));
    // (kTagged: the instance reads the node refs that carry order bits — every timed one, so that a scene's upload need not know
    // which of them will run it; kOrder: it acts on them)
    constexpr bool kTagged = !STATS;
    constexpr bool kOrder = trace_orders(STATS, FEAT);
    const uint32_t order_on = kOrder && !tune::ref_order(tuning) ? kOrderMask : 0u;
    // (a table that holds every node has at most kNodeCache of them: the mask is a literal there, no scalar register)
    const uint32_t node_mask = !kTagged ? RT_REF_INDEX_MASK : (CACHE > 0 && !PARTIAL) ? 0x00FFFFFFu : s.node_index_mask;
    __shared__ f64x2 nc_box[CACHE > 0 && !kF32 && !kF32G ? 3 * CACHE : 1];
    __shared__ u32x2 nc_ref[CACHE > 0 && !kF32 && !kF32G ? CACHE : 1];
    __shared__ uint32_t nc32[kF32 ? kNode32Words * CACHE : 1];
    // ... and, in every variant (384 bytes), the first records of the two small tables the arms go to most: movers (32 B
    // each) and media (MediumDev, 64 B each) — two of each in the book-2 final scene.
    constexpr uint32_t kLdsXforms = (FEAT & kFeatMovers) ? 8u : 0u, kLdsMedia = (FEAT & kFeatVolumes) ? 2u : 0u;
    __shared__ u32x4 xf_lds[kLdsXforms ? 2 * kLdsXforms : 1];
    __shared__ f64x2 md_lds[kLdsMedia ? 4 * kLdsMedia : 1];
    // PRIMS (sphere-only scenes small enough, C2): the sphere pools too — 32 B of centre and radius + 4 B of material
    // word per Sphere, the 80-byte record per MovingSphere; launched only when both pools fit whole.
    __shared__ f64x2 sp_lds[PRIMS ? 2 * kPrimSpheres : 1];
    __shared__ uint32_t spm_lds[PRIMS ? kPrimSpheres : 1];
    __shared__ f64x2 ms_lds[PRIMS ? 5 * kPrimMoving : 1];
    const PoolView pv{pool};
    const uint32_t tid = threadIdx.x;
    const unsigned lane = tid & 63u;
    Counters<STATS> cnt;
    TStack<STACK, WG> st{stack_lds + tid};
    // (the copies of the mover records and the list items whose node refs carry the order bits: SceneDev)
    const rt_xform *const xforms = kTagged ? s.xforms_ord : s.xforms;
    const uint32_t *const list_items = kTagged ? s.list_items_ord : s.list_items;
    const uint32_t n_cached = CACHE > 0 ? (s.n_nodes < (uint32_t)CACHE ? s.n_nodes : (uint32_t)CACHE) : 0u;
    if (CACHE > 0) {
        for (uint32_t i = tid; i < n_cached; i += (uint32_t)WG) {
            const f64x2 *np = reinterpret_cast<const f64x2 *>(s.nodes + i);
            f64x2 b0 = np[0], b1 = np[1], b2 = np[2];
            const u32x4 rw = reinterpret_cast<const u32x4 *>(np)[3];          // {left, right, push ref, left}: see rt_scene_create, t_children
            uint32_t c_left, c_push;
            t_children<kTagged>(rw, c_left, c_push);
            const u32x2 rr = {c_left, c_push};
            if (kF32) {
                const float lo[3] = {(float)b0.x, (float)b0.y, (float)b1.x}, hi[3] = {(float)b1.y, (float)b2.x, (float)b2.y};
                uint32_t *rec = nc32 + kNode32Words * i;
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    rec[3 * a] = __float_as_uint(lo[a]); rec[3 * a + 1] = __float_as_uint(hi[a]); rec[3 * a + 2] = __float_as_uint(lo[a]);
                }
                rec[9] = rr.x; rec[10] = rr.y;
            } else {
                nc_box[3 * i] = b0; nc_box[3 * i + 1] = b1; nc_box[3 * i + 2] = b2;
                nc_ref[i] = rr;
            }
        }
        if (PRIMS) {
            for (uint32_t i = tid; i < s.n_spheres && i < (uint32_t)kPrimSpheres; i += (uint32_t)WG) {
                const f64x2_a8 *qp = reinterpret_cast<const f64x2_a8 *>(s.spheres + i);
                sp_lds[2 * i] = qp[0]; sp_lds[2 * i + 1] = qp[1];
                spm_lds[i] = s.spheres[i].mat;
            }
            for (uint32_t i = tid; i < 5u * s.n_moving_spheres && i < 5u * (uint32_t)kPrimMoving; i += (uint32_t)WG)
                ms_lds[i] = reinterpret_cast<const f64x2 *>(s.moving_spheres)[i];
        }
    }
    if (kLdsXforms || kLdsMedia || CACHE > 0) {
        if (tid < 2 * kLdsXforms && tid < 2 * s.n_xforms) xf_lds[tid] = reinterpret_cast<const u32x4 *>(xforms)[tid];
        if (tid >= 64 && tid < 64 + 4 * kLdsMedia && tid < 64 + 4 * s.n_media) md_lds[tid - 64] = reinterpret_cast<const f64x2 *>(s.media_dev)[tid - 64];
        __syncthreads();
    }
    // A mover's record {kind, child | p[0] | p[1], p[2]} from wherever it lives.
    auto xform_words = [&](uint32_t idx, u32x4 &x0, f64x2 &x1) {
        if (kLdsXforms && idx < kLdsXforms) { x0 = xf_lds[2 * idx]; x1 = reinterpret_cast<const f64x2 *>(xf_lds)[2 * idx + 1]; }
        else { const u32x4 *xp = reinterpret_cast<const u32x4 *>(xforms + idx); x0 = xp[0]; x1 = reinterpret_cast<const f64x2 *>(xp)[1]; }
    };
    // ray_at_level of pt_common.hpp with the movers' records taken through xform_words.
    auto ray_at = [&](const Chain &ch, uint32_t level, XRay r) {
        for (uint32_t i = 0; i < level && i < RT_MAX_XFORM_DEPTH; i++) {
            const uint32_t ref = ch.at(i);
            u32x4 x0; f64x2 x1;
            xform_words(RT_REF_INDEX(ref), x0, x1);
            r = xform_ray_p(RT_REF_KIND(ref), rtm::u2d(((uint64_t)x0.w << 32) | x0.z), x1.x, x1.y, r);
        }
        return r;
    };
    double *const wray = wray_lds + (kStash ? tid : 0u);
    // (The node-table variant has no LDS left for the world rays and fetches them from the pool again. Keeping them in
    // twelve more registers instead — 128 in all, nothing spilled — measured the same: +0.3 %, A/B.)

    // Work of a pass = the ray lists of all segments (written by the preceding shade pass), cut into chunks of
    // kChunk entries and numbered slice-major: chunk id -> (slice = id / segments, segment = id % segments), so
    // that the counter hands out every segment's longest rays first. Each wave takes chunks from one global
    // counter as it runs dry — the waves, workgroups and CUs of the persistent grid therefore all finish within
    // one chunk of each other however unevenly they advance. (Bound statically to its segments, a workgroup's
    // speed depended on its CU and on its dispatch order within the CU — the arbiter serves the oldest wave
    // first — and a pass waited 10-25 % of its time for the slowest: rt_debug_pass_timing)
    const uint32_t n_seg = pool.n_blocks;
    const uint32_t total_ids = ((pool.max_list[parity] + kChunk - 1u) / kChunk) * n_seg;
    // This wave's chunk — entries [base + taken, base + n) of pool.list — and "the counter has run out": per-wave
    // state {base, n, taken, drained}, kept in LDS rather than in four more live registers. Written by the wave's
    // leader lane and read by whichever lanes publish next, as ONE volatile 16-byte access each way: volatile, so
    // every access is a real ds_read_b128 / ds_write_b128 in program order — one wave's LDS operations complete in
    // the order it issues them, and the compiler may not carry the words in registers from one round to the next.
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    __shared__ u32x4 chunk_lds[WG / 64];
    volatile u32x4 *const cs = &chunk_lds[tid >> 6];
    if (lane == 0) *cs = (u32x4){0u, 0u, 0u, 0u};
    const bool probe = PROBE && pool.dbg != nullptr;                  // (rt_debug_pass_timing: a build of its own, all arms)
    unsigned long long t_start = 0, t_dry = 0;
    bool dry_seen = false;
    if (probe) t_start = wall_clock64();

    TP_DECL;
#ifdef RT2022_F32_CENSUS
    unsigned f32_steps = 0, f32_undecided = 0, f32_wrong = 0;
#endif
    TLane L;
    L.flags = 0; L.op = OP_SHADE; L.top = REF_EMPTY; L.sp = 0; L.slot = 0; L.entry = 0; L.steps = 0;
    L.closest = rtm::F64_MAX; L.a_len = 0.0; L.tm = 0.0;
    L.t_lo = t_min; L.sub_closest = rtm::INF; L.med_t1 = 0.0; L.med_ref = 0;
    L.ctx.c0 = L.ctx.c1 = L.ctx.c2 = L.ctx.c3 = 0; L.ctx.n = 0;
    L.win_chain = L.ctx; L.win_leaf = REF_EMPTY; L.win_face = 0; L.win_mat = 0;
    L.stash_ix = 0.0; L.stash_iz = 0.0; L.stash_level = 0xFFFFFFFFu;
    const int node_quorum = (int)tune::quorum(tuning);
    constexpr int tail_factor = 2;
    const bool boxes_plain = tune::boxes_plain(tuning);              // host: every node box finite with min <= max
    unsigned census_rounds[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, census_lanes[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // What the node fast path keeps in registers across its turns (r3). The library is built without MachineLICM (Makefile:
    // hoisted f64 literals were being spilled), so nothing hoists a loop's constants any more — and in THIS loop every
    // instruction counts: rebuilding the classify table, the empty-stack ref and the two LDS table addresses each turn is five
    // more instructions per node step (C2: -5 %). The empty asm makes each an opaque value: it cannot be rebuilt inside.
    unsigned long long ctab = kClassifyTable;
    uint32_t ref_empty = REF_EMPTY;
    asm volatile("" : "+s"(ctab), "+v"(ref_empty));                  // (a select takes one scalar operand, and that is its lane mask)
    // (kSlabs: node table in LDS, the near / far box coordinate of each axis fetched by the sign of 1/d — no min / max per axis)
    constexpr bool kSlabs = CACHE > 0 && !PARTIAL && !(FEAT & kFeatMisc) && !kF32;      // (a partial table mixes both sources in one wave; the triangle kernels have no six registers to spare)
    typedef const __attribute__((address_space(3))) f64x2 *LdsBoxPtr;
    typedef const __attribute__((address_space(3))) u32x2 *LdsRefPtr;
    LdsBoxPtr ncb = (LdsBoxPtr)nc_box;
    LdsRefPtr ncr = (LdsRefPtr)nc_ref;
    if (CACHE > 0) asm volatile("" : "+v"(ncb), "+v"(ncr));
    uint32_t table32_at = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t *)nc32;
    if (kF32) asm volatile("" : "+v"(table32_at));
    const uint32_t table_at = kF32 ? table32_at : (uint32_t)(uintptr_t)ncb;              // (LDS byte address of node record 0's box)
    L.near_at[0] = L.near_at[1] = L.near_at[2] = L.far_at[0] = L.far_at[1] = L.far_at[2] = table_at;
    L.p32[0] = L.p32[1] = L.p32[2] = (f32x2){0.0f, 0.0f}; L.e_ray = __builtin_inff();
    uint32_t refs32_at = table32_at + 36u;                             // (kF32: the child refs of record 0)
    if (kF32) asm volatile("" : "+v"(refs32_at));

    for (;;) {
        // Fast path: keep stepping nodes while enough lanes want to — nn >= the quorum. Below the quorum the vote
        // decides, except where its outcome is known: node steps weigh 1 and everything else 2, so with
        // nn > 2 x (all other pending lanes) the vote would pick the node step anyway (the usual case at the tail of a
        // pass, when the list has run dry and a few long rays are left); staying here saves the vote.
        // Inside the loop a lane can only leave the node state (the others are parked), so the number of pending
        // lanes is fixed on entry and both conditions are ONE threshold on nn: nn >= quorum, or 3 nn > 2 pending.
        // The loop itself is a plain divergent loop over the node lanes — a lane that leaves the node state drops out
        // of it, and all that are left go together when their count falls below the threshold.
        {
            // a node step (OP_NODE is label 0) of a plain ray — and not one the single-precision test has handed on: one compare, one vote
            bool isn = (kF32 || kF32G) ? (L.op | ((L.flags ^ kPlain) & (kPlain | kNeed64))) == 0u : (L.op | (~L.flags & kPlain)) == 0u;
            int nn = __popcll(wballot(isn));
            const int pending = __popcll(wballot(L.op != OP_IDLE));
            const int tail_threshold = tail_factor * pending / (tail_factor + 1) + 1;
            const int threshold = node_quorum < tail_threshold ? node_quorum : tail_threshold;
            // (t_lo and t_hi do not change inside the loop: a lane can only leave it)
            double tlo_c = L.t_lo, thi_c = t_hi(L);
            asm volatile("" : "+v"(tlo_c), "+v"(thi_c));              // (in vector registers, once per entry)
            const bool entered = isn && nn >= threshold;
            // (kF32) the window's ends in single precision and the error bound of this entry: the ray's share plus what the
            // two conversions can be off by (an infinite end converts exactly)
            float tlo32 = 0.0f, thi32 = 0.0f;
            if ((kF32 || kF32G) && entered) {
                tlo32 = (float)tlo_c; thi32 = (float)thi_c;
                asm volatile("" : "+v"(tlo32), "+v"(thi32));
            }
            if (entered) do {
                if (STATS) { const unsigned long long am = wballot(true); if ((int)lane == __ffsll((long long)am) - 1) { census_rounds[8]++; census_lanes[8] += (unsigned)nn; } }
                {
                // BvhNode::hit, bvh/mod.rs:86-101 + AABB::hit, aabb.rs:15-32. The left child is taken
                // at once, the right one waits on the stack and is tested against the then-closest hit.
                //
                // For a `plain` ray (t_set_cur: every 1/d finite and non-zero, origin finite) against
                // finite boxes with min <= max, no t0 / t1 is NaN and the products are ordered by the
                // sign of 1/d, so the swap of aabb.rs:22-24 is min / max of the pair; the interval only
                // shrinks from axis to axis, so the per-axis `t_max <= t_min` exits equal one test at
                // the end. Any other ray takes the literal restatement in the voted arm below.
                //
                // Straight-line on purpose: the node's 64 bytes and the stack entry below the top are
                // requested together, before the arithmetic — no load waits for the outcome of the test.
                const uint32_t nidx = L.top & node_mask;             // (kTagged: bits 24..26 of a node ref are its order)
                const int below_sp = L.sp > 0 ? L.sp - 1 : 0;
                double bmin[3], bmax[3];
                uint32_t left, right, below;
                bool hit, undecided = false;
                if (kF32) {
                    // Single-precision slab test with a double-precision second opinion (r3). The node's box is held as floats
                    // (t_slabs32: one two-word LDS read per axis delivers the coordinates the ray meets first and last), the two
                    // slab distances of an axis are ONE packed multiply-add, max3 / min3 fold the axes: ten vector instructions
                    // where the double-precision test needs nineteen. Its verdict is taken only where it cannot differ from the
                    // double-precision one: |tmx - tmn| above the error bound of t_slabs32; a lane it leaves undecided (one node step
                    // in 200 on the book-2 final scene, one in 70 000 on the random spheres: tools/f32_census.py) hands the step to the
                    // voted node arm, which fetches the double-precision record. Same decisions, bit for bit.
                    uint32_t a0, a1, a2, ar;
                    asm("v_mad_u32_u24 %0, %1, 44, %2" : "=v"(a0) : "v"(L.top), "v"(L.near_at[0]));
                    asm("v_mad_u32_u24 %0, %1, 44, %2" : "=v"(a1) : "v"(L.top), "v"(L.near_at[1]));
                    asm("v_mad_u32_u24 %0, %1, 44, %2" : "=v"(a2) : "v"(L.top), "v"(L.near_at[2]));
                    asm("v_mad_u32_u24 %0, %1, 44, %2" : "=v"(ar) : "v"(L.top), "v"(refs32_at));
                    static_assert(kNode32Bytes == 44, "the multiply-adds above carry the record size");
                    const uint32_t below_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)(st.col + below_sp * WG);
                    f32x2 bx, by, bz, tx, ty, tz;
                    u32x2 cr;
                    asm volatile("ds_read2_b32 %0, %5 offset1:1\n\tds_read2_b32 %1, %6 offset1:1\n\tds_read2_b32 %2, %7 offset1:1\n\t"
                                 "ds_read2_b32 %3, %8 offset1:1\n\tds_read_b32 %4, %9\n\ts_waitcnt lgkmcnt(0)"
                                 : "=&v"(bx), "=&v"(by), "=&v"(bz), "=&v"(cr), "=&v"(below) : "v"(a0), "v"(a1), "v"(a2), "v"(ar), "v"(below_at) : "memory");
                    // {t first, t last} = {b first, b last} * (1/d) + (-o/d): low halves of both results take the pair's low word, the addend its high word
                    asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(tx) : "v"(bx), "v"(L.p32[0]));
                    asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(ty) : "v"(by), "v"(L.p32[1]));
                    asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(tz) : "v"(bz), "v"(L.p32[2]));
                    float tmn32, tmx32;
                    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(tmn32) : "v"(tx.x), "v"(ty.x), "v"(tz.x));
                    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(tmx32) : "v"(tx.y), "v"(ty.y), "v"(tz.y));
                    asm("v_max_f32 %0, %1, %2" : "=v"(tmn32) : "v"(tmn32), "v"(tlo32));
                    asm("v_min_f32 %0, %1, %2" : "=v"(tmx32) : "v"(tmx32), "v"(thi32));
                    const Verdict32 v32 = t_verdict32(tmn32, tmx32, L.e_ray);
                    hit = v32.hit; undecided = v32.undecided;
                    T_CENSUS32();
                    left = cr.x; right = cr.y;
                } else if (kF32G) {
                    // The single-precision test on the 32-byte record (see kF32G above): {min, max} of an axis are one register pair,
                    // one packed multiply-add gives the axis' two slab distances, ordered afterwards (a min and a max per axis —
                    // no per-lane addresses here: one base address serves both loads).
                    const u32x4 *np = reinterpret_cast<const u32x4 *>(s.nodes32) + 2u * (uint64_t)nidx;
                    u32x4 q0 = np[0], q1 = np[1];
                    below = st.col[below_sp * WG];
                    asm volatile("" : "+v"(q0), "+v"(q1), "+v"(below));              // (both halves and the stack entry asked for together)
                    const f32x2 bx = {__uint_as_float(q0.x), __uint_as_float(q0.y)}, by = {__uint_as_float(q0.z), __uint_as_float(q0.w)},
                                bz = {__uint_as_float(q1.x), __uint_as_float(q1.y)};
                    f32x2 tx, ty, tz;
                    asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(tx) : "v"(bx), "v"(L.p32[0]));
                    asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(ty) : "v"(by), "v"(L.p32[1]));
                    asm("v_pk_fma_f32 %0, %1, %2, %2 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(tz) : "v"(bz), "v"(L.p32[2]));
                    float nx, ny, nz, fx, fy, fz, tmn32, tmx32;
                    asm("v_min_f32 %0, %1, %2" : "=v"(nx) : "v"(tx.x), "v"(tx.y)); asm("v_max_f32 %0, %1, %2" : "=v"(fx) : "v"(tx.x), "v"(tx.y));
                    asm("v_min_f32 %0, %1, %2" : "=v"(ny) : "v"(ty.x), "v"(ty.y)); asm("v_max_f32 %0, %1, %2" : "=v"(fy) : "v"(ty.x), "v"(ty.y));
                    asm("v_min_f32 %0, %1, %2" : "=v"(nz) : "v"(tz.x), "v"(tz.y)); asm("v_max_f32 %0, %1, %2" : "=v"(fz) : "v"(tz.x), "v"(tz.y));
                    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(tmn32) : "v"(nx), "v"(ny), "v"(nz));
                    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(tmx32) : "v"(fx), "v"(fy), "v"(fz));
                    asm("v_max_f32 %0, %1, %2" : "=v"(tmn32) : "v"(tmn32), "v"(tlo32));
                    asm("v_min_f32 %0, %1, %2" : "=v"(tmx32) : "v"(tmx32), "v"(thi32));
                    const Verdict32 v32 = t_verdict32(tmn32, tmx32, L.e_ray);
                    hit = v32.hit; undecided = v32.undecided;
                    T_CENSUS32();
                    left = q1.z; right = q1.w;
                } else {
                if (CACHE > 0 && (!PARTIAL || nidx < n_cached)) {     // (PARTIAL: the table holds the first n_cached nodes — the top of the BVHs, rt_scene_create numbers them breadth-first)
                    // (LDS addresses are 32 bits and a table index is far below 2^24: one v_mad_u32_u24 instead of a 64-bit multiply-add)
                    // (the 24-bit multiply-add takes the low 24 bits of the ref: its index, un-masked)
                    const uint32_t box_at = (uint32_t)(uintptr_t)ncb + __umul24(L.top, 48u);
                    uint32_t ref_at;
                    asm("v_mad_u32_u24 %0, %1, 8, %2" : "=v"(ref_at) : "v"(L.top), "v"((uint32_t)(uintptr_t)ncr));     // (one instruction; left alone the compiler masks, shifts and adds)
                    const uint32_t below_at = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)(st.col + below_sp * WG);
                    // The five LDS reads of a node step, issued back to back and waited for ONCE — written out, because the compiler's
                    // own placement of the waits split them (seen in the ISA: the child refs were waited for before the box was even
                    // asked for: two LDS round trips per node step instead of one).
                    u32x2 cr;
                    if (kSlabs) {
                        // bmin[] / bmax[] here are the coordinates the ray meets FIRST / LAST on each axis (bmin or bmax by the sign of
                        // 1/d: t_slabs): for a plain ray min(t0, t1) is the product with the first, max(t0, t1) with the last.
                        const uint32_t off = __umul24(L.top, 48u);
                        asm volatile("ds_read_b64 %0, %8\n\tds_read_b64 %1, %9\n\tds_read_b64 %2, %10\n\tds_read_b64 %3, %11\n\t"
                                     "ds_read_b64 %4, %12\n\tds_read_b64 %5, %13\n\tds_read_b64 %6, %14\n\tds_read_b32 %7, %15\n\ts_waitcnt lgkmcnt(0)"
                                     : "=&v"(bmin[0]), "=&v"(bmin[1]), "=&v"(bmin[2]), "=&v"(bmax[0]), "=&v"(bmax[1]), "=&v"(bmax[2]), "=&v"(cr), "=&v"(below)
                                     : "v"(L.near_at[0] + off), "v"(L.near_at[1] + off), "v"(L.near_at[2] + off), "v"(L.far_at[0] + off), "v"(L.far_at[1] + off),
                                       "v"(L.far_at[2] + off), "v"(ref_at), "v"(below_at) : "memory");
                    } else {
                        f64x2 c0, c1, c2;
                        asm volatile("ds_read_b128 %0, %5\n\tds_read_b128 %1, %5 offset:16\n\tds_read_b128 %2, %5 offset:32\n\t"
                                     "ds_read_b64 %3, %6\n\tds_read_b32 %4, %7\n\ts_waitcnt lgkmcnt(0)"
                                     : "=&v"(c0), "=&v"(c1), "=&v"(c2), "=&v"(cr), "=&v"(below) : "v"(box_at), "v"(ref_at), "v"(below_at) : "memory");
                        bmin[0] = c0.x; bmin[1] = c0.y; bmin[2] = c1.x; bmax[0] = c1.y; bmax[1] = c2.x; bmax[2] = c2.y;
                    }
                    left = cr.x; right = cr.y;
                } else {
                    const uint4 *np = reinterpret_cast<const uint4 *>(s.nodes + nidx);
                    uint4 q0 = np[0], q1 = np[1], q2 = np[2];
                    u32x4 q3 = reinterpret_cast<const u32x4 *>(np)[3];
                    below = st.col[below_sp * WG];
                    asm volatile("" : "+v"(q3), "+v"(below));         // (q3 as ONE 16-byte load — left and the push ref are not neighbours in it — and the stack read beside the fetches)
                    bmin[0] = rtm::u2d(((uint64_t)q0.y << 32) | q0.x); bmin[1] = rtm::u2d(((uint64_t)q0.w << 32) | q0.z); bmin[2] = rtm::u2d(((uint64_t)q1.y << 32) | q1.x);
                    bmax[0] = rtm::u2d(((uint64_t)q1.w << 32) | q1.z); bmax[1] = rtm::u2d(((uint64_t)q2.y << 32) | q2.x); bmax[2] = rtm::u2d(((uint64_t)q2.w << 32) | q2.z);
                    t_children<kTagged>(q3, left, right);          // (the push ref: `right`, or "nothing" for a span-1 twin — rt_scene_create)
                }
                double tmn, tmx;
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    double t0 = (bmin[i] - L.cur.o[i]) * L.inv[i];
                    double t1 = (bmax[i] - L.cur.o[i]) * L.inv[i];
                    constexpr bool sorted = kSlabs;                               // (t0 <= t1 already: the coordinates came in that order)
                    const double lo = sorted ? t0 : __builtin_fmin(t0, t1), hi = sorted ? t1 : __builtin_fmax(t0, t1);
                    // fmax / fmin of a value that is not an arithmetic result of the same block first "canonicalises" it (a
                    // v_max_f64 x, x) — per node step, for the window's two ends, which never change in here. Written as the
                    // instruction fmax / fmin compile to. No operand is a NaN on this path, so it is the same value: the slab products
                    // are none for a plain ray (see above), the lower end is t_min or a boundary distance + 0.0001, and a lane whose
                    // upper end — the closest hit — has become a NaN is no longer plain (t_accept: v_min_f64 would return the OTHER
                    // operand for it and cull by the slabs alone, where the reference's `t1 < t_max ? t1 : t_max` keeps the NaN).
                    asm("v_max_f64 %0, %1, %2" : "=v"(tmn) : "v"(i == 0 ? tlo_c : tmn), "v"(lo));
                    asm("v_min_f64 %0, %1, %2" : "=v"(tmx) : "v"(i == 0 ? thi_c : tmx), "v"(hi));
                }
                hit = !(tmx <= tmn);
                }
                // A span-1 node holds the same object twice (bvh/mod.rs:44-47). Testing a plain
                // primitive a second time against t_max = its own t finds the same hit again, so
                // only the count of tests is kept; anything that can draw from the RNG or carry
                // movers (media, movers, nodes, lists) is really visited twice. rt_scene_create has
                // worked that out per node: `right` here is the node's PUSH REF — its right child, or
                // REF_EMPTY where the twin needs no second visit (r3: one compare instead of five).
                if ((kF32 || kF32G) && undecided) {
                    // Mostly a ray leaving a surface against a box that surface lies on the face of: the verdict hangs on t_min = 0.001
                    // against a distance of zero, which floats of the scene's size cannot tell apart. The lane keeps its node and leaves
                    // the loop; the voted node arm takes the step on the double-precision record (no lane here waits for that fetch).
                    L.flags |= kNeed64;
                    isn = false;
                } else {
                cnt.node();
                L.steps++;
                if (kOrder) {
                    // The nearer child first: the node's order k is the top byte of its ref, the lane's flags hold "the
                    // right child is nearer" for order k in bit 31 - k — one shift by that byte puts it into the sign bit.
                    uint32_t sh;
                    asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(sh) : "v"(L.top), "v"(L.flags));
                    // ... and the lanes that have it set exchange their two refs in ONE vector instruction, under a mask of their own
                    // (two selects otherwise; the mask is scalar work, beside the vector pipes this loop is bound by).
                    const unsigned long long swap = wballot((int32_t)sh < 0);
                    unsigned long long saved;
                    asm volatile("s_and_saveexec_b64 %2, %3\n\tv_swap_b32 %0, %1\n\ts_mov_b64 exec, %2" : "+v"(left), "+v"(right), "=&s"(saved) : "s"(swap));
                }
                const bool twin = right == ref_empty;
                const bool push = hit && !twin && L.sp < STACK;
                if (push) st.col[L.sp * WG] = right;
                if (STATS && hit && twin) cnt.prim(RT_REF_KIND(left));
                const uint32_t next = hit ? left : (L.sp > 0 ? below : ref_empty);
                L.sp = hit ? L.sp + (push ? 1 : 0) : below_sp;
                L.top = next;
                // (a node ref is kind 0 without the FlipFace bit — rt_scene_create refuses a flipped node — so "another node step"
                // is one compare; the label of whatever else came up is looked up once, when the lane leaves the loop)
                isn = next < (1u << RT_REF_KIND_SHIFT);
                }
                }
                nn = __popcll(wballot(isn));
            } while (isn && nn >= threshold);
            if (entered) L.op = classify(L.top, ctab);                // (media met in there start in their own arm)
        }
        TP_MARK(0);
        // Vote: the label most lanes are waiting on (ties -> lowest id).
        int best = -1, best_n = 0;
#pragma unroll
        for (int o = 0; o < (int)OP_COUNT; o++) {
            if (!(FEAT & kFeatMisc) && o == (int)OP_MISC) continue;
            if (!(FEAT & kFeatMovers) && o == (int)OP_CTX) continue;
            if (!(FEAT & kFeatVolumes) && (o == (int)OP_BOX || o == (int)OP_MEDIUM)) continue;
            int n = __popcll(wballot(L.op == (uint32_t)o));
            // Weights, four bits per label (rt_debug_set_tuning; default kWfVoteWeights): a node step outside the fast path and
            // the refill yield to everything else — node 2, refill 2, the rest 4 (refill at 4: -3 % on the headline, A/B).
            int score = n * (int)((vote_weights >> (4 * o)) & 0xFu);
            if (score > best_n) { best_n = score; best = o; }
        }
        if (best < 0) break;                                          // every lane idle
        TP_MARK(1);
        if (STATS) {
            unsigned served = (unsigned)__popcll(wballot(L.op == (uint32_t)best));
            if (lane == 0) { census_rounds[best]++; census_lanes[best] += served; }
        }
        if (L.op != (uint32_t)best) {
            // parked: this lane's operation did not win the vote
        } else if (best == OP_NODE) {
            // (a node step below the fast path's quorum — a handful of lanes: those whose next entry is a node again take it in the
            // same turn, like the leaf arms do with their pairs)
#pragma unroll 1
            for (int rep = 0; rep < kNodeReps && L.op == OP_NODE; rep++) {
            cnt.node();
            L.steps++;
            const uint32_t nidx = L.top & node_mask;
            f64x2 n0, n1, n2;
            u32x4 n3;
            bool decided = false, miss = false;
            if (kF32) {
                // (the single-precision test of the fast path for the plain rays that come through here — a node step below the
                // quorum; everything else, and what it leaves undecided, takes the literal test on the double-precision record)
                const uint32_t *rec = nc32 + kNode32Words * nidx;
                n3 = (u32x4){rec[9], 0u, rec[10], 0u};
                if ((L.flags & (kPlain | kNeed64)) == kPlain) {
                    const float tlo32 = (float)L.t_lo, thi32 = (float)t_hi(L);
                    float tmn32 = tlo32, tmx32 = thi32;
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        const bool neg = L.inv[i] < 0.0;
                        const float lo = __uint_as_float(rec[3 * i]), hi = __uint_as_float(rec[3 * i + 1]);
                        const float t0 = __builtin_fmaf(neg ? hi : lo, L.p32[i].x, L.p32[i].y), t1 = __builtin_fmaf(neg ? lo : hi, L.p32[i].x, L.p32[i].y);
                        tmn32 = __builtin_fmaxf(tmn32, t0); tmx32 = __builtin_fminf(tmx32, t1);
                    }
                    const float gap = tmx32 - tmn32;
                    const float e_tot = __builtin_fmaf(__builtin_fabsf(tmx32) + __builtin_fabsf(tmn32), kF32RelBound, L.e_ray);
                    decided = __builtin_fabsf(gap) > e_tot;
                    miss = decided && !(gap > 0.0f);
                }
            }
            if (kF32 && decided) {
                n0 = n1 = n2 = (f64x2){0.0, 0.0};
            } else if (CACHE > 0 && !kF32 && (!PARTIAL || nidx < n_cached)) {     // (PARTIAL: the table holds the first n_cached nodes — the top of the BVHs, rt_scene_create numbers them breadth-first)
                n0 = nc_box[3 * nidx]; n1 = nc_box[3 * nidx + 1]; n2 = nc_box[3 * nidx + 2];
                const u32x2 cr = nc_ref[nidx];
                n3 = (u32x4){cr.x, 0u, cr.y, 0u};
            } else {
                const f64x2 *np = reinterpret_cast<const f64x2 *>(s.nodes + nidx);
                n0 = np[0]; n1 = np[1]; n2 = np[2];
                const u32x4 rw = reinterpret_cast<const u32x4 *>(np)[3];
                uint32_t c_left, c_push;
                t_children<kTagged>(rw, c_left, c_push);
                n3 = (u32x4){c_left, 0u, c_push, 0u};
            }
            t_pin(n0); t_pin(n1); t_pin(n2); t_pin(n3);
            const double bmin[3] = {n0.x, n0.y, n1.x}, bmax[3] = {n1.y, n2.x, n2.y};
            double tmn = L.t_lo, tmx = t_hi(L);
            if (!(kF32 && decided)) {
#pragma unroll
            for (int i = 0; i < 3; i++) {
                double inv_d = L.inv[i];
                double t0 = (bmin[i] - L.cur.o[i]) * inv_d;
                double t1 = (bmax[i] - L.cur.o[i]) * inv_d;
                if (inv_d < 0.0) { double tmp = t0; t0 = t1; t1 = tmp; }
                tmn = t0 > tmn ? t0 : tmn;
                tmx = t1 < tmx ? t1 : tmx;
                miss = miss || (tmx <= tmn);
            }
            }
            if (kF32 || kF32G) L.flags &= ~kNeed64;
            if (!miss) {
                uint32_t left = n3.x, push_ref = n3.z;                 // (push ref: see the fast path)
                if (kOrder && (int32_t)(L.flags << (L.top >> 24)) < 0) { left = n3.z; push_ref = n3.x; }      // (the nearer child first: see the fast path)
                if (push_ref == REF_EMPTY) cnt.prim(RT_REF_KIND(left));
                else st.push(L, push_ref);
                L.top = left;
                L.op = classify(left);
            } else {
                L.top = st.pop(L);
                L.op = classify(L.top);
            }
            }
        } else if (best == OP_SPHERE) {                               // Sphere / MovingSphere::hit
            // BVH leaves come in pairs (span-2 nodes): a lane whose next entry is a sphere again takes
            // it here and now rather than waiting for another round.
#pragma unroll 1
            for (int rep = 0; rep < kSphereReps && L.op == OP_SPHERE; rep++) {
                uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
                cnt.prim(kind);
                Vec3 center;
                double radius;
                uint32_t mat_word;
                if (kind == RT_KIND_SPHERE) {                         // rt_sphere, 40 B: center, radius, mat
                    f64x2 q0, q1;
                    if (PRIMS) { q0 = sp_lds[2 * idx]; q1 = sp_lds[2 * idx + 1]; mat_word = spm_lds[idx]; }
                    else {
                        const f64x2_a8 *qp = reinterpret_cast<const f64x2_a8 *>(s.spheres + idx);
                        q0 = qp[0]; q1 = qp[1];
                        mat_word = s.spheres[idx].mat;
                    }
                    t_pin(q0); t_pin(q1); t_pin(mat_word);
                    center = Vec3(q0.x, q0.y, q1.x); radius = q1.y;
                } else {                                              // rt_moving_sphere, 80 B: center0, center1, time0, time1, radius, mat
                    const f64x2 *qp = PRIMS ? ms_lds + 5 * idx : reinterpret_cast<const f64x2 *>(s.moving_spheres + idx);
                    f64x2 q0 = qp[0], q1 = qp[1], q2 = qp[2], q3 = qp[3], q4 = qp[4];
                    t_pin(q0); t_pin(q1); t_pin(q2); t_pin(q3); t_pin(q4);
                    const Vec3 c0(q0.x, q0.y, q1.x), c1(q1.y, q2.x, q2.y);
                    center = c0 + (c1 - c0) * ((L.tm - q3.x) / (q3.y - q3.x));   // MovingSphere::center, sphere.rs:124-127
                    radius = q4.x;
                    mat_word = (uint32_t)rtm::d2u(q4.y);
                }
                double t;
                bool h = sphere_t(center, radius, L.cur, L.a_len, L.t_lo, t_hi(L), t);
                if (h) t_accept<kOrder>(s, L, t, 0, mat_word);
                T_NEXT();
            }
        } else if (best == OP_RECT) {
            cnt.prim(RT_KIND_RECT);
            const f64x2 *qp = reinterpret_cast<const f64x2 *>(s.rects + RT_REF_INDEX(L.top));      // rt_rect, 48 B: a0 a1 | b0 b1 | k, axis+mat
            f64x2 q0 = qp[0], q1 = qp[1], q2 = qp[2];
            t_pin(q0); t_pin(q1); t_pin(q2);
            const uint64_t am = rtm::d2u(q2.y);
            double t;
            if (rect_t((uint32_t)am, q0.x, q0.y, q1.x, q1.y, q2.x, L.cur, L.t_lo, t_hi(L), t)) t_accept<kOrder>(s, L, t, 0, (uint32_t)(am >> 32));
            T_NEXT();
        } else if ((FEAT & kFeatVolumes) && best == OP_BOX) {
            // (like the spheres: the leaves of a box BVH come in pairs, a lane whose next entry is a box again takes it in the same turn)
#pragma unroll 1
            for (int rep = 0; rep < kBoxReps && L.op == OP_BOX; rep++) {
            cnt.prim(RT_KIND_BOX);
            const uint32_t bidx = RT_REF_INDEX(L.top);
            const f64x2_a8 *bp = reinterpret_cast<const f64x2_a8 *>(s.boxes + bidx);                // rt_box, 56 B: p0, p1, mat
            f64x2 b0 = bp[0], b1 = bp[1], b2 = bp[2];
            uint32_t mat_word = s.boxes[bidx].mat;
            t_pin(b0); t_pin(b1); t_pin(b2); t_pin(mat_word);
            double t;
            uint32_t face = 0;
            bool h = t_box(b0.x, b0.y, b1.x, b1.y, b2.x, b2.y, L.cur, L.t_lo, t_hi(L), t, face);
            if (h) t_accept<kOrder>(s, L, t, face, mat_word, (L.flags & kPlain) == 0u);
            T_NEXT();
            }
        } else if ((FEAT & kFeatVolumes) && best == OP_MEDIUM) {      // ConstantMedium::hit, constantmedium.rs:49-83
            // (the medium's record — boundary sphere inline — in one fetch: MediumDev, pt_device.h)
            f64x2 m0{0.0, 0.0}, m1{0.0, 0.0}, m2{0.0, 0.0};
            u32x4 m3{0u, 0u, 0u, 0u};
            const bool is_leaf = RT_REF_KIND(L.top) == RT_KIND_MEDIUM;
            if (is_leaf) {
                const uint32_t midx = RT_REF_INDEX(L.top);
                if (kLdsMedia && midx < kLdsMedia) {
                    m0 = md_lds[4 * midx]; m1 = md_lds[4 * midx + 1]; m2 = md_lds[4 * midx + 2];
                    m3 = reinterpret_cast<const u32x4 *>(md_lds)[4 * midx + 3];
                } else {
                    const f64x2 *mp = reinterpret_cast<const f64x2 *>(s.media_dev + midx);
                    m0 = mp[0]; m1 = mp[1]; m2 = mp[2];
                    m3 = reinterpret_cast<const u32x4 *>(mp)[3];
                }
            }
            t_pin(m0); t_pin(m1); t_pin(m2); t_pin(m3);
            if (is_leaf && m3.x != 0u) {
                // ConstantMedium::hit with a Sphere boundary, constantmedium.rs:49-83 in one go: the two
                // boundary queries are Sphere::hit (sphere.rs:39-58) on the same sphere with different t_min.
                struct { double neg_inv_density; } m{m2.x};
                struct { double radius; } q{m1.y};
                const Vec3 center(m0.x, m0.y, m1.x);
                const uint32_t mat_word = (uint32_t)(rtm::d2u(m2.y) >> 32);
                cnt.prim(RT_KIND_MEDIUM);
                cnt.prim(RT_KIND_SPHERE);
                double t1 = 0.0, t2 = 0.0;
                bool first;
                const bool both = sphere_t_twice(center, q.radius, L.cur, L.a_len, t1, t2, first);
                if (first) cnt.prim(RT_KIND_SPHERE);
                if (both) {
                    t1 = rtm::fmax_(t1, t_min);
                    t2 = rtm::fmin_(t2, L.closest);
                    if (!(t1 >= t2)) {
                        t1 = rtm::fmax_(t1, 0.0);
                        double ray_length = L.cur.d.length();
                        double distance_inside_boundary = (t2 - t1) * ray_length;
                        double rnd = L.rng.gen_f64();
                        double hit_distance = m.neg_inv_density * (rtm::log_(rnd) / rtm::log_(rtm::E_));
                        if (!(hit_distance > distance_inside_boundary)) t_accept<kOrder>(s, L, t1 + hit_distance / ray_length, 0, mat_word);   // (L.top is the medium)
                    }
                }
                T_NEXT();
            } else if (L.top != REF_MED2) {
                T_SETTLE();                                           // a medium leaf or a finished first query: same steps as inline
            } else if (L.top == REF_MED2) {
                uint32_t mref = L.med_ref;
                bool both = (L.flags & kSubFound) != 0;
                double t2 = L.sub_closest;
                L.med_ref = 0; L.t_lo = t_min;                        // back in the main query
                if (both) {
                    const MediumDev &m = s.media_dev[RT_REF_INDEX(mref)];
                    double t1 = rtm::fmax_(L.med_t1, t_min);
                    t2 = rtm::fmin_(t2, L.closest);
                    if (!(t1 >= t2)) {
                        t1 = rtm::fmax_(t1, 0.0);
                        double ray_length = L.cur.d.length();
                        double distance_inside_boundary = (t2 - t1) * ray_length;
                        double rnd = L.rng.gen_f64();
                        double hit_distance = m.neg_inv_density * (rtm::log_(rnd) / rtm::log_(rtm::E_));
                        if (!(hit_distance > distance_inside_boundary)) {
                            L.top = mref;                             // the medium itself is the winning leaf
                            t_accept<kOrder>(s, L, t1 + hit_distance / ray_length, 0, m.mat);
                        }
                    }
                }
                T_NEXT();
            }
        } else if ((FEAT & kFeatMisc) && best == OP_MISC) {                                 // Triangle, Ring
#pragma unroll 1
            for (int rep = 0; rep < kMiscReps && L.op == OP_MISC; rep++) {
            uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
            cnt.prim(kind);
            double t;
            bool h;
            uint32_t mat_word;
            if (kind == RT_KIND_TRIANGLE) {                           // rt_triangle, 80 B: a, b, c, mat
                const f64x2 *qp = reinterpret_cast<const f64x2 *>(s.triangles + idx);
                f64x2 q0 = qp[0], q1 = qp[1], q2 = qp[2], q3 = qp[3], q4 = qp[4];
                t_pin(q0); t_pin(q1); t_pin(q2); t_pin(q3); t_pin(q4);
                rt_triangle tr;
                tr.a[0] = q0.x; tr.a[1] = q0.y; tr.a[2] = q1.x; tr.b[0] = q1.y; tr.b[1] = q2.x; tr.b[2] = q2.y;
                tr.c[0] = q3.x; tr.c[1] = q3.y; tr.c[2] = q4.x;
                mat_word = (uint32_t)rtm::d2u(q4.y);
                h = triangle_t(tr, L.cur, L.t_lo, t_hi(L), t);
            } else {
                mat_word = s.rings[idx].mat;
                h = ring_t(s.rings[idx], L.cur, L.t_lo, t_hi(L), t);
            }
            if (h) t_accept<kOrder>(s, L, t, 0, mat_word);
            T_NEXT();
            }
        } else if ((FEAT & kFeatMovers) && best == OP_CTX) {                                  // movers in / out, HittableList expansion
            // 1/d of the ray changes only where d does: RotateY (x and z). Translate and Zoom leave the direction alone
            // (hittable/mod.rs:165-167,321-323), so entering or leaving them keeps inv and a_len — the same values the
            // three divisions would give again.
            if (L.top == REF_POPCTX) {
                // Leaving a mover. When the next stack entry is the exit of the enclosing mover too — the movers were nested directly,
                // nothing else waits in the frames between — all of them are left in this turn: only the outermost frame's ray is ever
                // used again (r3b: three turns, three world-ray fetches and three re-derivations became one for the meshes of wwscene).
                bool rotated = false;
                uint32_t levels = 0;
                do {
                    L.ctx.n--;
                    rotated = rotated || RT_REF_KIND(L.ctx.at(L.ctx.n)) == RT_KIND_ROTATE_Y;           // (a mover being left)
                    L.top = st.pop(L);
                } while (L.top == REF_POPCTX && L.ctx.n > 0u && ++levels < RT_MAX_XFORM_DEPTH);
                // the world ray from this lane's LDS column (written at refill), then back down to the enclosing frame
                XRay world;
                if (kStash) {
                    world = XRay{Vec3(wray[0 * WG], wray[1 * WG], wray[2 * WG]), Vec3(wray[3 * WG], wray[4 * WG], wray[5 * WG])};
                } else {
                    Ray wr = pv.load_ray(L.slot);
                    world = XRay{wr.orig, wr.dir};
                }
                L.cur = ray_at(L.ctx, L.ctx.n, world);
                if (rotated) {
                    // 1/d.x, 1/d.z of the frame arrived in: the stash holds them for the frame its RotateY was entered from — this one, or
                    // one whose direction is this one's (only a RotateY changes d); otherwise the two divisions again (same values).
                    bool stash_ok = kStashInv && L.stash_level != 0xFFFFFFFFu && L.stash_level >= L.ctx.n;
                    for (uint32_t j = L.ctx.n; stash_ok && j < L.stash_level && j < RT_MAX_XFORM_DEPTH; j++)
                        stash_ok = RT_REF_KIND(L.ctx.at(j)) != RT_KIND_ROTATE_Y;
                    if (stash_ok) { L.inv.x = L.stash_ix; L.inv.z = L.stash_iz; }
                    else { L.inv.x = 1.0 / L.cur.d.x; L.inv.z = 1.0 / L.cur.d.z; }
                    L.stash_level = 0xFFFFFFFFu;
                    L.a_len = L.cur.d.length_sqr();
                }
                t_flags(L, boxes_plain, order_on);
                T_SLABS();
                T_SETTLE();
            } else {
                uint32_t kind = RT_REF_KIND(L.top), idx = RT_REF_INDEX(L.top);
                if (kind == RT_KIND_LIST) {
                    cnt.prim(kind);
                    const rt_list &l = s.lists[idx];
                    for (uint32_t i = l.count; i > 0; i--) st.push(L, list_items[l.first + i - 1]);
                    T_NEXT();
                } else if (L.ctx.n < RT_MAX_XFORM_DEPTH) {
                    // Entering a mover — and, in the same turn, the movers its child is wrapped in directly.
#pragma unroll 1
                    for (uint32_t rep = 0; rep < RT_MAX_XFORM_DEPTH; rep++) {
                        cnt.prim(kind);
                        u32x4 x0;                                     // rt_xform, 32 B: kind, child, p[3]
                        f64x2 x1;
                        xform_words(idx, x0, x1);
                        t_pin(x0); t_pin(x1);
                        const double p0 = rtm::u2d(((uint64_t)x0.w << 32) | x0.z), p1 = x1.x, p2 = x1.y;
                        if (kind == RT_KIND_TRANSLATE) {              // Translate::hit, mod.rs:165-167
                            L.cur.o = L.cur.o - Vec3(p0, p1, p2);
                        } else if (kind == RT_KIND_ROTATE_Y) {        // RotateY::hit, mod.rs:235-247 (p0 = sin, p1 = cos)
                            const double ox = p1 * L.cur.o.x - p0 * L.cur.o.z, oz = p0 * L.cur.o.x + p1 * L.cur.o.z;
                            const double dx = p1 * L.cur.d.x - p0 * L.cur.d.z, dz = p0 * L.cur.d.x + p1 * L.cur.d.z;
                            L.cur.o.x = ox; L.cur.o.z = oz; L.cur.d.x = dx; L.cur.d.z = dz;
                            if (kStashInv) { L.stash_ix = L.inv.x; L.stash_iz = L.inv.z; L.stash_level = L.ctx.n; }
                            L.inv.x = 1.0 / dx; L.inv.z = 1.0 / dz;
                            L.a_len = L.cur.d.length_sqr();
                        } else {                                      // Zoom::hit, mod.rs:321-323: the origin only
                            L.cur.o = L.cur.o / p0;
                        }
                        L.ctx.push(L.top);
                        st.push(L, REF_POPCTX);
                        L.top = x0.y;
                        kind = RT_REF_KIND(L.top); idx = RT_REF_INDEX(L.top);
                        if (!(kind >= RT_KIND_TRANSLATE && kind <= RT_KIND_ZOOM && L.ctx.n < RT_MAX_XFORM_DEPTH)) break;
                    }
                    t_flags(L, boxes_plain, order_on);
                    T_SLABS();
                    T_SETTLE();
                } else {
                    cnt.prim(kind);
                    T_NEXT();
                }
            }
        } else if (best == OP_SHADE) {
            // OP_SHADE here = "this lane's traversal is finished (or it has no ray yet)":
            // publish the winner, then pull the next ray from the block's list.
            // (kAgain: the ray accepted a NaN distance after visits in another order than the reference's — t_accept. Nothing of it
            // is published; the lane takes the same list entry once more, kNaN still set: literal steps, the reference's order)
            const bool again = kOrder && (L.flags & kAgain) != 0u;
            if ((L.flags & kHasRay) && !again) {
                uint32_t slot = L.slot;
                bool found = L.win_leaf != REF_EMPTY;
                uint32_t kind = SK_MISS;
                const uint32_t steps16 = (L.steps > 0xFFFFu ? 0xFFFFu : L.steps) << 16;
                if (found) {
                    pv.store_hit(slot, L.closest, L.win_leaf, L.win_face | (L.win_chain.n << 4) | steps16, L.win_chain, L.win_mat);
                    kind = L.win_mat >> kMatKindShift;                // (the word came with the winning primitive's record)
                }
                pool.kind[L.entry] = (uint8_t)kind;                   // (by list position: see wf_shade)
                if (L.rng.draws) { pv.store_rng(slot, L.rng.s); cnt.draws(L.rng.draws); }
                t_flag(L, kHasRay, false);
            }
            const unsigned long long m = wballot(!again);
            const int leader = __ffsll((long long)m) - 1;
            uint32_t need = (uint32_t)__popcll(m);
            uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            uint32_t entry_idx = again ? L.entry : 0xFFFFFFFFu;       // index into pool.list of the entry this lane takes
            const u32x4 cs_now = *cs;
            uint32_t ch_base = cs_now.x, ch_n = cs_now.y, ch_taken = cs_now.z;
            bool drained = cs_now.w != 0;
            for (;;) {
                const uint32_t avail = ch_n - ch_taken;
                if (entry_idx == 0xFFFFFFFFu) {
                    if (rank < avail) entry_idx = ch_base + ch_taken + rank;
                    else rank -= avail;
                }
                const uint32_t take = need < avail ? need : avail;
                ch_taken += take;
                need -= take;
                if (need == 0 || drained) break;
                uint32_t id = 0;                                      // next chunk
                if ((int)lane == leader) id = atomicAdd(pool.next_chunk, 1u);
                id = (uint32_t)__shfl((int)id, leader);
                if (id >= total_ids) { drained = true; break; }
                const uint32_t slice = id / n_seg, seg = id - slice * n_seg, first = slice * kChunk;
                const uint32_t n = pool.list_n[seg];
                ch_n = n > first ? (n - first < kChunk ? n - first : kChunk) : 0u;
                ch_base = seg * (uint32_t)S + first;
                ch_taken = 0;
            }
            if ((int)lane == leader) *cs = (u32x4){ch_base, ch_n, ch_taken, drained ? 1u : 0u};
            if (probe && !dry_seen && drained) { dry_seen = true; t_dry = wall_clock64(); }
            if (entry_idx != 0xFFFFFFFFu) {
                const uint32_t sbase = entry_idx & ~((uint32_t)S - 1u);
                L.entry = entry_idx;
                L.slot = sbase + pool.list[entry_idx];
                uint64_t rs;
                Ray wr = pv.load_ray(L.slot, rs);
                L.tm = wr.tm;
                L.rng = Rng(rs);
                L.flags &= (kOrder && (L.flags & kAgain)) ? ~kAgain : ~(kAgain | kNaN);   // (a ray taken again keeps its kNaN)
                t_set_cur(L, XRay{wr.orig, wr.dir}, boxes_plain, order_on);
                T_SLABS();
                if (FEAT & kFeatMovers) L.stash_level = 0xFFFFFFFFu;
                if (kStash) {                                         // what leaving a mover goes back to (OP_CTX)
                    wray[0 * WG] = wr.orig.x; wray[1 * WG] = wr.orig.y; wray[2 * WG] = wr.orig.z;
                    wray[3 * WG] = wr.dir.x; wray[4 * WG] = wr.dir.y; wray[5 * WG] = wr.dir.z;
                }
                L.closest = rtm::F64_MAX;
                L.steps = 0;
                L.t_lo = t_min; L.med_ref = 0;
                L.win_leaf = REF_EMPTY; L.win_face = 0;
                L.ctx.n = 0;
                L.sp = 0;
                L.top = kTagged ? s.root_ord : s.root;
                T_SETTLE();
                t_flag(L, kHasRay, true);
            } else {
                L.op = OP_IDLE;
            }
        }
        TP_MARK(2 + best);
    }
    TP_FLUSH();
#ifdef RT2022_F32_CENSUS
    if (f32_steps) atomicAdd(&g_f32_census[0], (unsigned long long)f32_steps);
    if (f32_undecided) atomicAdd(&g_f32_census[1], (unsigned long long)f32_undecided);
    if (f32_wrong) atomicAdd(&g_f32_census[2], (unsigned long long)f32_wrong);
#endif
    if (probe && lane == 0) {
        unsigned long long t_end = wall_clock64();
        atomicMin(&pool.dbg[0], t_start);
        atomicMax(&pool.dbg[1], t_end);
        atomicAdd(&pool.dbg[2], t_end - t_start);
        atomicAdd(&pool.dbg[3], t_end - (dry_seen ? t_dry : t_end));
        atomicAdd(&pool.dbg[4], 1ull);
        if (tid == 0) { pool.dbg[8 + 2 * blockIdx.x] = t_start; pool.dbg[9 + 2 * blockIdx.x] = t_end; }
    }
    if (STATS) {
        cnt.flush_wave(stats);
        if (stats)                                                // (each lane adds what it counted as a round's first lane)
            for (int o = 0; o < 9; o++) {
                if (census_rounds[o]) atomicAdd(&stats->op_rounds[o], (unsigned long long)census_rounds[o]);
                if (census_lanes[o]) atomicAdd(&stats->op_lanes[o], (unsigned long long)census_lanes[o]);
            }
    }
}

// ---- which traversal kernel a call gets: one choice (choose_trace), one dispatch (launch_trace); TraceChoice: pt_wavefront.hpp ----
using TraceKernel = void (*)(SceneDev, WfPool, double, uint32_t, uint32_t, StatsDev *, uint32_t);
// A scene whose every primitive is a sphere (see f32_lds).
static bool sphere_only(const SceneDev &scene, unsigned features) { return features == 0 && scene.n_rects == 0; }
// Which instance runs a scene's traversal passes: a constant of the call. Counters exist for FEAT = 7 only and never with a node
// table; the probe exists per feature set for the small stack only, as FEAT = 7 for the deeper ones, never with a node table.
// A scene takes a node-table variant when its stacks fit the variant's, and its node table fits the cache whole or — see below — in part.
// (tune::kNoNodeTable — rt_debug_set_tuning — keeps the plain kernels: A/B runs, and the test that the two give the same bits.)
TraceChoice choose_trace(const SceneDev &scene, uint32_t stack_need, uint32_t word, unsigned features, bool counters, bool probe) {
    const bool spheres = sphere_only(scene, features), lean = !counters && !probe;
    TraceChoice c{kTablePlain, 0, features & 7u, counters, probe && !counters, false};
    if (lean && !tune::no_node_table(word) && stack_need <= (uint32_t)kStackTiny) {
        if (spheres && scene.n_nodes <= (uint32_t)kPrimNodes && scene.n_spheres <= (uint32_t)kPrimSpheres &&
            scene.n_moving_spheres <= (uint32_t)kPrimMoving) c.table = kTablePrims;
        else if (scene.n_nodes <= (uint32_t)kNodeCache) c.table = kTableWhole;
        // A scene whose nodes are tested in single precision from 32-byte records (sphere-only, or a triangle mesh: wf_trace, kF32G) takes
        // the plain kernels when its table does not fit whole: five waves per SIMD there against four here, and half the bytes per node
        // step either way — the partial table measured 10 % slower (1e4 spheres: 1 854 against 2 039 Mrays/s, profiles/r3zp_partial_vs_plain.log).
        else if (!f32_hbm(features, kTablePlain, spheres)) c.table = kTablePartial;
    }
    c.stack = c.table != kTablePlain ? kStackTiny : stack_need <= (uint32_t)kStackSmall ? kStackSmall : stack_need <= (uint32_t)kStackMid ? kStackMid : kStackLarge;
    if (counters || (probe && c.stack != kStackSmall)) c.feat = 7;
    // SPHERES: the instance that tests node boxes in single precision — on SceneDev::nodes32 in the plain kernels (kF32G), on the
    // single-precision records of t_slabs32 in the whole table (the all-in-LDS instance has them as PRIMS).
    c.spheres = spheres && lean && (c.table == kTablePlain || c.table == kTableWhole);
    return c;
}
// make(FEAT as a type) for a run-time feature set: the one place it becomes a template argument.
template <class Make>
static TraceKernel by_feat(unsigned feat, Make make) {
    switch (feat & 7u) {
        case 0: return make(std::integral_constant<unsigned, 0>{});
        case 1: return make(std::integral_constant<unsigned, 1>{});
        case 2: return make(std::integral_constant<unsigned, 2>{});
        case 3: return make(std::integral_constant<unsigned, 3>{});
        case 4: return make(std::integral_constant<unsigned, 4>{});
        case 5: return make(std::integral_constant<unsigned, 5>{});
        case 6: return make(std::integral_constant<unsigned, 6>{});
        default: return make(std::integral_constant<unsigned, 7>{});
    }
}
// Only the combinations named here are instantiated (58 of wf_trace<STACK, STATS, FEAT, PROBE, TABLE, SPHERES>: each costs over a
// second of compile time).
template <int STACK>
static TraceKernel plain_kernel(const TraceChoice &c) {
    if (c.stats) return wf_trace<STACK, true, 7>;
    if (c.probe) {
        if constexpr (STACK == kStackSmall) return by_feat(c.feat, [](auto f) -> TraceKernel { return wf_trace<STACK, false, decltype(f)::value, true>; });
        else return wf_trace<STACK, false, 7, true>;
    }
    if (c.spheres) return wf_trace<STACK, false, 0, false, kTablePlain, true>;
    return by_feat(c.feat, [](auto f) -> TraceKernel { return wf_trace<STACK, false, decltype(f)::value>; });
}
static TraceKernel trace_kernel(const TraceChoice &c) {
    switch (c.table) {
        case kTablePrims: return wf_trace<kStackTiny, false, 0, false, kTablePrims>;
        case kTableWhole:
            if (c.spheres) return wf_trace<kStackTiny, false, 0, false, kTableWhole, true>;
            return by_feat(c.feat, [](auto f) -> TraceKernel { return wf_trace<kStackTiny, false, decltype(f)::value, false, kTableWhole>; });
        case kTablePartial:
            return by_feat(c.feat, [](auto f) -> TraceKernel { return wf_trace<kStackTiny, false, decltype(f)::value, false, kTablePartial>; });
        default: break;
    }
    return c.stack == kStackSmall ? plain_kernel<kStackSmall>(c) : c.stack == kStackMid ? plain_kernel<kStackMid>(c) : plain_kernel<kStackLarge>(c);
}
// A persistent grid: as many workgroups as the kernel's launch bounds keep resident, never more than the work (a segment holds
// at most 4096 / kChunk chunks for the 4 waves of a workgroup). The node-table variants: one workgroup of kCacheBlock threads
// per CU (see wf_trace).
void launch_trace(const TraceChoice &c, const WfLaunch &w, uint32_t parity) {
    const bool plain = c.table == kTablePlain;
    const uint32_t cus = w.pool.n_cus ? w.pool.n_cus : 1u;
    const uint32_t most = plain ? w.blocks * ((uint32_t)S / kChunk / 4u) : std::max(1u, w.blocks * ((uint32_t)S / kChunk) / (uint32_t)(kCacheBlock / 64));
    const uint32_t grid = std::min(plain ? (uint32_t)trace_blocks_per_cu(c.stack, c.stats, c.feat) * cus : cus, most);
    hipLaunchKernelGGL(trace_kernel(c), dim3(grid), dim3(trace_wg(c.table)), 0, w.stream, w.scene, w.pool, w.t_min,
                       w.tuning, parity, w.stats, w.vote_weights);
}

hipError_t f32_slab_census(unsigned long long out[5]) {
    unsigned long long c[3] = {0, 0, 0};
    hipError_t e = hipMemcpyFromSymbol(c, HIP_SYMBOL(g_f32_census), sizeof(c));
    if (e != hipSuccess) return e;
    const unsigned long long zero[3] = {0, 0, 0};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_f32_census), zero, sizeof(zero));
    out[0] = c[0]; out[1] = c[1]; out[4] = c[2];
#ifdef RT2022_F32_CENSUS
    out[2] = 1; out[3] = 2;
#else
    out[2] = 0; out[3] = 1;
#endif
    return e;
}

// From the same choice as the launches, asking f32_lds / f32_hbm with the choice's own template facts (bit 1 of out[3]: the
// instance tests node boxes in single precision — wf_trace: kF32, kF32G).
void trace_variant(const SceneDev &scene, uint32_t stack_need, uint32_t tuning, unsigned features, uint32_t out[4]) {
    const TraceChoice c = choose_trace(scene, stack_need, tuning, features, false, false);
    const bool table = c.table != kTablePlain;
    const bool f32 = f32_lds(c.feat, c.table, c.spheres) || f32_hbm(c.feat, c.table, c.spheres, c.stats, c.probe);
    out[0] = (uint32_t)(table ? kCacheBlock : kBlock);
    out[1] = (uint32_t)c.stack;
    out[2] = !table ? 0u : scene.n_nodes < (uint32_t)kNodeCache ? scene.n_nodes : (uint32_t)kNodeCache;
    // (bit 2: the timed instance visits the nearer child first — it is built to, the tuning word lets it, and the scene has an order
    // to go by; bit 3: the counting instance does — never)
    const bool orders = trace_orders(c.stats, c.feat) && !tune::ref_order(tuning) && scene.prim_rank != nullptr;
    out[3] = (c.table == kTablePrims ? 1u : 0u) | (f32 ? 2u : 0u) | (orders ? 4u : 0u) | (trace_orders(true, 7u) ? 8u : 0u);
}

// Diagnostic build: what the phase clock of the traversal kernel added up to over the render.
#ifdef RT2022_TRACE_PROBE
void print_trace_probe(const WfPool &pool) {
    unsigned long long h[12];
    if (hipMemcpy(h, pool.dbg + 96, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
        static const char *const names[12] = {"node_fast", "vote", "node", "sphere", "rect", "box", "medium", "misc", "ctx", "done", "rest", "-"};
        double tot = 0; for (int i = 0; i < 11; i++) tot += (double)h[i];
        fprintf(stderr, "trace probe (shader-clock ticks of all waves and passes; share):");
        for (int i = 0; i < 11; i++) fprintf(stderr, " %s %.3f", names[i], tot > 0 ? (double)h[i] / tot : 0.0);
        fprintf(stderr, "  total %.3e ticks\n", tot);
    }
    (void)hipMemset(pool.dbg + 96, 0, 12 * sizeof(unsigned long long));
}
#endif

} // namespace rt2022
