// pt_wavefront_shade.hip — the shade pass of the wavefront engine (pt_wavefront.hip): wf_shade and its launcher.
#include <cstdio>

#include "pt_wavefront.hpp"

namespace rt2022 {

namespace {

// list order: 16 classes of expected length x classes of where the ray starts (camera / sphere / box, rect / medium) x 8 direction octants
constexpr uint32_t kOriginClasses = 4u;
constexpr uint32_t kListBins = 16 * kOriginClasses * 8;
constexpr int kShadeWaves = 3;             // resident shade workgroups per CU = waves per SIMD (168 VGPRs; four: 128 VGPRs, 51 spilled)

// Bounce tape of one slot (see Tape in pt_kernel.hip): its records are contiguous in HBM,
// record k = 4 doubles {w.x, w.y, w.z, p} at tape[(slot*cap + k)*4], so unwinding a path reads
// a few adjacent cache lines; the loads of four records are issued together before use.
struct SlotTape {
    double *base;          // this slot's first record
    RT_DEV void put(uint32_t k, Vec3 w, double p) const {
        double2 *q = reinterpret_cast<double2 *>(base + (uint64_t)k * 4);
        q[0] = make_double2(w.x, w.y);
        q[1] = make_double2(w.z, p);
    }
    RT_DEV static Vec3 step(Vec3 Lr, double2 a, double2 b) {
        Vec3 w(a.x, a.y, b.x);
        return Vec3(0.0, 0.0, 0.0) + (w * Lr) / b.y;           // emitted + ((att*spdf) * L) / pdf_val, main.rs:267-271
    }
    RT_DEV Vec3 unwind(uint32_t nb, Vec3 Lr) const {
        const double2 *q = reinterpret_cast<const double2 *>(base);
        uint32_t k = nb;
        while (k >= 4) {
            double2 a3 = q[2 * (k - 1)], b3 = q[2 * (k - 1) + 1], a2 = q[2 * (k - 2)], b2 = q[2 * (k - 2) + 1];
            double2 a1 = q[2 * (k - 3)], b1 = q[2 * (k - 3) + 1], a0 = q[2 * (k - 4)], b0 = q[2 * (k - 4) + 1];
            Lr = step(Lr, a3, b3); Lr = step(Lr, a2, b2); Lr = step(Lr, a1, b1); Lr = step(Lr, a0, b0);
            k -= 4;
        }
        for (; k > 0; k--) Lr = step(Lr, q[2 * (k - 1)], q[2 * (k - 1) + 1]);
        return Lr;
    }
};

// Path bookkeeping of one slot, one 32-byte record: {item's index in the partial sums (u64), smp, smp_end, depth, px, py, frame}.
struct SlotState {
    uint64_t item;
    uint32_t smp, smp_end, depth, px, py, frame;
};
RT_DEV SlotState load_state(const WfPool &p, uint32_t slot) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p.state + (uint64_t)slot * kRecWords);
    uint4 a = q[0], b = q[1];
    SlotState st;
    st.item = ((uint64_t)a.y << 32) | a.x;
    st.smp = a.z; st.smp_end = a.w; st.depth = b.x; st.px = b.y; st.py = b.z; st.frame = b.w;
    return st;
}
// (A bounce changes the depth only: the first half is rewritten when a new sample or item starts.)
RT_DEV void store_state(const WfPool &p, uint32_t slot, const SlotState &st, bool whole) {
    uint4 *q = reinterpret_cast<uint4 *>(p.state + (uint64_t)slot * kRecWords);
    if (whole) q[0] = make_uint4((uint32_t)st.item, (uint32_t)(st.item >> 32), st.smp, st.smp_end);
    q[1] = make_uint4(st.depth, st.px, st.py, st.frame);
}

// The device copies of the primitive pools carry, above the material index, the slot kind a hit on the primitive
// leads to (kMatKindShift; rt_scene_create): publishing a winner then costs one dependent load, not three.
RT_DEV bool t_finite_s(double x) { return (rtm::d2u(x) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

RT_DEV uint32_t leaf_material_word(const SceneDev &s, uint32_t leaf) {
    uint32_t idx = RT_REF_INDEX(leaf);
    switch (RT_REF_KIND(leaf)) {
        case RT_KIND_SPHERE: return s.spheres[idx].mat;
        case RT_KIND_MOVING_SPHERE: return s.moving_spheres[idx].mat;
        case RT_KIND_RECT: return s.rects[idx].mat;
        case RT_KIND_BOX: return s.boxes[idx].mat;
        case RT_KIND_TRIANGLE: return s.triangles[idx].mat;
        case RT_KIND_RING: return s.rings[idx].mat;
        default: return s.media[idx].mat;
    }
}


// The winning primitive's record as the shade pass fetches it: a fixed 80 bytes from the record's address, whatever
// the kind (the longest records — Triangle, MovingSphere — are 80 bytes; shorter ones run on into their neighbour or
// into the pool's zeroed slack, rt_scene_create) — one address computation, five loads, no branch.
struct PrimRegs { f64x2 r0, r1, r2, r3, r4; };
// ... with the pools' base addresses and record sizes taken from a 16-entry table in LDS, indexed by kind (wf_shade fills it
// once): seven pointer pairs need not sit in scalar registers through the whole shade loop (r3: they were being spilled), and
// the select chain below becomes one 8-byte LDS read.
struct PrimTable { unsigned long long base[16]; uint32_t stride[16]; };
RT_DEV void prim_table_fill(const SceneDev &s, PrimTable &t, uint32_t tid) {
    if (tid < 16) {
        const void *b = s.media; uint32_t st = (uint32_t)sizeof(rt_medium);
        if (tid == RT_KIND_SPHERE) { b = s.spheres; st = (uint32_t)sizeof(rt_sphere); }
        else if (tid == RT_KIND_MOVING_SPHERE) { b = s.moving_spheres; st = (uint32_t)sizeof(rt_moving_sphere); }
        else if (tid == RT_KIND_RECT) { b = s.rects; st = (uint32_t)sizeof(rt_rect); }
        else if (tid == RT_KIND_BOX) { b = s.boxes; st = (uint32_t)sizeof(rt_box); }
        else if (tid == RT_KIND_TRIANGLE) { b = s.triangles; st = (uint32_t)sizeof(rt_triangle); }
        else if (tid == RT_KIND_RING) { b = s.rings; st = (uint32_t)sizeof(rt_ring); }
        t.base[tid] = (unsigned long long)reinterpret_cast<uintptr_t>(b);
        t.stride[tid] = st;
    }
}
RT_DEV const f64x2_a8 *prim_address(const PrimTable &t, uint32_t leaf) {
    const uint32_t kind = RT_REF_KIND(leaf), idx = RT_REF_INDEX(leaf);
    return reinterpret_cast<const f64x2_a8 *>(static_cast<uintptr_t>(t.base[kind] + (unsigned long long)idx * t.stride[kind]));
}
// winner_record (pt_common.hpp) fed from registers: the HitRecord of the winning candidate, rebuilt from (leaf, t) in
// the leaf's own frame (sphere.rs:59-65,158-164, aarect.rs:51-71, boxes.rs:24-66, triangle.rs:54-76, ring.rs:49-52,
// constantmedium.rs:66-74) and then carried out through its movers.
RT_DEV void winner_record_regs(const SceneDev &s, const Ray &wr, const Winner &w, const PrimRegs &q, HitRec &rec, bool want_uv) {
    const XRay world{wr.orig, wr.dir};
    XRay r = ray_at_level(s, w.chain, w.chain.n, world);
    const uint32_t kind = RT_REF_KIND(w.leaf);
    const double t = w.t;
    rec.mat = 0;
    switch (kind) {
        case RT_KIND_SPHERE: case RT_KIND_MOVING_SPHERE: {
            Vec3 center; double radius;
            if (kind == RT_KIND_SPHERE) { center = Vec3(q.r0.x, q.r0.y, q.r1.x); radius = q.r1.y; }
            else {
                const Vec3 c0(q.r0.x, q.r0.y, q.r1.x), c1(q.r1.y, q.r2.x, q.r2.y);
                center = c0 + (c1 - c0) * ((wr.tm - q.r3.x) / (q.r3.y - q.r3.x));
                radius = q.r4.x;
            }
            Vec3 at = r.o + r.d * t;
            Vec3 outward_normal = (at - center) / radius;
            rec.u = 0.0; rec.v = 0.0;
            if (want_uv) sphere_uv(outward_normal, rec.u, rec.v);
            rec.p = at; rec.t = t;
            rec.set_face_normal(r.d, outward_normal);
            break;
        }
        case RT_KIND_RECT: {
            RectP rp{(uint32_t)rtm::d2u(q.r2.y), q.r0.x, q.r0.y, q.r1.x, q.r1.y, q.r2.x};
            rect_record(rp, 0u, r, t, rec);
            break;
        }
        case RT_KIND_BOX: {
            const double p0x = q.r0.x, p0y = q.r0.y, p0z = q.r1.x, p1x = q.r1.y, p1y = q.r2.x, p1z = q.r2.y;
            const uint32_t i = w.face;
            RectP rp;                                                // boxes.rs:24-66
            if (i < 2) rp = RectP{RT_RECT_XY, p0x, p1x, p0y, p1y, i == 0 ? p1z : p0z};
            else if (i < 4) rp = RectP{RT_RECT_XZ, p0x, p1x, p0z, p1z, i == 2 ? p1y : p0y};
            else rp = RectP{RT_RECT_YZ, p0y, p1y, p0z, p1z, i == 4 ? p1x : p0x};
            rect_record(rp, 0u, r, t, rec);
            break;
        }
        case RT_KIND_TRIANGLE: {
            const Vec3 a(q.r0.x, q.r0.y, q.r1.x), b(q.r1.y, q.r2.x, q.r2.y), c(q.r3.x, q.r3.y, q.r4.x);
            Vec3 n = rtm::to_unit(rtm::cross(b - a, c - a));
            Vec3 p = r.o + r.d * t;
            double a1 = a.x - b.x, b1 = a.x - c.x, c1 = a.x - p.x;
            double a2 = a.y - b.y, b2 = a.y - c.y, c2 = a.y - p.y;
            rec.u = (c1 * b2 - b1 * c2) / (a1 * b2 - b1 * a2);
            rec.v = (a1 * c2 - a2 * c1) / (a1 * b2 - b1 * a2);
            rec.p = p; rec.t = t;
            rec.set_face_normal(r.d, n);
            break;
        }
        case RT_KIND_RING: {
            rec.p = r.o + r.d * t; rec.t = t; rec.u = 0.0; rec.v = 0.0;
            rec.set_face_normal(r.d, Vec3(0.0, 1.0, 0.0));
            break;
        }
        default: {
            rec.p = r.o + r.d * t; rec.normal = Vec3(1.0, 0.0, 0.0); rec.t = t; rec.u = 0.0; rec.v = 0.0;
            rec.front_face = true;
            break;
        }
    }
    if (w.leaf & RT_REF_FLIP) rec.front_face = !rec.front_face;
    for (uint32_t lvl = w.chain.n; lvl > 0; lvl--) {
        XRay moved = ray_at_level(s, w.chain, lvl, world);
        xform_record(s, w.chain.at(lvl - 1), moved, rec);
    }
}
// Texture::value of a material's texture whose top-level record came with the material (MaterialDev): a SolidColor
// answers from registers; everything else goes the general way.
RT_DEV Vec3 texture_value_top(const SceneDev &s, uint32_t tex, uint32_t tex_kind, Vec3 color, double u, double v, Vec3 p) {
    if (tex_kind == RT_TEX_SOLID) return color;
    return texture_value(s, tex, u, v, p);
}

} // namespace

// =====================================================================================
// Shade pass.
// =====================================================================================
// Section clock of the shade pass (diagnostic build -DRT2022_SHADE_PROBE only; tools/shade_probe.sh): wave 0's lane 0 of
// every workgroup adds the wall-clock ticks it spent in each section to pool.dbg[64 + section].
#ifdef RT2022_SHADE_PROBE
#define SP_DECL unsigned long long sp_t = wall_clock64(), sp_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define SP_MARK(i) do { unsigned long long sp_n = wall_clock64(); sp_acc[i] += sp_n - sp_t; sp_t = sp_n; } while (0)
#define SP_FLUSH() do { if (tid == 0 && pool.dbg) for (int sp_i = 0; sp_i < 10; sp_i++) atomicAdd(&pool.dbg[64 + sp_i], sp_acc[sp_i]); } while (0)
#else
#define SP_DECL do {} while (0)
#define SP_MARK(i) do {} while (0)
#define SP_FLUSH() do {} while (0)
#endif

// RING: the partial-sum ring of RenderArgs::ring is in use (a build of its own: the default instance carries none of its
// bookkeeping — bounded claims, starved slots, the oldest item in flight).
// SRC: where a new path starts. kSrcRows: the camera's ray for a pixel of the render's row list. kSrcRays: the caller's ray
// (RenderArgs::rays, rt_radiance*) instead of the camera's: "pixel" = ray index, no row ids, no camera draws. kSrcPixels: the
// camera's ray for an entry of a list of (frame, pixel) ids (RenderArgs::pixel_ids, rt_render_pixels*): "pixel" = list entry,
// no row ids; the camera's draws are the row source's, on the image's own width and height. Everything else — the first sweep,
// the unwinding, the planes and the ring — is the render's in all three.
constexpr int kSrcRows = 0, kSrcRays = 1, kSrcPixels = 2;
template <bool STATS, bool RING = false, int SRC = kSrcRows>
__global__ void __launch_bounds__(kBlock, kShadeWaves) wf_shade(const SceneDev s, const RenderArgs *__restrict__ ap, const WfPool pool, const uint32_t parity) {
    __shared__ uint32_t hist[SK_COUNT];
    __shared__ uint32_t cursor[SK_COUNT];
    __shared__ uint32_t sorted[S];
    __shared__ uint32_t n_sorted;
    __shared__ uint8_t new_kind[S];      // the slots' next state (| list class << 4), written back in one coalesced sweep
    __shared__ uint32_t bins[kListBins];
    __shared__ uint8_t new_oct[S];       // direction octant of the slot's next ray (second sort key of the list)
    __shared__ uint16_t fresh_q[S];      // slots that want a new path (| 0x8000: the slot holds an item whose state counts)
    static_assert(kSlotsPerBlock <= 32768 && kSlotsPerBlock % kBlock == 0, "a segment's slot index shares a u16 with one flag bit (fresh_q), and the sorts deal S / kBlock slots to every thread");
    static_assert(kSlotsPerBlock <= 65536, "`sorted` packs slot | kind << 16");
    __shared__ uint32_t n_fresh;
    const RenderArgs &a = *ap;
    const PoolView pv{pool};
    const uint32_t base = blockIdx.x * (uint32_t)S;
    const uint32_t tid = threadIdx.x;
    const unsigned lane = tid & 63u;
    Counters<STATS> cnt;

    // The light list with its primitives' numbers, in LDS when it is short (it is one or two entries in every scene of
    // the reference): MixturePdf's two visits per bounce (generate + value, pdf.rs:94-104) then cost no memory round trip.
    constexpr uint32_t kLdsLights = 8;
    __shared__ LightRec lights_lds[kLdsLights];
    __shared__ PrimTable prim_tab;
    prim_table_fill(s, prim_tab, tid);
    if (tid < kLdsLights && tid < s.n_lights) lights_lds[tid] = fetch_light(s, tid);
    auto light_at = [&](uint32_t li) { return li < kLdsLights ? lights_lds[li] : fetch_light(s, li); };
    SP_DECL;
    if (tid < SK_COUNT) hist[tid] = 0;
    if (tid == 0) n_fresh = 0;
    __syncthreads();
    // Counting sort by kind of the slots that carried a ray through the trace pass: the entries of the segment's list
    // (written by the previous shade pass, or by wf_init: every slot in use, FRESH) with the kind the trace pass left
    // at the same position. Slots not on the list are idle. (Kinds live by list position, not by slot: the lanes of a
    // traversal wave take neighbouring entries, so their one-byte results land in the same cache lines at about the same
    // time instead of dirtying a line per byte all over the segment.)
    const uint32_t n_rays = pool.list_n[blockIdx.x] < (uint32_t)S ? pool.list_n[blockIdx.x] : (uint32_t)S;
    // (ring mode: behind the rays sit the slots that found the ring full last pass, kind FRESH: they ask again now)
    const uint32_t n_starved_in = RING ? (pool.starved_n[blockIdx.x] < (uint32_t)S - n_rays ? pool.starved_n[blockIdx.x] : (uint32_t)S - n_rays) : 0u;
    const uint32_t n_listed = n_rays + n_starved_in;
    uint32_t my_kind[S / kBlock], my_slot[S / kBlock];
#pragma unroll
    for (int i = 0; i < S / kBlock; i++) {
        const uint32_t e = (uint32_t)(i * kBlock) + tid;
        uint32_t k = SK_IDLE, ls = 0;
        if (e < n_listed) { k = pool.kind[base + e]; ls = pool.list[base + e]; }
        my_kind[i] = k; my_slot[i] = ls;
        new_kind[e] = (uint8_t)SK_IDLE;
        if (k != SK_IDLE) atomicAdd(&hist[k], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < SK_COUNT; k++) { cursor[k] = acc; acc += hist[k]; }
        n_sorted = acc;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < S / kBlock; i++) {
        uint32_t k = my_kind[i];
        if (k != SK_IDLE) sorted[atomicAdd(&cursor[k], 1u)] = my_slot[i] | (k << 16);
    }
    __syncthreads();
    SP_MARK(0);                                                      // 0: counting sort
    const uint32_t total = n_sorted;
    const Vec3 background = ld3(a.background);
    // One sample per work item (spp_chunk = 1): the item's running sum needs no place of its own in the pool.
    const bool single = a.chunk == 1 && a.spp > 0 && a.max_depth > 0;
    const bool small_job = a.n_items <= 0xFFFFFFFFull;
    const uint32_t step_shift = tune::class_shift(a.tuning);          // list class = expected steps >> shift (0 = slot order)

    unsigned long long my_oldest = ~0ull;                            // (ring mode) the oldest work item among this thread's paths that go on
    for (uint32_t j0 = 0; j0 < total; j0 += kBlock) {
        const uint32_t j = j0 + tid;
        const bool on = j < total;
        uint32_t slot = 0, kind = SK_IDLE;
        if (on) { uint32_t e = sorted[j]; slot = base + (e & 0xFFFFu); kind = e >> 16; }
        // Every slot that carried a ray has been through the trace pass by now. One that has not would lose its
        // path without a trace (it is neither shaded nor re-listed): report it instead — the render then fails.
        if (on && kind == SK_TRACE) atomicOr(pool.fault, 1u);
        bool alive = false;          // path continues with a new ray
        bool ended = false;          // path ended: add to pixel, start the next sample
        Ray r;
        Rng rng;
        Vec3 Lterm(0.0, 0.0, 0.0);
        SlotTape tape{pool.tape + (uint64_t)slot * pool.tape_cap * 4};
        // Everything the slot owns is fetched up front, side by side (the records are independent of
        // `kind`; a FRESH slot's are stale but mapped), instead of one latency after another.
        SlotState stt{};
        Winner w;
        w.t = 0.0; w.leaf = 0; w.face = 0; w.chain.n = 0; w.chain.c0 = w.chain.c1 = w.chain.c2 = w.chain.c3 = 0;
        uint32_t steps = 0;          // node steps of the ray that has just been traced
        uint32_t mat_word = 0;
        PrimRegs prim{{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}};
        f64x2 md0{0.0, 0.0}, md1{0.0, 0.0}, md2{0.0, 0.0}, md3{0.0, 0.0}, md4{0.0, 0.0};      // MaterialDev
        if (on) {
            stt = load_state(pool, slot);
            if (kind > SK_MISS) {                                 // (a miss ends its path and a fresh slot has none: neither needs the ray or the winner)
                uint64_t rs;
                r = pv.load_ray(slot, rs);
                rng = Rng(rs);
                const u32x4 *hq = reinterpret_cast<const u32x4 *>(pool.hit + (uint64_t)slot * kRecWords);
                u32x4 ha = hq[0], hb = hq[1];
                t_pin(ha); t_pin(hb);
                bool have_mat;
                PoolView::decode_hit(ha, hb, w, steps, mat_word, have_mat);
                if (!have_mat) mat_word = leaf_material_word(s, w.leaf);      // (four movers deep: the chain needed the word's place)
                // second round trip, everything at once: the winning primitive's record and its material's
                const f64x2_a8 *pp = prim_address(prim_tab, w.leaf);
                const f64x2 *mp = reinterpret_cast<const f64x2 *>(s.materials_dev + (mat_word & kMatIndexMask));
                prim.r0 = pp[0]; prim.r1 = pp[1]; prim.r2 = pp[2]; prim.r3 = pp[3]; prim.r4 = pp[4];
                md0 = mp[0]; md1 = mp[1]; md2 = mp[2]; md3 = mp[3]; md4 = mp[4];
                t_pin(prim.r0); t_pin(prim.r1); t_pin(prim.r2); t_pin(prim.r3); t_pin(prim.r4);
                t_pin(md0); t_pin(md1); t_pin(md2); t_pin(md3); t_pin(md4);
            }
        }
        SP_MARK(1);                                                  // 1: slot, hit, primitive and material fetches
        // MaterialDev: tex, tex_kind | albedo | param | tex_color | tex_scale | tex_a, tex_b
        const uint32_t m_tex = (uint32_t)rtm::d2u(md0.x), m_tex_kind = (uint32_t)(rtm::d2u(md0.x) >> 32);
        const Vec3 m_albedo(md0.y, md1.x, md1.y), m_tex_color(md2.y, md3.x, md3.y);
        const double m_param = md2.x;
        // (top bit of the stored depth: some record of the path's tape is not "finite weight, pdf neither 0 nor NaN")
        uint32_t depth = stt.depth & 0x7FFFFFFFu;
        uint32_t tainted = stt.depth >> 31;
        // Expected length of the slot's next traversal, for the order of the trace pass's list: a bounce ray is taken
        // to resemble the ray before it; a new sample's camera ray goes with the short ones. (A per-slot record of the
        // previous camera ray's length predicts better, but costs a gather and a scatter per slot: measured -1.4 %.)
        // Ordering only: results never depend on it.
        uint32_t expect = steps;

        if (on && kind >= SK_MISS) {
            if (kind == SK_MISS) {
                Lterm = background;                                   // main.rs:275-276
                ended = true;
            } else {
                // (u, v) only matter to image textures (and to a checker that may select one).
                bool want_uv = false;
                const bool lambertian = kind >= SK_LAMB_SOLID && kind <= SK_LAMB_IMAGE;
                if (lambertian) {                                     // (the slot kind says which texture it is)
                    want_uv = kind == SK_LAMB_IMAGE || kind == SK_LAMB_CHECKER;
                } else if (kind == SK_LIGHT || kind == SK_ISOTROPIC) {
                    want_uv = m_tex_kind == RT_TEX_IMAGE || m_tex_kind == RT_TEX_CHECKER;
                }
                HitRec rec;
                winner_record_regs(s, r, w, prim, rec, want_uv);
                SP_MARK(2);                                           // 2: the winner's hit record
                if (kind == SK_LIGHT) {                               // emitted; scatter = None (material/mod.rs:16-18,174-180)
                    Lterm = rec.front_face ? texture_value_top(s, m_tex, m_tex_kind, m_tex_color, rec.u, rec.v, rec.p) : Vec3(0.0, 0.0, 0.0);
                    ended = true;
                } else {
                    Vec3 wgt;
                    double p = 1.0;
                    Vec3 dir;
                    double tm = r.tm;
                    if (lambertian) {                                 // material/mod.rs:51-65 + main.rs:263-271
                        Vec3 att = texture_value_top(s, m_tex, m_tex_kind, m_tex_color, rec.u, rec.v, rec.p);
                        rtm::Onb uvw = rtm::onb_from_w(rec.normal);
                        double cosv;
                        if (s.n_lights == 0) {                        // cosine-only mode
                            dir = uvw.local_vec(random_cosine_direction(rng));
                            cosv = rtm::dot(rtm::to_unit(dir), uvw.w);
                            p = cosv <= 0.0 ? 0.0 : cosv / rtm::PI;
                        } else {                                      // MixturePdf(lights, cos), pdf.rs:94-104
                            if (rng.gen_range(0.0, 1.0) < 0.5) dir = lights_random_of(s.n_lights, light_at, rec.p, rng);
                            else dir = uvw.local_vec(random_cosine_direction(rng));
                            double lp = lights_pdf_value_of<STATS>(s.n_lights, light_at, rec.p, dir, cnt);
                            cosv = rtm::dot(rtm::to_unit(dir), uvw.w);
                            double cp = cosv <= 0.0 ? 0.0 : cosv / rtm::PI;
                            p = 0.5 * lp + 0.5 * cp;
                        }
                        double cosine = rtm::dot(rec.normal, rtm::to_unit(dir));
                        double spdf = cosine < 0.0 ? 0.0 : cosine / rtm::PI;
                        wgt = att * spdf;
                    } else if (kind == SK_METAL) {                    // material/mod.rs:85-96
                        Vec3 reflected = rtm::reflect(rtm::to_unit(r.dir), rec.normal);
                        dir = reflected + random_in_unit_sphere(rng) * m_param;
                        wgt = m_albedo;
                        tm = 0.0;                                     // time = 0., mod.rs:91
                    } else if (kind == SK_DIELECTRIC) {               // material/mod.rs:120-147
                        double refraction_ratio = rec.front_face ? 1.0 / m_param : m_param;
                        Vec3 unit_direction = rtm::to_unit(r.dir);
                        double cos_theta = rtm::fmin_(rtm::dot(-unit_direction, rec.normal), 1.0);
                        double sin_theta = rtm::sqrt_(1.0 - cos_theta * cos_theta);
                        bool cannot_refract = refraction_ratio * sin_theta > 1.0;
                        double random_double = rng.gen_range(0.0, 1.0);
                        dir = (cannot_refract || reflectance(cos_theta, refraction_ratio) > random_double)
                                  ? rtm::reflect(unit_direction, rec.normal)
                                  : rtm::refract(unit_direction, rec.normal, refraction_ratio);
                        wgt = Vec3(1.0, 1.0, 1.0);
                    } else {                                          // Isotropic, material/mod.rs:207-213
                        wgt = texture_value_top(s, m_tex, m_tex_kind, m_tex_color, rec.u, rec.v, rec.p);
                        dir = random_in_unit_sphere(rng);
                    }
                    uint32_t nb = a.max_depth - depth;
                    tape.put(nb, wgt, p);
                    tainted |= (t_finite_s(wgt.x) && t_finite_s(wgt.y) && t_finite_s(wgt.z) && p == p && p != 0.0) ? 0u : 1u;
                    r = Ray(rec.p, dir, tm);
                    depth--;
                    if (depth == 0) ended = true;                     // the next ray_color returns (0,0,0), main.rs:240-242
                    else alive = true;
                }
            }
            SP_MARK(3);                                               // 3: emitted / scatter / pdfs / tape record
            if (ended) {
                uint32_t nb = a.max_depth - depth;
                // Unwinding from an exact zero through records with finite weights and usable pdfs gives 0 + (w * 0) / p =
                // +0 at every step (a black background, a light seen from behind, an exhausted depth): the tape need not
                // be read. Anything else — a pdf of 0, an infinite weight: the reference's NaN pixels — is unwound.
                Vec3 Lp(0.0, 0.0, 0.0);
                if (!(nb >= 1 && !tainted && Lterm.x == 0.0 && Lterm.y == 0.0 && Lterm.z == 0.0)) Lp = tape.unwind(nb, Lterm);
                if (single) {                                         // the item's one sample: 0 + L goes straight to its place
                    double *o = a.partial + stt.item * 3;                 // (ring mode: its plane is sample mod R — worked out when the path began)
                    o[0] = 0.0 + Lp.x; o[1] = 0.0 + Lp.y; o[2] = 0.0 + Lp.z;   // pixel_color = 0; pixel_color += ..., main.rs:143,150
                } else {
                    double2 *ps = reinterpret_cast<double2 *>(pool.pixel_sum + (uint64_t)slot * 4);
                    double2 s0 = ps[0], s1 = ps[1];
                    ps[0] = make_double2(s0.x + Lp.x, s0.y + Lp.y);       // pixel_color += ..., main.rs:150
                    ps[1] = make_double2(s1.x + Lp.z, 0.0);
                }
            }
            cnt.draws(rng.draws);                                     // words drawn while scattering
            rng.draws = 0;
        }

        SP_MARK(4);                                                   // 4: unwinding and the pixel
        // A slot whose path has ended (or that never had one) gets its next path in the second sweep below, where all
        // such slots of the segment sit side by side: aiming a camera ray (three hashes, the lens rejection loop, five
        // divisions) is the longest stretch of this kernel, and here it would run for the fifth of the lanes that need it.
        const bool want_path = on && (kind == SK_FRESH || ended);
        {
            const unsigned long long wm = wballot(want_path);
            if (wm) {
                const int leader = __ffsll((long long)wm) - 1;
                uint32_t qbase = 0;
                if ((int)lane == leader) qbase = atomicAdd(&n_fresh, (uint32_t)__popcll(wm));
                qbase = (uint32_t)__shfl((int)qbase, leader);
                if (want_path) fresh_q[qbase + (uint32_t)__popcll(wm & ((1ull << lane) - 1ull))] =
                    (uint16_t)((slot - base) | ((kind != SK_FRESH && !single) ? 0x8000u : 0u));
            }
        }

        if (RING && on && alive) { const unsigned long long grp = (stt.smp - 1u) / a.ring_group; my_oldest = grp < my_oldest ? grp : my_oldest; }      // (smp - 1: the sample in flight)
        if (on && alive) {
            cnt.ray();                                                // world.hit(r, 0.001, f64::MAX), main.rs:243
            pv.store_ray(slot, r, rng.s);
            stt.depth = depth | (tainted << 31);
            store_state(pool, slot, stt, false);
            uint32_t cls = step_shift ? (expect >> step_shift) : 0u;
            new_kind[slot - base] = (uint8_t)(SK_TRACE | ((cls > 15u ? 15u : cls) << 4));
            // (third key: what the ray starts from — a sphere, a box / rect, a medium)
            const uint32_t lk = RT_REF_KIND(w.leaf);
            const uint32_t org = (lk == RT_KIND_SPHERE || lk == RT_KIND_MOVING_SPHERE) ? 1u : (lk == RT_KIND_BOX || lk == RT_KIND_RECT) ? 2u : lk == RT_KIND_MEDIUM ? 3u : 0u;
            new_oct[slot - base] = (uint8_t)((r.dir.x < 0.0 ? 1u : 0u) | (r.dir.y < 0.0 ? 2u : 0u) | (r.dir.z < 0.0 ? 4u : 0u) | (org << 3));
        }
    }

    SP_MARK(5);                                                      // 5: queueing, stores of the bounce
    // Second sweep: the next sample of the item, or the next item (main.rs:140-152), for every slot that asked.
    // (The barrier also makes the first sweep's pixel sums visible to whichever thread finishes the item here.)
    __syncthreads();
    const uint32_t n_want = n_fresh;
    // One sample per item: every slot on the queue takes a new item, so the segment claims them with ONE atomic instead
    // of one per wave and sweep turn (which slot gets which item changes nothing, §5 of DESIGN.md).
    __shared__ unsigned long long seg_items;
    __shared__ uint32_t seg_take;        // (ring mode) how many of the n_want items the segment really got
    __shared__ uint32_t seg_more;        // (ring mode) 1: work items remain beyond the ring's limit — the slots left without one ask again
    const bool batch = single;
    if (batch) {
        if (tid == 0) {
            if (!RING) {
                seg_items = n_want ? atomicAdd(a.work_counter, (unsigned long long)n_want) : 0ull;
            } else {
                // Never USE an item beyond *claim_limit: sample c + R of a pixel shares its plane with sample c, which the host must
                // have added to the output first (it raises the limit behind the planes it consumes, between passes).
                // One add, like the plain path (a compare-and-swap loop on one word shared by thousands of segments fails most
                // of its tries: measured, a quarter of the frame); what lies beyond the limit is handed back. While a segment's
                // surplus is out, other segments may see the counter too high and take nothing this pass — never too much: an
                // item is only ever used by the segment whose add returned it, and only below the limit.
                const unsigned long long lim = *a.claim_limit;
                const unsigned long long old = n_want ? atomicAdd(a.work_counter, (unsigned long long)n_want) : 0ull;
                const uint32_t take = old < lim ? (uint32_t)((unsigned long long)n_want < lim - old ? (unsigned long long)n_want : lim - old) : 0u;
                const bool bound = lim < a.n_items;                 // the ring, not the end of the work, is what stops claims
                if (bound && take < n_want) atomicAdd(a.work_counter, 0ull - (unsigned long long)(n_want - take));      // (minus: modulo 2^64)
                seg_items = old; seg_take = take;
                seg_more = bound ? 1u : 0u;                          // (at lim == n_items nothing is handed back: beyond it the work IS done)
            }
        }
        __syncthreads();
    }
    for (uint32_t j0 = 0; j0 < n_want; j0 += kBlock) {
        const uint32_t j = j0 + tid;
        const bool on = j < n_want;
        const uint32_t e = on ? (uint32_t)fresh_q[j] : 0u;
        const uint32_t slot = base + (e & 0x7FFFu);                   // (bit 15 is the flag; a segment holds at most 32768 slots)
        bool alive = false;
        bool starved = false;        // (ring mode) wanted a work item, found the ring full: asks again next pass
        Ray r;
        Rng rng;
        uint32_t depth = 0;
        SlotState stt{};
        if (on) {
            // (one-sample items: the item is always finished, nothing of the old state is needed)
            bool have_item = (e & 0x8000u) != 0;
            if (have_item) stt = load_state(pool, slot);
            uint32_t smp = have_item ? stt.smp : 0u, smp_end = have_item ? stt.smp_end : 0u;
            for (int guard = 0; guard < 1 << 20; guard++) {           // loops only through degenerate items (spp or depth 0)
                bool need = !have_item || smp == smp_end;
                if (need && have_item) {                              // section_pixel_color.push(pixel_color), main.rs:152
                    if (!single) {
                        double *o = a.partial + stt.item * 3;
                        const double *ps = pool.pixel_sum + (uint64_t)slot * 4;
                        o[0] = ps[0]; o[1] = ps[1]; o[2] = ps[2];
                    }
                    have_item = false;
                }
                unsigned long long m = wballot(need);
                if (m) {
                    int leader = __ffsll((long long)m) - 1;
                    unsigned long long wbase = 0;
                    if (!batch) {
                        if ((int)lane == leader) wbase = atomicAdd(a.work_counter, (unsigned long long)__popcll(m));
                        wbase = __shfl(wbase, leader);
                    }
                    if (need) {
                        unsigned long long item = batch ? seg_items + j : wbase + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
                        if (RING && j >= seg_take) {                    // the ring (or the work) ran out before this slot's turn
                            item = a.n_items;
                            starved = seg_more != 0u;
                        }
                        if (item < a.n_items) {
                            uint64_t pix_slot, yi;
                            uint32_t chunk_id, px;
                            if (RING) {                                 // group-major: item = (group * n_pixels + pixel) * ring_group + sample in the group
                                if (small_job) {
                                    const uint32_t q32 = (uint32_t)item / a.ring_group, np32 = (uint32_t)a.n_pixels;     // group * n_pixels + pixel
                                    const uint32_t g32 = q32 / np32, ps32 = q32 - g32 * np32, y32 = ps32 / a.width;
                                    chunk_id = g32 * a.ring_group + ((uint32_t)item - q32 * a.ring_group);
                                    px = ps32 - y32 * a.width;
                                    pix_slot = ps32; yi = y32;
                                } else {
                                    const uint64_t q = item / a.ring_group, g = q / a.n_pixels;
                                    chunk_id = (uint32_t)(g * a.ring_group + (item - q * a.ring_group));
                                    pix_slot = q - g * a.n_pixels;
                                    yi = pix_slot / a.width;
                                    px = (uint32_t)(pix_slot - yi * a.width);
                                }
                            } else if (small_job) {                     // (32-bit divisions where everything fits: the usual case)
                                const uint32_t ps32 = (uint32_t)item / a.n_chunks, y32 = ps32 / a.width;
                                chunk_id = (uint32_t)item - ps32 * a.n_chunks;
                                px = ps32 - y32 * a.width;
                                pix_slot = ps32; yi = y32;
                            } else {
                                pix_slot = item / a.n_chunks;
                                chunk_id = (uint32_t)(item - pix_slot * a.n_chunks);
                                yi = pix_slot / a.width;
                                px = (uint32_t)(pix_slot - yi * a.width);
                            }
                            smp = chunk_id * a.chunk;
                            smp_end = smp + a.chunk < a.spp ? smp + a.chunk : a.spp;
                            stt.item = (uint64_t)(RING ? chunk_id % a.ring : chunk_id) * a.n_pixels + pix_slot;     // (kept as the item's place in the partial sums: ring mode, plane = sample mod R)
                            if constexpr (SRC == kSrcRays) {            // (width 1: pix_slot is the ray; n_rays < 2^32, checked by the host)
                                stt.px = (uint32_t)pix_slot; stt.py = 0; stt.frame = 0;
                            } else if constexpr (SRC == kSrcPixels) {   // id = frame * (width * height) + py * width + px, range-checked by the host
                                const uint64_t id = a.pixel_ids[pix_slot];
                                if ((uint64_t)a.width * ((uint64_t)a.height * a.n_frames) <= 0xFFFFFFFFull) {     // (every id fits 32 bits)
                                    const uint32_t i32 = (uint32_t)id, np32 = a.width * a.height;
                                    const uint32_t f32 = i32 / np32, r32 = i32 - f32 * np32, y32 = r32 / a.width;
                                    stt.px = r32 - y32 * a.width; stt.py = y32; stt.frame = f32;
                                } else {
                                    const uint64_t np = (uint64_t)a.width * a.height, f = id / np, rem = id - f * np, y = rem / a.width;
                                    stt.px = (uint32_t)(rem - y * a.width); stt.py = (uint32_t)y; stt.frame = (uint32_t)f;
                                }
                            } else {
                                uint32_t g = a.row_ids[yi];
                                uint32_t frame = g / a.height;
                                uint32_t py = g - frame * a.height;
                                stt.px = px; stt.py = py; stt.frame = frame;
                            }
                            if (!single) {
                                double2 *ps = reinterpret_cast<double2 *>(pool.pixel_sum + (uint64_t)slot * 4);
                                ps[0] = make_double2(0.0, 0.0);
                                ps[1] = make_double2(0.0, 0.0);
                            }
                            have_item = true;
                        }
                    }
                }
                if (!have_item) break;                                // no work left: the slot goes idle
                if (smp == smp_end) continue;                         // empty chunk (spp == 0): store zeros next turn
                if constexpr (SRC == kSrcRays) {                      // the caller's ray record, the engine's own layout: four 16-byte loads
                    const double2 *q = reinterpret_cast<const double2 *>(a.rays + stt.px);
                    const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
                    r = Ray(Vec3(q0.x, q0.y, q1.x), Vec3(q1.y, q2.x, q2.y), q3.x);
                    rng = Rng(rtm::path_key(rtm::d2u(q3.y), 0u, 0ull, smp));
                    depth = a.max_depth;
                    smp++;
                    cnt.path();
                } else {
                    uint32_t px = stt.px, py = stt.py, frame = stt.frame;
                    uint64_t pixel = (uint64_t)py * a.width + px;
                    rng = Rng(rtm::path_key(a.seed, frame, pixel, smp));  // main.rs:144-149
                    double rand_u = rng.gen_f64();
                    double rand_v = rng.gen_f64();
                    double u = ((double)px + rand_u) / (double)(a.width - 1);
                    double v = ((double)py + rand_v) / (double)(a.height - 1);
                    r = get_ray(a.cam, u, v, rng);
                    depth = a.max_depth;
                    smp++;
                    cnt.path();
                    cnt.draws(rng.draws);                             // words drawn while aiming the camera ray
                    rng.draws = 0;
                }
                if (depth == 0) continue;                             // MAX_DEPTH == 0: black at once
                alive = true;
                break;
            }
            stt.smp = smp;
            stt.smp_end = smp_end;
            if (alive) {
                cnt.ray();                                            // world.hit(r, 0.001, f64::MAX), main.rs:243
                pv.store_ray(slot, r, rng.s);
                stt.depth = depth;                                    // (a fresh tape: nothing tainted)
                store_state(pool, slot, stt, true);
                new_kind[slot - base] = (uint8_t)SK_TRACE;            // (a camera ray goes with the short ones: list class 0)
                new_oct[slot - base] = (uint8_t)((r.dir.x < 0.0 ? 1u : 0u) | (r.dir.y < 0.0 ? 2u : 0u) | (r.dir.z < 0.0 ? 4u : 0u));
                if (RING) { const unsigned long long grp = (smp - 1u) / a.ring_group; my_oldest = grp < my_oldest ? grp : my_oldest; }
            } else if (RING && starved) {
                new_kind[slot - base] = (uint8_t)SK_FRESH;            // (not a ray: listed behind the rays, see below)
            }
        }
    }
    SP_MARK(6);                                                      // 6: second sweep (new paths)
    // Paths handed to the trace pass (the host stops when the whole pool reports none).
    for (uint32_t k = tid; k < kListBins; k += kBlock) bins[k] = 0;
    __shared__ uint32_t list_total, n_starved_out;
    __shared__ unsigned long long seg_oldest;
    if (RING && tid == 0) { n_starved_out = 0; seg_oldest = ~0ull; }
    __syncthreads();
    // The segment's ray list, longest expected traversal first (counting sort, 16 classes): the stragglers of
    // the trace pass then start early instead of keeping a few lanes busy after the list has run dry.
    uint32_t my_key[S / kBlock];
    uint32_t my_starved[RING ? S / kBlock : 1];                        // (ring mode) place among the segment's starved slots, or none
    if (RING) {                                                        // the oldest work item in flight, over the segment
        unsigned long long v = my_oldest;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o < v ? o : v; }
        if (lane == 0 && v != ~0ull) atomicMin(&seg_oldest, v);
    }
#pragma unroll
    for (int i = 0; i < S / kBlock; i++) {
        uint32_t e = new_kind[i * kBlock + tid];
        uint32_t key = kListBins;                                      // carries no ray
        if (RING) my_starved[i] = e == (uint32_t)SK_FRESH ? atomicAdd(&n_starved_out, 1u) : 0xFFFFFFFFu;
        // (second key: rays that point into the same octant meet the boxes in a similar pattern, and the lanes of a
        // wave draw neighbouring list entries)
        // (new_oct: octant | origin class << 3; key: origin and octant first, expected length within. Bits 6-7 of new_oct held a
        // fourth key once and are always 0: the key still folds them in, which keeps the compiled shade pass as it was measured.)
        if ((e & 0xFu) == SK_TRACE) {
            const uint32_t o8 = new_oct[i * kBlock + tid];
            key = ((o8 >> 6) * (8u * kOriginClasses) + (o8 & 63u)) * 16u + (15u - (e >> 4));
            atomicAdd(&bins[key], 1u);
        }
        my_key[i] = key;
    }
    __syncthreads();
    // Exclusive prefix sums of the bins, in place: every thread takes kPer consecutive bins; scan over the wave by
    // shuffles, over the four waves through LDS.
    constexpr uint32_t kPer = kListBins > (uint32_t)kBlock ? kListBins / (uint32_t)kBlock : 1u;
    static_assert(kPer * (uint32_t)kBlock >= kListBins, "bins per thread");
    __shared__ uint32_t wave_tot[kBlock / 64];
    {
        uint32_t v[kPer], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) { const uint32_t k = tid * kPer + j; v[j] = k < kListBins ? bins[k] : 0u; sum += v[j]; }
        uint32_t inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)inc, d); if ((int)lane >= d) inc += t; }
        if (lane == 63) wave_tot[tid >> 6] = inc;
        __syncthreads();
        uint32_t excl = inc - sum;
        for (uint32_t wv = 0; wv < (tid >> 6); wv++) excl += wave_tot[wv];
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) { const uint32_t k = tid * kPer + j; if (k < kListBins) bins[k] = excl; excl += v[j]; }
    }
    if (tid == 0) {
        uint32_t acc = 0;
        for (int wv = 0; wv < kBlock / 64; wv++) acc += wave_tot[wv];
        pool.list_n[blockIdx.x] = acc;
        // Rays handed on by this pass (the host stops a group when a pass reports none). Two counters take
        // turns, so each pass can clear the one the next pass will add to.
        uint32_t going = acc;
        if (RING) {                                                    // (slots waiting for the ring keep the frame going too)
            list_total = acc;
            pool.starved_n[blockIdx.x] = n_starved_out;
            going += n_starved_out;
            if (seg_oldest != ~0ull) atomicMin(&pool.oldest[parity], seg_oldest);
            if (blockIdx.x == 0) pool.oldest[parity ^ 1u] = ~0ull;
        }
        if (going) atomicAdd(&pool.n_active[parity], going);
        if (acc) atomicMax(&pool.max_list[parity], acc);
        if (blockIdx.x == 0) { pool.n_active[parity ^ 1u] = 0; pool.max_list[parity ^ 1u] = 0; *pool.next_chunk = 0; }
    }
    __syncthreads();
    if (RING) {
#pragma unroll
        for (int i = 0; i < S / kBlock; i++)
            if (my_starved[i] != 0xFFFFFFFFu) {
                const uint32_t pos = base + list_total + my_starved[i];
                pool.list[pos] = (uint16_t)((uint32_t)(i * kBlock) + tid);
                pool.kind[pos] = (uint8_t)SK_FRESH;
            }
    }
#pragma unroll
    for (int i = 0; i < S / kBlock; i++)
        if (my_key[i] < kListBins) {
            const uint32_t pos = base + atomicAdd(&bins[my_key[i]], 1u);
            pool.list[pos] = (uint16_t)((uint32_t)(i * kBlock) + tid);
            pool.kind[pos] = (uint8_t)SK_TRACE;                       // until the trace pass has been there
        }
    if (STATS) cnt.flush_wave(a.stats);
    SP_MARK(7);                                                      // 7: kinds written back, ray list built
    SP_FLUSH();
}

// One instance per (STATS, RING, SRC): which one a launch takes.
using ShadeKernel = void (*)(SceneDev, const RenderArgs *, WfPool, uint32_t);
template <bool STATS>
static ShadeKernel shade_kernel(const WfLaunch &w) {
    if (w.rays) return w.ring ? wf_shade<STATS, true, kSrcRays> : wf_shade<STATS, false, kSrcRays>;
    if (w.pixels) return w.ring ? wf_shade<STATS, true, kSrcPixels> : wf_shade<STATS, false, kSrcPixels>;
    return w.ring ? wf_shade<STATS, true> : wf_shade<STATS, false>;
}
void launch_shade(const WfLaunch &w, bool stats, uint32_t parity) {
    hipLaunchKernelGGL(stats ? shade_kernel<true>(w) : shade_kernel<false>(w), dim3(w.blocks), dim3(kBlock), 0, w.stream, w.scene, w.d_args,
                       w.pool, parity);
}

// Diagnostic build: what the section clock of the shade kernel added up to over the render.
#ifdef RT2022_SHADE_PROBE
void print_shade_probe(const WfPool &pool) {
    unsigned long long h[10];
    if (hipMemcpy(h, pool.dbg + 64, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
        double tot = 0; for (int i = 0; i < 8; i++) tot += (double)h[i];
        fprintf(stderr, "shade probe (ticks of wave 0, all workgroups and passes; share):");
        for (int i = 0; i < 8; i++) fprintf(stderr, " [%d] %.3f", i, tot > 0 ? (double)h[i] / tot : 0.0);
        fprintf(stderr, "  total %.3e ticks\n", tot);
    }
    (void)hipMemset(pool.dbg + 64, 0, 10 * sizeof(unsigned long long));
}
#endif

} // namespace rt2022
