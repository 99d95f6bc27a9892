// pt_features.hip — first-hit feature buffers of a render's view (rt_features*, include/rt2022.h).
//
// For every pixel of the row list and every sample, the camera ray the render aims (the fresh-path code of wf_shade: the
// same key, sub-pixel jitter, lens sample and shutter time) and `world.hit(r, t_min, f64::MAX)` on it with the SAME RNG
// stream continuing into the hit; then the winner's albedo, normal and depth, summed per pixel in sample order. No bounce,
// no light sampling: the megakernel's traversal (pt_traverse.hpp) on its own, in the query kernel's shell (pt_traverse.hpp
// too: persistent wave64 grid, one-atomic-per-wave claim, start of a ray, scheduler tuning, instance by stack need —
// pt_query.hip describes it). What is this kernel's own:
//   - the work item is ONE PIXEL: a lane runs its pixel's samples in order and only then claims the next pixel;
//   - the lane owns its pixel's 64-byte record: each sample is added into it as four 16-byte load / add / store pieces,
//     the first sample stores (0 + f_0), so there are no atomics, no memset pass, and the order is the sample order;
//   - the world-frame ray is not kept in registers: the few steps that need it — leaving a mover, the winner's record —
//     aim it again from (row, px, sample), which is cheap beside a traversal (q_world's trick, pt_query.hip);
//   - the waves per SIMD its instances are built for (feat_waves below);
//   - the scheduler loop, written out here as in every kernel (pt_traverse.hpp says why) — and with it the LDS node
//     prefix and the lane's state before the loop, pt_query's line for line: through trav_cache_nodes / trav_lane_clear
//     the 1024-thread instance spills differently, and nobody has measured that.
// Two sources of work items (SRC, the way wf_shade has one): the rows of a render's row list (rt_features*), or a list of
// (frame, pixel) ids, rt_render_pixels' (rt_features_pixels*). With a list the work item is ONE ENTRY, the lane's record is
// out + entry, and f_camera decodes pixel_ids[entry] into frame, py and px where the row source reads row_ids[row]; all else
// — traversal, f_albedo, the record's four pieces, the claim, the scheduler loop — is the same code.
// A third source, the caller's rays (kFeatRays, rt_features_rays*): the work item is ONE RAY, the lane's record is out + entry, and
// f_camera loads rays[entry] and keys the stream path_key(rng_state, 0, 0, sample) as rt_radiance does, drawing nothing; the world
// ray is still not kept — f_world reads the 64-byte record again (L2-hot) where the other sources aim again.
// RT_FLAG_SURFACES (SURF, instances of their own): a ConstantMedium answers None at once — its leaf is popped where the
// medium arm would enter trav_medium, so no boundary is queried, no word drawn and nothing counted; an object that is also
// some medium's boundary is still reached through its own reference. Instances and not a uniform switch in FeatureArgs: with
// the switch five of the sixteen unflagged instances spilled more (up to +8 bytes of scratch per lane); as instances, those
// are compiled from the code they had and keep every register (profiles/features_surfaces_kernel_resources.txt).
// RT_FLAG_SPECULAR: a kernel of its own, pt_features_specular.hip, around the same pieces (pt_features.hpp); nothing of it is
// compiled into the instances here.
// One launcher serves the six calls (launch_features, at the end; the host side names the source as a number, pt_device.h): the
// switch from `src` to SRC is written once here and once in pt_features_specular.hip, which takes the flagged calls.
// One lane per pixel means a few-pixel x huge-spp job balances poorly; the intended use is a whole frame at modest spp.
// All arithmetic is f64 through rt_math.h with -ffp-contract=off, so every sum is the CPU oracle's composition bit for bit.
#include "pt_features.hpp"

namespace rt2022 {

namespace {

// (FLane, f_camera, f_albedo, f_add and f_take: pt_features.hpp, shared with the RT_FLAG_SPECULAR kernel)
template <int SRC>
RT_DEV Ray f_world(const FeatureArgs &a, const FLane &L) {
    Rng unused;
    return f_camera<SRC>(a, L.row, L.px, L.smp, unused);
}

// The finished sample's features, added into the lane's own record: {a.x, a.y} {a.z, n.x} {n.y, n.z} {depth, hits}.
template <int SRC>
RT_DEV void f_accumulate(const SceneDev &s, const FeatureArgs &a, const FLane &L) {
    Vec3 alb = ld3(a.background), n(0.0, 0.0, 0.0);
    double depth = 0.0, hits = 0.0;
    if (L.flags & kFound) {
        HitRec rec;
        winner_record(s, f_world<SRC>(a, L), L.win, rec, true);
        alb = f_albedo(s, rec);
        n = rec.normal; depth = rec.t; hits = 1.0;
    }
    f_add<SRC>(a, L, alb, n, depth, hits);
}

// Aim sample L.smp of the lane's pixel and start its traversal at the root (`have` false: nothing left, the lane idles).
template <int SRC>
RT_DEV void f_aim(const SceneDev &s, const FeatureArgs &a, FLane &L, bool have) {
    Rng rng;
    Ray r(Vec3(0.0, 0.0, 0.0), Vec3(0.0, 0.0, 0.0), 0.0);
    if (have) r = f_camera<SRC>(a, L.row, L.px, L.smp, rng);
    trav_begin(s, L, have, XRay{r.orig, r.dir}, r.tm, a.t_min, rtm::F64_MAX, rng);   // (rng's draws so far are the camera's: the hit's come on top)
    if (have) L.flags = kFHasPixel;
}

// Done: add the finished sample into the pixel's record, then aim the pixel's next sample — or take the next pixel (one
// atomic per wave for every lane that refills).
template <int SRC, bool STATS>
RT_DEV void f_done(const SceneDev &s, const FeatureArgs &a, FLane &L, unsigned lane, Counters<STATS> &cnt) {
    bool refill = true;
    if (L.flags & kFHasPixel) {
        f_accumulate<SRC>(s, a, L);
        cnt.draws(L.rng.draws);
        L.smp++;
        refill = L.smp >= a.spp;
    }
    const unsigned long long m = __ballot(refill);
    bool have = true;
    if (refill) {
        const unsigned long long i = wave_claim(a.counter, m, lane);
        have = f_take<SRC>(a, L, i);
    }
    f_aim<SRC>(s, a, L, have);
}

} // namespace

// Waves per SIMD the instances are built for. The 1024-thread LDS-prefix instance has no choice: one workgroup is 16 waves
// per CU = 4 per SIMD (128 VGPRs; its done arm spills into scratch: profiles/features_kernel_resources.txt). The 256-thread
// instances take 3 (168 VGPRs) where pt_query takes 4 — measured at 4 / 3 / 2 on the 800x800 default views at 4 spp: C5's
// mesh 169 / 333 / 291 Mrays/s, 1e5 spheres 143 / 299 / 278 (profiles/features_ab_occupancy.log).
constexpr int feat_waves(int stack, int wg) { return wg > 256 ? 4 : stack > 32 ? 2 : 3; }
// STACK: traversal stack entries; WG: threads per workgroup; CACHE: node records kept in LDS (0: none); STATS: counter instance;
// SRC: kFeatRows, kFeatPixels or kFeatRays; SURF: RT_FLAG_SURFACES (both defaulted: the earlier instances keep their names).
template <int STACK, int WG, int CACHE, bool STATS, int SRC = kFeatRows, bool SURF = false>
__global__ void __launch_bounds__(WG, feat_waves(STACK, WG)) pt_features(const SceneDev s, const FeatureArgs a) {
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

    FLane L;
    L.tm = 0.0;
    trav_set_cur(L, XRay{Vec3(0.0, 0.0, 0.0), Vec3(0.0, 0.0, 0.0)});
    L.t_min = L.t_lo = L.closest = L.sub_closest = L.med_t1 = 0.0;
    L.med_ref = 0;
    L.ctx.c0 = L.ctx.c1 = L.ctx.c2 = L.ctx.c3 = 0; L.ctx.n = 0;
    L.win.t = 0.0; L.win.leaf = 0; L.win.face = 0; L.win.chain = L.ctx;
    L.row = 0; L.px = 0; L.smp = 0; L.sp = 0; L.top = REF_EMPTY; L.op = OP_SHADE; L.flags = 0;

    const auto world = [&] { const Ray w = f_world<SRC>(a, L); return XRay{w.orig, w.dir}; };
    for (;;) {
        // Fast path: keep stepping nodes while enough lanes want to.
        for (;;) {
            const bool isn = L.op == OP_NODE;
            if (__popcll(__ballot(isn)) < kQueryNodeQuorum) break;
            if (isn) trav_node<false, STACK, WG, CACHE, STATS>(s, node_lds, n_cached, L, st, cnt);
        }
        // Vote: the label with the largest lanes x weight (ties -> lowest id).
        int best = -1, best_n = 0;
#pragma unroll
        for (int o = 0; o < (int)OP_COUNT; o++) {
            const int n = __popcll(__ballot(L.op == (uint32_t)o)) * (int)((kQueryVoteWeights >> (4 * o)) & 0xFu);
            if (n > best_n) { best_n = n; best = o; }
        }
        if (best < 0) break;                               // every lane idle: no pixels left
        if (L.op == (uint32_t)best) {
            switch (best) {
                case OP_NODE: trav_node<false, STACK, WG, CACHE, STATS>(s, node_lds, n_cached, L, st, cnt); break;
                case OP_SPHERE: trav_sphere<false>(s, L, st, cnt); break;
                case OP_RECT: trav_rect<false>(s, L, st, cnt); break;
                case OP_BOX: trav_box<false>(s, L, st, cnt); break;
                case OP_MEDIUM:                            // (SURF: the leaf is popped; no sentinel is ever pushed then)
                    if constexpr (SURF) trav_next<false>(L, st);
                    else trav_medium<false>(s, L, st, cnt);
                    break;
                case OP_MISC: trav_misc<false>(s, L, st, cnt); break;
                case OP_CTX: trav_ctx<false>(s, L, st, cnt, world); break;
                default: f_done<SRC, STATS>(s, a, L, lane, cnt); break;
            }
        }
    }
    if (STATS) cnt.flush_wave(a.stats);
}

namespace {

// The instance of a call: by the scene's stack need, then counters and RT_FLAG_SURFACES.
template <int SRC>
hipError_t launch_features_src(const SceneDev &scene, const FeatureArgs &args, uint32_t stack_need, bool counters, bool surfaces, hipStream_t stream) {
    if (args.n_pixels == 0 || args.spp == 0) return hipSuccess;
    return trav_dispatch(stack_need, [&](auto shape) {
        using S = decltype(shape);
        void (*const kernel)(SceneDev, FeatureArgs) =
            surfaces ? (counters ? pt_features<S::stack, S::wg, S::cache, true, SRC, true> : pt_features<S::stack, S::wg, S::cache, false, SRC, true>)
                     : (counters ? pt_features<S::stack, S::wg, S::cache, true, SRC> : pt_features<S::stack, S::wg, S::cache, false, SRC>);
        return launch_persistent(kernel, S::wg, args.n_pixels, scene, args, stream);
    });
}

} // namespace

hipError_t launch_features(const SceneDev &scene, const FeatureArgs &args, uint32_t stack_need, int src, bool counters, bool surfaces,
                           bool specular, hipStream_t stream) {
    if (specular) return launch_features_specular(scene, args, stack_need, src, counters, surfaces, stream);
    switch (src) {
        case kFeatRows: return launch_features_src<kFeatRows>(scene, args, stack_need, counters, surfaces, stream);
        case kFeatPixels: return launch_features_src<kFeatPixels>(scene, args, stack_need, counters, surfaces, stream);
        case kFeatRays: return launch_features_src<kFeatRays>(scene, args, stack_need, counters, surfaces, stream);
        default: return hipErrorInvalidValue;
    }
}

} // namespace rt2022
