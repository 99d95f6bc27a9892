// pt_features_specular.hip — RT_FLAG_SPECULAR on the six feature calls (include/rt2022.h): the records of the first
// non-specular vertex of the sample's own path, behind glass and mirrors.
//
// The kernel is pt_features' shell (pt_features.hpp, pt_traverse.hpp: persistent wave64 grid, one lane per pixel, the lane owns
// its record, one-atomic-per-wave claim, the voted scheduler) with another done arm. The lane draws from the render's own RNG
// stream, so it follows exactly the path the render's sample took: at a Dielectric or a fuzz-0 Metal it takes the winner's
// record, scatters as the render does (pt_kernel.hip's op_shade, material/mod.rs:85-147) and begins world.hit on the new
// segment with its rng continuing — no accumulate, the sample stays in flight; at any other vertex, at the ninth vertex
// (RT_FEATURE_SPECULAR_BOUNCES followed) or on a miss it multiplies the followed metals' albedos onto the terminal colour
// innermost first, adds the sample into the record and goes on to the next sample or claim as pt_features does.
//
// What the lane keeps beyond pt_features' state, all of it in registers:
//   - the world-frame ray of the segment in flight (7 doubles): from the second segment on it cannot be aimed again from
//     (row, px, sample), and leaving a mover and the winner's record need it. The first segment's is kept the same way, so
//     there is one code path;
//   - rec_0.t (depth is primary visibility) and the previous vertex's normal (a miss behind a specular vertex reports it);
//   - the material indices of the metals followed, at most 8, written and read with constant indices only (an indexed
//     private array would live in scratch); a Dielectric's factor is exactly 1 and is not kept.
// Where that state lives decides the shapes. It is some 30 registers on top of instances that already sit at the 168 VGPRs of
// three waves per SIMD, and the 1024-thread LDS-prefix shape (128 VGPRs, 64 KiB of stacks + 95.2 KiB of node prefix: under
// 1 KiB of LDS left) has room for it neither in registers nor in LDS. So: every instance here is a 256-thread one built for
// TWO waves per SIMD (256 VGPRs: no VGPR spills, no scratch — profiles/features_specular_kernel_resources.txt), and flagged
// calls on tiny-stack scenes take the kStackSmall shape. Chosen by the resource table, then measured: the same instances
// built for three waves (168 VGPRs, the cold state spilled) are 18-30 % slower on the 800 x 800 views at 4 spp — headline
// 3.2 against 2.7 ms, C2 5.3 against 4.1, 1e5 spheres 24 against 19.6 (profiles/features_specular_ab_occupancy.log, one GPU
// call, alternating). Beside the plain call: x 1.39 on C2 at 1.41 segments per sample, x 0.94 on the headline frame at 1.11,
// x 2.4 on 1e5 spheres at 1.49 (profiles/features_bench.log, tools/features_bench.py --specular). The state in LDS was never
// built, so whether that would be faster nobody has measured.
// RT_FLAG_SURFACES with it (SURF): a medium leaf is popped on every segment, as in pt_features.
// All arithmetic is f64 through rt_math.h with -ffp-contract=off: every record is the oracle composition of
// tests/specular_ref.py bit for bit.
#include "pt_features.hpp"

namespace rt2022 {

namespace {

struct SLane : FLane {
    Vec3 wo, wd;           // the world-frame ray of the segment in flight
    double wtm;
    double depth0;         // rec_0.t
    Vec3 n_prev;           // rec_{k-1}.normal
    uint32_t mats[RT_FEATURE_SPECULAR_BOUNCES];    // materials of the metal vertices followed, in path order
    uint32_t k, nm;        // vertices followed so far; metals among them
};

// Done. A lane with a sample in flight either follows its vertex (new segment, same sample) or finishes the sample; a lane
// that finished its pixel's last sample, or has none, claims the next pixel (one atomic per wave for all that do).
template <int SRC, bool STATS>
RT_DEV void s_done(const SceneDev &s, const FeatureArgs &a, SLane &L, unsigned lane, Counters<STATS> &cnt) {
    bool refill = true, follow = false;
    if (L.flags & kFHasPixel) {
        Vec3 c = ld3(a.background), n(0.0, 0.0, 0.0);
        double depth = 0.0, hits = 0.0;
        if (L.flags & kFound) {
            HitRec rec;
            winner_record(s, Ray(L.wo, L.wd, L.wtm), L.win, rec, true);
            const uint32_t mi = rec.mat & kMatIndexMask;
            const rt_material &mat = s.materials[mi];
            const uint32_t mk = mat.kind;
            if (L.k == 0) L.depth0 = rec.t;
            const bool metal = mk == RT_MAT_METAL && mat.param == 0.0;
            follow = L.k < (uint32_t)RT_FEATURE_SPECULAR_BOUNCES && (mk == RT_MAT_DIELECTRIC || metal);
            if (follow) {
                Vec3 dir;
                if (metal) {                                       // mod.rs:85-96 (the sampler is drawn although fuzz is 0)
                    const Vec3 reflected = rtm::reflect(rtm::to_unit(L.wd), rec.normal);
                    dir = reflected + random_in_unit_sphere(L.rng) * mat.param;
                    L.wtm = 0.0;                                   // time = 0., mod.rs:91
#pragma unroll
                    for (int i = 0; i < RT_FEATURE_SPECULAR_BOUNCES; i++) L.mats[i] = (uint32_t)i == L.nm ? mi : L.mats[i];
                    L.nm++;
                } else {                                           // mod.rs:120-147
                    const double refraction_ratio = rec.front_face ? 1.0 / mat.param : mat.param;
                    const Vec3 unit_direction = rtm::to_unit(L.wd);
                    const double cos_theta = rtm::fmin_(rtm::dot(-unit_direction, rec.normal), 1.0);
                    const double sin_theta = rtm::sqrt_(1.0 - cos_theta * cos_theta);
                    const bool cannot_refract = refraction_ratio * sin_theta > 1.0;
                    const double random_double = L.rng.gen_range(0.0, 1.0);
                    dir = (cannot_refract || reflectance(cos_theta, refraction_ratio) > random_double)
                              ? rtm::reflect(unit_direction, rec.normal)
                              : rtm::refract(unit_direction, rec.normal, refraction_ratio);
                }
                L.wo = rec.p; L.wd = dir;
                L.n_prev = rec.normal;
                L.k++;
            } else {
                c = f_albedo(s, rec);
                n = rec.normal;
            }
            depth = L.depth0; hits = 1.0;
        } else if (L.k > 0) {                                      // a miss behind a specular vertex: the background, seen in it
            n = L.n_prev; depth = L.depth0; hits = 1.0;
        }
        refill = false;
        if (!follow) {
            // a_0 * (a_1 * ( ... * (a_{j-1} * c))): ray_color's order, innermost first
#pragma unroll
            for (int i = RT_FEATURE_SPECULAR_BOUNCES - 1; i >= 0; i--)
                if ((uint32_t)i < L.nm) c = ld3(s.materials[L.mats[i]].albedo) * c;
            f_add<SRC>(a, L, c, n, depth, hits);
            cnt.draws(L.rng.draws);
            L.smp++;
            refill = L.smp >= a.spp;
        }
    }
    const unsigned long long m = __ballot(refill);
    bool have = true;
    if (refill) {
        const unsigned long long i = wave_claim(a.counter, m, lane);
        have = f_take<SRC>(a, L, i);
    }
    Rng rng = L.rng;
    if (!follow) {                                                 // a fresh sample: aim it (nothing left: the lane idles)
        Ray r(Vec3(0.0, 0.0, 0.0), Vec3(0.0, 0.0, 0.0), 0.0);
        rng = Rng();
        if (have) r = f_camera<SRC>(a, L.row, L.px, L.smp, rng);
        L.wo = r.orig; L.wd = r.dir; L.wtm = r.tm;
        L.k = 0; L.nm = 0;
    }
    trav_begin(s, L, have, XRay{L.wo, L.wd}, L.wtm, a.t_min, rtm::F64_MAX, rng);   // (rng's draws so far stay counted: the hit's come on top)
    if (have) { L.flags = kFHasPixel; cnt.ray(); }
}

} // namespace

// STACK: traversal stack entries (256-thread workgroups, no node prefix: see above); STATS: counter instance; SRC: kFeatRows,
// kFeatPixels or kFeatRays (the caller's ray is the first segment, kept in L.wo / L.wd / L.wtm like every other); SURF:
// RT_FLAG_SURFACES as well. Two waves per SIMD: the register budget that keeps the lane's state unspilled.
template <int STACK, bool STATS, int SRC, bool SURF>
__global__ void __launch_bounds__(kBlock, 2) pt_features_specular(const SceneDev s, const FeatureArgs a) {
    constexpr int WG = kBlock;
    __shared__ uint32_t stack_lds[STACK * WG];
    TravStack<STACK, WG> st{stack_lds + threadIdx.x};
    const unsigned lane = threadIdx.x & 63u;
    Counters<STATS> cnt;

    SLane L;
    trav_lane_clear(L);
    L.row = 0; L.px = 0; L.smp = 0;
    L.wo = L.wd = L.n_prev = Vec3(0.0, 0.0, 0.0);
    L.wtm = L.depth0 = 0.0;
#pragma unroll
    for (int i = 0; i < RT_FEATURE_SPECULAR_BOUNCES; i++) L.mats[i] = 0;
    L.k = 0; L.nm = 0;

    const auto world = [&] { return XRay{L.wo, L.wd}; };
    for (;;) {
        // Fast path: keep stepping nodes while enough lanes want to.
        for (;;) {
            const bool isn = L.op == OP_NODE;
            if (__popcll(__ballot(isn)) < kQueryNodeQuorum) break;
            if (isn) trav_node<false, STACK, WG, 0, STATS>(s, nullptr, 0u, L, st, cnt);
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
                case OP_NODE: trav_node<false, STACK, WG, 0, STATS>(s, nullptr, 0u, L, st, cnt); break;
                case OP_SPHERE: trav_sphere<false>(s, L, st, cnt); break;
                case OP_RECT: trav_rect<false>(s, L, st, cnt); break;
                case OP_BOX: trav_box<false>(s, L, st, cnt); break;
                case OP_MEDIUM:                            // (SURF: the leaf is popped; no sentinel is ever pushed then)
                    if constexpr (SURF) trav_next<false>(L, st);
                    else trav_medium<false>(s, L, st, cnt);
                    break;
                case OP_MISC: trav_misc<false>(s, L, st, cnt); break;
                case OP_CTX: trav_ctx<false>(s, L, st, cnt, world); break;
                default: s_done<SRC, STATS>(s, a, L, lane, cnt); break;
            }
        }
    }
    if (STATS) cnt.flush_wave(a.stats);
}

namespace {

template <int STACK, int SRC>
hipError_t launch_specular_shape(const SceneDev &scene, const FeatureArgs &args, bool counters, bool surfaces, hipStream_t stream) {
    void (*const kernel)(SceneDev, FeatureArgs) =
        surfaces ? (counters ? pt_features_specular<STACK, true, SRC, true> : pt_features_specular<STACK, false, SRC, true>)
                 : (counters ? pt_features_specular<STACK, true, SRC, false> : pt_features_specular<STACK, false, SRC, false>);
    return launch_persistent(kernel, kBlock, args.n_pixels, scene, args, stream);
}

// The instance of a call: by the scene's stack need (a tiny-stack scene takes the kStackSmall shape), then counters and surfaces.
template <int SRC>
hipError_t launch_specular_src(const SceneDev &scene, const FeatureArgs &args, uint32_t stack_need, bool counters, bool surfaces, hipStream_t stream) {
    if (args.n_pixels == 0 || args.spp == 0) return hipSuccess;
    if (stack_need > (uint32_t)kStackLarge) return hipErrorInvalidValue;
    if (stack_need <= (uint32_t)kStackSmall) return launch_specular_shape<kStackSmall, SRC>(scene, args, counters, surfaces, stream);
    if (stack_need <= (uint32_t)kStackMid) return launch_specular_shape<kStackMid, SRC>(scene, args, counters, surfaces, stream);
    return launch_specular_shape<kStackLarge, SRC>(scene, args, counters, surfaces, stream);
}

} // namespace

hipError_t launch_features_specular(const SceneDev &scene, const FeatureArgs &args, uint32_t stack_need, int src, bool counters, bool surfaces,
                                    hipStream_t stream) {
    switch (src) {
        case kFeatRows: return launch_specular_src<kFeatRows>(scene, args, stack_need, counters, surfaces, stream);
        case kFeatPixels: return launch_specular_src<kFeatPixels>(scene, args, stack_need, counters, surfaces, stream);
        case kFeatRays: return launch_specular_src<kFeatRays>(scene, args, stack_need, counters, surfaces, stream);
        default: return hipErrorInvalidValue;
    }
}

} // namespace rt2022
