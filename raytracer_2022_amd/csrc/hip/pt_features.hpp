// pt_features.hpp — what the feature kernels share (pt_features.hip: first-hit records; pt_features_specular.hip: the
// RT_FLAG_SPECULAR records): the lane's pixel, the three sources of work items, the camera ray of a sample, the first-hit
// albedo rule and the add of one sample into the lane's own record. Each kernel writes its own done arm and scheduler loop.
#ifndef RT2022_PT_FEATURES_HPP
#define RT2022_PT_FEATURES_HPP

#include "pt_traverse.hpp"

namespace rt2022 {

namespace {

constexpr uint32_t kFHasPixel = 1u;    // lane flag: the lane carries a pixel (a sample of it is in flight)

// (SRC — kFeatRows, kFeatPixels, kFeatRays: pt_device.h)
struct FLane : TravLane {
    uint32_t row, px;      // the pixel: entry of the row list, column (kFeatPixels, kFeatRays: the low and the high word of the entry's index)
    uint32_t smp;          // the sample in flight
};

// The camera ray of (row, px, sample) and the RNG behind it, as wf_shade's fresh-path code aims it (main.rs:144-149).
// kFeatRays: the caller's ray record in its place — four 16-byte loads, the stream keyed as rt_radiance keys sample smp of
// the ray, and nothing drawn.
template <int SRC>
RT_DEV Ray f_camera(const FeatureArgs &a, uint32_t row, uint32_t px, uint32_t smp, Rng &rng) {
    if constexpr (SRC == kFeatRays) {
        const double2 *q = reinterpret_cast<const double2 *>(a.rays + ((uint64_t)row | ((uint64_t)px << 32)));
        const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        rng = Rng(rtm::path_key(rtm::d2u(q3.y), 0u, 0ull, smp));
        return Ray(Vec3(q0.x, q0.y, q1.x), Vec3(q1.y, q2.x, q2.y), q3.x);
    }
    uint32_t frame, py;
    if constexpr (SRC == kFeatPixels) {
        // id = frame * (width * height) + py * width + px. Two 32-bit divisions where every id of the view fits 32 bits (a
        // uniform test on kernel arguments: the host checked the ids against width * height * n_frames), else 64-bit ones.
        const uint64_t id = a.pixel_ids[(uint64_t)row | ((uint64_t)px << 32)];
        if (a.ids32) {
            const uint32_t i = (uint32_t)id, ip = a.width * a.height;
            frame = i / ip;
            const uint32_t rem = i - frame * ip;
            py = rem / a.width;
            px = rem - py * a.width;
        } else {
            const uint64_t ip = (uint64_t)a.width * a.height, f = id / ip, rem = id - f * ip, y = rem / a.width;
            frame = (uint32_t)f;
            py = (uint32_t)y;
            px = (uint32_t)(rem - y * a.width);
        }
    } else {
        const uint32_t g = a.row_ids[row];
        frame = g / a.height; py = g - frame * a.height;
    }
    rng = Rng(rtm::path_key(a.seed, frame, (uint64_t)py * a.width + px, smp));
    const double rand_u = rng.gen_f64();
    const double rand_v = rng.gen_f64();
    const double u = ((double)px + rand_u) / (double)(a.width - 1);
    const double v = ((double)py + rand_v) / (double)(a.height - 1);
    return get_ray(a.cam, u, v, rng);
}

// scatter's attenuation where the material scatters, emitted where it does not (material/mod.rs).
RT_DEV Vec3 f_albedo(const SceneDev &s, const HitRec &rec) {
    const rt_material &m = s.materials[rec.mat & kMatIndexMask];
    const uint32_t kind = m.kind;
    if (kind == RT_MAT_METAL) return ld3(m.albedo);
    if (kind == RT_MAT_DIELECTRIC) return Vec3(1.0, 1.0, 1.0);
    if (kind == RT_MAT_DIFFUSE_LIGHT && !rec.front_face) return Vec3(0.0, 0.0, 0.0);
    return texture_value(s, m.tex, rec.u, rec.v, rec.p);
}

// One sample's features, added into the lane's own record: {a.x, a.y} {a.z, n.x} {n.y, n.z} {depth, hits}. The first sample
// stores (0 + f_0).
template <int SRC>
RT_DEV void f_add(const FeatureArgs &a, const FLane &L, Vec3 alb, Vec3 n, double depth, double hits) {
    double2 *o;
    if constexpr (SRC != kFeatRows) o = reinterpret_cast<double2 *>(a.out + ((uint64_t)L.row | ((uint64_t)L.px << 32)));
    else o = reinterpret_cast<double2 *>(a.out + ((uint64_t)L.row * a.width + L.px));
    double2 s0 = make_double2(0.0, 0.0), s1 = s0, s2 = s0, s3 = s0;
    if (L.smp > 0) { s0 = o[0]; s1 = o[1]; s2 = o[2]; s3 = o[3]; }
    o[0] = make_double2(s0.x + alb.x, s0.y + alb.y);
    o[1] = make_double2(s1.x + alb.z, s1.y + n.x);
    o[2] = make_double2(s2.x + n.y, s2.y + n.z);
    o[3] = make_double2(s3.x + depth, s3.y + hits);
}

// The next pixel (or entry) for a lane that has finished its own: its place i in the claim's order, or nothing left.
template <int SRC>
RT_DEV bool f_take(const FeatureArgs &a, FLane &L, unsigned long long i) {
    const bool have = i < a.n_pixels;
    const unsigned long long ii = have ? i : 0ull;
    if constexpr (SRC != kFeatRows) {
        L.row = (uint32_t)ii;
        L.px = (uint32_t)(ii >> 32);
    } else {
        L.row = (uint32_t)(ii / a.width);
        L.px = (uint32_t)(ii - (unsigned long long)L.row * a.width);
    }
    L.smp = 0;
    return have;
}

} // namespace

// launch_features' RT_FLAG_SPECULAR half (pt_features_specular.hip).
hipError_t launch_features_specular(const SceneDev &scene, const FeatureArgs &args, uint32_t stack_need, int src, bool counters, bool surfaces,
                                    hipStream_t stream);

} // namespace rt2022
#endif
