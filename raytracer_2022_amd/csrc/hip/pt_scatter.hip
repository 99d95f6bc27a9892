// pt_scatter.hip — one step of `ray_color` (main.rs:233-278) between two `world.hit` calls, for a batch of hit records on a
// device scene (rt_scatter*, include/rt2022.h): what the path's vertex emits, the weight and pdf of its scatter and the ray the
// path goes on with, written as a ready rt_query_ray. The loop rt_intersect_device -> rt_scatter_device -> ... is a wavefront
// path tracer the caller drives; unwound in the reference's order it is rt_radiance's sum bit for bit.
//   - one lane per entry, 256-thread blocks, the grid sized to the batch: a step costs about the same for every entry (no
//     traversal), so there is no persistent grid and no work counter;
//   - whole-record I/O in 16-byte pieces: an 80-byte ray and a 96-byte hit (and the 16 bytes of prev that hold its status) in, a
//     64-byte record and an 80-byte ray out. A lane reads all of its entry before it writes any of it: the next rays may be the rays, the records prev;
//   - the hit record is the caller's: nothing of the scene's geometry is read, only materials, textures and the light list
//     (straight from HBM), and a material index at or beyond the pool is refused (RT_SCATTER_INVALID) before the pool is read;
//   - the scatter arithmetic is wf_shade's (pt_wavefront_shade.hip) and the megakernel's (pt_kernel.hip: op_shade), restated.
// All arithmetic is f64 through rt_math.h with -ffp-contract=off, so every record is the CPU oracle's bit for bit.
#include "pt_common.hpp"
#include "pt_scatter.hpp"

namespace rt2022 {

namespace {

constexpr uint64_t kRngGolden = 0x9E3779B97F4A7C15ull;     // Rng::next_u64's increment: the state after k words is s + k * this

// The entry's two records: {w.x, w.y} {w.z, pdf} {rad.x, rad.y} {rad.z, status | draws} and
// {o.x, o.y} {o.z, d.x} {d.y, d.z} {tm, t_min} {t_max, rng_state}.
RT_DEV void sc_write(const ScatterArgs &a, uint64_t i, Vec3 w, double pdf, Vec3 rad, uint32_t status, uint32_t draws, Vec3 o, Vec3 d, double tm,
                     double t_min, double t_max, uint64_t state) {
    double2 *r = reinterpret_cast<double2 *>(a.out_recs + i);
    r[0] = make_double2(w.x, w.y);
    r[1] = make_double2(w.z, pdf);
    r[2] = make_double2(rad.x, rad.y);
    r[3] = make_double2(rad.z, rtm::u2d((uint64_t)status | ((uint64_t)draws << 32)));
    double2 *q = reinterpret_cast<double2 *>(a.out_next + i);
    q[0] = make_double2(o.x, o.y);
    q[1] = make_double2(o.z, d.x);
    q[2] = make_double2(d.y, d.z);
    q[3] = make_double2(tm, t_min);
    q[4] = make_double2(t_max, rtm::u2d(state));
}

} // namespace

template <bool STATS>
__global__ void __launch_bounds__(kScatterBlock) pt_scatter(const SceneDev s, const ScatterArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kScatterBlock + threadIdx.x;
    Counters<STATS> cnt;
    if (i < a.n) {
        const Vec3 zero(0.0, 0.0, 0.0);
        const double2 *q = reinterpret_cast<const double2 *>(a.rays + i);
        bool live = true;
        if (a.prev) {                                          // (status sits in the low word of the record's last double)
            const uint32_t ps = (uint32_t)rtm::d2u(reinterpret_cast<const double2 *>(a.prev + i)[3].y);
            live = ps == RT_SCATTER_SPECULAR || ps == RT_SCATTER_DIFFUSE;
        }
        if (!live) {                                           // the path ended before this step: only the ray's state is read
            sc_write(a, i, zero, 0.0, zero, RT_SCATTER_ENDED, 0u, zero, zero, 0.0, 0.0, 0.0, rtm::d2u(q[4].y));
        } else {
            const double2 q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
            const double2 *h = reinterpret_cast<const double2 *>(a.hits + i);
            const double2 h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5];
            const Vec3 r_dir(q1.y, q2.x, q2.y);
            const double r_tm = q3.x;
            const uint32_t hit = (uint32_t)rtm::d2u(h4.y), front = (uint32_t)(rtm::d2u(h4.y) >> 32);
            const uint32_t mat = (uint32_t)rtm::d2u(h5.x), hit_draws = (uint32_t)rtm::d2u(h5.y);
            // the stream behind the hit's own words (a medium's, constantmedium.rs:60)
            Rng rng(rtm::d2u(q4.y) + (uint64_t)hit_draws * kRngGolden);
            HitRec rec;
            rec.t = h0.x; rec.u = h0.y; rec.v = h1.x;
            rec.p = Vec3(h1.y, h2.x, h2.y);
            rec.normal = Vec3(h3.x, h3.y, h4.x);
            rec.front_face = front != 0;
            rec.mat = mat;
            if (hit == 0) {                                       // main.rs:275-276
                sc_write(a, i, zero, 0.0, ld3(a.background), RT_SCATTER_MISS, 0u, zero, zero, 0.0, 0.0, 0.0, rng.s);
            } else if (mat >= a.n_materials) {                    // a made-up record must not index out of the pool
                sc_write(a, i, zero, 0.0, zero, RT_SCATTER_INVALID, 0u, zero, zero, 0.0, 0.0, 0.0, rng.s);
            } else {
                const rt_material &m = s.materials[mat];
                const uint32_t mk = m.kind;
                if (mk == RT_MAT_DIFFUSE_LIGHT) {                 // emitted; scatter = None (material/mod.rs:16-18,174-180)
                    const Vec3 e = rec.front_face ? texture_value(s, m.tex, rec.u, rec.v, rec.p) : zero;
                    sc_write(a, i, zero, 0.0, e, RT_SCATTER_EMITTED, 0u, zero, zero, 0.0, 0.0, 0.0, rng.s);
                } else {
                    Vec3 w, dir;
                    double p = 1.0, tm = r_tm;
                    uint32_t status = RT_SCATTER_SPECULAR;
                    if (mk == RT_MAT_LAMBERTIAN) {                // material/mod.rs:51-65 + main.rs:263-271
                        const Vec3 att = texture_value(s, m.tex, rec.u, rec.v, rec.p);
                        const rtm::Onb uvw = rtm::onb_from_w(rec.normal);
                        double cosv;
                        if (s.n_lights == 0) {                    // cosine-only mode
                            dir = uvw.local_vec(random_cosine_direction(rng));
                            cosv = rtm::dot(rtm::to_unit(dir), uvw.w);
                            p = cosv <= 0.0 ? 0.0 : cosv / rtm::PI;
                        } else {                                  // MixturePdf(lights, cos), pdf.rs:94-104
                            if (rng.gen_range(0.0, 1.0) < 0.5) dir = lights_random(s, rec.p, rng);
                            else dir = uvw.local_vec(random_cosine_direction(rng));
                            const double lp = lights_pdf_value<STATS>(s, rec.p, dir, cnt);
                            cosv = rtm::dot(rtm::to_unit(dir), uvw.w);
                            const double cp = cosv <= 0.0 ? 0.0 : cosv / rtm::PI;
                            p = 0.5 * lp + 0.5 * cp;
                        }
                        const double cosine = rtm::dot(rec.normal, rtm::to_unit(dir));
                        const double spdf = cosine < 0.0 ? 0.0 : cosine / rtm::PI;
                        w = att * spdf;
                        status = RT_SCATTER_DIFFUSE;
                    } else if (mk == RT_MAT_METAL) {              // material/mod.rs:85-96
                        const Vec3 reflected = rtm::reflect(rtm::to_unit(r_dir), rec.normal);
                        dir = reflected + random_in_unit_sphere(rng) * m.param;
                        w = ld3(m.albedo);
                        tm = 0.0;                                 // time = 0., mod.rs:91
                    } else if (mk == RT_MAT_DIELECTRIC) {         // material/mod.rs:120-147
                        const double refraction_ratio = rec.front_face ? 1.0 / m.param : m.param;
                        const Vec3 unit_direction = rtm::to_unit(r_dir);
                        const double cos_theta = rtm::fmin_(rtm::dot(-unit_direction, rec.normal), 1.0);
                        const double sin_theta = rtm::sqrt_(1.0 - cos_theta * cos_theta);
                        const bool cannot_refract = refraction_ratio * sin_theta > 1.0;
                        const double random_double = rng.gen_range(0.0, 1.0);
                        dir = (cannot_refract || reflectance(cos_theta, refraction_ratio) > random_double)
                                  ? rtm::reflect(unit_direction, rec.normal)
                                  : rtm::refract(unit_direction, rec.normal, refraction_ratio);
                        w = Vec3(1.0, 1.0, 1.0);
                    } else {                                      // Isotropic, material/mod.rs:207-213
                        w = texture_value(s, m.tex, rec.u, rec.v, rec.p);
                        dir = random_in_unit_sphere(rng);
                    }
                    cnt.draws(rng.draws);
                    // world.hit(scattered, 0.001, f64::MAX), main.rs:243
                    sc_write(a, i, w, p, zero, status, rng.draws, rec.p, dir, tm, a.t_min, rtm::F64_MAX, rng.s);
                }
            }
        }
    }
    if (STATS) cnt.flush_wave(a.stats);
}

hipError_t launch_scatter(const SceneDev &scene, const ScatterArgs &args, bool counters, hipStream_t stream) {
    if (args.n == 0) return hipSuccess;
    if (args.n > kScatterMaxEntries) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((args.n + kScatterBlock - 1) / kScatterBlock);
    void (*const kernel)(SceneDev, ScatterArgs) = counters ? pt_scatter<true> : pt_scatter<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kScatterBlock), 0, stream, scene, args);
    return hipGetLastError();
}

} // namespace rt2022
