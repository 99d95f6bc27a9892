// pt_denoise.hip — edge-avoiding a-trous denoiser over a render's sums and its feature buffers (rt_denoise*,
// include/rt2022.h has the definition: every + - * / below is one of its operations, in its order; -ffp-contract=off).
//
// Two kernels on the caller's workspace (denoise_layout, host/post_check.hpp). A row list has been through the row kernel of
// pt_rows.hip before them: its map is a.inv. The pixel front end and the tap loop are pt_post.hpp's.
//   dn_prepare  buffer order -> image order: NaN -> 0, / sp, demodulation; writes the packed guides and colour plane 0
//               (with no iteration: the output).
//   dn_atrous   one launch per iteration, plane k & 1 -> plane ~k & 1; the last one remodulates and writes the output in
//               buffer order.
// Layout: a pixel's ten doubles are five 16-byte pieces, each piece a plane of its own — {n0, n1} {n2, z} {a0, a1} never
// change, {e0, e1} {e2, a2} ping-pong (a2 rides in the colour's spare half, so a tap is five loads with nothing wasted).
// A workgroup is 64 x 4 pixels and a wave 64 consecutive pixels of one image row, so every tap of a wave is five
// contiguous 1 KiB loads, served by the caches: neighbouring lanes, waves and workgroups read the same lines. The centre
// pixel stays in registers; a tap costs one division. (Staging steps 1 and 2 through an LDS tile with a halo was built and
// measured: 0.36-0.38 ms against 0.39-0.41 ms per 800x800 frame of five iterations, beside a 38 ms render — not worth two
// more instances and a 69 KB LDS opt-in: profiles/denoise_bench.log)
//
// The dual filter (rt_denoise_dual*: two half-sample renders A and B, their mean filtered under a colour distance measured
// in units of the variance estimated from A - B) adds three kernels on a workspace of its own (denoise_dual_layout):
//   dn_dual_prepare    both halves, buffer order -> image order: the mean e0, the variance estimate v0, the averaged guides.
//   dn_dual_prefilter  one launch per prefilter pass over v, weighted by the guides alone; the last one leaves u0 beside e2.
//   dn_dual_atrous     one launch per iteration: colour and variance together, the last one writes both outputs.
// Layout: a pixel has eleven doubles, so one of them cannot share a 16-byte piece: {n0, n1} {n2, z} {a0, a1} as above,
// {e0, e1} {e2, u} ping-pong — the variance takes a2's old place and travels with the colour it belongs to — and a2 and the
// prefilter's v are planes of single doubles. A colour tap is five 16-byte loads and one 8-byte load (88 bytes, all used;
// a wave reads 5 x 1 KiB + 512 B contiguous) and two divisions; a prefilter tap is three 16-byte and two 8-byte loads
// (64 bytes) and one division. The centre pixel stays in registers.
#include "../host/post_check.hpp"
#include "pt_post.hpp"

namespace rt2022 {

namespace {

struct DnPixel { double e[3], n[3], a[3], z; };

// The pixel at index i of five planes `stride` apart (guides: g, colour: c).
POST_DEV DnPixel dn_load(const double2 *g, const double2 *c, uint64_t stride, uint64_t i) {
    const double2 g0 = g[i], g1 = g[stride + i], g2 = g[2 * stride + i], c0 = c[i], c1 = c[stride + i];
    DnPixel p;
    p.n[0] = g0.x; p.n[1] = g0.y; p.n[2] = g1.x; p.z = g1.y; p.a[0] = g2.x; p.a[1] = g2.y;
    p.e[0] = c0.x; p.e[1] = c0.y; p.e[2] = c1.x; p.a[2] = c1.y;
    return p;
}

POST_DEV double dn_dist(const double p[3], const double q[3]) {
    const double d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

__global__ void __launch_bounds__(kPostBlock) dn_prepare(const DenoiseArgs a, double2 *guides, double2 *colour, bool final) {
    uint32_t x, y;
    post_pixel(a.width, x, y);
    if (x >= a.width || y >= a.height) return;
    const uint64_t n = (uint64_t)a.width * a.height, i = (uint64_t)y * a.width + x;
    const uint64_t src = post_src(a.inv, a.width, x, y);
    const PostRecord r = post_load(a.feat, src);
    double alb[3], e[3], m[3];
    post_albedo(r, a.sp, alb);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        m[c] = post_modulation(a.demodulate, a.albedo_floor, alb[c]);
        e[c] = post_colour(a.sum[3 * src + c], a.sp, m[c]);
    }
    if (final) {                                           // no iteration: e0 goes straight back out
#pragma unroll
        for (int c = 0; c < 3; c++) a.out[3 * src + c] = (e[c] * m[c]) * a.sp;
        return;
    }
    guides[i] = make_double2(r.f1.y / a.sp, r.f2.x / a.sp);
    guides[n + i] = make_double2(r.f2.y / a.sp, r.f3.x / a.sp);
    guides[2 * n + i] = make_double2(alb[0], alb[1]);
    colour[i] = make_double2(e[0], e[1]);
    colour[n + i] = make_double2(e[2], alb[2]);
}

// One iteration at step s. LAST: the result is remodulated and written to a.out in buffer order instead of the other
// colour plane.
template <bool LAST>
__global__ void __launch_bounds__(kPostBlock) dn_atrous(const DenoiseArgs a, const double2 *guides, const double2 *cin, double2 *cout, uint32_t s,
                                                        double inv_c) {
    uint32_t x, y;
    post_pixel(a.width, x, y);
    if (x >= a.width || y >= a.height) return;
    const uint64_t n = (uint64_t)a.width * a.height, ip = (uint64_t)y * a.width + x;
    const DnPixel p = dn_load(guides, cin, n, ip);
    double sw = 0.0, sv[3] = {0.0, 0.0, 0.0};
    dn_for_taps(x, y, s, a.width, a.height, [&](double h, uint64_t iq) {
        const DnPixel q = dn_load(guides, cin, n, iq);
        const double dc = dn_dist(p.e, q.e), dn = dn_dist(p.n, q.n), da = dn_dist(p.a, q.a), dz = p.z - q.z;
        const double den = (((1.0 + dc * inv_c) * (1.0 + dn * a.inv_n)) * (1.0 + (dz * dz) * a.inv_z)) * (1.0 + da * a.inv_a);
        const double w = h / den;
        sw = sw + w;
#pragma unroll
        for (int c = 0; c < 3; c++) sv[c] = sv[c] + w * q.e[c];
    });
    const double e[3] = {sv[0] / sw, sv[1] / sw, sv[2] / sw};
    if (LAST) {
        const uint64_t dst = post_src(a.inv, a.width, x, y);
#pragma unroll
        for (int c = 0; c < 3; c++) a.out[3 * dst + c] = (e[c] * post_modulation(a.demodulate, a.albedo_floor, p.a[c])) * a.sp;
    } else {
        cout[ip] = make_double2(e[0], e[1]);
        cout[n + ip] = make_double2(e[2], p.a[2]);
    }
}

// ---- the dual filter (rt_denoise_dual*) ---------------------------------------------------------------------------------
struct DnDualPixel { double e[3], u, n[3], a[3], z; };

// The three guide pieces and the a2 plane at index i.
POST_DEV void dn_dual_guides(const double2 *g, const double *a2, uint64_t stride, uint64_t i, double n[3], double a[3], double &z) {
    const double2 g0 = g[i], g1 = g[stride + i], g2 = g[2 * stride + i];
    n[0] = g0.x; n[1] = g0.y; n[2] = g1.x; z = g1.y; a[0] = g2.x; a[1] = g2.y; a[2] = a2[i];
}

POST_DEV DnDualPixel dn_dual_load(const double2 *g, const double *a2, const double2 *c, uint64_t stride, uint64_t i) {
    DnDualPixel p;
    dn_dual_guides(g, a2, stride, i, p.n, p.a, p.z);
    const double2 c0 = c[i], c1 = c[stride + i];
    p.e[0] = c0.x; p.e[1] = c0.y; p.e[2] = c1.x; p.u = c1.y;
    return p;
}

// Where the prepare kernel and the last prefilter pass leave the variance.
enum : int { kDnVarPlane = 0, kDnVarColour = 1, kDnVarOut = 2 };        // a v plane / colour plane 0's u / a.out_var

POST_DEV void dn_dual_store_var(const DenoiseDualArgs &d, int to, double *vplane, double2 *colour0, uint64_t n, uint64_t i, uint64_t buf, double v) {
    if (to == kDnVarPlane) vplane[i] = v;
    else if (to == kDnVarColour) reinterpret_cast<double *>(colour0 + n + i)[1] = v;
    else if (d.out_var) d.out_var[buf] = v;
}

// Buffer order -> image order for both halves. `final` (no colour iteration): the mean goes straight back out. `var_to`:
// where v0 goes — the first v plane (a prefilter follows), colour plane 0 (none does) or the output (nothing follows).
__global__ void __launch_bounds__(kPostBlock) dn_dual_prepare(const DenoiseDualArgs d, double2 *guides, double *a2, double2 *colour, double *vplane,
                                                              bool final, int var_to) {
    const DenoiseArgs &a = d.a;
    uint32_t x, y;
    post_pixel(a.width, x, y);
    if (x >= a.width || y >= a.height) return;
    const uint64_t n = (uint64_t)a.width * a.height, i = (uint64_t)y * a.width + x;
    const uint64_t src = post_src(a.inv, a.width, x, y);
    const PostRecord r = post_add(post_load(a.feat, src), post_load(d.feat_b, src));     // the guides are the two halves' mean
    double alb[3], e[3], h[3], m[3];
    post_albedo(r, d.sp2, alb);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double ca = post_mean(a.sum[3 * src + c], a.sp), cb = post_mean(d.sum_b[3 * src + c], a.sp);
        m[c] = post_modulation(a.demodulate, a.albedo_floor, alb[c]);
        e[c] = ((ca + cb) * 0.5) / m[c];
        h[c] = ((ca - cb) * 0.5) / m[c];
    }
    const double v = (h[0] * h[0] + h[1] * h[1]) + h[2] * h[2];
    if (final) {
#pragma unroll
        for (int c = 0; c < 3; c++) a.out[3 * src + c] = (e[c] * m[c]) * d.sp2;
        if (var_to == kDnVarOut) {                         // ... and no prefilter either: nothing else runs
            if (d.out_var) d.out_var[src] = v;
            return;
        }
    }
    guides[i] = make_double2(r.f1.y / d.sp2, r.f2.x / d.sp2);
    guides[n + i] = make_double2(r.f2.y / d.sp2, r.f3.x / d.sp2);
    guides[2 * n + i] = make_double2(alb[0], alb[1]);
    a2[i] = alb[2];
    colour[i] = make_double2(e[0], e[1]);
    colour[n + i] = make_double2(e[2], v);
    if (var_to == kDnVarPlane) vplane[i] = v;
}

// One prefilter pass over the variance at step s: the guides' weights alone. `var_to`: where the result goes (a v plane;
// after the last pass colour plane 0's u, or with no colour iteration the output, in buffer order).
__global__ void __launch_bounds__(kPostBlock) dn_dual_prefilter(const DenoiseDualArgs d, const double2 *guides, const double *a2, const double *vin,
                                                                double *vout, double2 *colour0, uint32_t s, int var_to) {
    const DenoiseArgs &a = d.a;
    uint32_t x, y;
    post_pixel(a.width, x, y);
    if (x >= a.width || y >= a.height) return;
    const uint64_t n = (uint64_t)a.width * a.height, ip = (uint64_t)y * a.width + x;
    double pn[3], pa[3], pz;
    dn_dual_guides(guides, a2, n, ip, pn, pa, pz);
    double sw = 0.0, sx = 0.0;
    dn_for_taps(x, y, s, a.width, a.height, [&](double h, uint64_t iq) {
        double qn[3], qa[3], qz;
        dn_dual_guides(guides, a2, n, iq, qn, qa, qz);
        const double dn = dn_dist(pn, qn), da = dn_dist(pa, qa), dz = pz - qz;
        const double g = ((1.0 + dn * a.inv_n) * (1.0 + (dz * dz) * a.inv_z)) * (1.0 + da * a.inv_a);
        const double w = h / g;
        sw = sw + w;
        sx = sx + w * vin[iq];
    });
    dn_dual_store_var(d, var_to, vout, colour0, n, ip, post_src(a.inv, a.width, x, y), sx / sw);
}

// One variance-aware iteration at step s. LAST: the colour is remodulated and written to a.out, the variance to d.out_var,
// both in buffer order, instead of the other colour plane.
template <bool LAST>
__global__ void __launch_bounds__(kPostBlock) dn_dual_atrous(const DenoiseDualArgs d, const double2 *guides, const double *a2, const double2 *cin,
                                                             double2 *cout, uint32_t s) {
    const DenoiseArgs &a = d.a;
    uint32_t x, y;
    post_pixel(a.width, x, y);
    if (x >= a.width || y >= a.height) return;
    const uint64_t n = (uint64_t)a.width * a.height, ip = (uint64_t)y * a.width + x;
    const DnDualPixel p = dn_dual_load(guides, a2, cin, n, ip);
    double sw = 0.0, su = 0.0, sv[3] = {0.0, 0.0, 0.0};
    dn_for_taps(x, y, s, a.width, a.height, [&](double h, uint64_t iq) {
        const DnDualPixel q = dn_dual_load(guides, a2, cin, n, iq);
        const double dc = dn_dist(p.e, q.e), dn = dn_dist(p.n, q.n), da = dn_dist(p.a, q.a), dz = p.z - q.z;
        const double r = (dc * d.inv_c) / ((p.u + q.u) + d.var_floor);
        const double den = (((1.0 + r) * (1.0 + dn * a.inv_n)) * (1.0 + (dz * dz) * a.inv_z)) * (1.0 + da * a.inv_a);
        const double w = h / den;
        sw = sw + w;
#pragma unroll
        for (int c = 0; c < 3; c++) sv[c] = sv[c] + w * q.e[c];
        su = su + (w * w) * q.u;
    });
    const double e[3] = {sv[0] / sw, sv[1] / sw, sv[2] / sw};
    const double u = su / (sw * sw);
    if (LAST) {
        const uint64_t dst = post_src(a.inv, a.width, x, y);
#pragma unroll
        for (int c = 0; c < 3; c++) a.out[3 * dst + c] = (e[c] * post_modulation(a.demodulate, a.albedo_floor, p.a[c])) * d.sp2;
        if (d.out_var) d.out_var[dst] = u;
    } else {
        cout[ip] = make_double2(e[0], e[1]);
        cout[n + ip] = make_double2(e[2], u);
    }
}

} // namespace

hipError_t launch_denoise(const DenoiseArgs &a, uint32_t n_iter, const double *inv_c, hipStream_t stream) {
    const DenoiseLayout l = denoise_layout(a.width, a.height);
    double2 *const guides = reinterpret_cast<double2 *>(a.ws + l.guides);
    double2 *const colour[2] = {reinterpret_cast<double2 *>(a.ws + l.colour[0]), reinterpret_cast<double2 *>(a.ws + l.colour[1])};
    const dim3 grid = post_grid(a.width, a.height), block(kPostBlock);
    hipLaunchKernelGGL(dn_prepare, grid, block, 0, stream, a, guides, colour[0], n_iter == 0);
    hipError_t e = hipGetLastError();
    for (uint32_t k = 0; k < n_iter && e == hipSuccess; k++) {
        hipLaunchKernelGGL(k + 1 == n_iter ? dn_atrous<true> : dn_atrous<false>, grid, block, 0, stream, a, guides, colour[k & 1u], colour[~k & 1u],
                           1u << k, inv_c[k]);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_denoise_dual(const DenoiseDualArgs &d, uint32_t var_iter, uint32_t n_iter, hipStream_t stream) {
    const DenoiseArgs &a = d.a;
    const DenoiseDualLayout l = denoise_dual_layout(a.width, a.height);
    double2 *const guides = reinterpret_cast<double2 *>(a.ws + l.guides);
    double *const a2 = reinterpret_cast<double *>(a.ws + l.a2);
    double2 *const colour[2] = {reinterpret_cast<double2 *>(a.ws + l.colour[0]), reinterpret_cast<double2 *>(a.ws + l.colour[1])};
    double *const var[2] = {reinterpret_cast<double *>(a.ws + l.var[0]), reinterpret_cast<double *>(a.ws + l.var[1])};
    const dim3 grid = post_grid(a.width, a.height), block(kPostBlock);
    const int var_end = n_iter ? kDnVarColour : kDnVarOut;                // where the variance the colour passes start from goes
    hipLaunchKernelGGL(dn_dual_prepare, grid, block, 0, stream, d, guides, a2, colour[0], var[0], n_iter == 0, var_iter ? kDnVarPlane : var_end);
    hipError_t e = hipGetLastError();
    for (uint32_t t = 0; t < var_iter && e == hipSuccess; t++) {
        hipLaunchKernelGGL(dn_dual_prefilter, grid, block, 0, stream, d, guides, a2, var[t & 1u], var[~t & 1u], colour[0], 1u << t,
                           t + 1 == var_iter ? var_end : kDnVarPlane);
        e = hipGetLastError();
    }
    for (uint32_t k = 0; k < n_iter && e == hipSuccess; k++) {
        hipLaunchKernelGGL(k + 1 == n_iter ? dn_dual_atrous<true> : dn_dual_atrous<false>, grid, block, 0, stream, d, guides, a2, colour[k & 1u],
                           colour[~k & 1u], 1u << k);
        e = hipGetLastError();
    }
    return e;
}

} // namespace rt2022
