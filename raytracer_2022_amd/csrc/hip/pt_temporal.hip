// pt_temporal.hip — temporal accumulation with reprojection (rt_temporal*, include/rt2022.h has the definition: every
// + - * / below is one of its operations, in its order; -ffp-contract=off).
//
// One kernel, tp_accumulate: one lane per pixel in the 64 x 4 tiles of pt_post.hpp (a wave is 64 consecutive pixels of one
// image row). A lane reads its sums (24 B) and its feature record (four 16-byte pieces) at the pixel's place in buffer order
// through that header's front end, finds the mean first-hit point from the record's depth, projects it into the previous
// camera by Cramer's rule and gathers the four bilinear taps of the previous state: records are 64 B and the two taps of a
// row are neighbours, so a lane reads two 128-byte spans of d_prev as 16-byte pieces. It writes its own state record (four
// 16-byte pieces, image order) and its three sums (buffer order). Nothing is staged: no LDS, and no workspace but the row
// kernel's map (pt_rows.hip; a.inv). fx / fy become integers only after the range test, so a tap's address is
// computed from numbers in [-1, width] x [-1, height] and is used only when it lies inside the image. A far miss
// (RT_TEMPORAL_FAR_MISSES) takes the same path with another right-hand side and another tap rule: the same four taps.
#include "pt_post.hpp"

namespace rt2022 {

namespace {

POST_DEV double tp_dot(const double u[3], const double v[3]) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

POST_DEV void tp_cross(const double u[3], const double v[3], double w[3]) {
    w[0] = u[1] * v[2] - u[2] * v[1];
    w[1] = u[2] * v[0] - u[0] * v[2];
    w[2] = u[0] * v[1] - u[1] * v[0];
}

__global__ void __launch_bounds__(kPostBlock) tp_accumulate(const TemporalArgs a) {
    uint32_t x, y;
    post_pixel(a.width, x, y);
    if (x >= a.width || y >= a.height) return;
    const uint64_t i = (uint64_t)y * a.width + x;
    const uint64_t src = post_src(a.inv, a.width, x, y);
    const PostRecord r = post_load(a.feat, src);
    const double2 f1 = r.f1, f2 = r.f2, f3 = r.f3;
    double alb[3], e[3], m[3];
    post_albedo(r, a.sp, alb);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        m[c] = post_modulation(a.demodulate, a.albedo_floor, alb[c]);
        e[c] = post_colour(a.sum[3 * src + c], a.sp, m[c]);
    }
    const double hits = f3.y;
    const bool covered = hits > 0.0;
    const double zb = covered ? f3.x / hits : 0.0;
    const double nb[3] = {covered ? f1.y / hits : 0.0, covered ? f2.x / hits : 0.0, covered ? f2.y / hits : 0.0};

    double eo[3] = {e[0], e[1], e[2]}, no = 1.0;           // the restart
    // RT_TEMPORAL_FAR_MISSES (a.far_misses, uniform): an uncovered pixel is a point at infinity — the pixel centre's
    // direction in place of P - o', no ze, and its taps are the previous state's uncovered pixels (depth == 0.0), untested.
    if (a.prev && (covered || a.far_misses)) {
        const double sc = ((double)x + 0.5) / a.wm1, tc = ((double)y + 0.5) / a.hm1;
        double c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double g = (a.llc[k] + sc * a.hor[k]) + tc * a.ver[k];
            if (covered) {
                const double p = a.o[k] + zb * (g - a.o[k]);
                c[k] = -(p - a.po[k]);
            } else {
                c[k] = -(g - a.o[k]);
            }
        }
        double bc[3], rc[3], br[3];
        tp_cross(a.pver, c, bc);
        tp_cross(a.pr, c, rc);
        tp_cross(a.pver, a.pr, br);
        const double det = tp_dot(a.phor, bc);
        const double s1 = tp_dot(a.pr, bc) / det, t1 = tp_dot(a.phor, rc) / det, lam = tp_dot(a.phor, br) / det;
        const double fx = s1 * a.wm1 - 0.5, fy = t1 * a.hm1 - 0.5;
        // (the range test refuses NaN and both infinities: only then are fx and fy turned into integers)
        if (lam > 0.0 && fx >= -1.0 && fx < a.wd && fy >= -1.0 && fy < a.hd) {
            const double ze = covered ? 1.0 / lam : 0.0;
            const double xf = floor(fx), yf = floor(fy);
            const double wx = fx - xf, wy = fy - yf;
            const int64_t x0 = (int64_t)xf, y0 = (int64_t)yf;
            const double bw[4] = {(1.0 - wx) * (1.0 - wy), wx * (1.0 - wy), (1.0 - wx) * wy, wx * wy};
            double sw = 0.0, sn = 0.0, se[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int64_t qx = x0 + (t & 1), qy = y0 + (t >> 1);
                if (qx < 0 || qx >= (int64_t)a.width || qy < 0 || qy >= (int64_t)a.height) continue;
                const double2 *q = reinterpret_cast<const double2 *>(a.prev + ((uint64_t)qy * a.width + (uint64_t)qx));
                const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];       // {e0, e1} {e2, n} {depth, n0} {n1, n2}
                const double pd = q2.x;
                if (!(covered ? pd > 0.0 : pd == 0.0)) continue;
                if (covered && a.depth_test) {
                    const double dd = pd - ze;
                    if (!((dd < 0.0 ? -dd : dd) <= a.tol_depth * ze)) continue;
                }
                if (covered && a.normal_test) {
                    const double d0 = nb[0] - q2.y, d1 = nb[1] - q3.x, d2 = nb[2] - q3.y;
                    if (!((d0 * d0 + d1 * d1) + d2 * d2 <= a.tol_normal)) continue;
                }
                sw = sw + bw[t];
                se[0] = se[0] + bw[t] * q0.x;
                se[1] = se[1] + bw[t] * q0.y;
                se[2] = se[2] + bw[t] * q1.x;
                sn = sn + bw[t] * q1.y;
            }
            if (sw >= a.w_min) {
                const double nh = sn / sw, t = nh + 1.0;
                no = t < a.n_max ? t : a.n_max;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double eh = se[k] / sw;
                    eo[k] = eh + (e[k] - eh) / no;
                }
            }
        }
    }
    double2 *st = reinterpret_cast<double2 *>(a.state + i);
    st[0] = make_double2(eo[0], eo[1]);
    st[1] = make_double2(eo[2], no);
    st[2] = make_double2(zb, nb[0]);
    st[3] = make_double2(nb[1], nb[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) a.out[3 * src + k] = (eo[k] * m[k]) * a.sp;
}

} // namespace

hipError_t launch_temporal(const TemporalArgs &a, hipStream_t stream) {
    hipLaunchKernelGGL(tp_accumulate, post_grid(a.width, a.height), dim3(kPostBlock), 0, stream, a);
    return hipGetLastError();
}

} // namespace rt2022
