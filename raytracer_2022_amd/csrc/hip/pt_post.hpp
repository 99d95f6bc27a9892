// pt_post.hpp — what the kernels on a render's buffers share (pt_denoise.hip, pt_temporal.hip): the 64 x 4 pixel tiles, the
// front end that takes a pixel from buffer order — its place, its feature record, its albedo, its demodulated colour — and
// the denoisers' 5 x 5 tap loop. Every + - * / is an operation of the definitions in include/rt2022.h, in its order.
#ifndef RT2022_PT_POST_HPP
#define RT2022_PT_POST_HPP
#include "pt_device.h"

namespace rt2022 {

#define POST_DEV __device__ __forceinline__

// A workgroup is 64 x 4 pixels and a wave 64 consecutive pixels of one image row. The tiles of a row are counted in 64
// bits: width + 63 wraps in 32 for the widest images RT_DENOISE_MAX_PIXELS admits.
constexpr int kPostBlock = 256;
inline dim3 post_grid(uint32_t width, uint32_t height) { return dim3((uint32_t)(((uint64_t)width + 63u) / 64u * (((uint64_t)height + 3u) / 4u))); }
// The lane's pixel — which may lie outside the image.
POST_DEV void post_pixel(uint32_t width, uint32_t &x, uint32_t &y) {
    const uint32_t nbx = (uint32_t)(((uint64_t)width + 63u) / 64u);
    const uint32_t by = blockIdx.x / nbx, bx = blockIdx.x - by * nbx;
    x = bx * 64u + (threadIdx.x & 63u); y = by * 4u + (threadIdx.x >> 6);
}

// Image pixel (x, y)'s index in buffer order (inv: image row -> buffer row, null: the identity).
POST_DEV uint64_t post_src(const uint32_t *inv, uint32_t width, uint32_t x, uint32_t y) { return (uint64_t)(inv ? inv[y] : y) * width + x; }

// A feature record as its four 16-byte pieces; the sum of two halves' records, field by field.
struct PostRecord { double2 f0, f1, f2, f3; };                         // {a0, a1} {a2, n0} {n1, n2} {depth, hits}
POST_DEV PostRecord post_load(const rt_feature *feat, uint64_t src) {
    const double2 *f = reinterpret_cast<const double2 *>(feat + src);
    return PostRecord{f[0], f[1], f[2], f[3]};
}
POST_DEV double2 post_add(double2 p, double2 q) { return make_double2(p.x + q.x, p.y + q.y); }
POST_DEV PostRecord post_add(const PostRecord &p, const PostRecord &q) {
    return PostRecord{post_add(p.f0, q.f0), post_add(p.f1, q.f1), post_add(p.f2, q.f2), post_add(p.f3, q.f3)};
}
POST_DEV void post_albedo(const PostRecord &r, double sp, double alb[3]) { alb[0] = r.f0.x / sp; alb[1] = r.f0.y / sp; alb[2] = r.f1.x / sp; }

POST_DEV double post_modulation(bool demodulate, double floor, double albedo) { return demodulate ? (albedo > floor ? albedo : floor) : 1.0; }
// A sum as a mean with NaN -> 0, and that mean demodulated.
POST_DEV double post_mean(double s, double sp) { return (s != s ? 0.0 : s) / sp; }
POST_DEV double post_colour(double s, double sp, double m) { return post_mean(s, sp) / m; }

// The 5 x 5 stencil at `step` round (x, y): f(h, q) for every tap inside the image, q its index in image order and h its
// B3-spline weight.
constexpr double dn_h(int t) { return (t == 0 || t == 4) ? 1.0 / 16.0 : t == 2 ? 3.0 / 8.0 : 1.0 / 4.0; }
template <class F>
POST_DEV void dn_for_taps(uint32_t x, uint32_t y, uint32_t s, uint32_t width, uint32_t height, F f) {
    const int64_t W = width, H = height, step = s;
#pragma unroll
    for (int j = -2; j <= 2; j++) {
        const int64_t qy = (int64_t)y + (int64_t)j * step;
#pragma unroll
        for (int i = -2; i <= 2; i++) {
            const int64_t qx = (int64_t)x + (int64_t)i * step;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            f(dn_h(j + 2) * dn_h(i + 2), (uint64_t)qy * width + (uint64_t)qx);
        }
    }
}

} // namespace rt2022
#endif
