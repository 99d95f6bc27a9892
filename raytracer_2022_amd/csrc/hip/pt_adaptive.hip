// pt_adaptive.hip — the sample planner of per-pixel adaptive sampling (rt_adaptive_*, include/rt2022.h has the definition:
// every * / + below is one of its operations, in its order; -ffp-contract=off), and the merge and resolve of its sums.
//
// A plan turns an error map into a list of (frame, pixel) ids for rt_render_pixels*: pixel b gets units[b] entries, one per
// unit of `spp` samples, at offsets[b] of the list — an exclusive prefix sum of the units over the image. The scan is the one
// kernel here that is more than a lane per pixel. It takes three launches on the caller's workspace (adaptive_layout of
// host/post_check.hpp; a row list has been through the row kernel of pt_rows.hip before them, its count is beside the totals):
//   ad_totals   a workgroup per tile of kAdTile pixels: the tile's units, summed, into totals[tile]
//   ad_offsets  ONE workgroup: the exclusive scan of the tile totals in place, kAdBlock at a time with a running carry,
//               and the grand total behind them
//   ad_emit     a workgroup per tile again: the units once more (one load and one multiply: cheaper than a plane of them
//               read back), their exclusive scan inside the tile on top of the tile's offset, then units, offsets and — if
//               the list fits the caller's capacity and the row list was good — the entries
// Inside a workgroup: a thread owns kAdPer consecutive pixels and adds them up serially; the thread sums are scanned by
// __shfl_up inside each wave64 and the four wave sums through LDS. No workgroup ever waits on another: the order of the
// three launches on the stream is the only dependence between tiles. (A single-pass scan with look-back would save the second
// read of the error map — 8 B per pixel, microseconds beside the render the plan feeds — and would spin on other workgroups'
// progress, which nothing on a shared device guarantees.)
//   ad_merge    a lane per pixel: the pixel's units of entry sums, added to its accumulator in entry order
//   ad_resolve  a lane per pixel: accumulator -> sums of spp_out samples
//   ad_merge_features / ad_resolve_features  the same two for rt_feature records: eight doubles a pixel, moved as four
//               16-byte pieces, every field linear (the sample count is the radiance merge's acc_n)
#include "../host/post_check.hpp"
#include "pt_device.h"

namespace rt2022 {

namespace {

constexpr int kAdBlock = 256;          // 4 waves
constexpr int kAdPer = 4;              // consecutive pixels per thread
constexpr uint32_t kAdTile = kAdBlock * kAdPer;
static_assert(kAdTile == kAdaptiveTile, "the layout's tiles (host/post_check.hpp) are the scan's");

#define AD_DEV __device__ __forceinline__

// units of one pixel: !(t >= 1) -> 0 (NaN and negatives included), t >= max_units -> max_units (+inf included), else trunc(t)
AD_DEV uint32_t ad_units(double err, double scale, uint32_t max_units) {
    const double t = err * scale;
    if (!(t >= 1.0)) return 0u;
    return t >= (double)max_units ? max_units : (uint32_t)t;
}

// Inclusive scan of v over the workgroup's kAdBlock threads; `total` = the workgroup's sum. (wave_sums: kAdBlock / 64 words of LDS.)
AD_DEV unsigned long long ad_block_scan(unsigned long long v, unsigned long long *wave_sums, unsigned long long &total) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(v, d);
        if (lane >= (unsigned)d) v += o;
    }
    __syncthreads();                   // (the words may still be read by the previous call's last step)
    if (lane == 63u) wave_sums[wave] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (unsigned w = 0; w < (unsigned)kAdBlock / 64u; w++) {
        const unsigned long long s = wave_sums[w];
        if (w < wave) before += s;
        all += s;
    }
    total = all;
    return v + before;
}

__global__ void __launch_bounds__(kAdBlock) ad_totals(const double *err, uint64_t n, double scale, uint32_t max_units, unsigned long long *totals) {
    __shared__ unsigned long long wave_sums[kAdBlock / 64];
    const uint64_t first = (uint64_t)blockIdx.x * kAdTile + (uint64_t)threadIdx.x * kAdPer;
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < kAdPer; k++)
        if (first + k < n) mine += ad_units(err[first + k], scale, max_units);
    unsigned long long total;
    (void)ad_block_scan(mine, wave_sums, total);
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// totals[0 .. n_tiles) -> their exclusive scan; totals[n_tiles] = the grand total.
__global__ void __launch_bounds__(kAdBlock) ad_offsets(unsigned long long *totals, uint64_t n_tiles) {
    __shared__ unsigned long long wave_sums[kAdBlock / 64];
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < n_tiles; base += kAdBlock) {
        const uint64_t i = base + threadIdx.x;
        const unsigned long long v = i < n_tiles ? totals[i] : 0ull;
        unsigned long long total;
        const unsigned long long incl = ad_block_scan(v, wave_sums, total);
        if (i < n_tiles) totals[i] = carry + (incl - v);
        carry += total;
    }
    if (threadIdx.x == 0) totals[n_tiles] = carry;
}

struct AdEmit {
    const double *err;
    const uint32_t *rows;              // buffer row -> image row (null: the identity)
    const uint32_t *bad_rows;          // the row kernel's count (null with null rows)
    const unsigned long long *totals;  // [n_tiles] tile offsets, [n_tiles] the total
    uint64_t n, n_tiles, capacity;
    uint32_t width, first_frame, max_units;
    uint64_t image_pixels;             // width * height
    double scale;
    uint32_t *units;
    uint64_t *offsets, *entries;
};

__global__ void __launch_bounds__(kAdBlock) ad_emit(const AdEmit a) {
    __shared__ unsigned long long wave_sums[kAdBlock / 64];
    const uint64_t first = (uint64_t)blockIdx.x * kAdTile + (uint64_t)threadIdx.x * kAdPer;
    uint32_t u[kAdPer];
    unsigned long long mine = 0;
#pragma unroll
    for (int k = 0; k < kAdPer; k++) {
        u[k] = first + k < a.n ? ad_units(a.err[first + k], a.scale, a.max_units) : 0u;
        mine += u[k];
    }
    unsigned long long tile_total;
    const unsigned long long incl = ad_block_scan(mine, wave_sums, tile_total);
    if (a.bad_rows && *a.bad_rows) return;                        // (a list that is no permutation: the call fails, nothing is written)
    const unsigned long long total = a.totals[a.n_tiles];
    const bool fits = total <= a.capacity;
    unsigned long long at = a.totals[blockIdx.x] + (incl - mine);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.offsets[a.n] = total;
#pragma unroll
    for (int k = 0; k < kAdPer; k++) {
        const uint64_t b = first + k;
        if (b >= a.n) break;
        a.units[b] = u[k];
        a.offsets[b] = at;
        if (fits && u[k]) {
            const uint64_t r = b / a.width, x = b - r * a.width;
            const uint64_t pixel = (uint64_t)(a.rows ? a.rows[r] : (uint32_t)r) * a.width + x;
            for (uint32_t j = 0; j < u[k]; j++) a.entries[at + j] = (uint64_t)(a.first_frame + j) * a.image_pixels + pixel;
        }
        at += u[k];
    }
}

__global__ void __launch_bounds__(kAdBlock) ad_merge(const double *sums, const uint32_t *units, const uint64_t *offsets, uint64_t n, uint32_t spp,
                                                     double *acc, double *acc_n) {
    const uint64_t b = (uint64_t)blockIdx.x * kAdBlock + threadIdx.x;
    if (b >= n) return;
    const uint32_t u = units[b];
    if (!u) return;
    const double *e = sums + offsets[b] * 3;
    double c0 = acc[3 * b], c1 = acc[3 * b + 1], c2 = acc[3 * b + 2];
    for (uint32_t k = 0; k < u; k++) { c0 = c0 + e[3 * k]; c1 = c1 + e[3 * k + 1]; c2 = c2 + e[3 * k + 2]; }
    acc[3 * b] = c0; acc[3 * b + 1] = c1; acc[3 * b + 2] = c2;
    acc_n[b] = acc_n[b] + (double)((uint64_t)u * spp);
}

__global__ void __launch_bounds__(kAdBlock) ad_resolve(const double *acc, const double *acc_n, uint64_t n, double spp_out, double *out) {
    const uint64_t b = (uint64_t)blockIdx.x * kAdBlock + threadIdx.x;
    if (b >= n) return;
    const double d = acc_n[b];
    const double c0 = acc[3 * b], c1 = acc[3 * b + 1], c2 = acc[3 * b + 2];       // (out may be acc)
    out[3 * b] = (c0 / d) * spp_out; out[3 * b + 1] = (c1 / d) * spp_out; out[3 * b + 2] = (c2 / d) * spp_out;
}

// A pixel's units of entry records, added field by field to its accumulated record in entry order.
__global__ void __launch_bounds__(kAdBlock) ad_merge_features(const double2 *entries, const uint32_t *units, const uint64_t *offsets, uint64_t n,
                                                              double2 *acc) {
    const uint64_t b = (uint64_t)blockIdx.x * kAdBlock + threadIdx.x;
    if (b >= n) return;
    const uint32_t u = units[b];
    if (!u) return;
    const double2 *e = entries + offsets[b] * 4;
    double2 *c = acc + b * 4;
    double2 c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
    for (uint32_t k = 0; k < u; k++) {
        const double2 e0 = e[4 * k], e1 = e[4 * k + 1], e2 = e[4 * k + 2], e3 = e[4 * k + 3];
        c0 = make_double2(c0.x + e0.x, c0.y + e0.y);
        c1 = make_double2(c1.x + e1.x, c1.y + e1.y);
        c2 = make_double2(c2.x + e2.x, c2.y + e2.y);
        c3 = make_double2(c3.x + e3.x, c3.y + e3.y);
    }
    c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
}

// Accumulated record -> sums of spp_out samples: (acc / acc_n) * spp_out on all eight fields.
__global__ void __launch_bounds__(kAdBlock) ad_resolve_features(const double2 *acc, const double *acc_n, uint64_t n, double spp_out, double2 *out) {
    const uint64_t b = (uint64_t)blockIdx.x * kAdBlock + threadIdx.x;
    if (b >= n) return;
    const double d = acc_n[b];
    const double2 c0 = acc[4 * b], c1 = acc[4 * b + 1], c2 = acc[4 * b + 2], c3 = acc[4 * b + 3];       // (out may be acc)
    out[4 * b] = make_double2((c0.x / d) * spp_out, (c0.y / d) * spp_out);
    out[4 * b + 1] = make_double2((c1.x / d) * spp_out, (c1.y / d) * spp_out);
    out[4 * b + 2] = make_double2((c2.x / d) * spp_out, (c2.y / d) * spp_out);
    out[4 * b + 3] = make_double2((c3.x / d) * spp_out, (c3.y / d) * spp_out);
}

} // namespace

hipError_t launch_adaptive_plan(const AdaptivePlanArgs &p, hipStream_t stream) {
    const AdaptiveLayout l = adaptive_layout(p.width, p.height);
    const uint64_t n = (uint64_t)p.width * p.height;
    unsigned long long *const totals = reinterpret_cast<unsigned long long *>(p.ws + l.totals);
    const uint32_t *const bad = reinterpret_cast<const uint32_t *>(p.ws + l.rows.bad);
    hipError_t e;
    hipLaunchKernelGGL(ad_totals, dim3((unsigned)l.n_tiles), dim3(kAdBlock), 0, stream, p.err, n, p.scale, p.max_units, totals);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(ad_offsets, dim3(1), dim3(kAdBlock), 0, stream, totals, l.n_tiles);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    AdEmit a{};
    a.err = p.err; a.rows = p.rows; a.bad_rows = p.rows ? bad : nullptr; a.totals = totals;
    a.n = n; a.n_tiles = l.n_tiles; a.capacity = p.capacity;
    a.width = p.width; a.first_frame = p.first_frame; a.max_units = p.max_units; a.image_pixels = n; a.scale = p.scale;
    a.units = p.units; a.offsets = p.offsets; a.entries = p.entries;
    hipLaunchKernelGGL(ad_emit, dim3((unsigned)l.n_tiles), dim3(kAdBlock), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_adaptive_merge(const double *sums, const uint32_t *units, const uint64_t *offsets, uint64_t n, uint32_t spp, double *acc,
                                 double *acc_n, hipStream_t stream) {
    hipLaunchKernelGGL(ad_merge, dim3((unsigned)((n + kAdBlock - 1) / kAdBlock)), dim3(kAdBlock), 0, stream, sums, units, offsets, n, spp, acc, acc_n);
    return hipGetLastError();
}

hipError_t launch_adaptive_resolve(const double *acc, const double *acc_n, uint64_t n, uint32_t spp_out, double *out, hipStream_t stream) {
    hipLaunchKernelGGL(ad_resolve, dim3((unsigned)((n + kAdBlock - 1) / kAdBlock)), dim3(kAdBlock), 0, stream, acc, acc_n, n, (double)spp_out, out);
    return hipGetLastError();
}

hipError_t launch_adaptive_merge_features(const rt_feature *entries, const uint32_t *units, const uint64_t *offsets, uint64_t n, rt_feature *acc,
                                          hipStream_t stream) {
    hipLaunchKernelGGL(ad_merge_features, dim3((unsigned)((n + kAdBlock - 1) / kAdBlock)), dim3(kAdBlock), 0, stream,
                       reinterpret_cast<const double2 *>(entries), units, offsets, n, reinterpret_cast<double2 *>(acc));
    return hipGetLastError();
}

hipError_t launch_adaptive_resolve_features(const rt_feature *acc, const double *acc_n, uint64_t n, uint32_t spp_out, rt_feature *out,
                                            hipStream_t stream) {
    hipLaunchKernelGGL(ad_resolve_features, dim3((unsigned)((n + kAdBlock - 1) / kAdBlock)), dim3(kAdBlock), 0, stream,
                       reinterpret_cast<const double2 *>(acc), acc_n, n, (double)spp_out, reinterpret_cast<double2 *>(out));
    return hipGetLastError();
}

} // namespace rt2022
