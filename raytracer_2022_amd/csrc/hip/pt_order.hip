// pt_order.hip — the kernels behind rt_ray_order* and the two moves of rt_intersect_ordered* (include/rt2022.h has the
// definition of the key; DESIGN.md §4.16 the reasoning). All arithmetic is f64, -ffp-contract=off.
//
//   order_box_partial, order_box_final   the box of the non-stragglers' origins (two stages, no atomics)
//   order_keys                           the key of every ray, value = the ray's index
//   rocprim::radix_sort_pairs            stable: equal keys keep index order, so the order is (key, index)
//   order_gather, order_scatter          rays into working order, hit records back: whole 16-byte pieces, one lane a piece
//
// The key the sort sees differs from the header's in one bit: a straggler's is 1 << key_bits instead of 1 << 63, key_bits
// being the bits the parameters use (at most 63). The order is the same, and the sort runs over key_bits + 1 bits, not 64.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "pt_order.hpp"

namespace rt2022 {

namespace {

constexpr int kOrderBlock = 256;
constexpr int kRayPieces = sizeof(rt_query_ray) / 16, kHitPieces = sizeof(rt_hit) / 16;

#define ORDER_DEV __device__ __forceinline__

struct OrderRay {
    double o[3], d[3];
    bool straggler;
};

// Origin and direction of ray i (three 16-byte loads), and whether it is keyed at all.
ORDER_DEV OrderRay order_load(const char *rays, uint32_t stride, uint64_t i) {
    const double2 *q = reinterpret_cast<const double2 *>(rays + i * stride);
    const double2 w0 = q[0], w1 = q[1], w2 = q[2];
    OrderRay r;
    r.o[0] = w0.x; r.o[1] = w0.y; r.o[2] = w1.x; r.d[0] = w1.y; r.d[1] = w2.x; r.d[2] = w2.y;
    bool ok = r.d[0] != 0.0 || r.d[1] != 0.0 || r.d[2] != 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++)        // (NaN fails every comparison)
        ok = ok && fabs(r.o[a]) <= kOrderMaxCoord && fabs(r.d[a]) < __builtin_inf();
    r.straggler = !ok;
    return r;
}

ORDER_DEV double order_min(double l, double r) { return r < l ? r : l; }      // (ties and signed zeros: the left operand)
ORDER_DEV double order_max(double l, double r) { return r > l ? r : l; }

ORDER_DEV void order_merge(OrderBox &s, const OrderBox &o) {
#pragma unroll
    for (int a = 0; a < 3; a++) { s.lo[a] = order_min(s.lo[a], o.lo[a]); s.hi[a] = order_max(s.hi[a], o.hi[a]); }
}

ORDER_DEV OrderBox order_empty_box() {
    OrderBox s;
    for (int a = 0; a < 3; a++) { s.lo[a] = __builtin_inf(); s.hi[a] = -__builtin_inf(); }
    return s;
}

// The block's box into *out (thread 0 writes it): lanes by shuffles, the four waves through LDS.
ORDER_DEV void order_block_box(OrderBox s, OrderBox *out) {
    __shared__ OrderBox part[kOrderBlock / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        OrderBox o = s;
#pragma unroll
        for (int a = 0; a < 3; a++) { o.lo[a] = __shfl_xor(s.lo[a], d); o.hi[a] = __shfl_xor(s.hi[a], d); }
        order_merge(s, o);
    }
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        OrderBox t = part[0];
        for (int w = 1; w < kOrderBlock / 64; w++) order_merge(t, part[w]);
        *out = t;
    }
}

// A grid-stride loop under a grid of at most kOrderReduceBlocks blocks: a thread reads a second ray from
// kOrderReduceBlocks * 256 + 1 rays on.
__global__ void __launch_bounds__(kOrderBlock) order_box_partial(const char *rays, uint32_t stride, uint64_t n, OrderBox *partials) {
    OrderBox s = order_empty_box();
    for (uint64_t i = (uint64_t)blockIdx.x * kOrderBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kOrderBlock) {
        const OrderRay r = order_load(rays, stride, i);
        if (r.straggler) continue;
#pragma unroll
        for (int a = 0; a < 3; a++) { s.lo[a] = order_min(s.lo[a], r.o[a]); s.hi[a] = order_max(s.hi[a], r.o[a]); }
    }
    order_block_box(s, partials + blockIdx.x);
}

__global__ void __launch_bounds__(kOrderBlock) order_box_final(const OrderBox *partials, uint32_t n_partials, OrderBox *box) {
    OrderBox s = order_empty_box();
    for (uint32_t i = threadIdx.x; i < n_partials; i += kOrderBlock) order_merge(s, partials[i]);
    order_block_box(s, box);
}

// 21 bits to every third bit of 63 (the builder's).
ORDER_DEV uint64_t order_spread3(uint32_t k) {
    uint64_t x = k & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// 8 bits to every second bit of 16.
ORDER_DEV uint32_t order_spread2(uint32_t k) {
    uint32_t x = k & 0xFFu;
    x = (x | (x << 4)) & 0x0F0Fu;
    x = (x | (x << 2)) & 0x3333u;
    x = (x | (x << 1)) & 0x5555u;
    return x;
}

// (uint32) min(x * scale, top), x * scale >= 0.
ORDER_DEV uint32_t order_cell(double x, double scale, double top) {
    const double s = x * scale;
    return (uint32_t)(s < top ? s : top);
}

__global__ void __launch_bounds__(kOrderBlock) order_keys(const char *rays, const rt_ray_order_params p, uint64_t n, const OrderBox *box,
                                                          uint64_t *keys, uint32_t *idx) {
    const uint64_t i = (uint64_t)blockIdx.x * kOrderBlock + threadIdx.x;
    if (i >= n) return;
    const OrderRay r = order_load(rays, p.ray_stride, i);
    const uint32_t ob = p.origin_bits, db = p.dir_bits;
    uint64_t key = 1ull << (3u * ob + 3u + 2u * db);           // a straggler's, one bit above every other key
    if (!r.straggler) {
        const double o_scale = (double)(1u << ob), o_top = (double)((1u << ob) - 1u);
        uint32_t k[3];
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double lo = box->lo[a], e = box->hi[a] - lo;
            const double q = e > 0.0 ? (r.o[a] - lo) / e : 0.0;
            k[a] = order_cell(q, o_scale, o_top);
        }
        const uint64_t O = (order_spread3(k[0]) << 2) | (order_spread3(k[1]) << 1) | order_spread3(k[2]);
        // The first axis of largest |d|, the two that follow it cyclically.
        const double ax = fabs(r.d[0]), ay = fabs(r.d[1]), az = fabs(r.d[2]);
        uint32_t a = 0;
        double m = ax, da = r.d[0], d1 = r.d[1], d2 = r.d[2];
        if (ay > m) { a = 1; m = ay; da = r.d[1]; d1 = r.d[2]; d2 = r.d[0]; }
        if (az > m) { a = 2; m = az; da = r.d[2]; d1 = r.d[0]; d2 = r.d[1]; }
        const uint64_t face = 2u * a + (da < 0.0 ? 1u : 0u);
        const double d_scale = 0.5 * (double)(1u << db), d_top = (double)((1u << db) - 1u);
        const uint32_t k1 = order_cell(d1 / m + 1.0, d_scale, d_top), k2 = order_cell(d2 / m + 1.0, d_scale, d_top);
        const uint64_t uv = (order_spread2(k1) << 1) | order_spread2(k2);
        const uint64_t D = (face << (2u * db)) | uv;
        key = p.layout == RT_ORDER_ORIGIN_FIRST      ? (O << (3u + 2u * db)) | D
              : p.layout == RT_ORDER_DIRECTION_FIRST ? (D << (3u * ob)) | O
                                                     : (face << (3u * ob + 2u * db)) | (O << (2u * db)) | uv;
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

// Piece `piece` of an inert ray: origin 0, direction (1, 1, 1), the window (0, -1) — t_max < t_min, nothing is ever accepted,
// and every slab test is finite, so the walk ends at the first box.
ORDER_DEV double2 order_inert_piece(uint32_t piece) {
    switch (piece) {
        case 1: return make_double2(0.0, 1.0);             // {o.z, d.x}
        case 2: return make_double2(1.0, 1.0);             // {d.y, d.z}
        case 4: return make_double2(-1.0, 0.0);            // {t_max, rng_state}
        default: return make_double2(0.0, 0.0);            // {o.x, o.y}, {time, t_min}
    }
}

// One lane a 16-byte piece: lane t moves piece t % 5 of work item t / 5.
template <bool COUNT>
__global__ void __launch_bounds__(kOrderBlock) order_gather(const rt_query_ray *rays, const uint32_t *order, uint64_t n, rt_query_ray *gathered,
                                                            unsigned long long *valid) {
    const uint64_t t = (uint64_t)blockIdx.x * kOrderBlock + threadIdx.x;
    const bool live = t < n * kRayPieces;
    const uint64_t w = t / kRayPieces;
    const uint32_t piece = (uint32_t)(t % kRayPieces);
    const uint64_t src = live ? order[w] : n;
    const bool named = src < n;                            // (an entry >= n is never used as an address)
    if (live) {
        const double2 v = named ? reinterpret_cast<const double2 *>(rays + src)[piece] : order_inert_piece(piece);
        reinterpret_cast<double2 *>(gathered + w)[piece] = v;
    }
    if (COUNT) {
        const int c = __popcll(__ballot(named && piece == 0));
        if ((threadIdx.x & 63u) == 0 && c) atomicAdd(valid, (unsigned long long)c);
    }
}

// ... and lane t piece t % 6 of record t / 6.
__global__ void __launch_bounds__(kOrderBlock) order_scatter(const rt_hit *gathered, const uint32_t *order, uint64_t n, rt_hit *hits) {
    const uint64_t t = (uint64_t)blockIdx.x * kOrderBlock + threadIdx.x;
    if (t >= n * kHitPieces) return;
    const uint64_t w = t / kHitPieces;
    const uint32_t piece = (uint32_t)(t % kHitPieces);
    const uint64_t dst = order[w];
    if (dst < n) reinterpret_cast<double2 *>(hits + dst)[piece] = reinterpret_cast<const double2 *>(gathered + w)[piece];
}

template <class T>
T *at(const OrderArgs &a, uint64_t offset) { return reinterpret_cast<T *>(a.ws + offset); }

uint32_t blocks_for(uint64_t items) { return (uint32_t)((items + kOrderBlock - 1) / kOrderBlock); }

} // namespace

void launch_ray_order(const OrderArgs &a, hipStream_t stream) {
    const OrderLayout l = order_layout(a.n);
    uint64_t *keys_in = at<uint64_t>(a, l.keys_in), *keys_out = at<uint64_t>(a, l.keys_out);
    uint32_t *idx_in = at<uint32_t>(a, l.idx_in);
    const unsigned end_bit = order_key_bits(a.p) + 1u;
    size_t tmp_bytes = 0;
    RT_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in, keys_out, idx_in, a.order, (size_t)a.n, 0u, end_bit, stream));
    RT_REQUIRE(tmp_bytes <= l.sort_tmp_bytes, RT_ERR_DEVICE, "rt_ray_order: the sort needs more temporary storage than the workspace sets aside");
    const uint32_t blocks = blocks_for(a.n) < kOrderReduceBlocks ? blocks_for(a.n) : kOrderReduceBlocks;
    hipLaunchKernelGGL(order_box_partial, dim3(blocks), dim3(kOrderBlock), 0, stream, a.rays, a.p.ray_stride, a.n, at<OrderBox>(a, l.partials));
    hipLaunchKernelGGL(order_box_final, dim3(1), dim3(kOrderBlock), 0, stream, at<const OrderBox>(a, l.partials), blocks, at<OrderBox>(a, l.box));
    hipLaunchKernelGGL(order_keys, dim3(blocks_for(a.n)), dim3(kOrderBlock), 0, stream, a.rays, a.p, a.n, at<const OrderBox>(a, l.box), keys_in, idx_in);
    RT_HIP(hipGetLastError());
    tmp_bytes = l.sort_tmp_bytes;
    RT_HIP(rocprim::radix_sort_pairs(a.ws + l.sort_tmp, tmp_bytes, keys_in, keys_out, idx_in, a.order, (size_t)a.n, 0u, end_bit, stream));
}

hipError_t launch_order_gather(const rt_query_ray *rays, const uint32_t *order, uint64_t n, rt_query_ray *gathered, unsigned long long *valid,
                               hipStream_t stream) {
    const dim3 grid(blocks_for(n * kRayPieces)), block(kOrderBlock);
    if (valid) hipLaunchKernelGGL(order_gather<true>, grid, block, 0, stream, rays, order, n, gathered, valid);
    else hipLaunchKernelGGL(order_gather<false>, grid, block, 0, stream, rays, order, n, gathered, valid);
    return hipGetLastError();
}

hipError_t launch_order_scatter(const rt_hit *gathered, const uint32_t *order, uint64_t n, rt_hit *hits, hipStream_t stream) {
    hipLaunchKernelGGL(order_scatter, dim3(blocks_for(n * kHitPieces)), dim3(kOrderBlock), 0, stream, gathered, order, n, hits);
    return hipGetLastError();
}

} // namespace rt2022
