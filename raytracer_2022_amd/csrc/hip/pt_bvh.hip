// pt_bvh.hip — the device BVH builder behind rt_bvh_build* (include/rt2022.h has the definition; DESIGN.md §4.15 the
// reasoning): a linear BVH — Morton order of the leaf boxes' centres, Karras' radix tree over the sorted keys (one thread per
// internal node, "Maximizing Parallelism in the Construction of BVHs, Octrees, and k-d Trees", HPG 2012), one bottom-up pass
// for the boxes, the stack needs and the child order. All arithmetic is f64, -ffp-contract=off.
//
//   bvh_box_partial, bvh_box_final   scene box + count of refused boxes (two stages, no atomics); nothing but workspace
//   bvh_keys                         63-bit Morton key per leaf, value = the leaf's index
//   rocprim::radix_sort_pairs        stable: equal keys keep index order, so the order is (key, index)
//   bvh_tree                         split position and parent links of every internal node
//   bvh_fit                          one thread per leaf walks up; the second thread to arrive at a node builds its record
//
// Node j of the radix tree is record j of the output whichever way its children are ordered; a record is written once, whole,
// as four 16-byte stores, by the thread that arrived second at it.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "pt_bvh.hpp"

namespace rt2022 {

namespace {

constexpr int kBvhBlock = 256;
constexpr uint32_t kLeftLeaf = 0x80000000u, kRightLeaf = 0x40000000u, kSplitMask = 0x3FFFFFFFu;

#define BVH_DEV __device__ __forceinline__

BVH_DEV double bvh_min(double l, double r) { return r < l ? r : l; }      // (ties and signed zeros: the left operand)
BVH_DEV double bvh_max(double l, double r) { return r > l ? r : l; }

BVH_DEV void bvh_merge(BvhBoxSum &s, const BvhBoxSum &o) {
#pragma unroll
    for (int a = 0; a < 3; a++) { s.lo[a] = bvh_min(s.lo[a], o.lo[a]); s.hi[a] = bvh_max(s.hi[a], o.hi[a]); }
    s.bad += o.bad;
}

// The block's sum into *out (thread 0 writes it): lanes by shuffles, the four waves through LDS.
BVH_DEV void bvh_block_sum(BvhBoxSum s, BvhBoxSum *out) {
    __shared__ BvhBoxSum part[kBvhBlock / 64];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        BvhBoxSum o;
#pragma unroll
        for (int a = 0; a < 3; a++) { o.lo[a] = __shfl_xor(s.lo[a], d); o.hi[a] = __shfl_xor(s.hi[a], d); }
        o.bad = __shfl_xor(s.bad, d);
        bvh_merge(s, o);
    }
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        BvhBoxSum t = part[0];
        for (int w = 1; w < kBvhBlock / 64; w++) bvh_merge(t, part[w]);
        t._pad = 0;
        *out = t;
    }
}

BVH_DEV BvhBoxSum bvh_empty_sum() {
    BvhBoxSum s;
    for (int a = 0; a < 3; a++) { s.lo[a] = __builtin_inf(); s.hi[a] = -__builtin_inf(); }
    s.bad = 0; s._pad = 0;
    return s;
}

__global__ void __launch_bounds__(kBvhBlock) bvh_box_partial(const double *boxes, uint32_t n, BvhBoxSum *partials) {
    BvhBoxSum s = bvh_empty_sum();
    for (uint64_t i = (uint64_t)blockIdx.x * kBvhBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBvhBlock) {
        const double *b = boxes + 6u * i;
        bool ok = true;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const double lo = b[a], hi = b[3 + a];
            // (NaN fails every comparison: refused with the infinities and whatever lies beyond the limit)
            ok = ok && fabs(lo) <= kBvhMaxCoord && fabs(hi) <= kBvhMaxCoord && lo <= hi;
            s.lo[a] = bvh_min(s.lo[a], lo);
            s.hi[a] = bvh_max(s.hi[a], hi);
        }
        s.bad += ok ? 0u : 1u;
    }
    bvh_block_sum(s, partials + blockIdx.x);
}

__global__ void __launch_bounds__(kBvhBlock) bvh_box_final(const BvhBoxSum *partials, uint32_t n_partials, BvhBoxSum *status) {
    BvhBoxSum s = bvh_empty_sum();
    for (uint32_t i = threadIdx.x; i < n_partials; i += kBvhBlock) bvh_merge(s, partials[i]);
    bvh_block_sum(s, status);
}

// 21 bits to every third bit of 63.
BVH_DEV uint64_t bvh_spread(uint32_t k) {
    uint64_t x = k & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

__global__ void __launch_bounds__(kBvhBlock) bvh_keys(const double *boxes, uint32_t n, const BvhBoxSum *status, uint64_t *keys, uint32_t *idx) {
    const uint64_t i = (uint64_t)blockIdx.x * kBvhBlock + threadIdx.x;
    if (i >= n) return;
    const double *b = boxes + 6u * i;
    uint32_t k[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = status->lo[a], hi = status->hi[a];
        const double c = 0.5 * (b[a] + b[3 + a]);
        const double e = hi - lo;
        const double q = e > 0.0 ? (c - lo) / e : 0.0;
        const double s = q * 2097152.0;
        k[a] = (uint32_t)(s < 2097151.0 ? s : 2097151.0);
    }
    keys[i] = (bvh_spread(k[0]) << 2) | (bvh_spread(k[1]) << 1) | bvh_spread(k[2]);
    idx[i] = (uint32_t)i;
}

// Length of the common prefix of the 96-bit keys (key << 32 | index) at sorted positions i (given) and j; -1 outside the range.
BVH_DEV int bvh_delta(const uint64_t *keys, const uint32_t *idx, int64_t n, uint64_t ki, uint32_t ii, int64_t j) {
    if (j < 0 || j >= n) return -1;
    const uint64_t kj = keys[j];
    if (kj != ki) return __clzll((long long)(ki ^ kj));
    return 64 + __clz((int)(ii ^ idx[j]));
}

// Karras 2012, one thread per internal node i in [0, n - 1): the range of keys it covers, its split, the links of its children.
__global__ void __launch_bounds__(kBvhBlock) bvh_tree(const uint64_t *keys, const uint32_t *idx, uint32_t n_leaves, uint32_t *split,
                                                      uint32_t *parent, uint32_t *leaf_parent) {
    const int64_t i = (int64_t)blockIdx.x * kBvhBlock + threadIdx.x, n = n_leaves;
    if (i >= n - 1) return;
    const uint64_t ki = keys[i];
    const uint32_t ii = idx[i];
    const int64_t d = bvh_delta(keys, idx, n, ki, ii, i + 1) > bvh_delta(keys, idx, n, ki, ii, i - 1) ? 1 : -1;
    const int dmin = bvh_delta(keys, idx, n, ki, ii, i - d);
    int64_t lmax = 2;
    while (bvh_delta(keys, idx, n, ki, ii, i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (bvh_delta(keys, idx, n, ki, ii, i + (l + t) * d) > dmin) l += t;
    const int64_t j = i + l * d;
    const int dnode = bvh_delta(keys, idx, n, ki, ii, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (bvh_delta(keys, idx, n, ki, ii, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = i + s * d + (d < 0 ? -1 : 0);            // children: [min(i, j), g] and [g + 1, max(i, j)]
    const int64_t first = d > 0 ? i : j, last = d > 0 ? j : i;
    uint32_t word = (uint32_t)g;
    if (first == g) { word |= kLeftLeaf; leaf_parent[g] = (uint32_t)i; } else parent[g] = (uint32_t)i;
    if (last == g + 1) { word |= kRightLeaf; leaf_parent[g + 1] = (uint32_t)i; } else parent[g + 1] = (uint32_t)i;
    split[i] = word;
}

struct BvhChild {
    double lo[3], hi[3];
    uint32_t ref, need;
};

// A child of a node the calling thread arrived second at: a leaf's box comes from the caller's array, an internal node's
// from its record, written by another thread before its arrival (read only behind the acquire of the arrival counter).
BVH_DEV BvhChild bvh_child(bool leaf, uint32_t pos, const uint32_t *refs, const double *boxes, const uint32_t *order, const rt_bvh_node *out,
                           const uint32_t *need, uint32_t node_base) {
    BvhChild c;
    if (leaf) {
        const uint32_t src = order[pos];
        const double *b = boxes + 6u * (uint64_t)src;
#pragma unroll
        for (int a = 0; a < 3; a++) { c.lo[a] = b[a]; c.hi[a] = b[3 + a]; }
        c.ref = refs[src];
        c.need = 1;
    } else {
        const double2 *r = reinterpret_cast<const double2 *>(out + pos);
        const double2 r0 = r[0], r1 = r[1], r2 = r[2];
        c.lo[0] = r0.x; c.lo[1] = r0.y; c.lo[2] = r1.x; c.hi[0] = r1.y; c.hi[1] = r2.x; c.hi[2] = r2.y;
        c.ref = RT_MAKE_REF(RT_KIND_NODE, node_base + pos);
        c.need = need[pos];
    }
    return c;
}

BVH_DEV void bvh_store(rt_bvh_node *rec, const double lo[3], const double hi[3], uint32_t left, uint32_t right) {
    double2 *r = reinterpret_cast<double2 *>(rec);
    r[0] = make_double2(lo[0], lo[1]);
    r[1] = make_double2(lo[2], hi[0]);
    r[2] = make_double2(hi[1], hi[2]);
    reinterpret_cast<uint4 *>(rec)[3] = make_uint4(left, right, 0u, 0u);
}

// One thread per leaf (sorted position) walks towards the root. At every node it adds one to the node's arrival counter
// (acquire-release, agent scope): the first to arrive stops, the second finds both children complete and builds the record.
__global__ void __launch_bounds__(kBvhBlock) bvh_fit(const uint32_t *refs, const double *boxes, const uint32_t *order, uint32_t n_leaves,
                                                     uint32_t node_base, const uint32_t *split, const uint32_t *parent, const uint32_t *leaf_parent,
                                                     uint32_t *counters, uint32_t *need, rt_bvh_node *out) {
    const uint64_t p = (uint64_t)blockIdx.x * kBvhBlock + threadIdx.x;
    if (p >= n_leaves) return;
    uint32_t node = leaf_parent[p];
    for (;;) {
        if (node >= n_leaves - 1u) return;                      // (never: every link was written by bvh_tree; no address is made from a bad one)
        const uint32_t before = __hip_atomic_fetch_add(counters + node, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (before == 0) return;
        const uint32_t word = split[node], g = word & kSplitMask;
        const BvhChild l = bvh_child((word & kLeftLeaf) != 0, g, refs, boxes, order, out, need, node_base);
        const BvhChild r = bvh_child((word & kRightLeaf) != 0, g + 1u, refs, boxes, order, out, need, node_base);
        double lo[3], hi[3];
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = bvh_min(l.lo[a], r.lo[a]); hi[a] = bvh_max(l.hi[a], r.hi[a]); }
        // The child that needs more stack goes second (it is walked with nothing waiting): max(1 + first, second).
        const bool swap = l.need > r.need;
        const uint32_t first = swap ? r.need : l.need, second = swap ? l.need : r.need;
        bvh_store(out + node, lo, hi, swap ? r.ref : l.ref, swap ? l.ref : r.ref);
        need[node] = 1u + first > second ? 1u + first : second;
        if (node == 0) return;
        node = parent[node];
    }
}

// n_leaves == 1: the reference's span-1 node, both children the leaf, its box the leaf's.
__global__ void bvh_single(const uint32_t *refs, const double *boxes, rt_bvh_node *out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double lo[3] = {boxes[0], boxes[1], boxes[2]}, hi[3] = {boxes[3], boxes[4], boxes[5]};
    bvh_store(out, lo, hi, refs[0], refs[0]);
}

template <class T>
T *at(const BvhArgs &a, uint64_t offset) { return reinterpret_cast<T *>(a.ws + offset); }

uint32_t blocks_for(uint64_t items) { return (uint32_t)((items + kBvhBlock - 1) / kBvhBlock); }

} // namespace

hipError_t launch_bvh_check(const BvhArgs &a, hipStream_t stream) {
    const BvhLayout l = bvh_layout(a.n);
    const uint32_t blocks = blocks_for(a.n) < kBvhReduceBlocks ? blocks_for(a.n) : kBvhReduceBlocks;
    hipLaunchKernelGGL(bvh_box_partial, dim3(blocks), dim3(kBvhBlock), 0, stream, a.boxes, a.n, at<BvhBoxSum>(a, l.partials));
    hipLaunchKernelGGL(bvh_box_final, dim3(1), dim3(kBvhBlock), 0, stream, at<const BvhBoxSum>(a, l.partials), blocks, at<BvhBoxSum>(a, l.status));
    return hipGetLastError();
}

void launch_bvh_build(const BvhArgs &a, hipStream_t stream) {
    const BvhLayout l = bvh_layout(a.n);
    if (a.n == 1) {
        hipLaunchKernelGGL(bvh_single, dim3(1), dim3(64), 0, stream, a.refs, a.boxes, a.out);
        RT_HIP(hipGetLastError());
        return;
    }
    uint64_t *keys_in = at<uint64_t>(a, l.keys_in), *keys_out = at<uint64_t>(a, l.keys_out);
    uint32_t *idx_in = at<uint32_t>(a, l.idx_in), *idx_out = at<uint32_t>(a, l.idx_out);
    size_t tmp_bytes = 0;
    RT_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in, keys_out, idx_in, idx_out, (size_t)a.n, 0u, 63u, stream));
    RT_REQUIRE(tmp_bytes <= l.sort_tmp_bytes, RT_ERR_DEVICE, "rt_bvh_build: the sort needs more temporary storage than the workspace sets aside");
    RT_HIP(hipMemsetAsync(a.ws + l.counters, 0, bvh_align16((uint64_t)a.n * 4u), stream));
    hipLaunchKernelGGL(bvh_keys, dim3(blocks_for(a.n)), dim3(kBvhBlock), 0, stream, a.boxes, a.n, at<const BvhBoxSum>(a, l.status), keys_in, idx_in);
    RT_HIP(hipGetLastError());
    tmp_bytes = l.sort_tmp_bytes;
    RT_HIP(rocprim::radix_sort_pairs(a.ws + l.sort_tmp, tmp_bytes, keys_in, keys_out, idx_in, idx_out, (size_t)a.n, 0u, 63u, stream));
    uint32_t *split = at<uint32_t>(a, l.split), *parent = at<uint32_t>(a, l.parent), *leaf_parent = at<uint32_t>(a, l.leaf_parent);
    hipLaunchKernelGGL(bvh_tree, dim3(blocks_for(a.n - 1u)), dim3(kBvhBlock), 0, stream, keys_out, idx_out, a.n, split, parent, leaf_parent);
    RT_HIP(hipGetLastError());
    hipLaunchKernelGGL(bvh_fit, dim3(blocks_for(a.n)), dim3(kBvhBlock), 0, stream, a.refs, a.boxes, idx_out, a.n, a.node_base, split, parent,
                       leaf_parent, at<uint32_t>(a, l.counters), at<uint32_t>(a, l.need), a.out);
    RT_HIP(hipGetLastError());
}

} // namespace rt2022
