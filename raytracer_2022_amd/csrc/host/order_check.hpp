// order_check.hpp — what rt_ray_order* and rt_intersect_ordered* refuse before any device call, and the layouts of their
// workspaces. Pure arithmetic on the caller's words, no HIP: every refusal here is testable without a GPU.
#ifndef RT2022_ORDER_CHECK_HPP
#define RT2022_ORDER_CHECK_HPP
#include <cstdint>

#include "../../../include/rt2022.h"

namespace rt2022 {

constexpr uint32_t kOrderReduceBlocks = 1024;      // partial records of the origin-box reduction's first stage, at the most
constexpr uint32_t kOrderMaxOriginBits = 16, kOrderMaxDirBits = 6;
constexpr double kOrderMaxCoord = 1e300;           // |origin| limit of a ray that is keyed: hi - lo stays finite
constexpr uint64_t kOrderMaxRays = 1ull << 32;     // an order entry is 32 bits

// One record of the origin-box reduction (48 B): the union of the non-stragglers' origins so far.
struct OrderBox {
    double lo[3], hi[3];
};

inline uint64_t order_align16(uint64_t b) { return (b + 15u) / 16u * 16u; }

// rt_ray_order_device's workspace (byte offsets, each a multiple of 16). Nothing in it outlives the call.
struct OrderLayout {
    uint64_t box;                      // OrderBox: the origin box
    uint64_t partials;                 // kOrderReduceBlocks x OrderBox
    uint64_t keys_in, keys_out;        // n x uint64 each
    uint64_t idx_in;                   // n x uint32 (the sorted indices go straight to the caller's order buffer)
    uint64_t sort_tmp, sort_tmp_bytes; // the sort's own temporary storage
    uint64_t bytes;
};

inline OrderLayout order_layout(uint64_t n) {
    OrderLayout l;
    uint64_t at = 0;
    l.box = at; at += sizeof(OrderBox);
    l.partials = at; at += (uint64_t)kOrderReduceBlocks * sizeof(OrderBox);
    l.keys_in = at; at += order_align16(n * 8u);
    l.keys_out = at; at += order_align16(n * 8u);
    l.idx_in = at; at += order_align16(n * 4u);
    // As in bvh_layout: a second copy of keys and values (12 B a pair) and digit tables of a size the device's tuning decides;
    // 20 B a pair and 1 MiB bound both, and the call checks the sort's own figure.
    l.sort_tmp = at; l.sort_tmp_bytes = n * 20u + (1u << 20); at += order_align16(l.sort_tmp_bytes);
    l.bytes = at;
    return l;
}

// rt_intersect_ordered_device's workspace: the rays and the hit records in working order, and the count of valid entries.
struct OrderedLayout {
    uint64_t valid;                    // unsigned long long: order entries < n_rays (counted only for rt_stats)
    uint64_t rays;                     // n x rt_query_ray
    uint64_t hits;                     // n x rt_hit
    uint64_t bytes;
};

inline OrderedLayout ordered_layout(uint64_t n) {
    OrderedLayout l;
    l.valid = 0;
    l.rays = 16;
    l.hits = l.rays + n * sizeof(rt_query_ray);
    l.bytes = l.hits + n * sizeof(rt_hit);
    return l;
}

// Bits of the key below the stragglers' bit.
inline uint32_t order_key_bits(const rt_ray_order_params &p) { return 3u * p.origin_bits + 3u + 2u * p.dir_bits; }

// What is wrong with the sizes and parameters of an ordering call (null: nothing).
inline const char *order_params_fault(uint64_t n, const rt_ray_order_params *p) {
    if (n >= kOrderMaxRays) return "n_rays must be below 2^32 (an order entry is 32 bits)";
    if (!p) return "null params";
    if (p->origin_bits > kOrderMaxOriginBits) return "origin_bits above 16";
    if (p->dir_bits > kOrderMaxDirBits) return "dir_bits above 6";
    if (p->layout > RT_ORDER_FACE_ORIGIN_UV) return "unknown layout";
    if (p->ray_stride < 48u || (p->ray_stride & 15u)) return "ray_stride must be a multiple of 16, at least 48";
    return nullptr;
}

// ... and with the device buffers of a call that has a workspace (n > 0): `need` bytes of it, rays (and hits) in 16-byte
// pieces, 32-bit order entries. `hits` may be null where the call has none.
inline const char *order_buffers_fault(const void *rays, const void *order, const void *hits, bool has_hits, const void *workspace,
                                       uint64_t workspace_bytes, uint64_t need) {
    if (!rays || !order || (has_hits && !hits)) return has_hits ? "null ray, order or hit buffer" : "null ray or order buffer";
    if (!workspace) return "null workspace";
    if ((uintptr_t)workspace & 15u) return "the workspace must be 16-byte aligned";
    if (workspace_bytes < need) return "the workspace is smaller than its _workspace_bytes(n_rays)";
    if (((uintptr_t)rays | (uintptr_t)hits) & 15u) return has_hits ? "ray and hit buffers must be 16-byte aligned" : "the rays must be 16-byte aligned";
    if ((uintptr_t)order & 3u) return "the order buffer must be 4-byte aligned";
    return nullptr;
}

} // namespace rt2022
#endif
