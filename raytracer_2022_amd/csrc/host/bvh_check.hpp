// bvh_check.hpp — what rt_bvh_build* refuses before any device call, and the layout of its workspace. Pure arithmetic on the
// caller's words, no HIP: every refusal here is testable without a GPU.
#ifndef RT2022_BVH_CHECK_HPP
#define RT2022_BVH_CHECK_HPP
#include <cstdint>

#include "../../../include/rt2022.h"

namespace rt2022 {

constexpr uint32_t kBvhMaxNodes = 1u << 27;        // a node ref's index field (RT_REF_INDEX_MASK + 1)
constexpr uint32_t kBvhReduceBlocks = 1024;        // partial records of the scene-box reduction's first stage, at the most
constexpr double kBvhMaxCoord = 1e300;             // |coordinate| limit: min + max and max - min stay finite

// One record of the box reduction (64 B): the union so far and how many boxes were refused.
struct BvhBoxSum {
    double lo[3], hi[3];
    unsigned long long bad, _pad;
};

// The workspace (byte offsets, each a multiple of 16). `zeroed` .. `zeroed + zeroed_bytes` is cleared by every call.
struct BvhLayout {
    uint64_t status;                   // BvhBoxSum: the scene box and the count of refused boxes
    uint64_t partials;                 // kBvhReduceBlocks x BvhBoxSum
    uint64_t counters;                 // n x uint32: arrivals per internal node (cleared by every call)
    uint64_t need;                     // n x uint32: stack need per internal node
    uint64_t parent;                   // n x uint32: parent of internal node j
    uint64_t leaf_parent;              // n x uint32: parent of the leaf at sorted position p
    uint64_t split;                    // n x uint32: split position of internal node j, bit 31 / 30: left / right child is a leaf
    uint64_t keys_in, keys_out;        // n x uint64 each
    uint64_t idx_in, idx_out;          // n x uint32 each
    uint64_t sort_tmp, sort_tmp_bytes; // the sort's own temporary storage
    uint64_t bytes;
};

inline uint64_t bvh_align16(uint64_t b) { return (b + 15u) / 16u * 16u; }

inline BvhLayout bvh_layout(uint32_t n) {
    BvhLayout l;
    const uint64_t w4 = bvh_align16((uint64_t)n * 4u), w8 = bvh_align16((uint64_t)n * 8u);
    uint64_t at = 0;
    l.status = at; at += sizeof(BvhBoxSum);
    l.partials = at; at += (uint64_t)kBvhReduceBlocks * sizeof(BvhBoxSum);
    l.counters = at; at += w4;
    l.need = at; at += w4;
    l.parent = at; at += w4;
    l.leaf_parent = at; at += w4;
    l.split = at; at += w4;
    l.keys_in = at; at += w8;
    l.keys_out = at; at += w8;
    l.idx_in = at; at += w4;
    l.idx_out = at; at += w4;
    // The sort keeps a second copy of keys and values (12 B a pair) and per-block digit tables whose size depends on the
    // device's tuning; 20 B a pair and 1 MiB bound both with room to spare, and the call checks the sort's own figure.
    l.sort_tmp = at; l.sort_tmp_bytes = (uint64_t)n * 20u + (1u << 20); at += bvh_align16(l.sort_tmp_bytes);
    l.bytes = at;
    return l;
}

inline uint32_t bvh_node_count(uint32_t n) { return n > 1 ? n - 1 : 1; }

// What is wrong with the sizes of a build (null: nothing).
inline const char *bvh_sizes_fault(uint32_t n, uint32_t node_base) {
    if (n == 0) return "n_leaves is 0";
    if ((uint64_t)node_base + bvh_node_count(n) > kBvhMaxNodes) return "node_base + node count exceeds 2^27 (a ref's index field)";
    return nullptr;
}

// ... and with the buffers. `device`: device pointers, with a workspace and alignment rules.
inline const char *bvh_buffers_fault(const void *refs, const void *boxes, const void *out, uint32_t n, const void *workspace,
                                     uint64_t workspace_bytes, bool device) {
    if (!refs || !boxes || !out) return "null leaf refs, boxes or output";
    if (device) {
        if (!workspace) return "null workspace";
        if ((uintptr_t)workspace & 15u) return "the workspace must be 16-byte aligned";
        if (workspace_bytes < bvh_layout(n).bytes) return "the workspace is smaller than rt_bvh_workspace_bytes(n_leaves)";
        if (((uintptr_t)out | (uintptr_t)boxes) & 15u) return "the node and box buffers must be 16-byte aligned";
        if ((uintptr_t)refs & 3u) return "the leaf refs must be 4-byte aligned";
    }
    return nullptr;
}

} // namespace rt2022
#endif
