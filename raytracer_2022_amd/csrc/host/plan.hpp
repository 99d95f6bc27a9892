// plan.hpp — how a render job is cut up: samples per work item, the ring of partial-sum planes, the wavefront engine's pool.
// Pure arithmetic, no HIP (tests/host_units.cpp holds it to recorded values).
#ifndef RT2022_PLAN_HPP
#define RT2022_PLAN_HPP
#include <algorithm>

#include "rt_constants.hpp"

namespace rt2022 {

// Samples per work item and work items per pixel of a call with `spp` samples whose caller asked for `spp_chunk` (0: all in one).
struct Chunks { uint32_t chunk, n_chunks; };
inline Chunks plan_chunks(uint32_t spp, uint32_t spp_chunk) {
    uint32_t chunk = (spp_chunk == 0 || spp_chunk > spp) ? spp : spp_chunk;
    if (chunk == 0) chunk = 1;
    return Chunks{chunk, spp == 0 ? 1u : (uint32_t)(((uint64_t)spp + chunk - 1) / chunk)};
}

// Ring of partial-sum planes (pt_device.h, RenderArgs::ring): one-sample work items of the wavefront engine only. Automatic
// when all spp planes would take more than 40 % of the device's memory (115 GB on an MI355X: C5's 99.5 GB stay below it —
// the ring's work-item order costs its traversal 10 %, the headline's 1.4 %: profiles/r3j_ring.log): then at most 24 GiB
// of planes; rt_debug_set_partial_ring forces a size (tests: down to one plane) or switches it off.
struct RingPlan { uint32_t planes = 0, group = 1; };       // RenderArgs::ring, ring_group (0 planes: no ring)
inline RingPlan plan_ring(uint32_t chunk, uint32_t n_chunks, uint64_t n_pixels, uint64_t n_items, int forced_planes, int forced_group, uint64_t threshold_bytes) {
    RingPlan r;
    if (chunk != 1 || n_chunks <= 1 || n_pixels == 0 || forced_planes < 0) return r;
    uint32_t want = 0;
    const uint64_t plane = n_pixels * 3 * sizeof(double);
    if (forced_planes > 0) want = (uint32_t)forced_planes;
    else if (n_items * 3 * sizeof(double) > threshold_bytes) want = (uint32_t)std::max<uint64_t>(8, (24ull << 30) / plane);
    if (!want || want >= n_chunks) return r;
    // samples are taken in groups: the largest divisor of spp up to 25 (and up to a quarter of the ring, so that it holds
    // a few groups); the ring is a whole number of groups. (A group's planes are free again only when its last straggler
    // has ended, ~60 passes after its first claim: the ring must hold what is claimed meanwhile — measured on C5: five
    // groups of 50 stall every pool fill, twenty of 25 never.)
    uint32_t grp = 1;
    const uint32_t group_max = forced_group > 0 ? (uint32_t)forced_group : 25u;
    for (uint32_t d = 1; d <= group_max && d * 4u <= std::max(want, 4u); d++) if (n_chunks % d == 0) grp = d;
    if (grp > want) grp = 1;
    r.group = grp;
    r.planes = want / grp * grp;
    if (r.planes == 0 || r.planes >= n_chunks) r = RingPlan{};
    return r;
}

// Pool of the wavefront engine = segments of 4096 path slots (one shade workgroup each). The trace pass is a persistent grid of
// kTraceBlocksPerCU workgroups per CU that draws on all segments' ray lists; the pool holds `segs` segments
// per such workgroup (default 8: 33.5 M slots, ~62 GB with a depth-50 tape — measured optimum of 2.5-10 K
// segments on the headline scene; sized for 288 GB of HBM). `segs`: tune::segments; `forced_blocks`: rt_debug_set_engine's
// max_pool_blocks; `have_slots`: the pool there is; `free_bytes()`: device memory free right now (asked only if the pool must grow).
struct PoolPlan { uint32_t segs, blocks; };                 // WfPool::segs, n_blocks
template <class FreeBytes>
PoolPlan plan_pool(uint64_t n_items, uint32_t n_cus, uint32_t max_depth, uint32_t segs, int forced_blocks, uint64_t have_slots, FreeBytes free_bytes) {
    if (segs < 1) segs = 1;
    if (segs > 8) segs = 8;
    uint32_t max_blocks = forced_blocks > 0 ? (uint32_t)forced_blocks : (uint32_t)kTraceBlocksPerCU * n_cus * segs;
    // Use every workgroup slot of the chip even for small jobs (64 paths per workgroup at least).
    uint64_t want = (n_items + 63) / 64;
    uint32_t blocks = (uint32_t)(want < 1 ? 1 : (want > max_blocks ? max_blocks : want));
    // A job of about as many paths as the pool has slots is better served by half the pool: every path starts in the first pass
    // either way, the passes are as many (a path lives its dozen bounces), and each shade pass sweeps half the segments
    // (book-1 final 400x225x100, four frames per call — 36 M paths for 33.5 M slots: +11 %, profiles/r3zh_segs.log). Two paths per
    // slot at least, for jobs large enough to fill the chip anyway; larger jobs keep the whole pool (they lose with a smaller one).
    const uint64_t two_per_slot = n_items / (2ull * (uint64_t)kSlotsPerBlock);
    const uint64_t floor_blocks = (uint64_t)kTraceBlocksPerCU * (uint64_t)n_cus * 2ull;      // (never below two segments per resident traversal workgroup)
    if (forced_blocks <= 0 && two_per_slot < blocks && blocks > floor_blocks)
        blocks = (uint32_t)(two_per_slot > floor_blocks ? two_per_slot : floor_blocks);
    // (deep paths: keep the bounce tape under 56 GB by taking fewer segments)
    const uint64_t tape_per_block = (uint64_t)kSlotsPerBlock * (max_depth ? max_depth : 1) * 4 * sizeof(double);
    while (blocks > segs && (uint64_t)blocks * tape_per_block > (56ull << 30)) blocks -= segs;
    // (and never plan for more than 60 % of the memory that is free right now: other scenes, other users of the GPU)
    if ((uint64_t)blocks * kSlotsPerBlock > have_slots) {
        const uint64_t free_b = free_bytes();                 // (~0: unknown, no limit)
        if (free_b != ~0ull) {
            const uint64_t per_block = (uint64_t)kSlotsPerBlock * 176 + tape_per_block;      // records + tape, bytes
            const uint64_t budget = (uint64_t)((double)free_b * 0.6) + have_slots / kSlotsPerBlock * per_block;
            while (blocks > segs && (uint64_t)blocks * per_block > budget) blocks -= segs;
        }
    }
    if (blocks < segs) segs = blocks;
    return PoolPlan{segs, blocks / segs * segs};
}

} // namespace rt2022
#endif
