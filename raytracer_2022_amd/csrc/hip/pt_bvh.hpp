// pt_bvh.hpp — what rt_bvh.hip (the entry points) and pt_bvh.hip (the kernels of the device BVH builder) share.
#ifndef RT2022_PT_BVH_HPP
#define RT2022_PT_BVH_HPP
#include "../host/bvh_check.hpp"
#include "hip_owned.hpp"

namespace rt2022 {

struct BvhArgs {
    const uint32_t *refs;              // n leaf refs, as they go into the tree
    const double *boxes;               // n x {min[3], max[3]}
    uint32_t n, node_base;
    rt_bvh_node *out;                  // max(1, n - 1) records; record j is the node ref node_base + j
    char *ws;                          // bvh_layout(n).bytes
};

// The two-stage reduction over the boxes: the scene box and the count of refused boxes, into the workspace's status record.
// Writes nothing but workspace.
hipError_t launch_bvh_check(const BvhArgs &a, hipStream_t stream);
// Keys, order, radix tree and the bottom-up pass, behind launch_bvh_check on the same stream. RT_ERR_DEVICE (Fail) if the
// sort asks for more temporary storage than the layout sets aside.
void launch_bvh_build(const BvhArgs &a, hipStream_t stream);

} // namespace rt2022
#endif
