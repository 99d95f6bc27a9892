// rt_bvh.hip — entry points of the device BVH builder (include/rt2022.h: rt_bvh_workspace_bytes, rt_bvh_build_device,
// rt_bvh_build). The argument rules live in host/bvh_check.hpp and are applied before the first device call; the kernels are
// pt_bvh.hip's. No rt_scene is involved: the builder works on the current device.
#include "pt_bvh.hpp"
#include "rt_internal.hpp"

namespace rt2022 {
namespace {

void check_bvh(const uint32_t *refs, const double *boxes, uint32_t n, uint32_t node_base, const rt_bvh_node *out, const void *ws,
               uint64_t ws_bytes, bool device, const std::string &w) {
    const char *fault = bvh_sizes_fault(n, node_base);
    if (!fault) fault = bvh_buffers_fault(refs, boxes, out, n, ws, ws_bytes, device);
    RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
}

// The build on `stream`, device buffers, arguments checked: the box reduction, ONE synchronisation to read its verdict, then
// everything else as plain enqueues.
void run_bvh(const BvhArgs &a, hipStream_t stream, const std::string &w) {
    RT_HIP(launch_bvh_check(a, stream));
    unsigned long long bad = 0;
    const BvhLayout l = bvh_layout(a.n);
    RT_HIP(hipMemcpyAsync(&bad, a.ws + l.status + offsetof(BvhBoxSum, bad), sizeof bad, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    RT_REQUIRE(bad == 0, RT_ERR_INVALID,
               w + ": " + std::to_string(bad) + " leaf box(es) with a non-finite coordinate, a coordinate beyond 1e300 or min > max");
    launch_bvh_build(a, stream);
}

} // namespace
} // namespace rt2022

using namespace rt2022;

extern "C" {

uint64_t rt_bvh_workspace_bytes(uint32_t n_leaves) {
    return bvh_layout(n_leaves ? n_leaves : 1u).bytes;
}

int rt_bvh_build_device(const uint32_t *d_leaf_refs, const double *d_boxes6, uint32_t n_leaves, uint32_t node_base, rt_bvh_node *d_out_nodes,
                        void *d_workspace, uint64_t workspace_bytes, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_bvh_build_device");
        check_bvh(d_leaf_refs, d_boxes6, n_leaves, node_base, d_out_nodes, d_workspace, workspace_bytes, true, w);
        run_bvh(BvhArgs{d_leaf_refs, d_boxes6, n_leaves, node_base, d_out_nodes, (char *)d_workspace}, (hipStream_t)hip_stream, w);
        return RT_OK;
    });
}

int rt_bvh_build(const uint32_t *leaf_refs, const double *boxes6, uint32_t n_leaves, uint32_t node_base, rt_bvh_node *out_nodes) {
    return guarded([&]() -> int {
        const std::string w("rt_bvh_build");
        check_bvh(leaf_refs, boxes6, n_leaves, node_base, out_nodes, nullptr, 0, false, w);
        const uint32_t n_nodes = bvh_node_count(n_leaves);
        DeviceBuf<uint32_t> d_refs(n_leaves);
        DeviceBuf<double> d_boxes(6ull * n_leaves);
        DeviceBuf<rt_bvh_node> d_out(n_nodes);
        DeviceBuf<char> d_ws(bvh_layout(n_leaves).bytes);
        RT_HIP(hipMemcpy(d_refs, leaf_refs, (uint64_t)n_leaves * sizeof(uint32_t), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_boxes, boxes6, 6ull * n_leaves * sizeof(double), hipMemcpyHostToDevice));
        run_bvh(BvhArgs{d_refs, d_boxes, n_leaves, node_base, d_out, d_ws}, nullptr, w);
        RT_HIP(hipMemcpy(out_nodes, d_out, (uint64_t)n_nodes * sizeof(rt_bvh_node), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

} // extern "C"
