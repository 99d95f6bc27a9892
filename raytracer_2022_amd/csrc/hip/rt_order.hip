// rt_order.hip — entry points of the ray ordering (include/rt2022.h: rt_ray_order_workspace_bytes, rt_ray_order_device,
// rt_ray_order). The argument rules live in host/order_check.hpp and are applied before the first device call; the kernels are
// pt_order.hip's. No rt_scene is involved: the call works on the current device. (rt_intersect_ordered* is rt_query.hip's.)
#include "pt_order.hpp"
#include "rt_internal.hpp"

using namespace rt2022;

extern "C" {

uint64_t rt_ray_order_workspace_bytes(uint64_t n_rays) {
    return order_layout(n_rays).bytes;
}

int rt_ray_order_device(const void *d_rays, uint64_t n_rays, const rt_ray_order_params *p, uint32_t *d_order, void *d_workspace,
                        uint64_t workspace_bytes, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_ray_order_device: ");
        const char *fault = order_params_fault(n_rays, p);
        if (!fault && n_rays) fault = order_buffers_fault(d_rays, d_order, nullptr, false, d_workspace, workspace_bytes, order_layout(n_rays).bytes);
        RT_REQUIRE(!fault, RT_ERR_INVALID, w + (fault ? fault : ""));
        if (n_rays == 0) return RT_OK;
        launch_ray_order(OrderArgs{(const char *)d_rays, n_rays, *p, d_order, (char *)d_workspace}, (hipStream_t)hip_stream);
        return RT_OK;
    });
}

int rt_ray_order(const void *rays, uint64_t n_rays, const rt_ray_order_params *p, uint32_t *order) {
    return guarded([&]() -> int {
        const std::string w("rt_ray_order: ");
        const char *fault = order_params_fault(n_rays, p);
        RT_REQUIRE(!fault, RT_ERR_INVALID, w + (fault ? fault : ""));
        RT_REQUIRE(n_rays == 0 || (rays && order), RT_ERR_INVALID, w + "null ray or order buffer");
        if (n_rays == 0) return RT_OK;
        DeviceBuf<char> d_rays(n_rays * p->ray_stride), d_ws(order_layout(n_rays).bytes);
        DeviceBuf<uint32_t> d_order(n_rays);
        RT_HIP(hipMemcpy(d_rays, rays, n_rays * p->ray_stride, hipMemcpyHostToDevice));
        launch_ray_order(OrderArgs{d_rays, n_rays, *p, d_order, d_ws}, nullptr);
        RT_HIP(hipMemcpy(order, d_order, n_rays * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

} // extern "C"
