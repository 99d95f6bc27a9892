// pt_order.hpp — what rt_order.hip and rt_query.hip (the entry points) and pt_order.hip (the kernels of rt_ray_order* and the
// gather and scatter of rt_intersect_ordered*) share.
#ifndef RT2022_PT_ORDER_HPP
#define RT2022_PT_ORDER_HPP
#include "../host/order_check.hpp"
#include "hip_owned.hpp"

namespace rt2022 {

struct OrderArgs {
    const char *rays;                  // n records, p.ray_stride bytes apart, 16-byte aligned
    uint64_t n;                        // 0 < n < 2^32
    rt_ray_order_params p;
    uint32_t *order;                   // n entries
    char *ws;                          // order_layout(n).bytes
};

// The origin box, the keys and the sort, all plain enqueues on `stream`. RT_ERR_DEVICE (Fail) if the sort asks for more
// temporary storage than the layout sets aside.
void launch_ray_order(const OrderArgs &a, hipStream_t stream);

// gathered[w] = rays[order[w]], or an inert ray where order[w] >= n; with `valid`, *valid (zeroed before) counts the entries < n.
hipError_t launch_order_gather(const rt_query_ray *rays, const uint32_t *order, uint64_t n, rt_query_ray *gathered, unsigned long long *valid,
                               hipStream_t stream);
// hits[order[w]] = gathered[w] where order[w] < n.
hipError_t launch_order_scatter(const rt_hit *gathered, const uint32_t *order, uint64_t n, rt_hit *hits, hipStream_t stream);

} // namespace rt2022
#endif
