// scene_check.hpp — what rt_scene_create finds out about a scene description before any device call: plain C++, no HIP.
#ifndef RT2022_SCENE_CHECK_HPP
#define RT2022_SCENE_CHECK_HPP
#include <vector>

#include "../../../include/rt2022.h"

namespace rt2022 {

// What rt_scene_create keeps of a description it accepts.
struct SceneFacts {
    uint32_t stack_need;               // stack entries a traversal needs (<= kStackLarge)
    int32_t xdepth;                    // deepest nesting of movers (<= RT_MAX_XFORM_DEPTH)
    bool general_boundaries;           // some medium boundary is more than a primitive under movers
    bool boxes_plain;                  // every node box finite with min <= max, every Boxes corner finite: the short node step applies
    unsigned features;                 // kFeat* arms of the traversal kernel the scene can reach
};
// Every index, ref, chain and cycle of `d` checked: throws Fail (RT_ERR_INVALID, RT_ERR_UNSUPPORTED) or returns the facts.
SceneFacts check_scene(const rt_scene_desc &d);

// New index of every BVH node in the device copy: breadth-first from the root (scene_check.cpp).
std::vector<uint32_t> breadth_first_nodes(const rt_scene_desc &d);

// Which child of a BVH node the timed wavefront traversal may visit first (wf_trace), and what keeps that exact.
// A node's `order` is 0 — keep the reference's order, left then right — or 1 + 2 * axis + sense: the axis on which the centres
// of its children's boxes lie furthest apart, sense 0 when the left child is the lower one there (a ray going down that axis
// meets the right child first), 1 when the right child is. Only a node whose subtree holds no ConstantMedium and whose children
// are two different, unflipped nodes or plain primitives gets one. `rank` is the device table of the tie rule: words 0..7 say
// where the ranks of kind k's pool start, the ranks follow — a primitive's (or medium's) place in the reference's depth-first
// order. Nothing is ordered (usable false, every order 0) when some node or primitive is reached along two paths — ranks
// would not be an order then — or the node indices need the ref bits the order travels in. And no order may make a traversal
// need more stack than the kernels chosen for the reference's order have (see child_order).
constexpr uint32_t kOrderShift = 24;               // a node ref carries its node's `order` in bits 24..26: indices below 2^24
constexpr int32_t kStackTiers[4] = {16, 22, 30, 64};    // the traversal stacks wf_trace is built with (pt_device.h: kStackTiny .. kStackLarge)
struct ChildOrder {
    std::vector<uint8_t> order;        // [n_nodes], by the description's node index
    std::vector<uint8_t> medium;       // [n_nodes]: 1 where the node's subtree holds a ConstantMedium
    std::vector<uint32_t> rank;
    bool usable;
};
ChildOrder child_order(const rt_scene_desc &d);

} // namespace rt2022
#endif
