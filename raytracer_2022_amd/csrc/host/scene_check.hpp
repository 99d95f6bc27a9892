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
    bool boxes_plain;                  // every node box finite with min <= max: the short node step applies
    unsigned features;                 // kFeat* arms of the traversal kernel the scene can reach
};
// Every index, ref, chain and cycle of `d` checked: throws Fail (RT_ERR_INVALID, RT_ERR_UNSUPPORTED) or returns the facts.
SceneFacts check_scene(const rt_scene_desc &d);

// New index of every BVH node in the device copy: breadth-first from the root (scene_check.cpp).
std::vector<uint32_t> breadth_first_nodes(const rt_scene_desc &d);

} // namespace rt2022
#endif
