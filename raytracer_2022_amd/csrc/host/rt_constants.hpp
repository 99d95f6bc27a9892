// rt_constants.hpp — the constants the host logic (scene_check.cpp, plan.hpp, the entry points) shares with the kernels:
// each is defined here and nowhere else. No HIP here; pt_device.h includes it.
#ifndef RT2022_RT_CONSTANTS_HPP
#define RT2022_RT_CONSTANTS_HPP
#include <stdint.h>
namespace rt2022 {

// `mat` of the device copies of the primitive pools = material index | slot kind of a hit on it << kMatKindShift.
constexpr uint32_t kMatKindShift = 24, kMatIndexMask = (1u << kMatKindShift) - 1u;
// CheckerTextures texture_value (pt_common.hpp) follows before the texture that answers: rt_scene_create refuses a deeper chain.
constexpr int kCheckerDepth = 8;
// Path slots of one segment of the wavefront engine's pool (WfPool, pt_device.h).
constexpr int kSlotsPerBlock = 4096;     // (a multiple of 256, at most 32768: list entries are u16)
// The largest traversal stack the kernels are instantiated for: a scene that needs more is refused.
constexpr int kStackLarge = 64;
// Four traversal workgroups per CU = 4 waves per SIMD = a budget of 128 VGPRs: the kernel then needs 116 and spills
// nothing. Five (96 VGPRs, 27 spilled, 84 B of scratch per lane) measured 3 % slower in the same run, three 8-9 %
// slower (profiles/r2_ab_occupancy.log): the kernel is bound by instruction issue far more than by latency.
constexpr int kTraceBlocksPerCU = 4;   // resident traversal workgroups per CU the lean kernels are built for
// Arms of the traversal kernel a scene can reach (template FEAT of wf_trace).
constexpr unsigned kFeatMisc = 1;      // triangles, rings
constexpr unsigned kFeatMovers = 2;    // Translate / RotateY / Zoom, HittableList objects
constexpr unsigned kFeatVolumes = 4;   // Boxes, ConstantMedium

} // namespace rt2022
#endif
