// scatter_check.hpp — what rt_scatter* refuses before any device call. Pure tests of the caller's words, no HIP: every
// refusal here is testable without a GPU.
#ifndef RT2022_SCATTER_CHECK_HPP
#define RT2022_SCATTER_CHECK_HPP
#include <cstdint>

#include "../../../include/rt2022.h"

namespace rt2022 {

// What is wrong with the arguments of a scatter call (null: nothing). `device`: the buffers are rt_scatter_device's, read and
// written in 16-byte pieces. The order of the rules is behaviour: of two faults, the one named is the one that comes first.
inline const char *scatter_fault(const void *scene, const rt_scatter_params *p, const void *rays, const void *hits, const void *prev,
                                 uint64_t n, const void *out_recs, const void *out_next, bool device) {
    if (!scene) return "null scene";
    if (!p) return "null params";
    if (p->flags & ~(uint32_t)RT_FLAG_COUNTERS) return "flag bits other than RT_FLAG_COUNTERS";
    if (n == 0) return nullptr;                        // (no buffer is looked at)
    if (!rays || !hits || !out_recs || !out_next) return "null ray, hit, record or next-ray buffer";
    if (device && (((uintptr_t)rays | (uintptr_t)hits | (uintptr_t)prev | (uintptr_t)out_recs | (uintptr_t)out_next) & 15u))
        return "ray, hit, record and next-ray buffers must be 16-byte aligned";
    return nullptr;
}

} // namespace rt2022
#endif
