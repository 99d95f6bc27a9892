// pt_scatter.hpp — the argument block of the scatter kernel (pt_scatter.hip, rt_scatter*) and its launcher.
#ifndef RT2022_PT_SCATTER_HPP
#define RT2022_PT_SCATTER_HPP

#include "pt_device.h"

namespace rt2022 {

constexpr int kScatterBlock = 256;                        // threads per workgroup: one lane per entry
constexpr uint64_t kScatterMaxEntries = 0x7FFFFFFFull * kScatterBlock;   // (the grid is sized to the batch: blocks fit gridDim.x; beyond it the launch fails, RT_ERR_DEVICE)

struct ScatterArgs {
    const rt_query_ray *rays;          // device, 16-byte aligned: direction, time and rng_state are read
    const rt_hit *hits;                // device, 16-byte aligned: the rt_hit of rays[i], or whatever the caller made up
    const rt_scatter_rec *prev;        // device, 16-byte aligned, or null: every entry is live
    uint64_t n;
    double background[3];
    double t_min;
    rt_scatter_rec *out_recs;          // device, 16-byte aligned (may be `prev`)
    rt_query_ray *out_next;            // device, 16-byte aligned (may be `rays`)
    uint32_t n_materials;              // records in SceneDev::materials: a record's `mat` at or beyond it is RT_SCATTER_INVALID
    uint32_t _pad;
    StatsDev *stats;                   // counter instance only
};
hipError_t launch_scatter(const SceneDev &scene, const ScatterArgs &args, bool counters, hipStream_t stream);

} // namespace rt2022
#endif
