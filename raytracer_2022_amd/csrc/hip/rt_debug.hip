// rt_debug.hip — include/rt2022_debug.h: the debug setters and readers of a scene, and the three probe families (device
// arithmetic, HBM counter calibration, VALU counter calibration) with their kernels.
#include "../../../include/rt2022_debug.h"
#include "rt_internal.hpp"

using namespace rt2022;

namespace {

// ---- HBM counter calibration (tools/traffic_calib.sh) -------------------------------------------------------------
// MI355X_MICROARCH.md: FETCH_SIZE / WRITE_SIZE are calibrated for wide streaming accesses only ("calibrate on a known
// byte count in your own access pattern before trusting an absolute"). These kernels move a KNOWN number of bytes in
// the path pool's patterns — a 128-byte record per slot, slots visited in random order over a buffer far larger than
// the 256 MiB Infinity Cache — so that the counters read under rocprofv3 can be set against them.
typedef uint32_t probe_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint64_t probe_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31);
}
// MODE 0: streaming read, 16 B per lane; 1: 64 B (first half) of a random record; 2: all 128 B of a random record;
// 3: streaming write; 4: 32 B written at +64 of a random record (a winner); 5: 64 + 32 B written (ray + bookkeeping);
// 6: one byte written at a random position (the old per-slot kind array).
template <int MODE>
__global__ void __launch_bounds__(256) traffic_probe_kernel(probe_u32x4 *buf, uint64_t n_records, uint64_t n_access, uint64_t seed, uint32_t *sink) {
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    probe_u32x4 acc = {0u, 0u, 0u, 0u};
    for (uint64_t i = gid; i < n_access; i += stride) {
        if (MODE == 0) { acc += buf[i]; continue; }
        if (MODE == 3) { buf[i] = (probe_u32x4){(uint32_t)i, 1u, 2u, 3u}; continue; }
        const uint64_t rec = probe_mix(i ^ seed) % n_records;
        probe_u32x4 *r = buf + rec * 8;                              // 128-byte record = 8 x 16 B
        if (MODE == 1) { acc += r[0]; acc += r[1]; acc += r[2]; acc += r[3]; }
        if (MODE == 2) { for (int k = 0; k < 8; k++) acc += r[k]; }
        if (MODE == 4) { r[4] = (probe_u32x4){(uint32_t)i, 1u, 2u, 3u}; r[5] = (probe_u32x4){4u, 5u, 6u, 7u}; }
        if (MODE == 5) { for (int k = 0; k < 4; k++) r[k] = (probe_u32x4){(uint32_t)i, (uint32_t)k, 2u, 3u}; r[6] = (probe_u32x4){1u, 1u, 1u, 1u}; r[7] = (probe_u32x4){2u, 2u, 2u, 2u}; }
        if (MODE == 6) { reinterpret_cast<uint8_t *>(buf)[probe_mix(i ^ seed ^ 0x5555) % (n_records * 128)] = (uint8_t)i; }
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) *sink = acc.x;      // (keeps the loads alive)
}
template <int MODE>
void launch_probe(probe_u32x4 *buf, uint64_t n_records, uint64_t n_access, uint64_t seed, uint32_t *sink) {
    hipLaunchKernelGGL((traffic_probe_kernel<MODE>), dim3(256 * 16), dim3(256), 0, nullptr, buf, n_records, n_access, seed, sink);
}

// ---- VALU counter calibration (tools/valu_calib.sh) ------------------------------------------------------------------
// What do SQ_INSTS_VALU / SQ_ACTIVE_INST_VALU / SQ_THREAD_CYCLES_VALU / SQ_BUSY_CYCLES read for a kernel whose vector
// pipes are KNOWN to be saturated? These kernels issue nothing but independent vector instructions of one kind at 8
// waves per SIMD on every CU, so their issue-slot occupancy is 1 by construction; the counters read under rocprofv3 give
// the normalisation bench.py uses to turn the traversal kernel's counters into a measured busy fraction.
// MODE 0: v_fma_f64, all lanes; 1: 32-bit integer VALU (v_add / v_xor), all lanes; 2: v_fma_f64 with half the lanes
// switched off (EXEC = low 32 lanes); 3: four f64 and four 32-bit instructions alternating; 4: v_fma_f64 at ONE wave per SIMD.
template <int MODE>
__global__ void __launch_bounds__(256) valu_probe_kernel(double *out, uint32_t iters, double b, double c, uint32_t k) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    double a0 = (double)gid, a1 = a0 + 1.0, a2 = a0 + 2.0, a3 = a0 + 3.0, a4 = a0 + 4.0, a5 = a0 + 5.0, a6 = a0 + 6.0, a7 = a0 + 7.0;
    uint32_t x0 = gid, x1 = gid + 1u, x2 = gid + 2u, x3 = gid + 3u, x4 = gid + 4u, x5 = gid + 5u, x6 = gid + 6u, x7 = gid + 7u;
    const bool on = MODE != 2 || (threadIdx.x & 63u) < 32u;
    if (on) {
        for (uint32_t i = 0; i < iters; i++) {
#pragma unroll
          for (int rep = 0; rep < 8; rep++) {                // (64 vector instructions between two loop branches)
            if (MODE == 0 || MODE == 2 || MODE == 4) {
                a0 = __builtin_fma(a0, b, c); a1 = __builtin_fma(a1, b, c); a2 = __builtin_fma(a2, b, c); a3 = __builtin_fma(a3, b, c);
                a4 = __builtin_fma(a4, b, c); a5 = __builtin_fma(a5, b, c); a6 = __builtin_fma(a6, b, c); a7 = __builtin_fma(a7, b, c);
            } else if (MODE == 1) {
                x0 = (x0 + k) ^ x4; x1 = (x1 + k) ^ x5; x2 = (x2 + k) ^ x6; x3 = (x3 + k) ^ x7;
                x4 = (x4 + k) ^ x0; x5 = (x5 + k) ^ x1; x6 = (x6 + k) ^ x2; x7 = (x7 + k) ^ x3;
            } else {
                a0 = __builtin_fma(a0, b, c); x0 = (x0 + k) ^ x4; a1 = __builtin_fma(a1, b, c); x1 = (x1 + k) ^ x5;
                a2 = __builtin_fma(a2, b, c); x2 = (x2 + k) ^ x6; a3 = __builtin_fma(a3, b, c); x3 = (x3 + k) ^ x7;
            }
            asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));   // (no folding of the loop)
          }
        }
    }
    out[gid] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + (double)(x0 ^ x1 ^ x2 ^ x3 ^ x4 ^ x5 ^ x6 ^ x7);
}
} // namespace

extern "C" {

// ---- probes (include/rt2022_debug.h) --------------------------------------------------
int rt_debug_math_device(int op, const double *a, const double *b, double *out, uint64_t n) {
    return guarded([&]() -> int {
        RT_REQUIRE(a && out, RT_ERR_INVALID, "rt_debug_math_device: null argument");
        DeviceBuf<double> da(n + 1), dout(n + 1), db;
        RT_HIP(hipMemcpy(da, a, n * 8, hipMemcpyHostToDevice));
        if (b) { db.reserve(n + 1); RT_HIP(hipMemcpy(db, b, n * 8, hipMemcpyHostToDevice)); }
        RT_HIP(launch_math_probe(op, da, db, dout, n, nullptr));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_debug_rng_device(uint64_t state, int mode, double lo, double hi, uint64_t bound, uint64_t *out, uint64_t n) {
    return guarded([&]() -> int {
        RT_REQUIRE(out, RT_ERR_INVALID, "rt_debug_rng_device: null argument");
        DeviceBuf<uint64_t> dout(n + 1);
        RT_HIP(launch_rng_probe(state, mode, lo, hi, bound, dout, n, nullptr));
        RT_HIP(hipDeviceSynchronize());
        RT_HIP(hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_debug_traffic_probe(int mode, uint64_t buffer_bytes, uint64_t n_access, uint64_t seed) {
    return guarded([&]() -> int {
        RT_REQUIRE(mode >= 0 && mode <= 6 && buffer_bytes >= 4096, RT_ERR_INVALID, "rt_debug_traffic_probe: bad arguments");
        DeviceBuf<char> buf_owner(buffer_bytes);
        DeviceBuf<uint32_t> sink(1);
        probe_u32x4 *const buf = reinterpret_cast<probe_u32x4 *>(buf_owner.p);
        RT_HIP(hipMemset(buf, 1, buffer_bytes));
        RT_HIP(hipDeviceSynchronize());
        const uint64_t n_records = buffer_bytes / 128;
        if (mode == 0 || mode == 3) n_access = buffer_bytes / 16;
        switch (mode) {
            case 0: launch_probe<0>(buf, n_records, n_access, seed, sink); break;
            case 1: launch_probe<1>(buf, n_records, n_access, seed, sink); break;
            case 2: launch_probe<2>(buf, n_records, n_access, seed, sink); break;
            case 3: launch_probe<3>(buf, n_records, n_access, seed, sink); break;
            case 4: launch_probe<4>(buf, n_records, n_access, seed, sink); break;
            case 5: launch_probe<5>(buf, n_records, n_access, seed, sink); break;
            default: launch_probe<6>(buf, n_records, n_access, seed, sink); break;
        }
        RT_HIP(hipGetLastError());
        RT_HIP(hipDeviceSynchronize());
        return RT_OK;
    });
}

int rt_debug_valu_probe(int mode, uint32_t iters) {
    return guarded([&]() -> int {
        RT_REQUIRE(mode >= 0 && mode <= 4 && iters > 0, RT_ERR_INVALID, "rt_debug_valu_probe: bad arguments");
        int dev = 0, cus = 0;
        RT_HIP(hipGetDevice(&dev));
        RT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        const uint32_t blocks = (uint32_t)cus * (mode == 4 ? 1u : 8u);       // 8 workgroups of 4 waves per CU = 8 waves per SIMD (mode 4: one)
        DeviceBuf<double> out((uint64_t)blocks * 256);
        const double b = 0.9999999, c = 1e-9;
        const uint32_t k = 0x9E3779B9u;
        switch (mode) {
            case 0: hipLaunchKernelGGL((valu_probe_kernel<0>), dim3(blocks), dim3(256), 0, nullptr, out.p, iters, b, c, k); break;
            case 1: hipLaunchKernelGGL((valu_probe_kernel<1>), dim3(blocks), dim3(256), 0, nullptr, out.p, iters, b, c, k); break;
            case 2: hipLaunchKernelGGL((valu_probe_kernel<2>), dim3(blocks), dim3(256), 0, nullptr, out.p, iters, b, c, k); break;
            case 3: hipLaunchKernelGGL((valu_probe_kernel<3>), dim3(blocks), dim3(256), 0, nullptr, out.p, iters, b, c, k); break;
            default: hipLaunchKernelGGL((valu_probe_kernel<4>), dim3(blocks), dim3(256), 0, nullptr, out.p, iters, b, c, k); break;
        }
        RT_HIP(hipGetLastError());
        RT_HIP(hipDeviceSynchronize());
        return RT_OK;
    });
}

int rt_debug_set_tuning(rt_scene *scene, uint32_t node_quorum, uint32_t vote_weights) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene, RT_ERR_INVALID, "rt_debug_set_tuning: null scene");
        RT_REQUIRE(tune::quorum(node_quorum) >= 1 && tune::quorum(node_quorum) <= 64, RT_ERR_INVALID,
                   "rt_debug_set_tuning: the quorum (bits 0-7 of node_quorum) must be 1..64; the other fields: include/rt2022_debug.h");
        if (vote_weights != 0)                  // (0 = the engine's default)
            for (int o = 0; o < 8; o++) RT_REQUIRE(((vote_weights >> (4 * o)) & 0xFu) != 0, RT_ERR_INVALID, "rt_debug_set_tuning: a vote weight is 0");
        scene->tuning = node_quorum;
        scene->vote_weights = vote_weights;
        return RT_OK;
    });
}

int rt_debug_set_engine(rt_scene *scene, int engine, int max_pool_blocks) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene, RT_ERR_INVALID, "rt_debug_set_engine: null scene");
        RT_REQUIRE(engine == 0 || engine == 1, RT_ERR_INVALID, "rt_debug_set_engine: engine must be 0 (megakernel) or 1 (wavefront)");
        RT_REQUIRE(max_pool_blocks >= 0 && max_pool_blocks <= 65535, RT_ERR_INVALID, "rt_debug_set_engine: bad max_pool_blocks");
        RT_REQUIRE(engine == 1 || !scene->general_boundaries, RT_ERR_UNSUPPORTED,
                   "the megakernel engine only handles media whose boundary is one primitive under movers");
        scene->engine = engine;
        scene->max_pool_blocks = max_pool_blocks;
        return RT_OK;
    });
}

int rt_debug_set_partial_ring(rt_scene *scene, int planes) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene, RT_ERR_INVALID, "rt_debug_set_partial_ring: null scene");
        RT_REQUIRE(planes >= -1, RT_ERR_INVALID, "rt_debug_set_partial_ring: planes must be -1 (never), 0 (automatic) or a plane count");
        scene->partial_ring = planes;
        return RT_OK;
    });
}

int rt_debug_pass_timing(const rt_scene *scene, double out[5]) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene && out, RT_ERR_INVALID, "rt_debug_pass_timing: null argument");
        for (int i = 0; i < 5; i++) out[i] = scene->pass_timing[i];
        return RT_OK;
    });
}

int rt_debug_census(const rt_scene *scene, uint64_t rounds[9], uint64_t lanes[9]) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene && rounds && lanes, RT_ERR_INVALID, "rt_debug_census: null argument");
        for (int o = 0; o < 9; o++) { rounds[o] = scene->census_rounds[o]; lanes[o] = scene->census_lanes[o]; }
        return RT_OK;
    });
}

int rt_debug_scene_info(const rt_scene *scene, uint32_t *stack_need, int32_t *grid_blocks) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene, RT_ERR_INVALID, "rt_debug_scene_info: null scene");
        if (stack_need) *stack_need = scene->stack_need;
        if (grid_blocks) *grid_blocks = render_grid_blocks(scene->stack_need, false);
        return RT_OK;
    });
}

int rt_debug_trace_variant(const rt_scene *scene, uint32_t *workgroup_threads, uint32_t *stack_entries, uint32_t *nodes_in_lds,
                           uint32_t *spheres_in_lds) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene, RT_ERR_INVALID, "rt_debug_trace_variant: null scene");
        uint32_t v[4] = {0, 0, 0, 0};
        if (scene->engine == 1) trace_variant(scene->dev, scene->stack_need, scene->tuning, scene->features, v);
        if (workgroup_threads) *workgroup_threads = v[0];
        if (stack_entries) *stack_entries = v[1];
        if (nodes_in_lds) *nodes_in_lds = v[2];
        if (spheres_in_lds) *spheres_in_lds = v[3];           // (bit 0: the sphere pools are in LDS; bit 1: node boxes are tested in single precision; bits 2, 3: child order)
        return RT_OK;
    });
}

int rt_debug_f32_slabs(uint64_t out[5]) {
    return guarded([&]() -> int {
        RT_REQUIRE(out, RT_ERR_INVALID, "rt_debug_f32_slabs: null output");
        unsigned long long v[5] = {0, 0, 0, 0, 0};
        RT_HIP(f32_slab_census(v));
        for (int i = 0; i < 5; i++) out[i] = v[i];
        return RT_OK;
    });
}

} // extern "C"
