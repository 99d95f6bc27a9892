// pt_rows.hip — the row kernel behind every row list that comes from the caller's HBM into rt_denoise*, rt_denoise_dual*,
// rt_temporal* and rt_adaptive_plan*. One workgroup: the inverse of the list (image row -> buffer row) and the count of ids
// that are out of range or repeated, both in the call's workspace (RowMapLayout, host/post_check.hpp). An id's slot is
// written by plain stores and read back behind a barrier: the entry that lost the race to a repeated id finds another's
// index there. The count is the only atomic.
#include "pt_device.h"

namespace rt2022 {

namespace {

constexpr uint32_t kNoRow = 0xFFFFFFFFu;

__global__ void __launch_bounds__(1024) post_rows(const uint32_t *rows, uint32_t height, uint32_t *inv, uint32_t *bad) {
    for (uint32_t i = threadIdx.x; i < height; i += blockDim.x) inv[i] = kNoRow;
    if (threadIdx.x == 0) *bad = 0u;
    __syncthreads();
    uint32_t n_bad = 0;
    for (uint32_t i = threadIdx.x; i < height; i += blockDim.x) {
        const uint32_t g = rows[i];
        if (g < height) inv[g] = i; else n_bad++;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < height; i += blockDim.x) {
        const uint32_t g = rows[i];
        if (g < height && inv[g] != i) n_bad++;
    }
    if (n_bad) atomicAdd(bad, n_bad);
}

} // namespace

hipError_t launch_row_list_check(const uint32_t *rows, uint32_t height, uint32_t *inv, uint32_t *bad, hipStream_t stream) {
    hipLaunchKernelGGL(post_rows, dim3(1), dim3(1024), 0, stream, rows, height, inv, bad);
    return hipGetLastError();
}

} // namespace rt2022
