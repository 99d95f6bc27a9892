// hip_owned.hpp — the four HIP resources the library holds, each owned by a small move-only struct: a device allocation,
// a pinned host allocation, an event, a stream. Creation throws Fail (RT_HIP); destructors ignore HIP errors. An empty
// owner (default-constructed, moved from) holds null and makes no HIP call when it dies. They are destroyed with the
// device they were created on current: the entry points (hip/rt_*.hip) see to that (DeviceGuard, rt_internal.hpp).
#ifndef RT2022_HIP_OWNED_HPP
#define RT2022_HIP_OWNED_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

#include "../../../include/rt2022.h"
#include "../host/rt_error.hpp"

namespace rt2022 {

#define RT_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) throw Fail{RT_ERR_DEVICE, std::string(#expr ": ") + hipGetErrorString(e_)}; } while (0)

template <class T>
struct DeviceBuf {
    T *p = nullptr;
    uint64_t n = 0;                    // elements
    DeviceBuf() = default;
    explicit DeviceBuf(uint64_t count) { reserve(count); }
    DeviceBuf(DeviceBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    ~DeviceBuf() { if (p) (void)hipFree(p); }
    operator T *() const { return p; }
    // Room for `count` elements; only ever grows (the contents are not kept), and says whether it did. What may still be
    // using the old block runs on the `n_sync` streams of `sync` (none: the caller knows that nothing is in flight): they
    // are waited for, the block is freed, the new one allocated — nothing is held, and n is 0, if that allocation fails.
    bool reserve(uint64_t count, const hipStream_t *sync = nullptr, int n_sync = 0) {
        if (count <= n) return false;
        for (int i = 0; i < n_sync; i++) RT_HIP(hipStreamSynchronize(sync[i]));
        if (p) RT_HIP(hipFree(p));
        p = nullptr; n = 0;
        RT_HIP(hipMalloc((void **)&p, count * sizeof(T)));
        n = count;
        return true;
    }
};

template <class T>
struct PinnedBuf {
    T *p = nullptr;
    PinnedBuf() = default;
    explicit PinnedBuf(uint64_t count) { RT_HIP(hipHostMalloc((void **)&p, count * sizeof(T))); }
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p, o.p); return *this; }
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    operator T *() const { return p; }
};

struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    explicit Event(unsigned flags) { RT_HIP(flags == hipEventDefault ? hipEventCreate(&ev) : hipEventCreateWithFlags(&ev, flags)); }
    Event(Event &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(ev, o.ev); return *this; }
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    operator hipEvent_t() const { return ev; }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    explicit Stream(unsigned flags) { RT_HIP(hipStreamCreateWithFlags(&s, flags)); }
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};

} // namespace rt2022
#endif
