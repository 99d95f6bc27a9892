// rt_api.hip — the device half of the C ABI (include/rt2022.h): scene validation,
// HBM residency, launches. No CPU fallback exists: every entry point here needs a
// HIP device and reports RT_ERR_DEVICE otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../../include/rt2022.h"
#include "../../../include/rt2022_debug.h"
#include "../host/rt_error.hpp"
#include "hip_owned.hpp"
#include "pt_device.h"

using namespace rt2022;

namespace {

template <class F>
int guarded(F &&f) {
    try {
        return f();
    } catch (const Fail &e) {
        set_error(e.msg);
        return e.code;
    } catch (const std::exception &e) {
        set_error(e.what());
        return RT_ERR_INVALID;
    }
}

// ---- validation -------------------------------------------------------------------
struct Validator {
    const rt_scene_desc &d;
    // What need() knows of a record that has children: the stack entries trace<> needs below it, the deepest nesting of
    // movers below it, and whether a medium lies below it (media do not nest inside a medium's boundary).
    struct Need {
        int32_t need = kUnknown, xdepth = 0;
        bool medium = false;
    };
    static constexpr int32_t kUnknown = -1, kOnStack = -2;       // Need::need of a record not yet walked / being walked
    std::vector<Need> node_memo, xform_memo, list_memo, medium_memo;     // one walk per record, however many paths lead to it
    mutable bool general_boundaries = false;   // some medium boundary is more than a primitive under movers
    explicit Validator(const rt_scene_desc &desc)
        : d(desc), node_memo(desc.n_nodes), xform_memo(desc.n_xforms), list_memo(desc.n_lists), medium_memo(desc.n_media) {}

    uint32_t pool_size(uint32_t kind) const {
        switch (kind) {
            case RT_KIND_NODE: return d.n_nodes;
            case RT_KIND_SPHERE: return d.n_spheres;
            case RT_KIND_MOVING_SPHERE: return d.n_moving_spheres;
            case RT_KIND_RECT: return d.n_rects;
            case RT_KIND_BOX: return d.n_boxes;
            case RT_KIND_TRIANGLE: return d.n_triangles;
            case RT_KIND_RING: return d.n_rings;
            case RT_KIND_MEDIUM: return d.n_media;
            case RT_KIND_TRANSLATE: case RT_KIND_ROTATE_Y: case RT_KIND_ZOOM: return d.n_xforms;
            case RT_KIND_LIST: return d.n_lists;
            default: return 0;
        }
    }
    void check_ref(uint32_t ref, const char *where) const {
        uint32_t kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        RT_REQUIRE(kind < RT_KIND_COUNT, RT_ERR_INVALID, std::string(where) + ": ref with unknown kind");
        RT_REQUIRE(idx < pool_size(kind), RT_ERR_INVALID, std::string(where) + ": ref index out of range");
        if (kind >= RT_KIND_TRANSLATE && kind <= RT_KIND_ZOOM)
            RT_REQUIRE(d.xforms[idx].kind == kind, RT_ERR_INVALID, std::string(where) + ": mover ref kind does not match its record");
    }
    // Node boxes as the reference builds them (min / max of real coordinates): finite and ordered.
    bool boxes_plain() const {
        for (uint32_t i = 0; i < d.n_nodes; i++)
            for (int a = 0; a < 3; a++) {
                double lo = d.nodes[i].bmin[a], hi = d.nodes[i].bmax[a];
                if (!(std::isfinite(lo) && std::isfinite(hi) && lo <= hi)) return false;
            }
        return true;
    }
    void check_mat(uint32_t mat, const char *where) const {
        RT_REQUIRE(mat < d.n_materials, RT_ERR_INVALID, std::string(where) + ": material index out of range");
    }

    void check_pools() const {
#define RT_NONNULL(n, p) RT_REQUIRE(d.n == 0 || d.p != nullptr, RT_ERR_INVALID, #p " is null but " #n " > 0")
        RT_NONNULL(n_nodes, nodes); RT_NONNULL(n_spheres, spheres); RT_NONNULL(n_moving_spheres, moving_spheres);
        RT_NONNULL(n_rects, rects); RT_NONNULL(n_boxes, boxes); RT_NONNULL(n_triangles, triangles); RT_NONNULL(n_rings, rings);
        RT_NONNULL(n_media, media); RT_NONNULL(n_xforms, xforms); RT_NONNULL(n_lists, lists); RT_NONNULL(n_list_items, list_items);
        RT_NONNULL(n_lights, lights); RT_NONNULL(n_materials, materials); RT_NONNULL(n_textures, textures);
        RT_NONNULL(n_images, images); RT_NONNULL(image_data_bytes, image_data); RT_NONNULL(n_perlins, perlins);
#undef RT_NONNULL
        for (uint32_t i = 0; i < d.n_nodes; i++) { check_ref(d.nodes[i].left, "node.left"); check_ref(d.nodes[i].right, "node.right"); }
        for (uint32_t i = 0; i < d.n_spheres; i++) check_mat(d.spheres[i].mat, "sphere");
        for (uint32_t i = 0; i < d.n_moving_spheres; i++) check_mat(d.moving_spheres[i].mat, "moving_sphere");
        for (uint32_t i = 0; i < d.n_rects; i++) { check_mat(d.rects[i].mat, "rect"); RT_REQUIRE(d.rects[i].axis <= RT_RECT_YZ, RT_ERR_INVALID, "rect: bad axis"); }
        for (uint32_t i = 0; i < d.n_boxes; i++) check_mat(d.boxes[i].mat, "box");
        for (uint32_t i = 0; i < d.n_triangles; i++) check_mat(d.triangles[i].mat, "triangle");
        for (uint32_t i = 0; i < d.n_rings; i++) check_mat(d.rings[i].mat, "ring");
        for (uint32_t i = 0; i < d.n_media; i++) {
            check_mat(d.media[i].mat, "medium");
            RT_REQUIRE(d.materials[d.media[i].mat].kind == RT_MAT_ISOTROPIC, RT_ERR_INVALID, "medium: phase function must be Isotropic");
            check_ref(d.media[i].boundary, "medium.boundary");
            // A boundary that is one primitive under movers is what the megakernel engine accepts;
            // anything else (a box of boxes, a BVH, a list) takes the wavefront engine.
            uint32_t ref = d.media[i].boundary;
            int lvl = 0;
            bool simple = true;
            while (RT_REF_KIND(ref) >= RT_KIND_TRANSLATE && RT_REF_KIND(ref) <= RT_KIND_ZOOM) {
                if (++lvl > RT_MAX_XFORM_DEPTH) { simple = false; break; }
                ref = d.xforms[RT_REF_INDEX(ref)].child;
                check_ref(ref, "medium.boundary chain");
            }
            uint32_t k = RT_REF_KIND(ref);
            if (!(k >= RT_KIND_SPHERE && k <= RT_KIND_RING)) simple = false;
            if (!simple) general_boundaries = true;
        }
        for (uint32_t i = 0; i < d.n_xforms; i++) {
            uint32_t k = d.xforms[i].kind;
            RT_REQUIRE(k >= RT_KIND_TRANSLATE && k <= RT_KIND_ZOOM, RT_ERR_INVALID, "xform: bad kind");
            check_ref(d.xforms[i].child, "xform.child");
        }
        for (uint32_t i = 0; i < d.n_lists; i++)
            RT_REQUIRE((uint64_t)d.lists[i].first + d.lists[i].count <= d.n_list_items, RT_ERR_INVALID, "list: items out of range");
        for (uint32_t i = 0; i < d.n_list_items; i++) check_ref(d.list_items[i], "list item");
        for (uint32_t i = 0; i < d.n_lights; i++) check_ref(d.lights[i], "light");
        for (uint32_t i = 0; i < d.n_materials; i++) {
            const rt_material &m = d.materials[i];
            RT_REQUIRE(m.kind <= RT_MAT_ISOTROPIC, RT_ERR_INVALID, "material: bad kind");
            if (m.kind == RT_MAT_LAMBERTIAN || m.kind == RT_MAT_DIFFUSE_LIGHT || m.kind == RT_MAT_ISOTROPIC)
                RT_REQUIRE(m.tex < d.n_textures, RT_ERR_INVALID, "material: texture index out of range");
        }
        for (uint32_t i = 0; i < d.n_textures; i++) {
            const rt_texture &t = d.textures[i];
            RT_REQUIRE(t.kind <= RT_TEX_IMAGE, RT_ERR_INVALID, "texture: bad kind");
            if (t.kind == RT_TEX_CHECKER) RT_REQUIRE(t.a < d.n_textures && t.b < d.n_textures, RT_ERR_INVALID, "checker: child out of range");
            if (t.kind == RT_TEX_NOISE) RT_REQUIRE(t.a < d.n_perlins, RT_ERR_INVALID, "noise: perlin index out of range");
            if (t.kind == RT_TEX_IMAGE) RT_REQUIRE(t.a < d.n_images, RT_ERR_INVALID, "image texture: image index out of range");
        }
        for (uint32_t i = 0; i < d.n_images; i++) {
            const rt_image &im = d.images[i];
            // offset + 3 * width * height <= image_data_bytes, without a sum or a product that can wrap
            const uint64_t pixels = (uint64_t)im.width * im.height;            // < 2^64: both are 32-bit
            RT_REQUIRE(im.offset <= d.image_data_bytes && pixels <= (d.image_data_bytes - im.offset) / 3, RT_ERR_INVALID, "image: data out of range");
        }
        check_checkers();
        for (uint32_t i = 0; i < d.n_perlins; i++)
            for (int k = 0; k < 256; k++) {
                const rt_perlin &p = d.perlins[i];
                RT_REQUIRE((uint32_t)p.perm_x[k] < 256 && (uint32_t)p.perm_y[k] < 256 && (uint32_t)p.perm_z[k] < 256, RT_ERR_INVALID, "perlin: permutation entry out of range");
            }
    }

    // Chains of CheckerTextures: texture_value (pt_common.hpp) follows at most kCheckerDepth checkers to the texture that
    // answers, where the reference recurses to the leaf (texture/mod.rs:51-60). A deeper chain would render differently and
    // a cyclic one has no leaf at all: both are refused. One walk per texture (depth[] memoises).
    void check_checkers() const {
        std::vector<int32_t> depth(d.n_textures, kUnknown);      // checkers on the longest chain from the texture to a leaf
        std::vector<uint32_t> stack;
        for (uint32_t t0 = 0; t0 < d.n_textures; t0++) {
            if (depth[t0] != kUnknown) continue;
            stack.push_back(t0);
            while (!stack.empty()) {
                const uint32_t t = stack.back();
                if (d.textures[t].kind != RT_TEX_CHECKER) { depth[t] = 0; stack.pop_back(); continue; }
                depth[t] = kOnStack;
                const uint32_t kids[2] = {d.textures[t].a, d.textures[t].b};
                bool pushed = false;
                for (uint32_t k : kids) {
                    RT_REQUIRE(depth[k] != kOnStack, RT_ERR_INVALID, "checker: cycle among checker children");      // (k == t too)
                    if (depth[k] == kUnknown) { stack.push_back(k); pushed = true; break; }
                }
                if (pushed) continue;
                depth[t] = 1 + std::max(depth[kids[0]], depth[kids[1]]);
                stack.pop_back();
            }
        }
        for (uint32_t t = 0; t < d.n_textures; t++)
            RT_REQUIRE(depth[t] <= kCheckerDepth, RT_ERR_UNSUPPORTED,
                       "checker: textures nested deeper than " + std::to_string(kCheckerDepth) + " checkers (kCheckerDepth)");
    }

    // Stack entries trace<> needs while processing `ref` (its own slot included), the deepest nesting of movers below it and
    // whether a medium lies below it. Every node, mover, list and medium is walked once and remembered, so the walk is linear
    // in the scene's records however many paths lead to a shared one; meeting a record that is still being walked is a cycle.
    Need need(uint32_t ref, int depth) {
        RT_REQUIRE(depth < 4096, RT_ERR_UNSUPPORTED, "scene graph too deep");
        uint32_t kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        Need *memo = kind == RT_KIND_NODE ? &node_memo[idx] : kind >= RT_KIND_TRANSLATE && kind <= RT_KIND_ZOOM ? &xform_memo[idx]
                   : kind == RT_KIND_LIST ? &list_memo[idx] : kind == RT_KIND_MEDIUM ? &medium_memo[idx] : nullptr;
        if (!memo) return Need{1, 0, false};                      // a primitive
        if (kind == RT_KIND_NODE) RT_REQUIRE(!(ref & RT_REF_FLIP), RT_ERR_UNSUPPORTED, "FlipFace directly on a BvhNode ref: push the flip down to the leaves");
        if (kind == RT_KIND_LIST) RT_REQUIRE(!(ref & RT_REF_FLIP), RT_ERR_UNSUPPORTED, "FlipFace directly on a HittableList ref: push the flip down to the items");
        RT_REQUIRE(memo->need != kOnStack, RT_ERR_INVALID,
                   kind == RT_KIND_NODE ? "cycle in the BVH" : "cycle in the scene graph (a list, mover or medium that contains itself)");
        if (memo->need != kUnknown) return *memo;
        memo->need = kOnStack;
        Need out;
        if (kind == RT_KIND_NODE) {
            const Need l = need(d.nodes[idx].left, depth + 1);
            const Need r = d.nodes[idx].right == d.nodes[idx].left ? l : need(d.nodes[idx].right, depth + 1);
            out = Need{std::max(1 + l.need, r.need), std::max(l.xdepth, r.xdepth), l.medium || r.medium};
        } else if (kind == RT_KIND_LIST) {
            const rt_list &l = d.lists[idx];
            out = Need{std::max<int32_t>(1, (int32_t)l.count), 0, false};
            for (uint32_t i = 0; i < l.count; i++) {
                const Need it = need(d.list_items[l.first + i], depth + 1);
                out.need = std::max(out.need, (int32_t)(l.count - 1 - i) + it.need);
                out.xdepth = std::max(out.xdepth, it.xdepth);
                out.medium = out.medium || it.medium;
            }
        } else if (kind == RT_KIND_MEDIUM) {
            // the medium's own slot becomes the sub-query sentinel while its boundary is traversed
            const Need b = need(d.media[idx].boundary, depth + 1);
            RT_REQUIRE(!b.medium, RT_ERR_UNSUPPORTED, "a medium inside another medium's boundary");
            out = Need{1 + b.need, b.xdepth, true};
        } else {
            const Need c = need(d.xforms[idx].child, depth + 1);
            out = Need{1 + c.need, 1 + c.xdepth, c.medium};
        }
        *memo = out;
        return out;
    }
};

// The scene's buffers, pools and streams live on the device that was current at rt_scene_create. Every entry
// point that touches them makes that device current for the call and puts the caller's back afterwards, so one
// process may hold scenes on several GPUs (one host thread per scene and stream) whatever its current device is.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int want) {
        RT_HIP(hipGetDevice(&prev));
        if (prev != want) { RT_HIP(hipSetDevice(want)); switched = true; }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// New index of every BVH node in the device copy: breadth-first from the root, through movers, lists and medium
// boundaries. The traversal kernels keep the FIRST records of the node table in LDS (pt_wavefront.hip); numbered this
// way those are the top levels of the BVHs — the nodes every ray goes through. (The flattener emits children before
// parents; the order of the records means nothing to the results.)
std::vector<uint32_t> breadth_first_nodes(const rt_scene_desc &d) {
    std::vector<uint32_t> new_of(d.n_nodes, 0xFFFFFFFFu), queue;
    std::vector<char> seen_x(d.n_xforms, 0), seen_l(d.n_lists, 0), seen_m(d.n_media, 0);
    uint32_t next = 0;
    queue.push_back(d.root);
    for (size_t h = 0; h < queue.size(); h++) {
        const uint32_t ref = queue[h], kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        if (kind == RT_KIND_NODE) {
            if (new_of[idx] != 0xFFFFFFFFu) continue;
            new_of[idx] = next++;
            queue.push_back(d.nodes[idx].left);
            if (d.nodes[idx].right != d.nodes[idx].left) queue.push_back(d.nodes[idx].right);
        } else if (kind >= RT_KIND_TRANSLATE && kind <= RT_KIND_ZOOM) {
            if (!seen_x[idx]) { seen_x[idx] = 1; queue.push_back(d.xforms[idx].child); }
        } else if (kind == RT_KIND_LIST) {
            if (!seen_l[idx]) { seen_l[idx] = 1; for (uint32_t i = 0; i < d.lists[idx].count; i++) queue.push_back(d.list_items[d.lists[idx].first + i]); }
        } else if (kind == RT_KIND_MEDIUM) {
            if (!seen_m[idx]) { seen_m[idx] = 1; queue.push_back(d.media[idx].boundary); }
        }
    }
    for (uint32_t i = 0; i < d.n_nodes; i++)
        if (new_of[i] == 0xFFFFFFFFu) new_of[i] = next++;            // (unreachable nodes keep a place behind the others)
    return new_of;
}

template <class T>
T *upload(const T *src, uint64_t n, std::vector<DeviceBuf<char>> &owned) {
    // Never hand the kernels a null pool: an empty pool gets one zeroed element.
    // (128 bytes of zeroed slack behind every pool: the shading kernel fetches a fixed 80 bytes from the winning
    // primitive's record whatever its kind, the last record of a pool included)
    uint64_t bytes = (n ? n : 1) * sizeof(T) + 128;
    owned.emplace_back(bytes);
    void *p = owned.back().p;
    RT_HIP(hipMemset(p, 0, bytes));
    if (n) RT_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return (T *)p;
}

// What the wavefront engine needs whatever the size of its pool; all of it is created when one is constructed.
struct EngineFixed {
    DeviceBuf<SceneDev> d_scene{1};
    DeviceBuf<RenderArgs> d_args{1};
    DeviceBuf<WfPool> d_pool{1};
    DeviceBuf<unsigned long long> d_limit{1};   // ring mode: RenderArgs::claim_limit
    WfStreams gs;                     // group streams / events / pinned words
};

// Largest of n device-resident row ids.
__global__ void __launch_bounds__(256) row_ids_max_kernel(const uint32_t *rows, uint32_t n, uint32_t *out) {
    uint32_t m = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) m = rows[i] > m ? rows[i] : m;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { uint32_t o = (uint32_t)__shfl_xor((int)m, d); m = o > m ? o : m; }
    if ((threadIdx.x & 63u) == 0 && m) atomicMax(out, m);
}
// The range check of row ids that came from the caller's HBM (rt_render_device's and rt_features_device's twin of the
// host-side check): the largest of them is reduced on the device and copied to a pinned word. Two halves, so that the
// check costs a render no synchronisation of its own: begin() is enqueued with the call's other preparations,
// and end() looks at the answer behind the synchronisation the call makes anyway before its first pass. (A row id out of
// range cannot fault a kernel — it only mis-keys a frame — so nothing is lost by finding out a moment later.) Every begin()
// starts from zero: a call that fails at either half leaves nothing the next call on the stream would trip over.
struct RowCheck {
    DeviceBuf<uint32_t> d_max;        // device word: largest row id of the call being checked (created on first use)
    PinnedBuf<uint32_t> h_max;        // ... and the pinned word it is copied to
    void begin(const uint32_t *d_rows, uint32_t n, hipStream_t stream) {      // n > 0
        if (!h_max) {                                  // (keyed on the one created last: a failure half-way is made good by the next call)
            d_max = DeviceBuf<uint32_t>(1);
            h_max = PinnedBuf<uint32_t>(1);
        }
        RT_HIP(hipMemsetAsync(d_max, 0, sizeof(uint32_t), stream));
        const uint32_t blocks = (n + 255u) / 256u;
        hipLaunchKernelGGL(row_ids_max_kernel, dim3(blocks > 64 ? 64 : blocks), dim3(256), 0, stream, d_rows, n, d_max.p);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpyAsync(h_max, d_max, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    void end(uint64_t limit, const char *who) const {      // (after a synchronisation of the stream)
        RT_REQUIRE((uint64_t)*h_max.p < limit, RT_ERR_INVALID, std::string(who) + ": row id out of range");
    }
};

// Ids of n device-resident (frame, pixel) entries that are >= limit.
__global__ void __launch_bounds__(256) pixel_ids_bad_kernel(const uint64_t *ids, uint64_t n, uint64_t limit, uint32_t *out) {
    uint32_t bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) bad += ids[i] >= limit ? 1u : 0u;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) bad += (uint32_t)__shfl_xor((int)bad, d);
    if ((threadIdx.x & 63u) == 0 && bad) atomicAdd(out, bad);
}
// RowCheck's twin for the entry list of rt_render_pixels_device: how many ids are out of range, counted on the device into a
// pinned word between begin() and the synchronisation the call makes anyway, looked at by end(). (An id out of range cannot
// fault a kernel either: it only mis-keys a path.) The count saturates nowhere that matters: any nonzero word refuses the call.
struct PixelCheck {
    DeviceBuf<uint32_t> d_bad;
    PinnedBuf<uint32_t> h_bad;
    void begin(const uint64_t *d_ids, uint64_t n, uint64_t limit, hipStream_t stream) {      // n > 0
        if (!h_bad) {
            d_bad = DeviceBuf<uint32_t>(1);
            h_bad = PinnedBuf<uint32_t>(1);
        }
        RT_HIP(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), stream));
        const uint64_t blocks = (n + 255u) / 256u;
        hipLaunchKernelGGL(pixel_ids_bad_kernel, dim3((unsigned)(blocks > 256 ? 256 : blocks)), dim3(256), 0, stream, d_ids, n, limit, d_bad.p);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpyAsync(h_bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    void end(const char *who) const {      // (after a synchronisation of the stream)
        RT_REQUIRE(*h_bad.p == 0, RT_ERR_INVALID, std::string(who) + ": pixel id out of range (>= width * height * n_frames)");
    }
};

// What one (scene, stream) keeps from render to render. Its members own their HIP resources; the ones every call needs —
// work counter, counter block, two events — are created when it is constructed.
struct Workspace {
    DeviceBuf<unsigned long long> work_counter{1};
    DeviceBuf<StatsDev> stats{1};
    DeviceBuf<double> partial, tape;  // partial sums (wavefront and megakernel), bounce tape (megakernel): grown as needed
    // wavefront engine
    WfPool pool{};
    std::vector<DeviceBuf<char>> pool_owned;
    uint32_t pool_slots = 0, pool_depth = 0;
    unsigned long long *pool_dbg = nullptr;    // (one of pool_owned)
    std::unique_ptr<EngineFixed> fx;  // (created on first use)
    uint32_t iterations = 0;
    Event ev0{hipEventDefault}, ev1{hipEventDefault};
    rt_stats *pending = nullptr;      // host stats to fill at rt_render_wait
    bool pending_counters = false;
    KernelTimes kt;                   // RT_FLAG_KERNEL_TIMES
    bool used_kt = false;
    uint32_t used_chunk = 0, used_passes = 0;
    uint64_t used_slots = 0;
    RowCheck rows;                    // rt_render_device's row ids
    uint64_t used_partial_bytes = 0;
    // rt_radiance (host buffers): the device copies of the caller's rays and of the sums, grown as needed
    DeviceBuf<rt_radiance_ray> rad_rays;
    DeviceBuf<double> rad_out;
    // rt_render_pixels*: the check of device ids, and rt_render_pixels' device copy of the caller's list (its sums go through rad_out)
    PixelCheck pixels;
    DeviceBuf<uint64_t> pix_ids;
    // RT_FLAG_ASYNC: the host thread that drives the passes of the call in flight on this (scene, stream), and what it ended with
    // (read by rt_render_wait after the join).
    std::thread async_worker;
    int async_rc = RT_OK;
    std::string async_err;
};

// Scratch of the closest-hit calls — queries (rt_intersect*) or feature buffers (rt_features*) — on one (scene, stream): the
// work counter of the persistent grid, a counter block and two events, created when it is constructed. Nothing of a render's
// Workspace: such a call may run beside an asynchronous render of the same scene.
struct QueryScratch {
    std::mutex mu;                    // one call at a time enqueues — and, with stats, reads back — on this (scene, stream)
    DeviceBuf<unsigned long long> counter{1};
    DeviceBuf<StatsDev> stats{1};
    Event ev0{hipEventDefault}, ev1{hipEventDefault};
    RowCheck rows;                    // rt_features_device's row ids
};

} // namespace

struct rt_scene {
    SceneDev dev{};
    std::vector<DeviceBuf<char>> owned;        // the pools behind `dev`
    uint32_t stack_need = 1;
    unsigned features = 7;
    bool general_boundaries = false;
    bool boxes_plain = false;         // every node box finite with min <= max: the short node step applies
    uint32_t tuning = tune::kDefault;          // the tuning word (pt_device.h, namespace tune)
    uint32_t vote_weights = 0;                 // 0: the wavefront engine's default (kWfVoteWeights, pt_device.h)
    int engine = 1;                   // 0 = megakernel, 1 = wavefront (shade / trace passes)
    unsigned long long census_rounds[9] = {}, census_lanes[9] = {};   // of the last counter run
    int max_pool_blocks = 0;          // 0 = 5 x CUs x segments per trace workgroup
    int partial_ring = 0;             // planes of the partial-sum ring: 0 automatic, -1 never, > 0 this many (rt_debug_set_partial_ring)
    int partial_ring_group = 0;       // largest sample group of the ring (0: 25); env RT2022_RING_GROUP at rt_scene_create (A/B)
    uint64_t ring_threshold_bytes = 64ull << 30;   // partial sums above this switch the ring on: 40 % of the device's memory (rt_scene_create)
    double pass_timing[5] = {};       // of the last render with tuning bit 29 (rt_debug_pass_timing)
    int device = 0;
    int n_cus = 0;                    // compute units of `device`
    std::mutex mu;
    std::map<hipStream_t, Workspace> ws;
    std::mutex qmu;                   // guards `qs` and `fs`
    // (two maps: a query and a feature call on one stream share no mutex and no counter, and run side by side)
    std::map<hipStream_t, std::unique_ptr<QueryScratch>> qs, fs;    // of rt_intersect*, of rt_features*
};

namespace {

Workspace &workspace_for(rt_scene *sc, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(sc->mu);
    return sc->ws.try_emplace(stream).first->second;      // (a new one is in the map once it is complete, or not at all)
}

// The view of a render or a feature call: an image, a shutter interval, row ids that fit 32 bits. (`empty_note`: what the
// caller's message adds to "empty image".)
void check_view(const rt_camera *cam, const rt_params *p, const std::string &prefix, const char *empty_note) {
    RT_REQUIRE(p->width > 0 && p->height > 0 && p->n_frames > 0, RT_ERR_INVALID, prefix + "empty image" + empty_note);
    RT_REQUIRE(cam->time0 < cam->time1, RT_ERR_INVALID, prefix + "camera time0 >= time1 (gen_range panics in the reference, camera.rs:71)");
    RT_REQUIRE((uint64_t)p->height * p->n_frames <= 0xFFFFFFFFull, RT_ERR_INVALID, prefix + "height * n_frames overflows a row id");
}

void check_params(const rt_scene *scene, const rt_camera *cam, const rt_params *p) {
    RT_REQUIRE(scene && cam && p, RT_ERR_INVALID, "null argument");
    check_view(cam, p, "", "");
    RT_REQUIRE(p->n_rows == 0 || p->row_ids, RT_ERR_INVALID, "row_ids is null");
}

template <class T>
T *pool_alloc(Workspace &w, uint64_t count) {
    w.pool_owned.emplace_back((count ? count : 1) * sizeof(T));
    return (T *)w.pool_owned.back().p;
}

// (Re)allocate the wavefront pool for `blocks` workgroups and `depth` tape records.
void ensure_pool(Workspace &w, uint32_t blocks, uint32_t depth, hipStream_t stream) {
    uint32_t slots = blocks * (uint32_t)kSlotsPerBlock;
    if (depth == 0) depth = 1;
    if (!w.fx) w.fx.reset(new EngineFixed());              // (stored once it is complete, or not at all)
    if (slots <= w.pool_slots && depth <= w.pool_depth) { w.pool.n_blocks = blocks; w.pool.n_slots = w.pool_slots; return; }
    // The pool is replaced as a whole — more slots may come with a shorter tape — behind everything that may still use it.
    RT_HIP(hipStreamSynchronize(stream));
    for (int g = 0; g < kMaxGroups; g++) RT_HIP(hipStreamSynchronize(w.fx->gs.stream[g]));    // (passes of an earlier call that failed half-way)
    w.pool_owned.clear();
    w.pool_slots = 0; w.pool_depth = 0;
    if (slots < w.pool.n_slots) slots = w.pool.n_slots;
    uint64_t tape_bytes = (uint64_t)slots * depth * 4 * sizeof(double);
    RT_REQUIRE(tape_bytes <= (64ull << 30), RT_ERR_UNSUPPORTED, "max_depth too large for the bounce tape");
    uint64_t P = slots;
    WfPool &q = w.pool;
    q.n_slots = slots;
    q.n_blocks = blocks;
    q.kind = pool_alloc<uint8_t>(w, P);
    q.ray = pool_alloc<double>(w, kRecDoubles * P);                       // the 128-byte slot records: ray | hit | state
    q.hit = reinterpret_cast<uint32_t *>(q.ray) + 16;
    q.state = reinterpret_cast<uint32_t *>(q.ray) + 24;
    q.pixel_sum = pool_alloc<double>(w, 4 * P);
    q.tape = pool_alloc<double>(w, (uint64_t)depth * 4 * P);
    q.tape_cap = depth;
    q.list = pool_alloc<uint16_t>(w, P);
    q.list_n = pool_alloc<uint32_t>(w, P / (uint64_t)kSlotsPerBlock);
    q.n_active = pool_alloc<uint32_t>(w, 2 * kMaxGroups);
    q.next_chunk = pool_alloc<uint32_t>(w, kMaxGroups);
    q.max_list = pool_alloc<uint32_t>(w, 2 * kMaxGroups);
    q.fault = pool_alloc<uint32_t>(w, 1);
    q.oldest = pool_alloc<unsigned long long>(w, 2);
    q.starved_n = pool_alloc<uint32_t>(w, P / (uint64_t)kSlotsPerBlock);
    w.pool_dbg = pool_alloc<unsigned long long>(w, 8 + 2 * 65536);
    w.pool_slots = slots;
    w.pool_depth = depth;
}

// Where the paths of an rt_radiance* call start: the caller's rays (device) instead of the camera's rows.
struct RaySource {
    const rt_radiance_ray *d_rays;
    uint64_t n_rays;
};
// Where the paths of an rt_render_pixels* call start: a list of (frame, pixel) ids (device) instead of the row list.
struct PixelSource {
    const uint64_t *d_ids;
    uint64_t n_entries;
    bool check;                       // the ids came from the caller's HBM: range-check them
    const char *who;
};
static_assert(sizeof(rt_radiance_ray) == 64 && offsetof(rt_radiance_ray, time) == 48 && offsetof(rt_radiance_ray, rng_state) == 56,
              "rt_radiance_ray is the path slot's ray record {ox, oy, oz, dx, dy, dz, tm, rng}: wf_shade reads it in four 16-byte pieces");

// Ring of partial-sum planes (pt_device.h, RenderArgs::ring): one-sample work items of the wavefront engine only. Automatic
// when all spp planes would take more than 40 % of the device's memory (115 GB on an MI355X: C5's 99.5 GB stay below it —
// the ring's work-item order costs its traversal 10 %, the headline's 1.4 %: profiles/r3j_ring.log): then at most 24 GiB
// of planes; rt_debug_set_partial_ring forces a size (tests: down to one plane) or switches it off.
struct RingPlan { uint32_t planes = 0, group = 1; };       // RenderArgs::ring, ring_group (0 planes: no ring)
RingPlan plan_ring(uint32_t chunk, uint32_t n_chunks, uint64_t n_pixels, uint64_t n_items, int forced_planes, int forced_group, uint64_t threshold_bytes) {
    RingPlan r;
    if (chunk != 1 || n_chunks <= 1 || n_pixels == 0 || forced_planes < 0) return r;
    uint32_t want = 0;
    const uint64_t plane = n_pixels * 3 * sizeof(double);
    if (forced_planes > 0) want = (uint32_t)forced_planes;
    else if (n_items * 3 * sizeof(double) > threshold_bytes) want = (uint32_t)std::max<uint64_t>(8, (24ull << 30) / plane);
    if (!want || want >= n_chunks) return r;
    // samples are taken in groups: the largest divisor of spp up to 25 (and up to a quarter of the ring, so that it holds
    // a few groups); the ring is a whole number of groups. (A group's planes are free again only when its last straggler
    // has ended, ~60 passes after its first claim: the ring must hold what is claimed meanwhile — measured on C5: five
    // groups of 50 stall every pool fill, twenty of 25 never.)
    uint32_t grp = 1;
    const uint32_t group_max = forced_group > 0 ? (uint32_t)forced_group : 25u;
    for (uint32_t d = 1; d <= group_max && d * 4u <= std::max(want, 4u); d++) if (n_chunks % d == 0) grp = d;
    if (grp > want) grp = 1;
    r.group = grp;
    r.planes = want / grp * grp;
    if (r.planes == 0 || r.planes >= n_chunks) r = RingPlan{};
    return r;
}

// Pool of the wavefront engine = segments of 4096 path slots (one shade workgroup each). The trace pass is a persistent grid of
// kTraceBlocksPerCU workgroups per CU that draws on all segments' ray lists; the pool holds `segs` segments
// per such workgroup (default 8: 33.5 M slots, ~62 GB with a depth-50 tape — measured optimum of 2.5-10 K
// segments on the headline scene; sized for 288 GB of HBM). `segs`: tune::segments; `forced_blocks`: rt_debug_set_engine's
// max_pool_blocks; `have_slots`: the pool there is; `free_bytes()`: device memory free right now (asked only if the pool must grow).
struct PoolPlan { uint32_t segs, blocks; };                 // WfPool::segs, n_blocks
template <class FreeBytes>
PoolPlan plan_pool(uint64_t n_items, uint32_t n_cus, uint32_t max_depth, uint32_t segs, int forced_blocks, uint64_t have_slots, FreeBytes free_bytes) {
    if (segs < 1) segs = 1;
    if (segs > 8) segs = 8;
    uint32_t max_blocks = forced_blocks > 0 ? (uint32_t)forced_blocks : (uint32_t)kTraceBlocksPerCU * n_cus * segs;
    // Use every workgroup slot of the chip even for small jobs (64 paths per workgroup at least).
    uint64_t want = (n_items + 63) / 64;
    uint32_t blocks = (uint32_t)(want < 1 ? 1 : (want > max_blocks ? max_blocks : want));
    // A job of about as many paths as the pool has slots is better served by half the pool: every path starts in the first pass
    // either way, the passes are as many (a path lives its dozen bounces), and each shade pass sweeps half the segments
    // (book-1 final 400x225x100, four frames per call — 36 M paths for 33.5 M slots: +11 %, profiles/r3zh_segs.log). Two paths per
    // slot at least, for jobs large enough to fill the chip anyway; larger jobs keep the whole pool (they lose with a smaller one).
    const uint64_t two_per_slot = n_items / (2ull * (uint64_t)kSlotsPerBlock);
    const uint64_t floor_blocks = (uint64_t)kTraceBlocksPerCU * (uint64_t)n_cus * 2ull;      // (never below two segments per resident traversal workgroup)
    if (forced_blocks <= 0 && two_per_slot < blocks && blocks > floor_blocks)
        blocks = (uint32_t)(two_per_slot > floor_blocks ? two_per_slot : floor_blocks);
    // (deep paths: keep the bounce tape under 56 GB by taking fewer segments)
    const uint64_t tape_per_block = (uint64_t)kSlotsPerBlock * (max_depth ? max_depth : 1) * 4 * sizeof(double);
    while (blocks > segs && (uint64_t)blocks * tape_per_block > (56ull << 30)) blocks -= segs;
    // (and never plan for more than 60 % of the memory that is free right now: other scenes, other users of the GPU)
    if ((uint64_t)blocks * kSlotsPerBlock > have_slots) {
        const uint64_t free_b = free_bytes();                 // (~0: unknown, no limit)
        if (free_b != ~0ull) {
            const uint64_t per_block = (uint64_t)kSlotsPerBlock * 176 + tape_per_block;      // records + tape, bytes
            const uint64_t budget = (uint64_t)((double)free_b * 0.6) + have_slots / kSlotsPerBlock * per_block;
            while (blocks > segs && (uint64_t)blocks * per_block > budget) blocks -= segs;
        }
    }
    if (blocks < segs) segs = blocks;
    return PoolPlan{segs, blocks / segs * segs};
}

// Enqueue one render on `stream`; row ids and output are device pointers. With `src` the call is an rt_radiance*: its
// "pixels" are the rays of src (p: width 1, no rows, spp_chunk 1; cam unused). With `pix` it is an rt_render_pixels*: its
// "pixels" are the entries of pix (p: the image's own; n_rows and row_ids unused; wavefront engine only).
void enqueue(rt_scene *sc, const rt_camera *cam, const rt_params *p, const uint32_t *d_rows, double *d_out,
             hipStream_t stream, rt_stats *stats, bool check_rows = false /* the row ids came from the caller's HBM: range-check them */,
             const RaySource *src = nullptr, const PixelSource *pix = nullptr) {
    Workspace &w = workspace_for(sc, stream);
    if (p->n_rows == 0 || pix) check_rows = false;
    const uint64_t row_limit = (uint64_t)p->height * p->n_frames;
    RenderArgs a{};
    a.cam = *cam;
    a.width = p->width; a.height = p->height; a.spp = p->spp; a.max_depth = p->max_depth;
    a.n_frames = p->n_frames; a.n_rows = p->n_rows;
    uint32_t chunk = (p->spp_chunk == 0 || p->spp_chunk > p->spp) ? p->spp : p->spp_chunk;
    if (chunk == 0) chunk = 1;
    a.chunk = chunk;
    a.n_chunks = p->spp == 0 ? 1 : (p->spp + chunk - 1) / chunk;
    std::memcpy(a.background, p->background, sizeof a.background);
    a.t_min = p->t_min;
    a.seed = p->seed;
    a.n_pixels = src ? src->n_rays : pix ? pix->n_entries : (uint64_t)p->n_rows * p->width;
    a.n_items = a.n_pixels * a.n_chunks;
    // The partial sums' byte counts below (24 B per work item) must not wrap: a wrapped size would allocate too little and the
    // shade pass would write past it. (rt_radiance*'s own limit, RT_RADIANCE_MAX_ITEMS, keeps its calls far below this.)
    RT_REQUIRE(a.n_pixels == 0 || (a.n_items / a.n_pixels == a.n_chunks && a.n_items <= (~0ull >> 1) / (3 * sizeof(double))),
               RT_ERR_INVALID, "work items of the call overflow the partial sums' 64-bit byte counts");
    a.row_ids = d_rows;
    a.rays = src ? src->d_rays : nullptr;
    a.pixel_ids = pix ? pix->d_ids : nullptr;
    bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    const bool want_kt = stats && (p->flags & RT_FLAG_KERNEL_TIMES) && sc->engine == 1;
    const RingPlan rp = sc->engine == 1 ? plan_ring(a.chunk, a.n_chunks, a.n_pixels, a.n_items, sc->partial_ring, sc->partial_ring_group, sc->ring_threshold_bytes)
                                        : RingPlan{};
    a.ring = rp.planes; a.ring_group = rp.group;
    if (a.n_chunks > 1) {
        uint64_t bytes = (a.ring ? (uint64_t)a.ring * a.n_pixels : a.n_items) * 3 * sizeof(double);
        w.used_partial_bytes = bytes;
        w.partial.reserve(bytes / sizeof(double), &stream, 1);     // (an earlier call on the stream may still be summing the old ones)
        a.partial = w.partial;
    } else {
        a.partial = d_out;
        w.used_partial_bytes = 0;
    }
    a.tuning = tune::for_kernels(sc->tuning, sc->boxes_plain);       // (see wf_trace's fast path)
    a.vote_weights = sc->vote_weights ? sc->vote_weights : kWfVoteWeights;      // (read by the wavefront engine only)
    a.work_counter = w.work_counter;
    a.stats = counters ? w.stats.p : nullptr;
    if (sc->engine == 1) {
        // Wavefront engine: pool of path slots, shade / trace passes until it drains.
        const PoolPlan pp = plan_pool(a.n_items, (uint32_t)sc->n_cus, p->max_depth, tune::segments(sc->tuning), sc->max_pool_blocks, w.pool_slots, [] {
            size_t free_b = 0, total_b = 0;
            return hipMemGetInfo(&free_b, &total_b) == hipSuccess ? (uint64_t)free_b : ~0ull;
        });
        const uint32_t segs = pp.segs, blocks = pp.blocks;
        ensure_pool(w, blocks, p->max_depth, stream);
        EngineFixed &fx = *w.fx;
        a.claim_limit = fx.d_limit;
        w.pool.segs = segs;
        w.pool.n_cus = (uint32_t)sc->n_cus;
        const bool timing = tune::pass_timing(sc->tuning);
        // Groups of pool segments passing independently, each on a stream of its own: one group's shade pass then runs beside another's
        // traversal pass and fills what its stragglers leave idle. 0 in the tuning word = the library's choice: two — measured
        // (profiles/r3ze_groups.log, bench.py --groups): 1e5 random spheres +18 %, Cornell box +3 %, random spheres +1 %, book-2 final
        // +0.4 % — except for meshes (wwscene: -3 % at two, -7 % at three), which keep one.
        fx.gs.n = (int)tune::groups(sc->tuning);
        if (fx.gs.n < 1) fx.gs.n = (sc->features & kFeatMisc) ? 1 : 2;
        if (fx.gs.n > kMaxGroups) fx.gs.n = kMaxGroups;
        w.pool.dbg = timing ? w.pool_dbg : nullptr;
#if defined(RT2022_SHADE_PROBE) || defined(RT2022_TRACE_PROBE)
        w.pool.dbg = w.pool_dbg;                                  // (diagnostic builds: the section clocks of the shade / traversal kernels)
        RT_HIP(hipMemsetAsync(w.pool_dbg + 64, 0, 48 * sizeof(unsigned long long), stream));
#endif
        if (timing) for (double &t : sc->pass_timing) t = 0.0;
        a.tape = nullptr;
        RT_HIP(hipMemsetAsync(w.work_counter, 0, sizeof(unsigned long long), stream));
        if (counters) RT_HIP(hipMemsetAsync(w.stats, 0, sizeof(StatsDev), stream));
        RT_HIP(hipMemcpyAsync(fx.d_args, &a, sizeof(RenderArgs), hipMemcpyHostToDevice, stream));
        if (check_rows) w.rows.begin(p->row_ids, p->n_rows, stream);
        const bool check_pixels = pix && pix->check && pix->n_entries > 0;
        if (check_pixels) w.pixels.begin(pix->d_ids, pix->n_entries, (uint64_t)p->width * row_limit, stream);
        RT_HIP(hipStreamSynchronize(stream));      // the three structs above live on this thread's stack
        if (check_rows) w.rows.end(row_limit, "rt_render_device");
        if (check_pixels) w.pixels.end(pix->who);
        RT_HIP(hipEventRecord(w.ev0, stream));
        WfRender r;
        r.scene = &sc->dev; r.args = &a; r.d_args = fx.d_args; r.pool = &w.pool;
        r.stack_need = sc->stack_need; r.features = sc->features; r.counters = counters;
        r.gs = &fx.gs; r.stream = stream;
        r.progress.cb = pix ? nullptr : p->progress_cb; r.progress.user = p->progress_user;
        r.progress.total = a.n_pixels * p->spp; r.progress.per_item = a.chunk;
        r.ring.planes = a.ring; r.ring.out = d_out; r.ring.d_limit = fx.d_limit;
        // (watchdog of the ring's pass loop: a frame needs about items / slots pool fills of at most max_depth + 1 passes each)
        // (... plus one drain per ring-full of planes when the ring is small)
        r.ring.max_passes = (uint32_t)std::min<uint64_t>(1u << 26, 64 + 8 * (a.n_items / ((uint64_t)w.pool.n_blocks * kSlotsPerBlock) + 2 + (a.ring ? a.n_chunks / a.ring : 0)) *
                                                                       ((uint64_t)p->max_depth + 2));
        r.timing = timing ? sc->pass_timing : nullptr;
        r.kt = want_kt ? &w.kt : nullptr;
        if (a.n_items > 0) {
            RT_HIP(launch_render_wavefront(r));
            w.iterations = r.passes;
            RT_REQUIRE(r.fault == 0, RT_ERR_DEVICE, "wavefront engine: a path slot reached the shade pass without having been traced (internal error; the frame is incomplete)");
            if (a.n_chunks > 1 && !a.ring) RT_HIP(launch_chunk_sum(a.partial, d_out, a.n_pixels * 3, a.n_chunks, stream));
        }
        RT_HIP(hipEventRecord(w.ev1, stream));
        w.pending = stats;
        w.pending_counters = counters;
        w.used_chunk = a.chunk; w.used_passes = w.iterations; w.used_slots = (uint64_t)w.pool.n_blocks * kSlotsPerBlock;
        w.used_kt = want_kt && a.n_items > 0;
        // (every pass of the frame has been issued and observed: the render is complete up to the chunk sums queued behind it)
        if (r.progress.cb) r.progress.cb(r.progress.user, 0u, r.progress.total, r.progress.total);
        return;
    }
    // Megakernel engine. Bounce tape: max_depth records of 4 doubles for every lane of the persistent grid.
    int blocks = render_grid_blocks(sc->stack_need, counters);
    uint64_t want_blocks = (a.n_items + kBlock - 1) / kBlock;
    if ((uint64_t)blocks > want_blocks) blocks = (int)(want_blocks ? want_blocks : 1);
    uint64_t tape_bytes = (uint64_t)blocks * kBlock * (uint64_t)(p->max_depth ? p->max_depth : 1) * 4 * sizeof(double);
    RT_REQUIRE(tape_bytes <= (32ull << 30), RT_ERR_UNSUPPORTED, "max_depth too large for the bounce tape");
    w.tape.reserve(tape_bytes / sizeof(double), &stream, 1);
    a.tape = w.tape;
    if (check_rows) {                              // (the A/B engine enqueues without a synchronisation of its own)
        w.rows.begin(p->row_ids, p->n_rows, stream);
        RT_HIP(hipStreamSynchronize(stream));
        w.rows.end(row_limit, "rt_render_device");
    }
    RT_HIP(hipMemsetAsync(w.work_counter, 0, sizeof(unsigned long long), stream));
    if (counters) RT_HIP(hipMemsetAsync(w.stats, 0, sizeof(StatsDev), stream));
    RT_HIP(hipEventRecord(w.ev0, stream));
    if (a.n_items > 0) {
        RT_HIP(launch_render(sc->dev, a, sc->stack_need, counters, blocks, stream));
        if (a.n_chunks > 1) RT_HIP(launch_chunk_sum(a.partial, d_out, a.n_pixels * 3, a.n_chunks, stream));
    }
    RT_HIP(hipEventRecord(w.ev1, stream));
    w.pending = stats;
    w.pending_counters = counters;
    w.used_chunk = a.chunk; w.used_passes = 0; w.used_slots = 0; w.used_kt = false;
    if (p->progress_cb) {                          // (the A/B engine is one launch: nothing to report in between)
        RT_HIP(hipStreamSynchronize(stream));
        p->progress_cb(p->progress_user, 0u, a.n_pixels * p->spp, a.n_pixels * p->spp);
    }
}

// rt_stats of a finished call (its stream has been synchronised): the time between its two events and, with `d_stats`, the
// counter block of the run as rt_stats reports it (the whole block is left in `h` for the caller that wants more of it).
rt_stats read_stats(hipEvent_t ev0, hipEvent_t ev1, const StatsDev *d_stats, StatsDev &h) {
    rt_stats out;
    std::memset(&out, 0, sizeof out);
    if (d_stats) {
        RT_HIP(hipMemcpy(&h, d_stats, sizeof h, hipMemcpyDeviceToHost));
        out.paths = h.paths; out.rays = h.rays; out.node_visits = h.node_visits;
        for (int k = 0; k < RT_KIND_COUNT; k++) out.prim_tests[k] = h.prim_tests[k];
        out.light_pdf_tests = h.light_pdf_tests; out.rng_draws = h.rng_draws;
    }
    float ms = 0.f;
    RT_HIP(hipEventElapsedTime(&ms, ev0, ev1));
    out.ms = (double)ms;
    return out;
}

// The scratch of `stream` in sc->qs or sc->fs.
QueryScratch &scratch_for(rt_scene *sc, std::map<hipStream_t, std::unique_ptr<QueryScratch>> &of, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(sc->qmu);
    std::unique_ptr<QueryScratch> &q = of[stream];
    if (!q) q.reset(new QueryScratch());                   // (stored once it is complete, or not at all)
    return *q;
}

// One closest-hit call on `stream`, q locked: the counters reset, `launch()` — the kernel, on q.counter and, with `counters`,
// q.stats — and with stats the wait for it and what read_stats makes of it.
template <class Launch>
void run_counted(QueryScratch &q, bool counters, hipStream_t stream, rt_stats *stats, Launch launch) {
    RT_HIP(hipMemsetAsync(q.counter, 0, sizeof(unsigned long long), stream));
    if (counters) RT_HIP(hipMemsetAsync(q.stats, 0, sizeof(StatsDev), stream));
    if (stats) RT_HIP(hipEventRecord(q.ev0, stream));
    RT_HIP(launch());
    if (!stats) return;
    RT_HIP(hipEventRecord(q.ev1, stream));
    RT_HIP(hipStreamSynchronize(stream));
    StatsDev h;
    *stats = read_stats(q.ev0, q.ev1, counters ? q.stats.p : nullptr, h);
}

void check_query(const rt_scene *scene, const void *rays, uint64_t n_rays, uint32_t flags, const void *hits, const char *who) {
    RT_REQUIRE(scene, RT_ERR_INVALID, std::string(who) + ": null scene");
    RT_REQUIRE(n_rays == 0 || (rays && hits), RT_ERR_INVALID, std::string(who) + ": null ray or hit buffer");
    RT_REQUIRE(!(flags & ~(RT_FLAG_COUNTERS | RT_FLAG_ANY_HIT)), RT_ERR_INVALID, std::string(who) + ": unknown flag bits");
    RT_REQUIRE(!(flags & RT_FLAG_ANY_HIT) || scene->dev.n_media == 0, RT_ERR_UNSUPPORTED,
               std::string(who) + ": RT_FLAG_ANY_HIT on a scene with a ConstantMedium (its verdict depends on the closest hit so far)");
}

// Enqueue one query on `stream` (the scene's device is current); with stats, wait for it and fill them.
void run_query(rt_scene *sc, const rt_query_ray *d_rays, uint64_t n_rays, uint32_t flags, rt_hit *d_hits, hipStream_t stream,
               rt_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_rays == 0) return;
    QueryScratch &q = scratch_for(sc, sc->qs, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    const bool counters = stats && (flags & RT_FLAG_COUNTERS);
    const QueryArgs a{d_rays, d_hits, n_rays, q.counter, counters ? q.stats.p : nullptr};
    run_counted(q, counters, stream, stats, [&] { return launch_query(sc->dev, a, sc->stack_need, counters, (flags & RT_FLAG_ANY_HIT) != 0, stream); });
    if (stats) stats->rays = n_rays;               // (a query counts no paths, rays or light tests of its own)
}

// The arguments of rt_features* (host side only; the scene comes last so that a bad argument is reported as such whatever
// the scene). `device`: rows and output are rt_features_device's — the rows are range-checked on the device later.
void check_features(const rt_scene *scene, const rt_camera *cam, const rt_params *p, const void *out, bool device, const char *who) {
    const std::string w(who);
    RT_REQUIRE(p, RT_ERR_INVALID, w + ": null params");
    RT_REQUIRE(cam, RT_ERR_INVALID, w + ": null camera");
    RT_REQUIRE(!(p->flags & ~RT_FLAG_COUNTERS), RT_ERR_INVALID, w + ": flag bits other than RT_FLAG_COUNTERS");
    check_view(cam, p, w + ": ", " (width, height or n_frames is 0)");
    const bool need_rows = p->n_rows > 0 && p->spp > 0;
    RT_REQUIRE(p->n_rows == 0 || out, RT_ERR_INVALID, w + ": null output");
    RT_REQUIRE(!need_rows || p->row_ids, RT_ERR_INVALID, w + ": null row_ids");
    RT_REQUIRE((uint64_t)p->n_rows * p->width <= (1ull << 40), RT_ERR_INVALID, w + ": n_rows * width too large");
    if (device) {
        RT_REQUIRE(p->n_rows == 0 || !((uintptr_t)out & 15u), RT_ERR_INVALID, w + ": the output must be 16-byte aligned");
        RT_REQUIRE(!need_rows || !((uintptr_t)p->row_ids & 3u), RT_ERR_INVALID, w + ": row_ids must be 4-byte aligned");
    } else if (need_rows) {
        for (uint32_t i = 0; i < p->n_rows; i++)
            RT_REQUIRE(p->row_ids[i] < (uint64_t)p->height * p->n_frames, RT_ERR_INVALID, w + ": row id out of range");
    }
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
}

// Enqueue one feature call on `stream` (the scene's device is current, the arguments checked); with stats, wait for it and
// fill them. `check_rows`: the row ids came from the caller's HBM — range-check them first (one synchronisation of the stream).
void run_features(rt_scene *sc, const rt_camera *cam, const rt_params *p, const uint32_t *d_rows, rt_feature *d_out,
                  hipStream_t stream, rt_stats *stats, bool check_rows, const char *who) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    const uint64_t n_pixels = (uint64_t)p->n_rows * p->width;
    if (n_pixels == 0) return;
    if (p->spp == 0) {                                     // no sample: zeros, no kernel
        RT_HIP(hipMemsetAsync(d_out, 0, n_pixels * sizeof(rt_feature), stream));
        if (stats) RT_HIP(hipStreamSynchronize(stream));
        return;
    }
    QueryScratch &q = scratch_for(sc, sc->fs, stream);
    std::lock_guard<std::mutex> lock(q.mu);
    if (check_rows) {
        q.rows.begin(d_rows, p->n_rows, stream);
        RT_HIP(hipStreamSynchronize(stream));
        q.rows.end((uint64_t)p->height * p->n_frames, who);
    }
    const bool counters = stats && (p->flags & RT_FLAG_COUNTERS);
    FeatureArgs a{};
    a.cam = *cam;
    a.width = p->width; a.height = p->height; a.spp = p->spp; a.n_rows = p->n_rows;
    std::memcpy(a.background, p->background, sizeof a.background);
    a.t_min = p->t_min;
    a.seed = p->seed;
    a.n_pixels = n_pixels;
    a.row_ids = d_rows;
    a.out = d_out;
    a.counter = q.counter;
    a.stats = counters ? q.stats.p : nullptr;
    run_counted(q, counters, stream, stats, [&] { return launch_features(sc->dev, a, sc->stack_need, counters, stream); });
    if (stats) stats->paths = stats->rays = n_pixels * p->spp;     // (one camera path, one world.hit per sample; the kernel counts neither)
}

// The arguments of rt_radiance* (host side only, before the scene is looked at: the scene comes last so that a bad argument
// is reported as such whatever the scene). `device`: the buffers are rt_radiance_device's, read and written in 16-byte pieces.
void check_radiance(const rt_scene *scene, const void *rays, uint64_t n_rays, const rt_radiance_params *p, const void *out,
                    bool device, const char *who) {
    const std::string w(who);
    RT_REQUIRE(p, RT_ERR_INVALID, w + ": null params");
    RT_REQUIRE(!(p->flags & ~(RT_FLAG_COUNTERS | RT_FLAG_KERNEL_TIMES)), RT_ERR_INVALID,
               w + ": flag bits other than RT_FLAG_COUNTERS / RT_FLAG_KERNEL_TIMES");
    RT_REQUIRE(n_rays == 0 || (rays && out), RT_ERR_INVALID, w + ": null ray or output buffer");
    RT_REQUIRE(!device || n_rays == 0 || !(((uintptr_t)rays | (uintptr_t)out) & 15u), RT_ERR_INVALID,
               w + ": ray and output buffers must be 16-byte aligned");
    RT_REQUIRE(n_rays <= RT_RADIANCE_MAX_RAYS, RT_ERR_INVALID, w + ": n_rays > RT_RADIANCE_MAX_RAYS");
    // (a division, not a product: n_rays * spp itself may not fit 64 bits)
    RT_REQUIRE(p->spp == 0 || n_rays <= RT_RADIANCE_MAX_ITEMS / p->spp, RT_ERR_INVALID, w + ": n_rays * spp > RT_RADIANCE_MAX_ITEMS");
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
    RT_REQUIRE(scene->engine == 1, RT_ERR_UNSUPPORTED, w + ": only the wavefront engine traces caller rays (rt_debug_set_engine)");
}

// The arguments of rt_render_pixels* (host side only, the scene last, like check_radiance). `device`: the buffers are
// rt_render_pixels_device's — ids read as 8-byte words, sums written in 16-byte pieces.
void check_render_pixels(const rt_scene *scene, const rt_camera *cam, const rt_params *p, const void *ids, uint64_t n_entries, const void *out,
                         bool device, const char *who) {
    const std::string w(who);
    RT_REQUIRE(cam && p, RT_ERR_INVALID, w + ": null camera or params");
    check_view(cam, p, w + ": ", "");
    RT_REQUIRE(!(p->flags & ~(RT_FLAG_COUNTERS | RT_FLAG_KERNEL_TIMES)), RT_ERR_INVALID,
               w + ": flag bits other than RT_FLAG_COUNTERS / RT_FLAG_KERNEL_TIMES");
    RT_REQUIRE(n_entries == 0 || (ids && out), RT_ERR_INVALID, w + ": null id or output buffer");
    RT_REQUIRE(!device || n_entries == 0 || !((uintptr_t)ids & 7u), RT_ERR_INVALID, w + ": the id buffer must be 8-byte aligned");
    RT_REQUIRE(!device || n_entries == 0 || !((uintptr_t)out & 15u), RT_ERR_INVALID, w + ": the output buffer must be 16-byte aligned");
    RT_REQUIRE(n_entries <= RT_RADIANCE_MAX_RAYS, RT_ERR_INVALID, w + ": n_entries > RT_RADIANCE_MAX_RAYS");
    const uint32_t chunk = (p->spp_chunk == 0 || p->spp_chunk > p->spp) ? p->spp : p->spp_chunk;
    const uint64_t n_chunks = p->spp == 0 ? 1 : ((uint64_t)p->spp + chunk - 1) / chunk;
    // (a division, not a product: n_entries * n_chunks itself may not fit 64 bits)
    RT_REQUIRE(n_entries <= RT_RADIANCE_MAX_ITEMS / n_chunks, RT_ERR_INVALID, w + ": n_entries * ceil(spp / spp_chunk) > RT_RADIANCE_MAX_ITEMS");
    if (!device) {                                             // (device ids: the counting kernel, PixelCheck)
        const uint64_t limit = (uint64_t)p->width * p->height * p->n_frames;
        const uint64_t *host_ids = static_cast<const uint64_t *>(ids);
        for (uint64_t i = 0; i < n_entries; i++)
            RT_REQUIRE(host_ids[i] < limit, RT_ERR_INVALID, w + ": pixel id out of range (>= width * height * n_frames)");
    }
    RT_REQUIRE(scene, RT_ERR_INVALID, w + ": null scene");
    RT_REQUIRE(scene->engine == 1, RT_ERR_UNSUPPORTED, w + ": only the wavefront engine renders pixel lists (rt_debug_set_engine)");
}

// What is wrong with the parameters of rt_adaptive_plan* (null: nothing) — rt_adaptive_workspace_bytes answers 0 to the same faults.
const char *adaptive_params_fault(const rt_adaptive_params *p) {
    if (!p) return "null params";
    if (p->width == 0 || p->height == 0) return "empty image (width or height is 0)";
    if ((uint64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return "width * height > RT_DENOISE_MAX_PIXELS";
    if (p->max_units == 0) return "max_units is 0";
    if ((uint64_t)p->first_frame + p->max_units > 0xFFFFFFFFull) return "first_frame + max_units > 2^32 - 1";
    if (!(p->scale > 0.0) || std::isinf(p->scale)) return "scale is <= 0, NaN or infinite";
    if (p->flags != 0 || p->_pad != 0) return "flags must be 0";
    return nullptr;
}

// One plan on `stream`: device buffers, the arguments checked. The kernels, then ONE synchronisation behind which the total
// and the row kernel's count are read together.
void run_adaptive_plan(const double *d_err, const uint32_t *d_rows, const rt_adaptive_params *p, uint32_t *d_units, uint64_t *d_offsets,
                       uint64_t *d_entries, uint64_t capacity, char *d_ws, hipStream_t stream, uint64_t *out_total, const std::string &w) {
    AdaptivePlanArgs a{};
    a.width = p->width; a.height = p->height; a.first_frame = p->first_frame; a.max_units = p->max_units; a.scale = p->scale;
    a.err = d_err; a.rows = d_rows; a.units = d_units; a.offsets = d_offsets; a.entries = d_entries; a.capacity = capacity; a.ws = d_ws;
    const AdaptiveLayout l = adaptive_layout(p->width, p->height);
    RT_HIP(launch_adaptive_plan(a, stream));
    unsigned long long total = 0;
    uint32_t bad = 0;
    RT_HIP(hipMemcpyAsync(&total, d_ws + l.totals + l.n_tiles * sizeof(unsigned long long), sizeof total, hipMemcpyDeviceToHost, stream));
    if (d_rows) RT_HIP(hipMemcpyAsync(&bad, d_ws + l.bad_rows, sizeof bad, hipMemcpyDeviceToHost, stream));
    RT_HIP(hipStreamSynchronize(stream));
    RT_REQUIRE(bad == 0, RT_ERR_INVALID, w + ": row_ids is not a permutation of the image's rows");
    if (out_total) *out_total = total;
}

// What is wrong with the parameters of rt_denoise* (null: nothing) — rt_denoise_workspace_bytes answers 0 to the same faults.
const char *denoise_params_fault(const rt_denoise_params *p) {
    if (!p) return "null params";
    if (p->width == 0 || p->height == 0) return "empty image (width or height is 0)";
    if (p->spp == 0) return "spp is 0";
    if (p->n_iter > RT_DENOISE_MAX_ITER) return "n_iter > RT_DENOISE_MAX_ITER";
    for (double s : {p->sigma_color, p->sigma_normal, p->sigma_depth, p->sigma_albedo})
        if (!(s > 0.0)) return "a sigma is <= 0 or NaN";
    if (!(p->albedo_floor > 0.0) || std::isinf(p->albedo_floor)) return "albedo_floor is <= 0, NaN or infinite";
    if (p->flags & ~RT_DENOISE_NO_DEMODULATE) return "flag bits other than RT_DENOISE_NO_DEMODULATE";
    if ((uint64_t)p->width * p->height > RT_DENOISE_MAX_PIXELS) return "width * height > RT_DENOISE_MAX_PIXELS";
    return nullptr;
}

void check_denoise(const double *sum, const rt_feature *feat, const rt_denoise_params *p, const double *out, const std::string &w) {
    const char *fault = denoise_params_fault(p);
    RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
    RT_REQUIRE(sum && feat && out, RT_ERR_INVALID, w + ": null sums, features or output");
}

// Enqueue one denoise on `stream`: device buffers, the arguments checked. `check_rows`: the row list came from the caller's
// HBM — its fault count is read behind one synchronisation of the stream before anything that writes the output is enqueued.
void run_denoise(const double *d_sum, const rt_feature *d_feat, const uint32_t *d_rows, const rt_denoise_params *p, double *d_out,
                 char *d_ws, hipStream_t stream, bool check_rows, const std::string &w) {
    DenoiseArgs a{};
    a.width = p->width; a.height = p->height;
    a.sp = (double)p->spp;
    a.inv_n = 1.0 / (p->sigma_normal * p->sigma_normal);
    a.inv_z = 1.0 / (p->sigma_depth * p->sigma_depth);
    a.inv_a = 1.0 / (p->sigma_albedo * p->sigma_albedo);
    a.albedo_floor = p->albedo_floor;
    a.demodulate = !(p->flags & RT_DENOISE_NO_DEMODULATE);
    a.sum = d_sum; a.feat = d_feat; a.rows = d_rows; a.out = d_out; a.ws = d_ws;
    double inv_c[RT_DENOISE_MAX_ITER];
    for (uint32_t k = 0; k < p->n_iter; k++) {
        const double sigma_k = std::ldexp(p->sigma_color, -(int)k);
        inv_c[k] = 1.0 / (sigma_k * sigma_k);
    }
    if (d_rows) {
        RT_HIP(launch_denoise_rows(a, stream));
        if (check_rows) {
            uint32_t bad = 0;
            RT_HIP(hipMemcpyAsync(&bad, d_ws + denoise_layout(p->width, p->height).bad_rows, sizeof bad, hipMemcpyDeviceToHost, stream));
            RT_HIP(hipStreamSynchronize(stream));
            RT_REQUIRE(bad == 0, RT_ERR_INVALID, w + ": row_ids is not a permutation of the image's rows");
        }
    }
    RT_HIP(launch_denoise(a, p->n_iter, inv_c, stream));
}

// The arguments of rt_denoise_dual*: what rt_denoise* refuses, then the dual filter's own.
void check_denoise_dual(const double *sum_a, const double *sum_b, const rt_feature *feat_a, const rt_feature *feat_b, const rt_denoise_params *p,
                        const rt_denoise_dual_params *q, const double *out, const std::string &w) {
    check_denoise(sum_a, feat_a, p, out, w);
    RT_REQUIRE(q, RT_ERR_INVALID, w + ": null dual params");
    RT_REQUIRE(sum_b && feat_b, RT_ERR_INVALID, w + ": null sums or features of the second half");
    RT_REQUIRE(q->var_iter <= RT_DENOISE_MAX_VAR_ITER, RT_ERR_INVALID, w + ": var_iter > RT_DENOISE_MAX_VAR_ITER");
    RT_REQUIRE(q->var_floor > 0.0 && !std::isinf(q->var_floor), RT_ERR_INVALID, w + ": var_floor is <= 0, NaN or infinite");
    RT_REQUIRE(q->flags == 0, RT_ERR_INVALID, w + ": dual flags must be 0");
}

// Enqueue one dual denoise on `stream`, like run_denoise.
void run_denoise_dual(const double *d_sum_a, const double *d_sum_b, const rt_feature *d_feat_a, const rt_feature *d_feat_b, const uint32_t *d_rows,
                      const rt_denoise_params *p, const rt_denoise_dual_params *q, double *d_out, double *d_out_var, char *d_ws,
                      hipStream_t stream, bool check_rows, const std::string &w) {
    DenoiseDualArgs d{};
    DenoiseArgs &a = d.a;
    a.width = p->width; a.height = p->height;
    a.sp = (double)p->spp;
    a.inv_n = 1.0 / (p->sigma_normal * p->sigma_normal);
    a.inv_z = 1.0 / (p->sigma_depth * p->sigma_depth);
    a.inv_a = 1.0 / (p->sigma_albedo * p->sigma_albedo);
    a.albedo_floor = p->albedo_floor;
    a.demodulate = !(p->flags & RT_DENOISE_NO_DEMODULATE);
    a.sum = d_sum_a; a.feat = d_feat_a; a.rows = d_rows; a.out = d_out; a.ws = d_ws;
    d.sum_b = d_sum_b; d.feat_b = d_feat_b; d.out_var = d_out_var;
    d.sp2 = a.sp + a.sp;
    d.inv_c = 1.0 / (p->sigma_color * p->sigma_color);
    d.var_floor = q->var_floor;
    if (d_rows) {
        RT_HIP(launch_denoise_dual_rows(d, stream));
        if (check_rows) {
            uint32_t bad = 0;
            RT_HIP(hipMemcpyAsync(&bad, d_ws + denoise_dual_layout(p->width, p->height).bad_rows, sizeof bad, hipMemcpyDeviceToHost, stream));
            RT_HIP(hipStreamSynchronize(stream));
            RT_REQUIRE(bad == 0, RT_ERR_INVALID, w + ": row_ids is not a permutation of the image's rows");
        }
    }
    RT_HIP(launch_denoise_dual(d, q->var_iter, p->n_iter, stream));
}

void finish(rt_scene *sc, hipStream_t stream) {
    Workspace &w = workspace_for(sc, stream);
    RT_HIP(hipStreamSynchronize(stream));
    if (w.pending) {
        StatsDev h;
        rt_stats out = read_stats(w.ev0, w.ev1, w.pending_counters ? w.stats.p : nullptr, h);
        if (w.pending_counters) {
            std::lock_guard<std::mutex> lock(sc->mu);
            for (int o = 0; o < 9; o++) { sc->census_rounds[o] = h.op_rounds[o]; sc->census_lanes[o] = h.op_lanes[o]; }
        }
        out.spp_chunk = w.used_chunk; out.passes = w.used_passes; out.pool_slots = w.used_slots;
        out.partial_bytes = w.used_partial_bytes;
        if (w.used_kt) { out.trace_ms = w.kt.trace_ms; out.shade_ms = w.kt.shade_ms; }
        *w.pending = out;
        w.pending = nullptr;
    }
}

} // namespace

extern "C" {

int rt_scene_create(const rt_scene_desc *desc, rt_scene **out) {
    return guarded([&]() -> int {
        RT_REQUIRE(desc && out, RT_ERR_INVALID, "rt_scene_create: null argument");
        RT_REQUIRE(desc->abi_version == RT2022_ABI_VERSION, RT_ERR_INVALID, "rt_scene_create: abi_version mismatch");
        Validator v(*desc);
        v.check_pools();
        v.check_ref(desc->root, "root");
        const Validator::Need root = v.need(desc->root, 0);
        const int32_t need = root.need, xdepth = root.xdepth;
        RT_REQUIRE(need <= kStackLarge, RT_ERR_UNSUPPORTED, "scene needs a deeper traversal stack than the kernel provides");
        RT_REQUIRE(xdepth <= RT_MAX_XFORM_DEPTH, RT_ERR_UNSUPPORTED, "movers nested deeper than RT_MAX_XFORM_DEPTH");
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        RT_REQUIRE(e == hipSuccess && ndev > 0, RT_ERR_DEVICE, "rt_scene_create: no HIP device available (the path has no CPU fallback)");
        std::unique_ptr<rt_scene> sc(new rt_scene());         // (an error below frees what has been uploaded so far)
        if (const char *eg = getenv("RT2022_RING_GROUP")) sc->partial_ring_group = atoi(eg);
        RT_HIP(hipGetDevice(&sc->device));
        RT_HIP(hipDeviceGetAttribute(&sc->n_cus, hipDeviceAttributeMultiprocessorCount, sc->device));
        RT_REQUIRE(sc->n_cus > 0, RT_ERR_DEVICE, "rt_scene_create: device reports no compute units");
        {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b) sc->ring_threshold_bytes = (uint64_t)((double)total_b * 0.4);
        }
        SceneDev &s = sc->dev;
        // Node refs of the device copy follow the breadth-first numbering (breadth_first_nodes).
        const std::vector<uint32_t> new_of = breadth_first_nodes(*desc);
        auto node_ref = [&](uint32_t ref) {
            return RT_REF_KIND(ref) == RT_KIND_NODE ? (ref & ~RT_REF_INDEX_MASK) | new_of[RT_REF_INDEX(ref)] : ref;
        };
        {
            std::vector<rt_bvh_node> nodes(desc->n_nodes);
            for (uint32_t i = 0; i < desc->n_nodes; i++) {
                rt_bvh_node q = desc->nodes[i];
                q.left = node_ref(q.left); q.right = node_ref(q.right);
                // The PUSH REF of the node, for the wavefront traversal kernels (third word of the record's last 16 bytes): what
                // goes on the stack when the box is hit — the right child, or "nothing" (14 << 27, their REF_EMPTY) for a span-1
                // node holding the same plain primitive twice (bvh/mod.rs:44-47), whose second test finds the first one's hit again
                // (counted, not repeated). Media, movers, lists and nodes are really visited twice: they draw from the RNG or recurse.
                const uint32_t lk = RT_REF_KIND(q.left);
                q._pad[0] = (q.left == q.right && lk >= RT_KIND_SPHERE && lk <= RT_KIND_RING) ? (14u << RT_REF_KIND_SHIFT) : q.right;
                nodes[new_of[i]] = q;
            }
            s.nodes = upload(nodes.data(), nodes.size(), sc->owned);
            std::vector<uint32_t> n32((size_t)8 * nodes.size() + 8);         // (never empty: upload of nothing is a null pointer)
            for (size_t i = 0; i < nodes.size(); i++) {
                const rt_bvh_node &q = nodes[i];
                for (int ax = 0; ax < 3; ax++) {
                    const float lo = (float)q.bmin[ax], hi = (float)q.bmax[ax];
                    std::memcpy(&n32[8 * i + 2 * ax], &lo, 4);
                    std::memcpy(&n32[8 * i + 2 * ax + 1], &hi, 4);
                }
                n32[8 * i + 6] = q.left; n32[8 * i + 7] = q._pad[0];
            }
            s.nodes32 = upload(n32.data(), n32.size(), sc->owned);
        }
        // Primitive pools go up with the slot kind of their material packed above the material index (pt_device.h).
        RT_REQUIRE(desc->n_materials <= kMatIndexMask, RT_ERR_UNSUPPORTED, "more than 2^24 materials");
        auto packed = [&](auto *src, uint64_t n) {
            using T = std::remove_const_t<std::remove_pointer_t<decltype(src)>>;
            std::vector<T> v(src, src + n);
            for (T &q : v) {
                const rt_material &m = desc->materials[q.mat];
                uint32_t sk = m.kind == RT_MAT_DIFFUSE_LIGHT ? SK_LIGHT : m.kind == RT_MAT_METAL ? SK_METAL : m.kind == RT_MAT_DIELECTRIC ? SK_DIELECTRIC
                            : m.kind == RT_MAT_ISOTROPIC ? SK_ISOTROPIC : (uint32_t)SK_LAMB_SOLID + desc->textures[m.tex].kind;
                q.mat |= sk << kMatKindShift;
            }
            return upload(v.data(), n, sc->owned);
        };
        s.spheres = packed(desc->spheres, desc->n_spheres);
        s.moving_spheres = packed(desc->moving_spheres, desc->n_moving_spheres);
        s.rects = packed(desc->rects, desc->n_rects);
        s.boxes = packed(desc->boxes, desc->n_boxes);
        s.triangles = packed(desc->triangles, desc->n_triangles);
        s.rings = packed(desc->rings, desc->n_rings);
        {
            std::vector<rt_medium> media(desc->media, desc->media + desc->n_media);
            for (rt_medium &m : media) m.boundary = node_ref(m.boundary);
            s.media = packed(media.data(), media.size());
        }
        {
            std::vector<MediumDev> md(desc->n_media);
            uint32_t n_sph = 0;
            for (uint32_t i = 0; i < desc->n_media; i++) {
                const rt_medium &m = desc->media[i];
                MediumDev &q = md[i];
                std::memset(&q, 0, sizeof q);
                q.neg_inv_density = m.neg_inv_density;
                q.boundary = node_ref(m.boundary);
                q.mat = m.mat | ((uint32_t)SK_ISOTROPIC << kMatKindShift);
                if (RT_REF_KIND(m.boundary) == RT_KIND_SPHERE && !(m.boundary & RT_REF_FLIP)) {
                    const rt_sphere &sp = desc->spheres[RT_REF_INDEX(m.boundary)];
                    q.center[0] = sp.center[0]; q.center[1] = sp.center[1]; q.center[2] = sp.center[2]; q.radius = sp.radius;
                    q.sphere_boundary = 1;
                    n_sph++;
                }
            }
            s.media_dev = upload(md.data(), md.size(), sc->owned);
            s.media_mode = n_sph == 0 ? 0u : n_sph == desc->n_media ? 1u : 2u;
        }
        {
            std::vector<rt_xform> xforms(desc->xforms, desc->xforms + desc->n_xforms);
            for (rt_xform &x : xforms) x.child = node_ref(x.child);
            s.xforms = upload(xforms.data(), xforms.size(), sc->owned);
            std::vector<uint32_t> items(desc->list_items, desc->list_items + desc->n_list_items);
            for (uint32_t &r : items) r = node_ref(r);
            s.list_items = upload(items.data(), items.size(), sc->owned);
        }
        s.lists = upload(desc->lists, desc->n_lists, sc->owned);
        s.lights = upload(desc->lights, desc->n_lights, sc->owned);
        s.materials = upload(desc->materials, desc->n_materials, sc->owned);
        s.textures = upload(desc->textures, desc->n_textures, sc->owned);
        {
            std::vector<MaterialDev> md(desc->n_materials);
            for (uint32_t i = 0; i < desc->n_materials; i++) {
                const rt_material &m = desc->materials[i];
                MaterialDev &q = md[i];
                std::memset(&q, 0, sizeof q);
                q.tex = m.tex;
                std::memcpy(q.albedo, m.albedo, sizeof q.albedo);
                q.param = m.param;
                if (m.kind == RT_MAT_LAMBERTIAN || m.kind == RT_MAT_DIFFUSE_LIGHT || m.kind == RT_MAT_ISOTROPIC) {
                    const rt_texture &t = desc->textures[m.tex];
                    q.tex_kind = t.kind; q.tex_a = t.a; q.tex_b = t.b; q.tex_scale = t.scale;
                    std::memcpy(q.tex_color, t.color, sizeof q.tex_color);
                }
            }
            s.materials_dev = upload(md.data(), md.size(), sc->owned);
        }
        s.images = upload(desc->images, desc->n_images, sc->owned);
        s.image_data = upload(desc->image_data, desc->image_data_bytes, sc->owned);
        s.perlins = upload(desc->perlins, desc->n_perlins, sc->owned);
        s.root = node_ref(desc->root);
        s.n_lights = desc->n_lights;
        s.n_nodes = desc->n_nodes;
        s.n_xforms = desc->n_xforms;
        s.n_media = desc->n_media;
        s.n_spheres = desc->n_spheres;
        s.n_moving_spheres = desc->n_moving_spheres;
        s.n_rects = desc->n_rects;
        sc->stack_need = (uint32_t)need;
        sc->general_boundaries = v.general_boundaries;
        sc->boxes_plain = v.boxes_plain();
        sc->features = ((desc->n_triangles || desc->n_rings) ? kFeatMisc : 0u) |
                       ((desc->n_xforms || desc->n_lists) ? kFeatMovers : 0u) |
                       ((desc->n_boxes || desc->n_media) ? kFeatVolumes : 0u);
        *out = sc.release();
        return RT_OK;
    });
}

int rt_scene_destroy(rt_scene *scene) {
    return guarded([&]() -> int {
        if (!scene) return RT_OK;
        DeviceGuard guard(scene->device);
        for (auto &kv : scene->ws)                    // (asynchronous calls still in flight: let their host threads finish)
            if (kv.second.async_worker.joinable()) kv.second.async_worker.join();
        (void)hipDeviceSynchronize();                 // (every stream of the scene's device, the group streams included)
        delete scene;                                 // (its workspaces, query scratch and pools free themselves, this device current)
        return RT_OK;
    });
}

// Joins the worker of an RT_FLAG_ASYNC call in flight on (scene, stream), if any; returns what it ended with.
static int join_async(rt_scene *scene, hipStream_t stream, std::string *err, bool *joined = nullptr) {
    Workspace &w = workspace_for(scene, stream);
    if (joined) *joined = w.async_worker.joinable();
    if (!w.async_worker.joinable()) return RT_OK;
    w.async_worker.join();
    const int rc = w.async_rc;
    if (err) *err = w.async_err;
    w.async_rc = RT_OK; w.async_err.clear();
    return rc;
}

// One call at a time per (scene, stream): an asynchronous one still in flight there is joined and finished first — its rt_stats,
// as rt_render_wait would have filled them — and its failure is the failure of `who`, the call that found it.
static void finish_previous_async(rt_scene *sc, hipStream_t stream, const char *who) {
    std::string err;
    bool joined = false;
    const int rc = join_async(sc, stream, &err, &joined);
    RT_REQUIRE(rc == RT_OK, rc, std::string(who) + ": the previous asynchronous call on this stream failed: " + err);
    if (joined) finish(sc, stream);
}

int rt_render_device(rt_scene *scene, const rt_camera *cam, const rt_params *params,
                     double *d_out_rgb_sum, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_params(scene, cam, params);
        RT_REQUIRE(d_out_rgb_sum || params->n_rows == 0, RT_ERR_INVALID, "rt_render_device: output is null");
        DeviceGuard guard(scene->device);
        const hipStream_t stream = (hipStream_t)hip_stream;
        finish_previous_async(scene, stream, "rt_render_device");
        if (!(params->flags & RT_FLAG_ASYNC)) {
            enqueue(scene, cam, params, params->row_ids, d_out_rgb_sum, stream, stats, true);
            return RT_OK;
        }
        // RT_FLAG_ASYNC: the engine drives its passes from a host thread (it polls one word per batch) — here a thread of the
        // library's own instead of the caller's. The arguments are copied; the device buffers are the caller's until the wait.
        Workspace &w = workspace_for(scene, stream);
        const rt_camera cam_copy = *cam;
        const rt_params params_copy = *params;
        w.async_rc = RT_OK; w.async_err.clear();
        w.async_worker = std::thread([scene, cam_copy, params_copy, d_out_rgb_sum, stream, stats, &w]() {
            try {
                DeviceGuard worker_guard(scene->device);
                enqueue(scene, &cam_copy, &params_copy, params_copy.row_ids, d_out_rgb_sum, stream, stats, true);
            } catch (const Fail &e) {
                w.async_rc = e.code; w.async_err = e.msg;
            } catch (const std::exception &e) {
                w.async_rc = RT_ERR_INVALID; w.async_err = e.what();
            }
        });
        return RT_OK;
    });
}

int rt_render_wait(rt_scene *scene, void *hip_stream) {
    return guarded([&]() -> int {
        RT_REQUIRE(scene, RT_ERR_INVALID, "rt_render_wait: null scene");
        DeviceGuard guard(scene->device);
        std::string err;
        const int rc = join_async(scene, (hipStream_t)hip_stream, &err);
        RT_REQUIRE(rc == RT_OK, rc, err);
        finish(scene, (hipStream_t)hip_stream);
        return RT_OK;
    });
}

// An rt_radiance* call runs in the render's workspace of (scene, stream): an asynchronous render still in flight there (its host
// thread drives passes on that workspace) is joined and finished first (finish_previous_async), as rt_render_device does. Each
// entry point does so once, before it touches the workspace in any way — rt_radiance before its staging buffers, which live in
// the workspace too.

// One rt_radiance* call on `stream` (the scene's device is current, the arguments checked, finish_previous_async done): the
// passes, and stats.
static void run_radiance(rt_scene *sc, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *rp, double *d_out,
                         hipStream_t stream, rt_stats *stats) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (n_rays == 0) {
        if (stats) stats->spp_chunk = 1;
        return;
    }
    if (rp->spp == 0 || rp->max_depth == 0) {                 // ray_color at depth 0 is black, no sample is black: zeros, no pass
        RT_HIP(hipMemsetAsync(d_out, 0, n_rays * 3 * sizeof(double), stream));
        RT_HIP(hipStreamSynchronize(stream));
        if (stats) { stats->paths = n_rays * rp->spp; stats->spp_chunk = 1; }
        return;
    }
    rt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    rt_params p;
    std::memset(&p, 0, sizeof p);
    p.width = 1; p.height = 1; p.n_frames = 1;                 // (one "pixel" per ray: RenderArgs::rays)
    p.spp = rp->spp; p.max_depth = rp->max_depth;
    std::memcpy(p.background, rp->background, sizeof p.background);
    p.t_min = rp->t_min;
    p.spp_chunk = 1;                                           // one sample per work item: the sum is 0 + L_0 + L_1 + ... in order
    p.flags = rp->flags;
    const RaySource src{d_rays, n_rays};
    enqueue(sc, &cam, &p, nullptr, d_out, stream, stats, false, &src);
    finish(sc, stream);
    if (stats) stats->paths = n_rays * rp->spp;               // (the counter block's own count, also without RT_FLAG_COUNTERS)
}

int rt_radiance(rt_scene *scene, const rt_radiance_ray *rays, uint64_t n_rays, const rt_radiance_params *p, double *out_rgb_sum,
                rt_stats *stats) {
    return guarded([&]() -> int {
        check_radiance(scene, rays, n_rays, p, out_rgb_sum, false, "rt_radiance");
        DeviceGuard guard(scene->device);
        finish_previous_async(scene, nullptr, "rt_radiance");       // (first: the staging buffers below belong to the workspace)
        Workspace &w = workspace_for(scene, nullptr);
        // staging buffers of the workspace, kept for the next call (the calls that used them were synchronous: nothing is in flight)
        w.rad_rays.reserve(n_rays);
        w.rad_out.reserve(n_rays * 3);
        if (n_rays) {
            RT_HIP(hipMemcpy(w.rad_rays, rays, n_rays * sizeof(rt_radiance_ray), hipMemcpyHostToDevice));
            // Poison the output so an unwritten sum cannot pass for a result.
            RT_HIP(hipMemset(w.rad_out, 0xFF, n_rays * 3 * sizeof(double)));
        }
        run_radiance(scene, w.rad_rays, n_rays, p, w.rad_out, nullptr, stats);
        if (n_rays) RT_HIP(hipMemcpy(out_rgb_sum, w.rad_out, n_rays * 3 * sizeof(double), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_radiance_device(rt_scene *scene, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *p,
                       double *d_out_rgb_sum, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_radiance(scene, d_rays, n_rays, p, d_out_rgb_sum, true, "rt_radiance_device");
        DeviceGuard guard(scene->device);
        finish_previous_async(scene, (hipStream_t)hip_stream, "rt_radiance_device");
        run_radiance(scene, d_rays, n_rays, p, d_out_rgb_sum, (hipStream_t)hip_stream, stats);
        return RT_OK;
    });
}

// One rt_render_pixels* call on `stream` (the scene's device is current, the arguments checked, finish_previous_async done;
// host ids already range-checked, device ids checked here or by the enqueue): the passes, and stats.
static void run_render_pixels(rt_scene *sc, const rt_camera *cam, const rt_params *params, const uint64_t *d_ids, uint64_t n_entries,
                              double *d_out, hipStream_t stream, rt_stats *stats, bool check_ids, const char *who) {
    if (stats) std::memset(stats, 0, sizeof *stats);
    uint32_t chunk = (params->spp_chunk == 0 || params->spp_chunk > params->spp) ? params->spp : params->spp_chunk;
    if (chunk == 0) chunk = 1;
    if (n_entries == 0) {
        if (stats) stats->spp_chunk = chunk;
        return;
    }
    if (params->spp == 0 || params->max_depth == 0) {           // no sample, or ray_color at depth 0: zeros, no pass
        Workspace &w = workspace_for(sc, stream);
        if (check_ids) w.pixels.begin(d_ids, n_entries, (uint64_t)params->width * params->height * params->n_frames, stream);
        RT_HIP(hipStreamSynchronize(stream));
        if (check_ids) w.pixels.end(who);
        RT_HIP(hipMemsetAsync(d_out, 0, n_entries * 3 * sizeof(double), stream));
        RT_HIP(hipStreamSynchronize(stream));
        if (stats) { stats->paths = n_entries * params->spp; stats->spp_chunk = chunk; }
        return;
    }
    rt_params p = *params;
    p.n_rows = 0; p.row_ids = nullptr; p.progress_cb = nullptr; p.progress_user = nullptr;
    const PixelSource pix{d_ids, n_entries, check_ids, who};
    enqueue(sc, cam, &p, nullptr, d_out, stream, stats, false, nullptr, &pix);
    finish(sc, stream);
    if (stats) stats->paths = n_entries * params->spp;          // (the counter block's own count, also without RT_FLAG_COUNTERS)
}

int rt_render_pixels(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *pixel_ids, uint64_t n_entries,
                     double *out_rgb_sum, rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_render_pixels";
        check_render_pixels(scene, cam, params, pixel_ids, n_entries, out_rgb_sum, false, who);
        DeviceGuard guard(scene->device);
        finish_previous_async(scene, nullptr, who);             // (first: the staging buffers below belong to the workspace)
        Workspace &w = workspace_for(scene, nullptr);
        w.pix_ids.reserve(n_entries);
        w.rad_out.reserve(n_entries * 3);
        if (n_entries) {
            RT_HIP(hipMemcpy(w.pix_ids, pixel_ids, n_entries * sizeof(uint64_t), hipMemcpyHostToDevice));
            // Poison the output so an unwritten sum cannot pass for a result.
            RT_HIP(hipMemset(w.rad_out, 0xFF, n_entries * 3 * sizeof(double)));
        }
        run_render_pixels(scene, cam, params, w.pix_ids, n_entries, w.rad_out, nullptr, stats, false, who);
        if (n_entries) RT_HIP(hipMemcpy(out_rgb_sum, w.rad_out, n_entries * 3 * sizeof(double), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_render_pixels_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *d_pixel_ids, uint64_t n_entries,
                            double *d_out_rgb_sum, void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        const char *who = "rt_render_pixels_device";
        check_render_pixels(scene, cam, params, d_pixel_ids, n_entries, d_out_rgb_sum, true, who);
        DeviceGuard guard(scene->device);
        finish_previous_async(scene, (hipStream_t)hip_stream, who);
        run_render_pixels(scene, cam, params, d_pixel_ids, n_entries, d_out_rgb_sum, (hipStream_t)hip_stream, stats, true, who);
        return RT_OK;
    });
}

uint64_t rt_adaptive_workspace_bytes(const rt_adaptive_params *p) {
    return adaptive_params_fault(p) ? 0 : adaptive_layout(p->width, p->height).bytes;
}

int rt_adaptive_plan_device(const double *d_err, const uint32_t *d_row_ids, const rt_adaptive_params *p, uint32_t *d_units, uint64_t *d_offsets,
                            uint64_t *d_entries, uint64_t capacity, void *d_workspace, void *hip_stream, uint64_t *out_total) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_plan_device");
        const char *fault = adaptive_params_fault(p);
        RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
        RT_REQUIRE(d_err && d_units && d_offsets, RT_ERR_INVALID, w + ": null error map, units or offsets");
        RT_REQUIRE(d_entries || capacity == 0, RT_ERR_INVALID, w + ": null entries with a capacity");
        RT_REQUIRE(d_workspace, RT_ERR_INVALID, w + ": null workspace");
        RT_REQUIRE(!(((uintptr_t)d_err | (uintptr_t)d_workspace) & 15u), RT_ERR_INVALID, w + ": the error map and the workspace must be 16-byte aligned");
        RT_REQUIRE(!(((uintptr_t)d_offsets | (uintptr_t)d_entries) & 7u), RT_ERR_INVALID, w + ": offsets and entries must be 8-byte aligned");
        RT_REQUIRE(!(((uintptr_t)d_units | (uintptr_t)d_row_ids) & 3u), RT_ERR_INVALID, w + ": units and row_ids must be 4-byte aligned");
        run_adaptive_plan(d_err, d_row_ids, p, d_units, d_offsets, d_entries, capacity, (char *)d_workspace, (hipStream_t)hip_stream, out_total, w);
        return RT_OK;
    });
}

int rt_adaptive_plan(const double *err, const uint32_t *row_ids, const rt_adaptive_params *p, uint32_t *units, uint64_t *offsets,
                     uint64_t *entries, uint64_t capacity, uint64_t *out_total) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_plan");
        const char *fault = adaptive_params_fault(p);
        RT_REQUIRE(!fault, RT_ERR_INVALID, w + ": " + (fault ? fault : ""));
        RT_REQUIRE(err && units && offsets, RT_ERR_INVALID, w + ": null error map, units or offsets");
        RT_REQUIRE(entries || capacity == 0, RT_ERR_INVALID, w + ": null entries with a capacity");
        if (row_ids) {                                         // a permutation of [0, height)?
            std::vector<char> seen(p->height, 0);
            for (uint32_t i = 0; i < p->height; i++) {
                RT_REQUIRE(row_ids[i] < p->height && !seen[row_ids[i]], RT_ERR_INVALID, w + ": row_ids is not a permutation of the image's rows");
                seen[row_ids[i]] = 1;
            }
        }
        const uint64_t n = (uint64_t)p->width * p->height;
        DeviceBuf<double> d_err(n);
        DeviceBuf<uint32_t> d_rows(row_ids ? p->height : 0), d_units(n);
        DeviceBuf<uint64_t> d_offsets(n + 1), d_entries(capacity);
        DeviceBuf<char> d_ws(adaptive_layout(p->width, p->height).bytes);
        RT_HIP(hipMemcpy(d_err, err, n * sizeof(double), hipMemcpyHostToDevice));
        if (row_ids) RT_HIP(hipMemcpy(d_rows, row_ids, p->height * sizeof(uint32_t), hipMemcpyHostToDevice));
        uint64_t total = 0;
        run_adaptive_plan(d_err, row_ids ? d_rows.p : nullptr, p, d_units, d_offsets, capacity ? d_entries.p : nullptr, capacity, d_ws, nullptr, &total, w);
        RT_HIP(hipMemcpy(units, d_units, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        RT_HIP(hipMemcpy(offsets, d_offsets, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (total && total <= capacity) RT_HIP(hipMemcpy(entries, d_entries, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (out_total) *out_total = total;
        return RT_OK;
    });
}

int rt_adaptive_merge_device(const double *d_entry_sums, const uint32_t *d_units, const uint64_t *d_offsets, uint64_t n_pixels, uint32_t spp,
                             double *d_acc_sum, double *d_acc_n, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_merge_device");
        RT_REQUIRE(n_pixels <= RT_DENOISE_MAX_PIXELS, RT_ERR_INVALID, w + ": n_pixels > RT_DENOISE_MAX_PIXELS");
        if (n_pixels == 0) return RT_OK;
        RT_REQUIRE(d_entry_sums && d_units && d_offsets && d_acc_sum && d_acc_n, RT_ERR_INVALID, w + ": null buffer");
        RT_REQUIRE(!(((uintptr_t)d_entry_sums | (uintptr_t)d_offsets | (uintptr_t)d_acc_sum | (uintptr_t)d_acc_n) & 7u), RT_ERR_INVALID,
                   w + ": sums, offsets and accumulators must be 8-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_units & 3u), RT_ERR_INVALID, w + ": units must be 4-byte aligned");
        RT_HIP(launch_adaptive_merge(d_entry_sums, d_units, d_offsets, n_pixels, spp, d_acc_sum, d_acc_n, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

int rt_adaptive_resolve_device(const double *d_acc_sum, const double *d_acc_n, uint64_t n_pixels, uint32_t spp_out, double *d_out, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_adaptive_resolve_device");
        RT_REQUIRE(n_pixels <= RT_DENOISE_MAX_PIXELS, RT_ERR_INVALID, w + ": n_pixels > RT_DENOISE_MAX_PIXELS");
        if (n_pixels == 0) return RT_OK;
        RT_REQUIRE(d_acc_sum && d_acc_n && d_out, RT_ERR_INVALID, w + ": null buffer");
        RT_REQUIRE(!(((uintptr_t)d_acc_sum | (uintptr_t)d_acc_n | (uintptr_t)d_out) & 7u), RT_ERR_INVALID, w + ": the buffers must be 8-byte aligned");
        RT_HIP(launch_adaptive_resolve(d_acc_sum, d_acc_n, n_pixels, spp_out, d_out, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

int rt_intersect(rt_scene *scene, const rt_query_ray *rays, uint64_t n_rays, uint32_t flags, rt_hit *out_hits, rt_stats *stats) {
    return guarded([&]() -> int {
        check_query(scene, rays, n_rays, flags, out_hits, "rt_intersect");
        if (n_rays == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        RT_REQUIRE(n_rays <= (1ull << 40), RT_ERR_INVALID, "rt_intersect: n_rays too large");
        DeviceGuard guard(scene->device);
        DeviceBuf<rt_query_ray> d_rays(n_rays);                // (after the guard: freed with the scene's device current)
        DeviceBuf<rt_hit> d_hits(n_rays);
        RT_HIP(hipMemcpy(d_rays, rays, n_rays * sizeof(rt_query_ray), hipMemcpyHostToDevice));
        run_query(scene, d_rays, n_rays, flags, d_hits, nullptr, stats);
        RT_HIP(hipMemcpy(out_hits, d_hits, n_rays * sizeof(rt_hit), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_intersect_device(rt_scene *scene, const rt_query_ray *d_rays, uint64_t n_rays, uint32_t flags, rt_hit *d_out_hits,
                        void *hip_stream, rt_stats *stats) {
    return guarded([&]() -> int {
        check_query(scene, d_rays, n_rays, flags, d_out_hits, "rt_intersect_device");
        RT_REQUIRE(n_rays == 0 || !(((uintptr_t)d_rays | (uintptr_t)d_out_hits) & 15u), RT_ERR_INVALID,
                   "rt_intersect_device: ray and hit buffers must be 16-byte aligned");
        if (n_rays == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        run_query(scene, d_rays, n_rays, flags, d_out_hits, (hipStream_t)hip_stream, stats);
        return RT_OK;
    });
}

int rt_features(rt_scene *scene, const rt_camera *cam, const rt_params *params, rt_feature *out_features, rt_stats *stats) {
    return guarded([&]() -> int {
        check_features(scene, cam, params, out_features, false, "rt_features");
        const uint64_t n_pixels = (uint64_t)params->n_rows * params->width;
        if (n_pixels == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        if (params->spp == 0) {                                // zeros, and nothing for the device to do
            if (stats) std::memset(stats, 0, sizeof *stats);
            std::memset(out_features, 0, n_pixels * sizeof(rt_feature));
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        DeviceBuf<uint32_t> d_rows(params->n_rows);            // (after the guard: freed with the scene's device current)
        DeviceBuf<rt_feature> d_out(n_pixels);
        RT_HIP(hipMemcpy(d_rows, params->row_ids, params->n_rows * sizeof(uint32_t), hipMemcpyHostToDevice));
        // Poison the output so an unwritten record cannot pass for a result.
        RT_HIP(hipMemset(d_out, 0xFF, n_pixels * sizeof(rt_feature)));
        run_features(scene, cam, params, d_rows, d_out, nullptr, stats, false, "rt_features");
        RT_HIP(hipMemcpy(out_features, d_out, n_pixels * sizeof(rt_feature), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

int rt_features_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, rt_feature *d_out_features, void *hip_stream,
                       rt_stats *stats) {
    return guarded([&]() -> int {
        check_features(scene, cam, params, d_out_features, true, "rt_features_device");
        if ((uint64_t)params->n_rows * params->width == 0) {
            if (stats) std::memset(stats, 0, sizeof *stats);
            return RT_OK;
        }
        DeviceGuard guard(scene->device);
        run_features(scene, cam, params, params->row_ids, d_out_features, (hipStream_t)hip_stream, stats, true, "rt_features_device");
        return RT_OK;
    });
}

uint64_t rt_denoise_workspace_bytes(const rt_denoise_params *p) {
    return denoise_params_fault(p) ? 0 : denoise_layout(p->width, p->height).bytes;
}

int rt_denoise_device(const double *d_rgb_sum, const rt_feature *d_features, const uint32_t *d_row_ids, const rt_denoise_params *p,
                      double *d_out_rgb_sum, void *d_workspace, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_device");
        check_denoise(d_rgb_sum, d_features, p, d_out_rgb_sum, w);
        RT_REQUIRE(d_workspace, RT_ERR_INVALID, w + ": null workspace");
        RT_REQUIRE(!(((uintptr_t)d_rgb_sum | (uintptr_t)d_features | (uintptr_t)d_out_rgb_sum | (uintptr_t)d_workspace) & 15u), RT_ERR_INVALID,
                   w + ": the buffers and the workspace must be 16-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_row_ids & 3u), RT_ERR_INVALID, w + ": row_ids must be 4-byte aligned");
        run_denoise(d_rgb_sum, d_features, d_row_ids, p, d_out_rgb_sum, (char *)d_workspace, (hipStream_t)hip_stream, true, w);
        return RT_OK;
    });
}

int rt_denoise(const double *rgb_sum, const rt_feature *features, const uint32_t *row_ids, const rt_denoise_params *p,
               double *out_rgb_sum, double *ms) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise");
        check_denoise(rgb_sum, features, p, out_rgb_sum, w);
        if (row_ids) {                                         // a permutation of [0, height)?
            std::vector<char> seen(p->height, 0);
            for (uint32_t i = 0; i < p->height; i++) {
                RT_REQUIRE(row_ids[i] < p->height && !seen[row_ids[i]], RT_ERR_INVALID, w + ": row_ids is not a permutation of the image's rows");
                seen[row_ids[i]] = 1;
            }
        }
        const uint64_t n = (uint64_t)p->width * p->height;
        DeviceBuf<double> d_sum(3 * n);                        // (filtered in place)
        DeviceBuf<rt_feature> d_feat(n);
        DeviceBuf<uint32_t> d_rows(row_ids ? p->height : 0);
        DeviceBuf<char> d_ws(denoise_layout(p->width, p->height).bytes);
        Event ev0{hipEventDefault}, ev1{hipEventDefault};
        RT_HIP(hipMemcpy(d_sum, rgb_sum, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_feat, features, n * sizeof(rt_feature), hipMemcpyHostToDevice));
        if (row_ids) RT_HIP(hipMemcpy(d_rows, row_ids, p->height * sizeof(uint32_t), hipMemcpyHostToDevice));
        RT_HIP(hipEventRecord(ev0, nullptr));
        run_denoise(d_sum, d_feat, row_ids ? d_rows.p : nullptr, p, d_sum, d_ws, nullptr, false, w);
        RT_HIP(hipEventRecord(ev1, nullptr));
        RT_HIP(hipStreamSynchronize(nullptr));
        RT_HIP(hipMemcpy(out_rgb_sum, d_sum, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        if (ms) {
            float t = 0.f;
            RT_HIP(hipEventElapsedTime(&t, ev0, ev1));
            *ms = (double)t;
        }
        return RT_OK;
    });
}

uint64_t rt_denoise_dual_workspace_bytes(const rt_denoise_params *p) {
    return denoise_params_fault(p) ? 0 : denoise_dual_layout(p->width, p->height).bytes;
}

int rt_denoise_dual_device(const double *d_sum_a, const double *d_sum_b, const rt_feature *d_feat_a, const rt_feature *d_feat_b,
                           const uint32_t *d_row_ids, const rt_denoise_params *p, const rt_denoise_dual_params *q, double *d_out_rgb_sum,
                           double *d_out_variance, void *d_workspace, void *hip_stream) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_dual_device");
        check_denoise_dual(d_sum_a, d_sum_b, d_feat_a, d_feat_b, p, q, d_out_rgb_sum, w);
        RT_REQUIRE(d_workspace, RT_ERR_INVALID, w + ": null workspace");
        RT_REQUIRE(!(((uintptr_t)d_sum_a | (uintptr_t)d_sum_b | (uintptr_t)d_feat_a | (uintptr_t)d_feat_b | (uintptr_t)d_out_rgb_sum |
                      (uintptr_t)d_out_variance | (uintptr_t)d_workspace) & 15u),
                   RT_ERR_INVALID, w + ": the buffers and the workspace must be 16-byte aligned");
        RT_REQUIRE(!((uintptr_t)d_row_ids & 3u), RT_ERR_INVALID, w + ": row_ids must be 4-byte aligned");
        run_denoise_dual(d_sum_a, d_sum_b, d_feat_a, d_feat_b, d_row_ids, p, q, d_out_rgb_sum, d_out_variance, (char *)d_workspace,
                         (hipStream_t)hip_stream, true, w);
        return RT_OK;
    });
}

int rt_denoise_dual(const double *sum_a, const double *sum_b, const rt_feature *feat_a, const rt_feature *feat_b, const uint32_t *row_ids,
                    const rt_denoise_params *p, const rt_denoise_dual_params *q, double *out_rgb_sum, double *out_variance, double *ms) {
    return guarded([&]() -> int {
        const std::string w("rt_denoise_dual");
        check_denoise_dual(sum_a, sum_b, feat_a, feat_b, p, q, out_rgb_sum, w);
        if (row_ids) {                                         // a permutation of [0, height)?
            std::vector<char> seen(p->height, 0);
            for (uint32_t i = 0; i < p->height; i++) {
                RT_REQUIRE(row_ids[i] < p->height && !seen[row_ids[i]], RT_ERR_INVALID, w + ": row_ids is not a permutation of the image's rows");
                seen[row_ids[i]] = 1;
            }
        }
        const uint64_t n = (uint64_t)p->width * p->height;
        DeviceBuf<double> d_a(3 * n), d_b(3 * n);              // (A is filtered in place)
        DeviceBuf<rt_feature> d_fa(n), d_fb(n);
        DeviceBuf<double> d_var(out_variance ? n : 0);
        DeviceBuf<uint32_t> d_rows(row_ids ? p->height : 0);
        DeviceBuf<char> d_ws(denoise_dual_layout(p->width, p->height).bytes);
        Event ev0{hipEventDefault}, ev1{hipEventDefault};
        RT_HIP(hipMemcpy(d_a, sum_a, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_b, sum_b, 3 * n * sizeof(double), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_fa, feat_a, n * sizeof(rt_feature), hipMemcpyHostToDevice));
        RT_HIP(hipMemcpy(d_fb, feat_b, n * sizeof(rt_feature), hipMemcpyHostToDevice));
        if (row_ids) RT_HIP(hipMemcpy(d_rows, row_ids, p->height * sizeof(uint32_t), hipMemcpyHostToDevice));
        RT_HIP(hipEventRecord(ev0, nullptr));
        run_denoise_dual(d_a, d_b, d_fa, d_fb, row_ids ? d_rows.p : nullptr, p, q, d_a, out_variance ? d_var.p : nullptr, d_ws, nullptr, false, w);
        RT_HIP(hipEventRecord(ev1, nullptr));
        RT_HIP(hipStreamSynchronize(nullptr));
        RT_HIP(hipMemcpy(out_rgb_sum, d_a, 3 * n * sizeof(double), hipMemcpyDeviceToHost));
        if (out_variance) RT_HIP(hipMemcpy(out_variance, d_var, n * sizeof(double), hipMemcpyDeviceToHost));
        if (ms) {
            float t = 0.f;
            RT_HIP(hipEventElapsedTime(&t, ev0, ev1));
            *ms = (double)t;
        }
        return RT_OK;
    });
}

int rt_render(rt_scene *scene, const rt_camera *cam, const rt_params *params, double *out_rgb_sum, rt_stats *stats) {
    return guarded([&]() -> int {
        check_params(scene, cam, params);
        RT_REQUIRE(out_rgb_sum || params->n_rows == 0, RT_ERR_INVALID, "rt_render: output is null");
        for (uint32_t i = 0; i < params->n_rows; i++)
            RT_REQUIRE(params->row_ids[i] < (uint64_t)params->height * params->n_frames, RT_ERR_INVALID, "rt_render: row id out of range");
        uint64_t n_values = (uint64_t)params->n_rows * params->width * 3;
        DeviceGuard guard(scene->device);
        DeviceBuf<uint32_t> d_rows(params->n_rows ? params->n_rows : 1);     // (after the guard: freed with the scene's device current)
        DeviceBuf<double> d_out(n_values ? n_values : 1);
        if (params->n_rows) RT_HIP(hipMemcpy(d_rows, params->row_ids, params->n_rows * sizeof(uint32_t), hipMemcpyHostToDevice));
        // Poison the output so an unwritten pixel cannot pass for a result.
        RT_HIP(hipMemset(d_out, 0xFF, (n_values ? n_values : 1) * sizeof(double)));
        enqueue(scene, cam, params, d_rows, d_out, nullptr, stats);
        finish(scene, nullptr);
        if (n_values) RT_HIP(hipMemcpy(out_rgb_sum, d_out, n_values * sizeof(double), hipMemcpyDeviceToHost));
        return RT_OK;
    });
}

// ---- one call, several GPUs (rt2022.h) ----------------------------------------------------------------------
struct rt_scene_set {
    std::vector<int> devices;
    std::vector<rt_scene *> scenes;
};

int rt_scene_set_create(const rt_scene_desc *desc, uint64_t device_mask, rt_scene_set **out) {
    return guarded([&]() -> int {
        RT_REQUIRE(desc && out, RT_ERR_INVALID, "rt_scene_set_create: null argument");
        RT_REQUIRE(device_mask != 0, RT_ERR_INVALID, "rt_scene_set_create: empty device mask");
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        RT_REQUIRE(e == hipSuccess && ndev > 0, RT_ERR_DEVICE, "rt_scene_set_create: no HIP device available (the path has no CPU fallback)");
        RT_REQUIRE(ndev >= 64 || (device_mask >> ndev) == 0, RT_ERR_DEVICE, "rt_scene_set_create: device_mask names a device this process cannot see");
        int prev = 0;
        RT_HIP(hipGetDevice(&prev));
        rt_scene_set *set = new rt_scene_set();
        int rc = RT_OK;
        for (int d = 0; d < ndev && d < 64 && rc == RT_OK; d++) {
            if (!((device_mask >> d) & 1ull)) continue;
            if (hipSetDevice(d) != hipSuccess) { set_error("rt_scene_set_create: hipSetDevice failed"); rc = RT_ERR_DEVICE; break; }
            rt_scene *sc = nullptr;
            rc = rt_scene_create(desc, &sc);                   // (leaves its own message on failure)
            if (rc == RT_OK) { set->devices.push_back(d); set->scenes.push_back(sc); }
        }
        (void)hipSetDevice(prev);
        if (rc != RT_OK) {
            std::string msg = rt_last_error();
            for (rt_scene *sc : set->scenes) (void)rt_scene_destroy(sc);
            delete set;
            set_error(msg);
            return rc;
        }
        *out = set;
        return RT_OK;
    });
}

int rt_scene_set_destroy(rt_scene_set *set) {
    return guarded([&]() -> int {
        if (!set) return RT_OK;
        for (rt_scene *sc : set->scenes) (void)rt_scene_destroy(sc);
        delete set;
        return RT_OK;
    });
}

int rt_render_multi(rt_scene_set *set, const rt_camera *cam, const rt_params *params, double *out_rgb_sum, rt_stats *stats) {
    return guarded([&]() -> int {
        RT_REQUIRE(set && !set->scenes.empty() && cam && params, RT_ERR_INVALID, "rt_render_multi: null argument");
        RT_REQUIRE(params->n_rows == 0 || (params->row_ids && out_rgb_sum), RT_ERR_INVALID, "rt_render_multi: null rows or output");
        const size_t n = set->scenes.size();
        const size_t row_doubles = (size_t)params->width * 3;
        struct Share {
            std::vector<uint32_t> rows;
            std::vector<double> out;
            rt_stats st;
            int rc = RT_OK;
            std::string err;
        };
        std::vector<Share> shares(n);
        for (uint32_t i = 0; i < params->n_rows; i++) shares[i % n].rows.push_back(params->row_ids[i]);
        std::vector<std::thread> workers;
        for (size_t k = 0; k < n; k++) {
            workers.emplace_back([&, k]() {
                Share &sh = shares[k];
                std::memset(&sh.st, 0, sizeof sh.st);
                rt_params p = *params;
                p.n_rows = (uint32_t)sh.rows.size();
                p.row_ids = sh.rows.data();
                // per-worker progress: this device's share under its place in the set (main.rs:124-127: one bar per thread)
                struct Relay { void (*cb)(void *, uint32_t, uint64_t, uint64_t); void *user; uint32_t worker; } relay{params->progress_cb, params->progress_user, (uint32_t)k};
                if (params->progress_cb) {
                    p.progress_user = &relay;
                    p.progress_cb = [](void *u, uint32_t, uint64_t done, uint64_t total) { const Relay *r = static_cast<const Relay *>(u); r->cb(r->user, r->worker, done, total); };
                }
                sh.out.resize(sh.rows.size() * row_doubles);
                // (rt_render makes the scene's device current for this thread and leaves the caller's alone)
                sh.rc = rt_render(set->scenes[k], cam, &p, sh.out.data(), &sh.st);
                if (sh.rc != RT_OK) sh.err = rt_last_error();
            });
        }
        for (std::thread &t : workers) t.join();
        for (size_t k = 0; k < n; k++)
            if (shares[k].rc != RT_OK) throw Fail{shares[k].rc, "rt_render_multi: device " + std::to_string(set->devices[k]) + ": " + shares[k].err};
        std::vector<size_t> taken(n, 0);
        for (uint32_t i = 0; i < params->n_rows; i++) {
            Share &sh = shares[i % n];
            std::memcpy(out_rgb_sum + (size_t)i * row_doubles, sh.out.data() + taken[i % n]++ * row_doubles, row_doubles * sizeof(double));
        }
        if (stats) {
            rt_stats tot;
            std::memset(&tot, 0, sizeof tot);
            for (const Share &sh : shares) {
                tot.paths += sh.st.paths; tot.rays += sh.st.rays; tot.node_visits += sh.st.node_visits;
                for (int k = 0; k < RT_KIND_COUNT; k++) tot.prim_tests[k] += sh.st.prim_tests[k];
                tot.light_pdf_tests += sh.st.light_pdf_tests; tot.rng_draws += sh.st.rng_draws;
                tot.ms = sh.st.ms > tot.ms ? sh.st.ms : tot.ms;
                tot.trace_ms = sh.st.trace_ms > tot.trace_ms ? sh.st.trace_ms : tot.trace_ms;
                tot.shade_ms = sh.st.shade_ms > tot.shade_ms ? sh.st.shade_ms : tot.shade_ms;
                tot.spp_chunk = sh.st.spp_chunk; tot.passes = sh.st.passes > tot.passes ? sh.st.passes : tot.passes;
                tot.pool_slots += sh.st.pool_slots;
            }
            *stats = tot;
        }
        return RT_OK;
    });
}

int rt_tonemap_device(const double *d_rgb_sum, uint64_t n_pixels, int32_t spp, uint8_t *d_rgb8, void *hip_stream) {
    return guarded([&]() -> int {
        RT_REQUIRE((d_rgb_sum && d_rgb8) || n_pixels == 0, RT_ERR_INVALID, "rt_tonemap_device: null argument");
        if (n_pixels) RT_HIP(launch_tonemap(d_rgb_sum, n_pixels, spp, d_rgb8, (hipStream_t)hip_stream));
        return RT_OK;
    });
}

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

} // extern "C"

// ---- HBM counter calibration (tools/traffic_calib.sh) -------------------------------------------------------------
// MI355X_MICROARCH.md: FETCH_SIZE / WRITE_SIZE are calibrated for wide streaming accesses only ("calibrate on a known
// byte count in your own access pattern before trusting an absolute"). These kernels move a KNOWN number of bytes in
// the path pool's patterns — a 128-byte record per slot, slots visited in random order over a buffer far larger than
// the 256 MiB Infinity Cache — so that the counters read under rocprofv3 can be set against them.
namespace {
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
} // namespace

extern "C" {

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

} // extern "C"

// ---- VALU counter calibration (tools/valu_calib.sh) ------------------------------------------------------------------
// What do SQ_INSTS_VALU / SQ_ACTIVE_INST_VALU / SQ_THREAD_CYCLES_VALU / SQ_BUSY_CYCLES read for a kernel whose vector
// pipes are KNOWN to be saturated? These kernels issue nothing but independent vector instructions of one kind at 8
// waves per SIMD on every CU, so their issue-slot occupancy is 1 by construction; the counters read under rocprofv3 give
// the normalisation bench.py uses to turn the traversal kernel's counters into a measured busy fraction.
namespace {
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
        if (spheres_in_lds) *spheres_in_lds = v[3];           // (bit 0: the sphere pools are in LDS; bit 1: node boxes are tested in single precision)
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
