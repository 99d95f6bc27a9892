// rt_scene.hip — rt_scene_create / rt_scene_destroy and the scene sets: a checked description (host/scene_check.cpp) goes up
// into HBM. No CPU fallback exists: without a HIP device the call reports RT_ERR_DEVICE.
#include <cstdlib>
#include <type_traits>

#include "rt_internal.hpp"

using namespace rt2022;

static_assert(kStackTiers[0] == kStackTiny && kStackTiers[1] == kStackSmall && kStackTiers[2] == kStackMid && kStackTiers[3] == kStackLarge,
              "child_order (host/scene_check.cpp) bounds the ordered traversal's stack need by the capacities wf_trace is built with");

namespace {

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

} // namespace

extern "C" {

int rt_scene_create(const rt_scene_desc *desc, rt_scene **out) {
    return guarded([&]() -> int {
        RT_REQUIRE(desc && out, RT_ERR_INVALID, "rt_scene_create: null argument");
        RT_REQUIRE(desc->abi_version == RT2022_ABI_VERSION, RT_ERR_INVALID, "rt_scene_create: abi_version mismatch");
        const SceneFacts facts = check_scene(*desc);
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        RT_REQUIRE(e == hipSuccess && ndev > 0, RT_ERR_DEVICE, "rt_scene_create: no HIP device available (the path has no CPU fallback)");
        std::unique_ptr<rt_scene> sc(new rt_scene(facts));         // (an error below frees what has been uploaded so far)
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
        // ... and, where the timed wavefront traversal reads them, carry the node's child order in bits 24..26 (child_order).
        const ChildOrder ord = child_order(*desc);
        auto node_ref_ord = [&](uint32_t ref) {
            return RT_REF_KIND(ref) == RT_KIND_NODE ? node_ref(ref) | ((uint32_t)ord.order[RT_REF_INDEX(ref)] << kOrderShift) : ref;
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
                // (Both last words are the timed wavefront kernels': the push ref and the left child again, node refs with their order bits.)
                q._pad[0] = (q.left == q.right && lk >= RT_KIND_SPHERE && lk <= RT_KIND_RING) ? (14u << RT_REF_KIND_SHIFT) : node_ref_ord(desc->nodes[i].right);
                q._pad[1] = node_ref_ord(desc->nodes[i].left);
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
                n32[8 * i + 6] = q._pad[1]; n32[8 * i + 7] = q._pad[0];
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
            for (uint32_t i = 0; i < desc->n_xforms; i++) xforms[i].child = node_ref_ord(desc->xforms[i].child);
            s.xforms_ord = upload(xforms.data(), xforms.size(), sc->owned);
            for (uint32_t i = 0; i < desc->n_list_items; i++) items[i] = node_ref_ord(desc->list_items[i]);
            s.list_items_ord = upload(items.data(), items.size(), sc->owned);
        }
        s.root_ord = node_ref_ord(desc->root);
        s.node_index_mask = ord.usable ? (1u << kOrderShift) - 1u : RT_REF_INDEX_MASK;
        s.prim_rank = ord.usable ? upload(ord.rank.data(), ord.rank.size(), sc->owned) : nullptr;
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
        sc->n_materials = desc->n_materials;
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

// ---- one call, several GPUs (rt2022.h) ----------------------------------------------------------------------
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

} // extern "C"
