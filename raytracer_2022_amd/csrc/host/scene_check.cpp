// scene_check.cpp — validation of a scene description (the host half of rt_scene_create): pure host arithmetic, no HIP.
#include "scene_check.hpp"

#include <algorithm>
#include <cmath>
#include <string>

#include "rt_constants.hpp"
#include "rt_error.hpp"

namespace rt2022 {
namespace {

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
    // Node boxes as the reference builds them (min / max of real coordinates): finite and ordered. And the corners of every
    // Boxes object finite: a plain ray then meets no NaN between two faces of one (wf_trace: t_accept, `tainted`).
    bool boxes_plain() const {
        for (uint32_t i = 0; i < d.n_nodes; i++)
            for (int a = 0; a < 3; a++) {
                double lo = d.nodes[i].bmin[a], hi = d.nodes[i].bmax[a];
                if (!(std::isfinite(lo) && std::isfinite(hi) && lo <= hi)) return false;
            }
        for (uint32_t i = 0; i < d.n_boxes; i++)
            for (int a = 0; a < 3; a++)
                if (!(std::isfinite(d.boxes[i].p0[a]) && std::isfinite(d.boxes[i].p1[a]))) return false;
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

} // namespace

SceneFacts check_scene(const rt_scene_desc &d) {
    Validator v(d);
    v.check_pools();
    v.check_ref(d.root, "root");
    const Validator::Need root = v.need(d.root, 0);
    RT_REQUIRE(root.need <= kStackLarge, RT_ERR_UNSUPPORTED, "scene needs a deeper traversal stack than the kernel provides");
    RT_REQUIRE(root.xdepth <= RT_MAX_XFORM_DEPTH, RT_ERR_UNSUPPORTED, "movers nested deeper than RT_MAX_XFORM_DEPTH");
    const unsigned features = ((d.n_triangles || d.n_rings) ? kFeatMisc : 0u) | ((d.n_xforms || d.n_lists) ? kFeatMovers : 0u) |
                              ((d.n_boxes || d.n_media) ? kFeatVolumes : 0u);
    return SceneFacts{(uint32_t)root.need, root.xdepth, v.general_boundaries, v.boxes_plain(), features};
}

// New index of every BVH node in the device copy: breadth-first from the root, through movers, lists and medium
// boundaries. The traversal kernels keep the FIRST records of the node table in LDS (pt_wavefront_trace.hip); numbered this
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

// ---- child order of the timed wavefront traversal -----------------------------------------------------------------------
namespace {

struct OrderWalk {
    const rt_scene_desc &d;
    ChildOrder &out;
    std::vector<int8_t> node_medium, xform_medium, list_medium;      // -1: not walked yet
    std::vector<char> node_seen;
    uint32_t next_rank = 0;
    bool shared = false;
    static constexpr uint32_t kNoRank = 0xFFFFFFFFu;
    OrderWalk(const rt_scene_desc &desc, ChildOrder &o)
        : d(desc), out(o), node_medium(desc.n_nodes, -1), xform_medium(desc.n_xforms, -1), list_medium(desc.n_lists, -1), node_seen(desc.n_nodes, 0) {}

    static bool is_prim(uint32_t kind) { return kind >= RT_KIND_SPHERE && kind <= RT_KIND_RING; }

    // (a) a ConstantMedium below `ref` — through nodes, lists and movers; a medium's own boundary counts as holding one.
    bool holds_medium(uint32_t ref) {
        const uint32_t kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        if (kind == RT_KIND_MEDIUM) return true;
        if (is_prim(kind)) return false;
        int8_t &memo = kind == RT_KIND_NODE ? node_medium[idx] : kind == RT_KIND_LIST ? list_medium[idx] : xform_medium[idx];
        if (memo >= 0) return memo != 0;
        bool m = false;
        if (kind == RT_KIND_NODE) {
            m = holds_medium(d.nodes[idx].left);
            m = holds_medium(d.nodes[idx].right) || m;
        } else if (kind == RT_KIND_LIST) {
            for (uint32_t i = 0; i < d.lists[idx].count; i++) m = holds_medium(d.list_items[d.lists[idx].first + i]) || m;
        } else {
            m = holds_medium(d.xforms[idx].child);
        }
        memo = m ? 1 : 0;
        return m;
    }

    // Every node of a medium's boundary counts as holding one: the boundary queries are the medium's own.
    void mark_boundary(uint32_t ref) {
        const uint32_t kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        if (kind == RT_KIND_NODE) {
            if (out.medium[idx] == 2) return;
            out.medium[idx] = 2;                                  // (2 while marking: a shared subtree is walked once)
            mark_boundary(d.nodes[idx].left);
            mark_boundary(d.nodes[idx].right);
        } else if (kind == RT_KIND_LIST) {
            for (uint32_t i = 0; i < d.lists[idx].count; i++) mark_boundary(d.list_items[d.lists[idx].first + i]);
        } else if (kind >= RT_KIND_TRANSLATE && kind <= RT_KIND_ZOOM) {
            mark_boundary(d.xforms[idx].child);
        }
    }

    // Ranks: the reference's depth-first order of what the main query can accept — left before right, a list's items in turn.
    // A medium is one such candidate; its boundary answers the medium's own two queries and is not walked (the final scene's
    // subsurface ball is a world object and a boundary at once).
    uint32_t &rank_of(uint32_t kind, uint32_t idx) { return out.rank[out.rank[kind] + idx]; }
    void rank_walk(uint32_t ref) {
        const uint32_t kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        if (is_prim(kind) || kind == RT_KIND_MEDIUM) {
            if (rank_of(kind, idx) != kNoRank) shared = true;
            else rank_of(kind, idx) = next_rank++;
        } else if (kind == RT_KIND_NODE) {
            if (node_seen[idx]) { shared = true; return; }
            node_seen[idx] = 1;
            rank_walk(d.nodes[idx].left);
            if (d.nodes[idx].right != d.nodes[idx].left) rank_walk(d.nodes[idx].right);       // (a span-1 twin: one primitive, one rank)
        } else if (kind == RT_KIND_LIST) {
            for (uint32_t i = 0; i < d.lists[idx].count; i++) rank_walk(d.list_items[d.lists[idx].first + i]);
        } else {
            rank_walk(d.xforms[idx].child);
        }
    }

    // min + max of the child's box per axis — twice its centre: a node's record, or the reference's own bounding_box of the
    // primitive (sphere.rs:68-73,167-177, aarect.rs:40-45,123-128,206-211, boxes.rs:77-79, triangle.rs:79-92, ring.rs:55-62).
    bool centre2(uint32_t ref, double c[3]) const {
        const uint32_t kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        if (ref & RT_REF_FLIP) return false;
        switch (kind) {
            case RT_KIND_NODE:
                for (int a = 0; a < 3; a++) c[a] = d.nodes[idx].bmin[a] + d.nodes[idx].bmax[a];
                return true;
            case RT_KIND_SPHERE: {
                const rt_sphere &s = d.spheres[idx];
                for (int a = 0; a < 3; a++) c[a] = (s.center[a] - s.radius) + (s.center[a] + s.radius);
                return true;
            }
            case RT_KIND_MOVING_SPHERE: {                         // the union of its boxes at time0 and time1: center0's and center1's
                const rt_moving_sphere &s = d.moving_spheres[idx];
                for (int a = 0; a < 3; a++)
                    c[a] = (std::min(s.center0[a], s.center1[a]) - s.radius) + (std::max(s.center0[a], s.center1[a]) + s.radius);
                return true;
            }
            case RT_KIND_RECT: {
                const rt_rect &r = d.rects[idx];
                const int ia = r.axis == RT_RECT_YZ ? 1 : 0, ib = r.axis == RT_RECT_XY ? 1 : 2, ik = 3 - ia - ib;
                c[ia] = r.a0 + r.a1; c[ib] = r.b0 + r.b1; c[ik] = (r.k - 0.0001) + (r.k + 0.0001);
                return true;
            }
            case RT_KIND_BOX:
                for (int a = 0; a < 3; a++) c[a] = d.boxes[idx].p0[a] + d.boxes[idx].p1[a];
                return true;
            case RT_KIND_TRIANGLE: {
                const rt_triangle &t = d.triangles[idx];
                for (int a = 0; a < 3; a++) c[a] = std::min(t.a[a], std::min(t.b[a], t.c[a])) + std::max(t.a[a], std::max(t.b[a], t.c[a]));
                return true;
            }
            case RT_KIND_RING:                                    // a ring lies round the origin of its frame
                c[0] = c[1] = c[2] = 0.0;
                return true;
            default: return false;                                // a mover, a list, a medium: keep
        }
    }
    // Stack entries a traversal of `ref` needs (Validator::need's count): reference order everywhere, or — `ordered` — with
    // either child first at the nodes that have an order: the child visited second waits on the stack, so 1 + the larger need.
    std::vector<int32_t> need_memo[2];
    int32_t need(uint32_t ref, bool ordered) {
        const uint32_t kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        if (is_prim(kind)) return 1;
        if (kind == RT_KIND_MEDIUM) return 1 + need(d.media[idx].boundary, ordered);
        if (kind >= RT_KIND_TRANSLATE && kind <= RT_KIND_ZOOM) return 1 + need(d.xforms[idx].child, ordered);
        if (kind == RT_KIND_LIST) {
            const rt_list &l = d.lists[idx];
            int32_t n = std::max<int32_t>(1, (int32_t)l.count);
            for (uint32_t i = 0; i < l.count; i++) n = std::max(n, (int32_t)(l.count - 1 - i) + need(d.list_items[l.first + i], ordered));
            return n;
        }
        std::vector<int32_t> &memo = need_memo[ordered ? 1 : 0];
        if (memo.empty()) memo.assign(d.n_nodes, -1);
        if (memo[idx] >= 0) return memo[idx];
        const int32_t l = need(d.nodes[idx].left, ordered);
        const int32_t r = d.nodes[idx].right == d.nodes[idx].left ? l : need(d.nodes[idx].right, ordered);
        return memo[idx] = (ordered && out.order[idx]) ? 1 + std::max(l, r) : std::max(1 + l, r);
    }
    uint8_t order_of(uint32_t i) const {
        const rt_bvh_node &n = d.nodes[i];
        if (out.medium[i] || n.left == n.right) return 0;
        double cl[3], cr[3];
        if (!centre2(n.left, cl) || !centre2(n.right, cr)) return 0;
        int axis = -1;
        double best = 0.0;
        for (int a = 0; a < 3; a++) {
            const double diff = cr[a] - cl[a];
            if (!std::isfinite(diff)) return 0;
            if (std::fabs(diff) > best) { best = std::fabs(diff); axis = a; }
        }
        if (axis < 0) return 0;                                   // equal centres on every axis
        return (uint8_t)(1 + 2 * axis + (cr[axis] - cl[axis] > 0.0 ? 0 : 1));
    }
};

} // namespace

ChildOrder child_order(const rt_scene_desc &d) {
    ChildOrder out;
    out.order.assign(d.n_nodes, 0);
    out.medium.assign(d.n_nodes, 0);
    const uint64_t pools[8] = {0, d.n_spheres, d.n_moving_spheres, d.n_rects, d.n_boxes, d.n_triangles, d.n_rings, d.n_media};
    uint64_t at = 8;
    out.rank.assign(8, 0);
    for (int k = 0; k < 8; k++) { out.rank[k] = (uint32_t)at; at += pools[k]; }
    out.rank.resize(at, OrderWalk::kNoRank);
    OrderWalk w(d, out);
    for (uint32_t i = 0; i < d.n_nodes; i++) out.medium[i] = w.holds_medium(RT_MAKE_REF(RT_KIND_NODE, i)) ? 1 : 0;
    for (uint32_t i = 0; i < d.n_media; i++) w.mark_boundary(d.media[i].boundary);
    for (uint32_t i = 0; i < d.n_nodes; i++) out.medium[i] = out.medium[i] ? 1 : 0;
    w.rank_walk(d.root);
    out.usable = !w.shared && d.n_nodes <= (1u << kOrderShift) && at < (1ull << 32);
    if (out.usable) {
        for (uint32_t i = 0; i < d.n_nodes; i++) out.order[i] = w.order_of(i);
        // The traversal stack is sized for the reference's order (check_scene: stack_need → the kernels' capacity, kStackTiers).
        // With the right child first the LEFT one waits on the stack: where that can outgrow the capacity the scene's kernels
        // have, only the nodes whose right subtree needs no more than their left keep their order — swapped, such a node needs
        // max(1 + r, l) <= 1 + l, what it needs in the reference's order, so by induction the whole scene does.
        const int32_t ref_need = w.need(d.root, false);
        int32_t capacity = ref_need;
        for (int t = 3; t >= 0; t--) if (ref_need <= kStackTiers[t]) capacity = kStackTiers[t];
        if (w.need(d.root, true) > capacity)
            for (uint32_t i = 0; i < d.n_nodes; i++)
                if (out.order[i] && w.need(d.nodes[i].right, false) > w.need(d.nodes[i].left, false)) out.order[i] = 0;
    }
    return out;
}

} // namespace rt2022
