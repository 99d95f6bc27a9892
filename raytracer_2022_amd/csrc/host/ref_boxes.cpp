// ref_boxes.cpp — rtb_ref_boxes (include/rt2022_host.h): the reference's bounding_box(time0, time1) of any ref of a flattened
// description, restated on the records from the rules of scene_api.cpp (which apply them to the object graph). Pure host code.
#include <string>

#include "../../../include/rt2022_host.h"
#include "../rt_math.h"
#include "rt_error.hpp"

namespace rt2022 {
namespace {

struct Box6 { double lo[3], hi[3]; };

struct RefBoxes {
    const rt_scene_desc &d;

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

    // AABB::surrounding_box(b0, b1), aabb.rs:34-46.
    static Box6 surrounding(const Box6 &b0, const Box6 &b1) {
        Box6 o;
        for (int a = 0; a < 3; a++) { o.lo[a] = rtm::fmin_(b0.lo[a], b1.lo[a]); o.hi[a] = rtm::fmax_(b0.hi[a], b1.hi[a]); }
        return o;
    }

    Box6 box(uint32_t ref, double time0, double time1, int depth) const {
        RT_REQUIRE(depth < 64, RT_ERR_INVALID, "rtb_ref_boxes: movers, lists and media nested deeper than 64 (or a cycle)");
        const uint32_t kind = RT_REF_KIND(ref), idx = RT_REF_INDEX(ref);
        RT_REQUIRE(kind < RT_KIND_COUNT && idx < pool_size(kind), RT_ERR_INVALID, "rtb_ref_boxes: ref of an unknown kind or out of its pool");
        Box6 o{};
        switch (kind) {
            case RT_KIND_NODE:
                for (int a = 0; a < 3; a++) { o.lo[a] = d.nodes[idx].bmin[a]; o.hi[a] = d.nodes[idx].bmax[a]; }
                return o;
            case RT_KIND_SPHERE: {                                             // sphere.rs:68-73
                const rt_sphere &s = d.spheres[idx];
                for (int a = 0; a < 3; a++) { o.lo[a] = s.center[a] - s.radius; o.hi[a] = s.center[a] + s.radius; }
                return o;
            }
            case RT_KIND_MOVING_SPHERE: {                                      // sphere.rs:124-127, 167-177
                const rt_moving_sphere &s = d.moving_spheres[idx];
                Box6 b[2];
                const double times[2] = {time0, time1};
                for (int k = 0; k < 2; k++)
                    for (int a = 0; a < 3; a++) {
                        const double c = s.center0[a] + (s.center1[a] - s.center0[a]) * ((times[k] - s.time0) / (s.time1 - s.time0));
                        b[k].lo[a] = c - s.radius; b[k].hi[a] = c + s.radius;
                    }
                return surrounding(b[0], b[1]);
            }
            case RT_KIND_RECT: {                                               // aarect.rs:40-45, 123-128, 206-211
                const rt_rect &r = d.rects[idx];
                RT_REQUIRE(r.axis <= RT_RECT_YZ, RT_ERR_INVALID, "rtb_ref_boxes: rect with a bad axis");
                const int ia = r.axis == RT_RECT_YZ ? 1 : 0, ib = r.axis == RT_RECT_XY ? 1 : 2, ik = 3 - ia - ib;
                o.lo[ia] = r.a0; o.hi[ia] = r.a1; o.lo[ib] = r.b0; o.hi[ib] = r.b1;
                o.lo[ik] = r.k - 0.0001; o.hi[ik] = r.k + 0.0001;
                return o;
            }
            case RT_KIND_BOX:                                                  // boxes.rs:77-79
                for (int a = 0; a < 3; a++) { o.lo[a] = d.boxes[idx].p0[a]; o.hi[a] = d.boxes[idx].p1[a]; }
                return o;
            case RT_KIND_TRIANGLE: {                                           // triangle.rs:79-92: no padding
                const rt_triangle &t = d.triangles[idx];
                for (int a = 0; a < 3; a++) {
                    o.lo[a] = rtm::fmin_(t.a[a], rtm::fmin_(t.b[a], t.c[a]));
                    o.hi[a] = rtm::fmax_(t.a[a], rtm::fmax_(t.b[a], t.c[a]));
                }
                return o;
            }
            case RT_KIND_RING: {                                               // ring.rs:55-62
                const double thickness = 0.0001, rr = d.rings[idx].r + d.rings[idx].t;
                o.lo[0] = -rr; o.lo[1] = -thickness; o.lo[2] = -rr;
                o.hi[0] = rr; o.hi[1] = thickness; o.hi[2] = rr;
                return o;
            }
            case RT_KIND_MEDIUM:                                               // constantmedium.rs: the boundary's
                return box(d.media[idx].boundary, time0, time1, depth + 1);
            case RT_KIND_LIST: {                                               // mod.rs:102-120
                const rt_list &l = d.lists[idx];
                RT_REQUIRE(l.count > 0, RT_ERR_INVALID, "rtb_ref_boxes: an empty list has no bounding box");
                RT_REQUIRE((uint64_t)l.first + l.count <= d.n_list_items, RT_ERR_INVALID, "rtb_ref_boxes: list items out of range");
                for (int a = 0; a < 3; a++) { o.lo[a] = rtm::INF; o.hi[a] = -rtm::INF; }
                for (uint32_t i = 0; i < l.count; i++) o = surrounding(o, box(d.list_items[l.first + i], time0, time1, depth + 1));
                return o;
            }
            default: break;
        }
        const rt_xform &x = d.xforms[idx];
        RT_REQUIRE(x.kind == kind, RT_ERR_INVALID, "rtb_ref_boxes: mover ref kind does not match its record");
        if (kind == RT_KIND_TRANSLATE) {                                       // mod.rs:154-163
            const Box6 b = box(x.child, time0, time1, depth + 1);
            for (int a = 0; a < 3; a++) { o.lo[a] = b.lo[a] + x.p[a]; o.hi[a] = b.hi[a] + x.p[a]; }
            return o;
        }
        if (kind == RT_KIND_ZOOM) {                                            // mod.rs:310-319
            const Box6 b = box(x.child, time0, time1, depth + 1);
            for (int a = 0; a < 3; a++) { o.lo[a] = b.lo[a] * x.p[0]; o.hi[a] = b.hi[a] * x.p[0]; }
            return o;
        }
        // RotateY::new, mod.rs:188-228: the eight corners of the child's box over (0, 1), whatever interval was asked for.
        const Box6 b = box(x.child, 0.0, 1.0, depth + 1);
        const double sin_theta = x.p[0], cos_theta = x.p[1];
        for (int a = 0; a < 3; a++) { o.lo[a] = rtm::INF; o.hi[a] = -rtm::INF; }
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 2; j++)
                for (int k = 0; k < 2; k++) {
                    const double px = (double)i * b.hi[0] + (double)(1 - i) * b.lo[0];
                    const double py = (double)j * b.hi[1] + (double)(1 - j) * b.lo[1];
                    const double pz = (double)k * b.hi[2] + (double)(1 - k) * b.lo[2];
                    const double tester[3] = {cos_theta * px + sin_theta * pz, py, -sin_theta * px + cos_theta * pz};
                    for (int c = 0; c < 3; c++) { o.lo[c] = rtm::fmin_(o.lo[c], tester[c]); o.hi[c] = rtm::fmax_(o.hi[c], tester[c]); }
                }
        return o;
    }
};

} // namespace
} // namespace rt2022

extern "C" int rtb_ref_boxes(const rt_scene_desc *desc, const uint32_t *refs, uint32_t n, double time0, double time1, double *out_boxes6) {
    using namespace rt2022;
    try {
        RT_REQUIRE(desc && (n == 0 || (refs && out_boxes6)), RT_ERR_INVALID, "rtb_ref_boxes: null argument");
        const RefBoxes rb{*desc};
        for (uint32_t i = 0; i < n; i++) {
            const Box6 b = rb.box(refs[i], time0, time1, 0);
            for (int a = 0; a < 3; a++) { out_boxes6[6 * (size_t)i + a] = b.lo[a]; out_boxes6[6 * (size_t)i + 3 + a] = b.hi[a]; }
        }
        return RT_OK;
    } catch (const Fail &e) {
        set_error(e.msg);
        return e.code;
    }
}
