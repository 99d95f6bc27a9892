// host_order_units.cpp — the upload pass behind the ordered node steps of the wavefront traversal (child_order,
// csrc/host/scene_check.cpp) on hand-made scene graphs: which nodes hold a medium, the order axis and sense
// per primitive kind, the cases that keep the reference's order, the ranks against a literal depth-first walk — and a
// restatement of the ordered traversal with its tie rule, run against the literal left-then-right walk on random small trees
// with planted exact ties. Built with the address and undefined-behaviour sanitizers and run by
// tests/test_host_order_units.py; exits 0 if everything holds, 1 with one line per failure otherwise.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../include/rt2022.h"
#include "../raytracer_2022_amd/csrc/host/scene_check.hpp"

using namespace rt2022;

namespace {

int failures = 0;
void fail(const std::string &what) {
    std::printf("FAIL: %s\n", what.c_str());
    failures++;
}
void expect(bool ok, const std::string &what) { if (!ok) fail(what); }

// ---- a scene description from pools that grow -------------------------------------------------------------------------
struct Build {
    std::vector<rt_bvh_node> nodes;
    std::vector<rt_sphere> spheres;
    std::vector<rt_moving_sphere> moving;
    std::vector<rt_rect> rects;
    std::vector<rt_box> boxes;
    std::vector<rt_triangle> triangles;
    std::vector<rt_ring> rings;
    std::vector<rt_medium> media;
    std::vector<rt_xform> xforms;
    std::vector<rt_list> lists;
    std::vector<uint32_t> items;
    uint32_t root = 0;

    uint32_t sphere(double x, double y, double z, double r) {
        rt_sphere s{}; s.center[0] = x; s.center[1] = y; s.center[2] = z; s.radius = r;
        spheres.push_back(s);
        return RT_MAKE_REF(RT_KIND_SPHERE, spheres.size() - 1);
    }
    uint32_t moving_sphere(double x0, double y0, double z0, double x1, double y1, double z1, double r) {
        rt_moving_sphere s{}; s.center0[0] = x0; s.center0[1] = y0; s.center0[2] = z0; s.center1[0] = x1; s.center1[1] = y1; s.center1[2] = z1;
        s.time0 = 0.0; s.time1 = 1.0; s.radius = r;
        moving.push_back(s);
        return RT_MAKE_REF(RT_KIND_MOVING_SPHERE, moving.size() - 1);
    }
    uint32_t rect(uint32_t axis, double a0, double a1, double b0, double b1, double k) {
        rt_rect r{}; r.a0 = a0; r.a1 = a1; r.b0 = b0; r.b1 = b1; r.k = k; r.axis = axis;
        rects.push_back(r);
        return RT_MAKE_REF(RT_KIND_RECT, rects.size() - 1);
    }
    uint32_t box(double x0, double y0, double z0, double x1, double y1, double z1) {
        rt_box b{}; b.p0[0] = x0; b.p0[1] = y0; b.p0[2] = z0; b.p1[0] = x1; b.p1[1] = y1; b.p1[2] = z1;
        boxes.push_back(b);
        return RT_MAKE_REF(RT_KIND_BOX, boxes.size() - 1);
    }
    uint32_t triangle(const double a[3], const double b[3], const double c[3]) {
        rt_triangle t{};
        for (int i = 0; i < 3; i++) { t.a[i] = a[i]; t.b[i] = b[i]; t.c[i] = c[i]; }
        triangles.push_back(t);
        return RT_MAKE_REF(RT_KIND_TRIANGLE, triangles.size() - 1);
    }
    uint32_t ring(double r, double t) {
        rt_ring q{}; q.r = r; q.t = t;
        rings.push_back(q);
        return RT_MAKE_REF(RT_KIND_RING, rings.size() - 1);
    }
    uint32_t medium(uint32_t boundary) {
        rt_medium m{}; m.boundary = boundary;
        media.push_back(m);
        return RT_MAKE_REF(RT_KIND_MEDIUM, media.size() - 1);
    }
    uint32_t xform(uint32_t kind, uint32_t child) {
        rt_xform x{}; x.kind = kind; x.child = child;
        xforms.push_back(x);
        return RT_MAKE_REF(kind, xforms.size() - 1);
    }
    uint32_t list(const std::vector<uint32_t> &refs) {
        rt_list l{(uint32_t)items.size(), (uint32_t)refs.size()};
        items.insert(items.end(), refs.begin(), refs.end());
        lists.push_back(l);
        return RT_MAKE_REF(RT_KIND_LIST, lists.size() - 1);
    }
    // (the boxes of hand-made nodes are given where a test is about them; elsewhere any box does)
    uint32_t node(uint32_t left, uint32_t right, double lo = -1.0, double hi = 1.0) {
        rt_bvh_node n{};
        for (int a = 0; a < 3; a++) { n.bmin[a] = lo; n.bmax[a] = hi; }
        n.left = left; n.right = right;
        nodes.push_back(n);
        return RT_MAKE_REF(RT_KIND_NODE, nodes.size() - 1);
    }
    uint32_t node_at(uint32_t left, uint32_t right, const double lo[3], const double hi[3]) {
        const uint32_t r = node(left, right);
        for (int a = 0; a < 3; a++) { nodes.back().bmin[a] = lo[a]; nodes.back().bmax[a] = hi[a]; }
        return r;
    }
    rt_scene_desc desc() const {
        rt_scene_desc d{};
        d.abi_version = RT2022_ABI_VERSION; d.root = root;
        d.n_nodes = (uint32_t)nodes.size(); d.nodes = nodes.data();
        d.n_spheres = (uint32_t)spheres.size(); d.spheres = spheres.data();
        d.n_moving_spheres = (uint32_t)moving.size(); d.moving_spheres = moving.data();
        d.n_rects = (uint32_t)rects.size(); d.rects = rects.data();
        d.n_boxes = (uint32_t)boxes.size(); d.boxes = boxes.data();
        d.n_triangles = (uint32_t)triangles.size(); d.triangles = triangles.data();
        d.n_rings = (uint32_t)rings.size(); d.rings = rings.data();
        d.n_media = (uint32_t)media.size(); d.media = media.data();
        d.n_xforms = (uint32_t)xforms.size(); d.xforms = xforms.data();
        d.n_lists = (uint32_t)lists.size(); d.lists = lists.data();
        d.n_list_items = (uint32_t)items.size(); d.list_items = items.data();
        return d;
    }
};
uint32_t idx(uint32_t ref) { return RT_REF_INDEX(ref); }
uint8_t order_code(int axis, int sense) { return (uint8_t)(1 + 2 * axis + sense); }

// ---- (a) medium flags ------------------------------------------------------------------------------------------------
void medium_flags() {
    Build b;
    const uint32_t plain = b.node(b.sphere(-2, 0, 0, 1), b.sphere(2, 0, 0, 1));
    const uint32_t fog = b.medium(b.sphere(0, 5, 0, 1));
    const uint32_t direct = b.node(b.sphere(-3, 0, 0, 1), fog);                                        // a medium for a child
    const uint32_t in_list = b.node(b.sphere(-4, 0, 0, 1), b.list({b.sphere(0, 1, 0, 1), b.medium(b.sphere(0, 7, 0, 1))}));
    const uint32_t in_mover = b.node(b.xform(RT_KIND_TRANSLATE, b.xform(RT_KIND_ROTATE_Y, b.medium(b.box(0, 0, 0, 1, 1, 1)))), b.sphere(5, 0, 0, 1));
    const uint32_t nested = b.node(b.xform(RT_KIND_ZOOM, b.node(b.sphere(0, 0, 1, 1), b.medium(b.sphere(0, 0, 4, 1)))), b.sphere(6, 0, 0, 1));
    const uint32_t free_list = b.node(b.list({b.sphere(1, 1, 1, 1), b.sphere(2, 2, 2, 1)}), b.sphere(7, 0, 0, 1));
    // a medium whose boundary is a BVH of its own: the boundary's nodes count as holding one
    const uint32_t shell = b.node(b.box(0, 0, 0, 1, 1, 1), b.box(2, 0, 0, 3, 1, 1));
    const uint32_t shelled = b.node(b.medium(shell), b.sphere(8, 0, 0, 1));
    const uint32_t top = b.node(b.node(b.node(plain, direct), b.node(in_list, in_mover)), b.node(b.node(nested, free_list), shelled));
    b.root = top;
    const rt_scene_desc d = b.desc();
    const ChildOrder o = child_order(d);
    expect(o.usable, "medium flags: the graph is a tree, the order is usable");
    expect(!o.medium[idx(plain)], "a node of two spheres holds no medium");
    expect(o.medium[idx(direct)], "a node with a medium child holds one");
    expect(o.medium[idx(in_list)], "a medium inside a list child");
    expect(o.medium[idx(in_mover)], "a medium under two movers");
    expect(o.medium[idx(nested)], "a medium in a BVH under a mover");
    expect(o.medium[idx(RT_REF_INDEX(b.xforms[2].child))], "the nested BVH's own node holds the medium");
    expect(!o.medium[idx(free_list)], "a list of spheres holds no medium");
    expect(o.medium[idx(shelled)] && o.medium[idx(top)], "a medium's parent, and the root, hold one");
    for (uint32_t r : {direct, in_list, in_mover, nested, shelled, top})
        expect(o.order[idx(r)] == 0, "a node that holds a medium keeps the reference's order");
    expect(o.order[idx(plain)] == order_code(0, 0), "the medium-free node beside them is ordered");
    expect(o.medium[idx(shell)] && o.order[idx(shell)] == 0, "a boundary's own BVH counts as holding the medium and keeps the reference's order");
}

// ---- (b) axis and sense per primitive kind -----------------------------------------------------------------------------
void axis_and_sense() {
    Build b;
    struct Case { const char *name; uint32_t node; uint8_t want; };
    std::vector<Case> cases;
    const double ta[3] = {0, 0, 0}, tb[3] = {1, 0, 0}, tc[3] = {0, 1, 0};                // centre2 = (1, 1, 0)
    const double ua[3] = {0, 0, -9}, ub[3] = {1, 0, -8}, uc[3] = {0, 1, -8.5};             // centre2 = (1, 1, -17)
    cases.push_back({"spheres along +x", b.node(b.sphere(-2, 0, 0, 1), b.sphere(2, 0.5, 0, 1)), order_code(0, 0)});
    cases.push_back({"spheres along -y", b.node(b.sphere(0, 3, 0, 1), b.sphere(1, -3, 0, 0.2)), order_code(1, 1)});
    cases.push_back({"a moving sphere: the union of both ends", b.node(b.moving_sphere(0, 0, 0, 0, 8, 0, 1), b.sphere(0, 4, 1.5, 1)), order_code(2, 0)});
    cases.push_back({"moving sphere below a sphere on y", b.node(b.sphere(0, 9, 0, 1), b.moving_sphere(0, 0, 0, 0, 8, 0, 1)), order_code(1, 1)});
    cases.push_back({"XY rects by k", b.node(b.rect(RT_RECT_XY, 0, 1, 0, 1, 5.0), b.rect(RT_RECT_XY, 0, 1, 0, 1, -5.0)), order_code(2, 1)});
    cases.push_back({"XZ rects by k", b.node(b.rect(RT_RECT_XZ, 0, 1, 0, 1, -1.0), b.rect(RT_RECT_XZ, 0, 1, 0, 1, 4.0)), order_code(1, 0)});
    cases.push_back({"YZ rects by k", b.node(b.rect(RT_RECT_YZ, 0, 1, 0, 1, 2.0), b.rect(RT_RECT_YZ, 0, 1, 0, 1, 1.0)), order_code(0, 1)});
    cases.push_back({"XZ rects by their z extent", b.node(b.rect(RT_RECT_XZ, 0, 1, 0, 2, 0.0), b.rect(RT_RECT_XZ, 0, 1, 6, 8, 0.0)), order_code(2, 0)});
    cases.push_back({"YZ rects by their y extent", b.node(b.rect(RT_RECT_YZ, 4, 6, 0, 1, 0.0), b.rect(RT_RECT_YZ, 0, 1, 0, 1, 0.0)), order_code(1, 1)});
    cases.push_back({"boxes", b.node(b.box(0, 0, 0, 1, 9, 1), b.box(2, 0, 0, 3, 1, 1)), order_code(1, 1)});
    cases.push_back({"triangles", b.node(b.triangle(ta, tb, tc), b.triangle(ua, ub, uc)), order_code(2, 1)});
    cases.push_back({"a ring lies round its origin", b.node(b.ring(1.0, 0.2), b.sphere(0, 0, 3, 1)), order_code(2, 0)});
    const double lo1[3] = {0, 0, 0}, hi1[3] = {2, 2, 2}, lo2[3] = {-10, 0, 0}, hi2[3] = {-4, 2, 2};
    const uint32_t n1 = b.node_at(b.sphere(1, 1, 1, 1), b.sphere(1, 1, 1, 0.5), lo1, hi1), n2 = b.node_at(b.sphere(-7, 1, 1, 1), b.sphere(-6, 1, 1, 1), lo2, hi2);
    cases.push_back({"node children by their records", b.node(n1, n2), order_code(0, 1)});
    const uint32_t n3 = b.node_at(b.sphere(1, 1, 1, 1), b.sphere(1, 1, 1, 0.5), lo1, hi1);
    cases.push_back({"a node and a primitive", b.node(n3, b.sphere(1, 1, 30, 1)), order_code(2, 0)});
    // the largest difference decides, the first axis among equals
    cases.push_back({"first axis among equal differences", b.node(b.sphere(0, 0, 0, 1), b.sphere(2, -2, 2, 1)), order_code(0, 0)});
    uint32_t root = cases[0].node;
    for (size_t i = 1; i < cases.size(); i++) root = b.node(root, cases[i].node);
    b.root = root;
    const rt_scene_desc d = b.desc();
    const ChildOrder o = child_order(d);
    expect(o.usable, "axis and sense: usable");
    for (const Case &c : cases)
        if (o.order[idx(c.node)] != c.want)
            fail(std::string("order of ") + c.name + ": got " + std::to_string(o.order[idx(c.node)]) + ", want " + std::to_string(c.want));
}

// ---- (c) the cases that keep the reference's order -----------------------------------------------------------------------
void keep_cases() {
    Build b;
    const uint32_t s = b.sphere(0, 0, 0, 1);
    std::vector<std::pair<const char *, uint32_t>> keep;
    keep.push_back({"a mover child", b.node(b.xform(RT_KIND_TRANSLATE, b.sphere(1, 0, 0, 1)), b.sphere(9, 0, 0, 1))});
    keep.push_back({"a list child", b.node(b.sphere(-9, 0, 0, 1), b.list({b.sphere(2, 0, 0, 1)}))});
    keep.push_back({"a flipped child", b.node(b.sphere(-8, 0, 0, 1), b.rect(RT_RECT_XZ, 0, 1, 0, 1, 3.0) | RT_REF_FLIP)});
    keep.push_back({"a span-1 twin", b.node(s, s)});
    keep.push_back({"equal centres", b.node(b.sphere(3, 3, 3, 1), b.sphere(3, 3, 3, 2))});
    keep.push_back({"a medium child", b.node(b.sphere(4, 0, 0, 1), b.medium(b.sphere(40, 0, 0, 1)))});
    const uint32_t ordered = b.node(b.sphere(-5, 0, 0, 1), b.sphere(5, 0, 0, 1));
    uint32_t root = ordered;
    for (auto &k : keep) root = b.node(root, k.second);
    b.root = root;
    const rt_scene_desc d = b.desc();
    const ChildOrder o = child_order(d);
    expect(o.usable, "keep cases: usable");
    for (auto &k : keep) expect(o.order[idx(k.second)] == 0, std::string("keeps the reference's order: ") + k.first);
    expect(o.order[idx(ordered)] == order_code(0, 0), "the plain pair beside them is ordered");
    // a primitive reached along two paths: ranks are no order any more, nothing is ordered
    Build c;
    const uint32_t shared = c.sphere(0, 0, 0, 1);
    const uint32_t pair = c.node(c.sphere(-5, 0, 0, 1), c.sphere(5, 0, 0, 1));
    c.root = c.node(c.node(pair, shared), c.xform(RT_KIND_TRANSLATE, shared));
    const rt_scene_desc dc = c.desc();
    const ChildOrder oc = child_order(dc);
    expect(!oc.usable, "a primitive under two parents: not usable");
    for (uint8_t v : oc.order) expect(v == 0, "... and every node keeps the reference's order");
    // a node reached along two paths likewise
    Build e;
    const uint32_t sub = e.node(e.sphere(-5, 0, 0, 1), e.sphere(5, 0, 0, 1));
    e.root = e.node(e.xform(RT_KIND_TRANSLATE, sub), e.xform(RT_KIND_ZOOM, sub));
    const rt_scene_desc de = e.desc();
    expect(!child_order(de).usable, "a node under two parents: not usable");
}

// ---- (c2) no order may outgrow the traversal stack ------------------------------------------------------------------------
// A chain leaning RIGHT needs two stack entries in the reference's order however long it is (the left leaf is done before the
// right child is entered); entered right child first, every link leaves its left leaf waiting: one entry per link.
void stack_bound() {
    for (int links : {10, 40}) {
        Build b;
        uint32_t ref = b.node(b.sphere(0, 0, 0, 0.4), b.sphere(1, 0, 0, 0.4));
        std::vector<uint32_t> chain;
        for (int i = 0; i < links; i++) {
            const double lo[3] = {-1.0, -1.0, -1.0}, hi[3] = {3.0 + i, 1.0, 1.0};
            ref = b.node_at(b.sphere(-5.0 - i, 0, 0, 0.4), ref, lo, hi);
            chain.push_back(ref);
        }
        b.root = ref;
        const rt_scene_desc d = b.desc();
        const ChildOrder o = child_order(d);
        expect(o.usable, "right-leaning chain: usable");
        int ordered = 0;
        for (uint32_t r : chain) ordered += o.order[idx(r)] != 0;
        // 10 links: 12 entries at most, within the 16 of the smallest stack — every link keeps its order; 40 links: 42, beyond
        // the 16 the reference's need of 2 selects — the links, whose right subtree is the deeper one, lose theirs
        if (links == 10) expect(ordered == links, "a short right-leaning chain keeps its order: the need stays within the stack");
        else expect(ordered == 0, "a long right-leaning chain loses its order: it would outgrow the stack");
        expect(o.order[0] != 0, "the pair of leaves at the bottom is ordered either way");
    }
}

// ---- (d) ranks: a literal depth-first walk ---------------------------------------------------------------------------
void literal_walk(const rt_scene_desc &d, uint32_t ref, std::vector<uint32_t> &out) {
    const uint32_t kind = RT_REF_KIND(ref), i = RT_REF_INDEX(ref);
    if (kind == RT_KIND_NODE) {
        literal_walk(d, d.nodes[i].left, out);
        if (d.nodes[i].right != d.nodes[i].left) literal_walk(d, d.nodes[i].right, out);
    } else if (kind == RT_KIND_LIST) {
        for (uint32_t k = 0; k < d.lists[i].count; k++) literal_walk(d, d.list_items[d.lists[i].first + k], out);
    } else if (kind >= RT_KIND_TRANSLATE && kind <= RT_KIND_ZOOM) {
        literal_walk(d, d.xforms[i].child, out);
    } else {
        out.push_back(ref & ~RT_REF_FLIP);                      // (a medium is one candidate of the main query; its boundary is its own affair)
    }
}
void ranks() {
    Build b;
    const double ta[3] = {0, 0, 0}, tb[3] = {1, 0, 0}, tc[3] = {0, 1, 0};
    const uint32_t twin_s = b.sphere(9, 9, 9, 1);
    const uint32_t left = b.node(b.node(b.sphere(0, 0, 0, 1), b.rect(RT_RECT_XY, 0, 1, 0, 1, 0) | RT_REF_FLIP), b.node(twin_s, twin_s));
    const uint32_t mid = b.list({b.box(0, 0, 0, 1, 1, 1), b.xform(RT_KIND_TRANSLATE, b.xform(RT_KIND_ROTATE_Y, b.node(b.triangle(ta, tb, tc), b.ring(1, 0.1)))),
                                 b.medium(b.xform(RT_KIND_TRANSLATE, b.box(0, 0, 0, 2, 2, 2))), b.moving_sphere(0, 0, 0, 0, 1, 0, 1)});
    const uint32_t right = b.node(b.sphere(1, 0, 0, 1), b.node(b.sphere(2, 0, 0, 1), b.sphere(3, 0, 0, 1)));
    b.root = b.list({left, mid, right});
    const rt_scene_desc d = b.desc();
    const ChildOrder o = child_order(d);
    expect(o.usable, "ranks: usable");
    std::vector<uint32_t> walk;
    literal_walk(d, d.root, walk);
    expect(walk.size() == 11, "the literal walk meets 10 primitives and one medium");
    for (size_t r = 0; r < walk.size(); r++) {
        const uint32_t kind = RT_REF_KIND(walk[r]), i = RT_REF_INDEX(walk[r]);
        expect(kind < 8 && o.rank[kind] + i < o.rank.size(), "rank table: in range");
        if (o.rank[o.rank[kind] + i] != r) fail("rank of walk entry " + std::to_string(r) + ": got " + std::to_string(o.rank[o.rank[kind] + i]));
    }
    const uint64_t pools = d.n_spheres + d.n_moving_spheres + d.n_rects + d.n_boxes + d.n_triangles + d.n_rings + d.n_media;
    expect(o.rank.size() == 8 + pools, "rank table: eight bases and one word per primitive and medium");
    // the final scene's subsurface ball: one sphere, a world object and a medium's boundary at once — still a tree to the main query
    Build f;
    const uint32_t ball = f.sphere(0, 0, 0, 1);
    const uint32_t pair = f.node(f.sphere(-5, 0, 0, 1), f.sphere(5, 0, 0, 1));
    f.root = f.list({pair, ball, f.medium(ball)});
    const rt_scene_desc df = f.desc();
    const ChildOrder of = child_order(df);
    expect(of.usable && of.order[idx(pair)] == order_code(0, 0), "a primitive that is also a medium's boundary does not count as shared");
}

// ---- (e) ordered traversal with the tie rule == the literal walk --------------------------------------------------------
// One ray against a random tree: a leaf is hit at a distance drawn from a handful of values — exact ties are the rule, not
// the exception — or missed; a node's box is entered before every hit below it. The literal walk is BvhNode::hit: left, then
// right against the closest so far, a candidate accepted unless t < t_min or t_max < t. The ordered walk visits the right
// child first wherever a coin says so and settles ties between different leaves by rank, as wf_trace does.
struct TNode { int left, right; double entry; };        // children: >= 0 a node, < 0 leaf ~child
struct Tree {
    std::vector<TNode> nodes;
    std::vector<double> leaf_t;                          // inf: missed
    std::vector<uint32_t> leaf_rank;
    std::vector<char> swap;
};
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)((rng_state >> 33) % n);
}
int grow(Tree &t, int leaves, double &lowest) {
    if (leaves == 1) {
        const uint32_t pick = rnd(6);
        const double v = pick == 5 ? std::numeric_limits<double>::infinity() : 1.0 + 0.5 * pick;
        t.leaf_t.push_back(v);
        t.leaf_rank.push_back((uint32_t)t.leaf_rank.size());                // (leaves are made in depth-first order: left subtree first)
        lowest = v;
        return ~(int)(t.leaf_t.size() - 1);
    }
    const int nl = 1 + (int)rnd((uint32_t)leaves - 1);
    const int me = (int)t.nodes.size();
    t.nodes.push_back(TNode{0, 0, 0.0});
    t.swap.push_back((char)rnd(2));
    double lo_l, lo_r;
    const int l = grow(t, nl, lo_l), r = grow(t, leaves - nl, lo_r);
    lowest = std::fmin(lo_l, lo_r);
    t.nodes[me] = TNode{l, r, std::isinf(lowest) ? 100.0 : lowest - 0.25};
    return me;
}
struct Win { double t; int leaf; };
void visit(const Tree &t, int ref, bool ordered, double t_min, Win &w) {
    if (ref < 0) {
        const int leaf = ~ref;
        const double v = t.leaf_t[leaf];
        if (v < t_min || w.t < v) return;
        if (ordered && v == w.t && w.leaf >= 0 && w.leaf != leaf && t.leaf_rank[leaf] < t.leaf_rank[w.leaf]) return;
        w.t = v; w.leaf = leaf;
        return;
    }
    const TNode &n = t.nodes[ref];
    if (w.t <= std::fmax(n.entry, t_min)) return;                           // AABB::hit: t_max <= t_min
    const bool sw = ordered && t.swap[ref];
    visit(t, sw ? n.right : n.left, ordered, t_min, w);
    visit(t, sw ? n.left : n.right, ordered, t_min, w);
}
void ordered_equals_literal() {
    int ties_seen = 0;
    for (int round = 0; round < 4000; round++) {
        Tree t;
        double lowest;
        const int root = grow(t, 2 + (int)rnd(14), lowest);
        const double t_min = rnd(4) == 0 ? 1.25 : 0.001;
        Win a{std::numeric_limits<double>::max(), -1}, b = a;
        visit(t, root, false, t_min, a);
        visit(t, root, true, t_min, b);
        if (a.leaf != b.leaf || !(a.t == b.t)) { fail("ordered walk: another winner than the literal walk in round " + std::to_string(round)); return; }
        int at_best = 0;
        for (double v : t.leaf_t) at_best += a.leaf >= 0 && v == a.t;
        ties_seen += at_best > 1;
    }
    expect(ties_seen > 500, "the random trees hold exact ties at the closest distance");
}

} // namespace

int main() {
    medium_flags();
    axis_and_sense();
    keep_cases();
    stack_bound();
    ranks();
    ordered_equals_literal();
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("host order units ok\n");
    return 0;
}
