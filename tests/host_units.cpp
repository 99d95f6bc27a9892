// host_units.cpp — the library's host logic that needs no device, held to account on the CPU: the planners of
// csrc/host/plan.hpp against values recorded from them, and the scene validator of csrc/host/scene_check.cpp against the
// hostile descriptions of tests/test_abi.py. Built with the address and undefined-behaviour sanitizers and run by
// tests/test_host_units.py; exits 0 if everything holds, 1 with one line per failure otherwise.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/rt2022.h"
#include "../raytracer_2022_amd/csrc/host/plan.hpp"
#include "../raytracer_2022_amd/csrc/host/rt_error.hpp"
#include "../raytracer_2022_amd/csrc/host/scene_check.hpp"

using namespace rt2022;

namespace {

int failures = 0;
void fail(const std::string &what) {
    std::printf("FAIL: %s\n", what.c_str());
    failures++;
}

// ---- (a) the planners ---------------------------------------------------------------------------------------------
constexpr uint64_t kUnknownFree = ~0ull;
void expect_pool(const char *name, uint64_t n_items, uint32_t max_depth, uint32_t want_segs, uint32_t want_blocks, uint32_t segs = 8,
                 int forced_blocks = 0, uint64_t have_slots = 0, uint64_t free_b = kUnknownFree) {
    const PoolPlan p = plan_pool(n_items, 256u, max_depth, segs, forced_blocks, have_slots, [free_b] { return free_b; });
    if (p.segs != want_segs || p.blocks != want_blocks)
        fail(std::string("plan_pool ") + name + ": got " + std::to_string(p.segs) + ", " + std::to_string(p.blocks) + ", want " +
             std::to_string(want_segs) + ", " + std::to_string(want_blocks));
}
void expect_ring(const char *name, uint32_t n_chunks, uint64_t n_pixels, int forced_planes, int forced_group, uint32_t want_planes,
                 uint32_t want_group, uint32_t chunk = 1) {
    const RingPlan r = plan_ring(chunk, n_chunks, n_pixels, n_pixels * n_chunks, forced_planes, forced_group, 115ull << 30);
    if (r.planes != want_planes || r.group != want_group)
        fail(std::string("plan_ring ") + name + ": got " + std::to_string(r.planes) + ", " + std::to_string(r.group) + ", want " +
             std::to_string(want_planes) + ", " + std::to_string(want_group));
}
void expect_chunks(uint32_t spp, uint32_t spp_chunk, uint32_t want_chunk, uint32_t want_n) {
    const Chunks c = plan_chunks(spp, spp_chunk);
    if (c.chunk != want_chunk || c.n_chunks != want_n)
        fail("plan_chunks(" + std::to_string(spp) + ", " + std::to_string(spp_chunk) + "): got " + std::to_string(c.chunk) + ", " + std::to_string(c.n_chunks));
}

void planners() {
    const uint64_t headline = 640000000ull;
    expect_pool("headline", headline, 50, 8, 8192);
    expect_pool("no item", 0, 50, 1, 1);
    expect_pool("one item", 1, 50, 1, 1);
    expect_pool("4096 items", 4096, 50, 8, 64);
    expect_pool("half-pool rule", 36000000ull, 50, 8, 4392);
    expect_pool("20 M items", 20000000ull, 50, 8, 2440);
    expect_pool("56 GB tape clamp", headline, 100, 8, 4584);
    expect_pool("16 GiB free", headline, 50, 8, 1416, 8, 0, 0, 16ull << 30);
    expect_pool("16 GiB free, the pool is there", headline, 50, 8, 8192, 8, 0, 8192ull * 4096ull, 16ull << 30);
    expect_pool("one forced block", headline, 50, 1, 1, 8, 1);
    expect_pool("two segments, seven forced blocks", headline, 50, 2, 6, 2, 7);
    expect_pool("segs 0", headline, 50, 1, 1024, 0);
    expect_pool("segs 15", headline, 50, 8, 8192, 15);

    expect_ring("small frame", 1000, 640000, 0, 0, 0, 1);
    expect_ring("99.5 GB: below the threshold", 1000, 4147200, 0, 0, 0, 1);
    expect_ring("above the threshold", 1000, 8294400, 0, 0, 125, 25);
    expect_ring("one forced plane", 7, 384, 1, 0, 1, 1);
    expect_ring("two forced planes", 7, 384, 2, 0, 2, 1);
    expect_ring("three planes, 37 samples", 37, 64, 3, 0, 3, 1);
    expect_ring("100 forced planes", 1000, 640000, 100, 0, 100, 25);
    expect_ring("100 forced planes, groups of 10", 1000, 640000, 100, 10, 100, 10);
    expect_ring("ring >= chunks", 1000, 640000, 1000, 0, 0, 1);
    expect_ring("forced off", 1000, 8294400, -1, 0, 0, 1);
    expect_ring("two samples per item", 1000, 8294400, 0, 0, 0, 1, 2);
    expect_ring("one chunk", 1, 8294400, 0, 0, 0, 1);
    expect_ring("no pixel", 1000, 0, 0, 0, 0, 1);

    // samples per work item, items per pixel: all in one item by default, the last item short, never an item of no sample
    expect_chunks(100, 0, 100, 1);
    expect_chunks(100, 1, 1, 100);
    expect_chunks(100, 30, 30, 4);
    expect_chunks(100, 200, 100, 1);
    expect_chunks(0, 0, 1, 1);
    expect_chunks(0, 5, 1, 1);
    expect_chunks(0xFFFFFFFFu, 2, 2, 0x80000000u);
}

// ---- (b) the validator --------------------------------------------------------------------------------------------
uint32_t make_ref(uint32_t kind, uint32_t index) { return (kind << RT_REF_KIND_SHIFT) | index; }

// A scene description under construction: the pools of tests' DescBuilder, one record per call, refs returned.
struct Builder {
    std::vector<rt_bvh_node> nodes;
    std::vector<rt_sphere> spheres;
    std::vector<rt_medium> media;
    std::vector<rt_xform> xforms;
    std::vector<rt_list> lists;
    std::vector<uint32_t> list_items;
    std::vector<rt_material> materials;
    std::vector<rt_texture> textures;
    std::vector<rt_image> images;
    std::vector<uint8_t> image_data;
    uint32_t root = 0;

    uint32_t texture(uint32_t kind, uint32_t a = 0, uint32_t b = 0) {
        rt_texture t;
        std::memset(&t, 0, sizeof t);
        t.kind = kind; t.a = a; t.b = b; t.scale = 1.0;
        textures.push_back(t);
        return (uint32_t)textures.size() - 1;
    }
    uint32_t solid() { return texture(RT_TEX_SOLID); }
    uint32_t checker(uint32_t a, uint32_t b) { return texture(RT_TEX_CHECKER, a, b); }
    uint32_t material(uint32_t kind, uint32_t tex = 0) {
        rt_material m;
        std::memset(&m, 0, sizeof m);
        m.kind = kind; m.tex = tex; m.param = 1.5;
        materials.push_back(m);
        return (uint32_t)materials.size() - 1;
    }
    uint32_t lambertian() { return material(RT_MAT_LAMBERTIAN, solid()); }
    uint32_t isotropic() { return material(RT_MAT_ISOTROPIC, solid()); }
    uint32_t dielectric() { return material(RT_MAT_DIELECTRIC); }
    uint32_t sphere(uint32_t mat) {
        rt_sphere s;
        std::memset(&s, 0, sizeof s);
        s.radius = 1.0; s.mat = mat;
        spheres.push_back(s);
        return make_ref(RT_KIND_SPHERE, (uint32_t)spheres.size() - 1);
    }
    uint32_t node(uint32_t left, uint32_t right) {
        rt_bvh_node n;
        std::memset(&n, 0, sizeof n);
        for (int a = 0; a < 3; a++) { n.bmin[a] = -9.0; n.bmax[a] = 9.0; }
        n.left = left; n.right = right;
        nodes.push_back(n);
        return make_ref(RT_KIND_NODE, (uint32_t)nodes.size() - 1);
    }
    uint32_t translate(uint32_t child) {
        rt_xform x;
        std::memset(&x, 0, sizeof x);
        x.kind = RT_KIND_TRANSLATE; x.child = child;
        xforms.push_back(x);
        return make_ref(RT_KIND_TRANSLATE, (uint32_t)xforms.size() - 1);
    }
    uint32_t medium(uint32_t boundary, uint32_t mat) {
        media.push_back(rt_medium{boundary, mat, -2.0});
        return make_ref(RT_KIND_MEDIUM, (uint32_t)media.size() - 1);
    }
    uint32_t list(const std::vector<uint32_t> &items) {
        lists.push_back(rt_list{(uint32_t)list_items.size(), (uint32_t)items.size()});
        list_items.insert(list_items.end(), items.begin(), items.end());
        return make_ref(RT_KIND_LIST, (uint32_t)lists.size() - 1);
    }
    // A list of two spheres of its own (to be overwritten by the caller): its ref, and the index of its first item.
    uint32_t own_list(uint32_t *first) {
        *first = (uint32_t)list_items.size();
        const uint32_t m = lambertian();
        return list({sphere(m), sphere(m)});
    }
    rt_scene_desc desc() const {
        rt_scene_desc d;
        std::memset(&d, 0, sizeof d);
        d.abi_version = RT2022_ABI_VERSION;
        d.root = root;
        d.n_nodes = (uint32_t)nodes.size(); d.nodes = nodes.data();
        d.n_spheres = (uint32_t)spheres.size(); d.spheres = spheres.data();
        d.n_media = (uint32_t)media.size(); d.media = media.data();
        d.n_xforms = (uint32_t)xforms.size(); d.xforms = xforms.data();
        d.n_lists = (uint32_t)lists.size(); d.lists = lists.data();
        d.n_list_items = (uint32_t)list_items.size(); d.list_items = list_items.data();
        d.n_materials = (uint32_t)materials.size(); d.materials = materials.data();
        d.n_textures = (uint32_t)textures.size(); d.textures = textures.data();
        d.n_images = (uint32_t)images.size(); d.images = images.data();
        d.image_data_bytes = image_data.size(); d.image_data = image_data.data();
        return d;
    }
};

// check_scene's verdict on `b`: the code (RT_OK: accepted) and, refused, a message that holds `needle`.
void expect(const char *name, const Builder &b, int want_code, const char *needle = "") {
    int code = RT_OK;
    std::string msg;
    try {
        (void)check_scene(b.desc());
        (void)breadth_first_nodes(b.desc());           // (what rt_scene_create does next with an accepted description)
    } catch (const Fail &e) {
        code = e.code;
        msg = e.msg;
    }
    if (code != want_code || msg.find(needle) == std::string::npos)
        fail(std::string("validator, ") + name + ": code " + std::to_string(code) + " \"" + msg + "\", want " + std::to_string(want_code) + " \"" + needle + "\"");
}

// A Lambertian sphere whose texture is `depth` checkers deep, alternating sides, distinct solids below.
Builder checker_chain(int depth) {
    Builder b;
    uint32_t tex = b.solid();
    for (int lvl = 0; lvl < depth; lvl++) {
        const uint32_t other = b.solid();
        tex = lvl % 2 ? b.checker(other, tex) : b.checker(tex, other);
    }
    b.root = b.sphere(b.material(RT_MAT_LAMBERTIAN, tex));
    return b;
}

Builder with_image(uint32_t width, uint32_t height, uint64_t offset, size_t data_bytes = 12) {
    Builder b;
    b.images.push_back(rt_image{width, height, offset});
    b.image_data.assign(data_bytes, 0);
    b.root = b.sphere(b.material(RT_MAT_LAMBERTIAN, b.texture(RT_TEX_IMAGE, 0)));
    return b;
}

void validator() {
    // test_scene_validation_errors_are_reported_not_crashed
    {
        Builder b;
        b.sphere(b.lambertian());
        b.root = make_ref(RT_KIND_SPHERE, 7);
        expect("root index out of range", b, RT_ERR_INVALID, "out of range");
    }
    {
        Builder b;
        b.root = b.sphere(3);
        expect("material index out of range", b, RT_ERR_INVALID);
    }
    {
        Builder b;
        const uint32_t sph = b.sphere(b.lambertian());
        const uint32_t n0 = b.node(sph, sph);
        b.nodes[0].left = n0;
        b.root = n0;
        expect("a node that is its own child", b, RT_ERR_INVALID, "cycle");
    }
    {
        Builder b;
        const uint32_t lam = b.lambertian();
        b.root = b.medium(b.sphere(lam), lam);
        expect("phase function must be Isotropic", b, RT_ERR_INVALID);
    }
    // test_checker_chains_are_validated: 8 deep accepted, 9 deep refused with the limit in the message, cycles refused
    expect("checkers 8 deep", checker_chain(8), RT_OK);
    {
        Builder b;
        uint32_t tex = b.solid();
        for (int i = 0; i < 8; i++) tex = b.checker(tex, tex);
        b.root = b.sphere(b.material(RT_MAT_LAMBERTIAN, tex));
        expect("checkers 8 deep, every child shared", b, RT_OK);
    }
    for (int depth : {9, 10, 40}) {
        expect("checkers too deep (8)", checker_chain(depth), RT_ERR_UNSUPPORTED, "8");
        expect("checkers too deep (checker)", checker_chain(depth), RT_ERR_UNSUPPORTED, "checker");
    }
    {
        Builder b = checker_chain(2);
        uint32_t unused = b.solid();
        for (int i = 0; i < 9; i++) unused = b.checker(unused, unused);
        expect("checkers too deep in a texture no material uses", b, RT_ERR_UNSUPPORTED);
    }
    {
        Builder b = checker_chain(1);
        const uint32_t top = (uint32_t)b.textures.size() - 1;
        b.textures[top].a = top;
        expect("a checker that is its own child", b, RT_ERR_INVALID, "cycle");
    }
    {
        Builder b = checker_chain(2);
        const uint32_t top = (uint32_t)b.textures.size() - 1, inner = b.textures[top].b;
        if (b.textures[inner].kind != RT_TEX_CHECKER) fail("checker_chain(2): the inner checker is not where the case expects it");
        b.textures[inner].b = top;
        expect("a cycle of two checkers", b, RT_ERR_INVALID, "cycle");
    }
    {
        Builder b = checker_chain(1);
        const uint32_t s0 = b.solid(), x = b.checker(s0, s0), y = b.checker(s0, x);
        b.textures[x].b = y;
        b.checker(s0, y);                                      // (sound itself; its child lies on the cycle)
        expect("a checker cycle reached through a sound checker", b, RT_ERR_INVALID, "cycle");
    }
    // test_scene_graph_cycles_are_refused_and_shared_records_walked_once
    {
        Builder b;
        uint32_t first;
        const uint32_t me = b.own_list(&first);
        b.list_items[first] = b.list_items[first + 1] = me;
        b.root = me;
        expect("a list that holds itself twice", b, RT_ERR_INVALID, "cycle");
    }
    {
        Builder b;
        uint32_t f0, f1;
        const uint32_t l0 = b.own_list(&f0), l1 = b.own_list(&f1);
        b.list_items[f0] = b.list_items[f0 + 1] = l1;
        b.list_items[f1] = b.list_items[f1 + 1] = l0;
        b.root = l0;
        expect("two lists that hold each other twice", b, RT_ERR_INVALID, "cycle");
    }
    {
        Builder b;
        const uint32_t t = b.translate(b.sphere(b.lambertian()));
        b.xforms[0].child = t;
        b.root = t;
        expect("a mover that is its own child", b, RT_ERR_INVALID, "cycle");
    }
    {
        Builder b;
        const uint32_t inner = b.translate(b.sphere(b.dielectric()));
        const uint32_t fog = b.medium(inner, b.isotropic());
        b.xforms[0].child = fog;
        b.root = fog;
        expect("a medium whose boundary leads back to it through a mover", b, RT_ERR_INVALID, "cycle");
    }
    {
        Builder b;
        b.sphere(b.dielectric());
        uint32_t first;
        const uint32_t inner = b.own_list(&first);
        const uint32_t fog = b.medium(inner, b.isotropic());
        b.list_items[first + 1] = fog;
        b.root = fog;
        expect("a medium whose boundary leads back to it through a list", b, RT_ERR_INVALID, "cycle");
    }
    {
        Builder b;
        const uint32_t fog = b.medium(b.sphere(b.dielectric()), b.isotropic());
        const uint32_t shared = b.list({fog, b.sphere(b.dielectric())});
        b.root = b.list({shared, b.medium(shared, b.isotropic())});      // (walked from the root first, then as a boundary)
        expect("a medium below a list shared with another medium's boundary", b, RT_ERR_UNSUPPORTED, "medium");
    }
    {
        Builder b;
        const uint32_t sph = b.sphere(b.lambertian());
        uint32_t ref = b.list({sph, sph});
        for (int i = 0; i < 39; i++) ref = b.list({ref, ref});
        b.root = ref;
        if (b.lists.size() != 40 || b.list_items.size() != 80) fail("the shared-list DAG is not 40 lists of 2 items");
        expect("40 lists, each holding the next twice", b, RT_OK);
    }
    {
        Builder b;
        const uint32_t sph = b.sphere(b.dielectric());
        uint32_t ref = b.translate(sph);
        for (int i = 0; i < 30; i++) ref = i % 2 ? b.list({ref, ref}) : b.node(ref, b.list({ref}));
        b.root = b.list({b.medium(ref, b.isotropic()), ref});
        expect("sharing through movers, nodes and a medium's boundary", b, RT_OK);
    }
    // test_image_bounds_check_does_not_wrap
    expect("image 2 x 2 at 0", with_image(2, 2, 0), RT_OK);
    expect("image ending exactly at the end of the data", with_image(2, 2, 4, 16), RT_OK);
    expect("an empty image at the very end", with_image(0, 0, 12), RT_OK);
    const struct { uint32_t width, height; uint64_t offset; } wrapping[] = {
        {2, 2, ~0ull - 7}, {0xFFFFFFFFu, 0xFFFFFFFFu, 0}, {0xFFFFFFFFu, 0xFFFFFFFFu, ~0ull - 7}, {2, 2, 1}, {2, 3, 0}, {0, 0, 13}, {0x80000000u, 2, 0},
        {1, 1, ~0ull}};
    for (const auto &w : wrapping) expect("image out of range", with_image(w.width, w.height, w.offset), RT_ERR_INVALID, "image");
}

} // namespace

int main() {
    planners();
    validator();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("host units ok\n");
    return 0;
}
