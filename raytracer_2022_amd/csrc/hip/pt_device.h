// pt_device.h — device-side views of the flattened scene and the launch interface
// between the entry points (hip/rt_*.hip: C ABI, HBM residency) and the kernels (pt_*.hip).
#ifndef RT2022_PT_DEVICE_H
#define RT2022_PT_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../../include/rt2022.h"
#include "../host/rt_constants.hpp"
#include "hip_owned.hpp"

namespace rt2022 {

// ConstantMedium as the traversal kernel wants it: one 64-byte record = one fetch, with the boundary's data inline
// when the boundary is a plain Sphere (the fog and the subsurface ball of the final scene) — rt_medium alone would cost
// a dependent second fetch of the sphere record.
struct MediumDev {
    double center[3], radius;          // boundary sphere (zeros when the boundary is something else)
    double neg_inv_density;
    uint32_t boundary, mat;            // mat = material index | slot kind << kMatKindShift, like the primitive pools
    uint32_t sphere_boundary;          // 1: the boundary is a plain Sphere
    uint32_t _pad[3];
};

// A material as the shading kernel wants it: one 80-byte record = one fetch, with the top-level record of its texture
// inline (kind, children / table ids, scale, colour) — a SolidColor albedo then needs no second, dependent fetch.
struct MaterialDev {
    uint32_t tex, tex_kind;            // rt_material::tex and that texture's kind
    double albedo[3];                  // Metal
    double param;                      // Metal fuzz / Dielectric ir
    double tex_color[3];               // rt_texture::color
    double tex_scale;                  // rt_texture::scale
    uint32_t tex_a, tex_b;             // rt_texture::a, b
};

// Pointers into HBM, one pool per kind (layouts = include/rt2022.h).
struct SceneDev {
    const rt_bvh_node *nodes;
    // The node table once more in single precision, 32 bytes per node: {min.x, max.x, min.y, max.y | min.z, max.z, left, push ref}
    // (floats rounded to nearest from the doubles of `nodes`, same numbering) — what the sphere-scene traversal kernels that cannot
    // keep the whole table in LDS fetch per node step (wf_trace, kF32G; the double-precision record serves the undecided steps).
    const uint32_t *nodes32;
    const rt_sphere *spheres;
    const rt_moving_sphere *moving_spheres;
    const rt_rect *rects;
    const rt_box *boxes;
    const rt_triangle *triangles;
    const rt_ring *rings;
    const rt_medium *media;
    const rt_xform *xforms;
    const rt_list *lists;
    const uint32_t *list_items;
    const uint32_t *lights;
    const rt_material *materials;
    const rt_texture *textures;
    const rt_image *images;
    const uint8_t *image_data;
    const rt_perlin *perlins;
    uint32_t root;
    uint32_t n_lights;
    const MaterialDev *materials_dev;  // [n_materials], shading kernel's view of `materials` + `textures`
    const MediumDev *media_dev;        // [n_media], traversal kernel's view of `media`
    uint32_t media_mode;               // 0: no medium has a plain-sphere boundary, 1: all have, 2: mixed (look at the record)
    uint32_t n_nodes;                  // records in `nodes`
    uint32_t n_xforms, n_media;        // records in `xforms`, `media_dev`
    uint32_t n_spheres, n_moving_spheres;
    uint32_t n_rects;                  // (0 with FEAT 0: every primitive is a sphere — the scenes that take the single-precision slab test)
    // Child order of the timed wavefront traversal (host/scene_check.hpp: child_order; wf_trace). A node ref
    // READ BY THOSE KERNELS carries its node's order in bits 24..26 (0: the reference's order): the last two words of a node
    // record — {push ref, left} so tagged, beside the plain {left, right} every other kernel reads — nodes32, and these copies
    // of the root ref, the list items and the mover records. node_index_mask takes the index out of such a ref (24 bits, or
    // all 27 where nothing is tagged). prim_rank: the tie rule's table (null: no rule), ranks of kind k's pool from word [k] on.
    const uint32_t *list_items_ord;
    const rt_xform *xforms_ord;
    const uint32_t *prim_rank;
    uint32_t root_ord;
    uint32_t node_index_mask;
};

// Counter block in HBM (same order as rt_stats' integer fields).
struct StatsDev {
    unsigned long long paths, rays, node_visits;
    unsigned long long prim_tests[RT_KIND_COUNT];
    unsigned long long light_pdf_tests, rng_draws;
    // Scheduler census of the traversal kernel (counter builds only): per operation label, how many
    // times a wave ran it and how many lanes it served; [8] = the node fast path.
    unsigned long long op_rounds[9], op_lanes[9];
};

struct RenderArgs {
    rt_camera cam;
    uint32_t width, height, spp, max_depth;
    uint32_t n_frames, n_rows;
    uint32_t chunk, n_chunks;          // samples per work item, items per pixel
    double background[3];
    double t_min;
    uint64_t seed;
    uint64_t n_pixels;                 // n_rows * width
    uint64_t n_items;                  // n_pixels * n_chunks
    const uint32_t *row_ids;           // device
    double *partial;                   // [n_chunks][n_pixels][3] (== out when n_chunks == 1)
    unsigned long long *work_counter;  // zeroed before launch
    double *tape;                      // bounce records: max_depth * 4 doubles per launched lane
    // Ring of partial-sum planes (r3; one-sample work items only). 0: `partial` holds all n_chunks planes and chunk_sum adds
    // them at the end. R > 0: the samples are taken in GROUPS of ring_group consecutive ones (a divisor of spp, R a multiple of
    // it): work items are numbered group-major — item = (group * n_pixels + pixel) * ring_group + sample within the group, so
    // that the samples of a pixel in a group are still neighbours on the work counter (their camera rays stay coherent: plain
    // sample-major order cost the traversal kernel 8 % on the headline and 30 % on C5) — sample c of a pixel goes to plane c mod R,
    // the host adds finished groups of planes to the output in sample order as the frame goes (ring_accumulate) and raises
    // *claim_limit — the number of work items that may be handed out — behind them: R planes instead of spp, the same sums bit
    // for bit (pixel_color += ..., main.rs:150, in sample order).
    uint32_t ring, ring_group;
    const unsigned long long *claim_limit;
    uint32_t tuning;                   // the tuning word (namespace tune below), bit 31 set by the host
    uint32_t vote_weights;             // 4 bits per operation label: the vote picks max(lanes * weight)
    StatsDev *stats;                   // may be null
    // rt_radiance* (device, null for a render): the caller's rays take the place of the camera. The "pixels" are the
    // rays (n_pixels = n_rays, width = 1, no row ids), one sample per work item, the path of sample s of ray i keyed
    // path_key(rays[i].rng_state, 0, 0, s); wf_shade's rays instances read them in its fresh-path sweep.
    const rt_radiance_ray *rays;
    // rt_render_pixels* (device, null otherwise): a list of (frame, pixel) ids takes the place of the row list. The "pixels" are
    // the entries (n_pixels = n_entries, no row ids); entry e renders id = frame * (width * height) + py * width + px with the
    // render's own keying and camera draws — width, height and n_frames stay the image's. wf_shade's pixel instances decode it.
    const uint64_t *pixel_ids;
};

// ---- wavefront engine (pt_wavefront.hip) -------------------------------------------
// What a path slot waits for.
enum SlotKind : uint32_t {
    SK_IDLE = 0,        // nothing left to do
    SK_FRESH = 1,       // no path yet: start the first sample
    SK_TRACE = 2,       // carries a ray: world.hit pending
    SK_MISS = 3,
    SK_LIGHT = 4,
    // Lambertian by albedo texture: a wave that holds one noise-textured hit pays seven octaves of
    // Perlin for all 64 lanes, so the texture kind is part of the sort key.
    SK_LAMB_SOLID = 5,
    SK_LAMB_CHECKER = 6,
    SK_LAMB_NOISE = 7,
    SK_LAMB_IMAGE = 8,
    SK_METAL = 9,
    SK_DIELECTRIC = 10,
    SK_ISOTROPIC = 11,
    SK_COUNT = 12
};


// A pool of path slots in HBM, one array of records per field; segment b (= shade workgroup b) owns
// the slots [b*kSlotsPerBlock, (b+1)*kSlotsPerBlock) for the whole frame (kSlotsPerBlock: rt_constants.hpp).
constexpr uint64_t kRecBytes = 128, kRecDoubles = kRecBytes / 8, kRecWords = kRecBytes / 4;      // the slot record
struct WfPool {
    uint32_t n_slots;
    uint32_t n_blocks;      // segments
    uint8_t *kind;          // [P]    what a listed slot waits for (SlotKind), BY POSITION ON ITS SEGMENT'S RAY LIST (see `list`)
    // ONE 128-byte record per slot = one cache line, three parts (`ray`, `hit`, `state` point at their part of slot 0;
    // stride kRecDoubles doubles / kRecWords words): the shade pass, which visits slots in sorted order, then pulls one
    // line per slot instead of one line from each of three arrays (measured: shade's HBM reads per ray segment).
    //   +0   ray:   {ox oy oz dx dy dz tm, rng state}                                                        64 B
    //   +64  hit:   {t (f64), leaf ref, box face | movers << 4 | node steps << 16, 3 mover refs, 4th ref or material word}   32 B
    //   +96  state: {item = pixel slot * n_chunks + chunk (u64), next sample, end sample, remaining depth, px, py, frame}    32 B
    double *ray;
    uint32_t *hit;
    uint32_t *state;
    double *pixel_sum;      // [P][4]  running sum of the item (4th double unused)
    double *tape;           // [P][tape_cap][4] bounce records {w.x, w.y, w.z, p}
    uint32_t tape_cap;      // records per slot (>= max_depth)
    // Ray list of every segment (= the 4096 slots one shade workgroup owns), written by the shade pass:
    // local indices of the slots that carry a ray, longest expected traversal first. A trace workgroup
    // works through the lists of `segs` consecutive segments.
    uint16_t *list;         // [P]
    uint32_t *list_n;       // [n_blocks]
    uint32_t segs;          // segments per trace workgroup (n_blocks is a multiple of it)
    uint32_t *next_chunk;   // trace pass: the next chunk of list entries to hand out (cleared by the shade pass)
    uint32_t *max_list;     // [2] longest segment list of the pass, by pass parity (bounds the chunk ids)
    uint32_t n_cus;         // compute units of the device (size of the persistent trace grid)
    uint32_t *n_active;     // [2] rays handed to the next trace pass, by pass parity (polled by the host)
    uint32_t *fault;        // [1] engine invariants found broken on the device (bit 0: a slot reached the shade pass untraced)
    // Ring mode (RenderArgs::ring): the oldest sample GROUP with a path still in flight after a shade pass, by pass parity (every
    // group below it is finished: the host consumes their planes), and per segment the slots that asked for a work item and found
    // the ring full: listed behind the segment's rays, with kind FRESH, so that the next shade pass asks again.
    unsigned long long *oldest;     // [2]
    uint32_t *starved_n;            // [n_blocks]
    // Pass-timing probe (rt_debug_pass_timing; null otherwise): {first wave start, last wave end, sum of
    // wave lifetimes, sum of wave time after the list ran dry, waves} in wall_clock64 ticks.
    unsigned long long *dbg;
};

// ---- the tuning word ----------------------------------------------------------------
// rt_scene::tuning / RenderArgs::tuning, set by rt_debug_set_tuning (its node_quorum argument): scheduler knobs of the engines,
// speed only, never results. This is the one description of its fields; every reader goes through these accessors.
//   0-7    quorum: lanes that must want a BVH-node step before the wave takes the node fast path without a vote (1..64; the
//          one field the megakernel and nothing else of the word reads)
//   8-14   accepted and ignored: extra sphere tests per turn (8-11) and the tail factor (12-14) went with the build switches
//          that read them (two sphere tests per turn and a tail factor of 2 are built in); callers still pass 1 and 2 here
//   15     kRefOrder: the timed wavefront traversal visits a node's children in the reference's order, left then right, whatever
//          the node's order bits say (A/B runs, bit-parity tests)
//   16-19  segments: pool size of the wavefront engine, segments of kSlotsPerBlock path slots per resident traversal workgroup (1..8)
//   20-23  class_shift s: every segment's ray list is ordered longest-first by (expected node steps) >> s, 0 = slot order
//   24-27  groups the pool is cut into, each alternating its passes on a stream of its own (1..kMaxGroups; 0: the library's choice)
//   28     kNoNodeTable: the plain traversal kernels even where a node-table variant applies (A/B runs, bit-parity tests)
//   29     kPassTiming: run the pass-timing probe (rt_debug_pass_timing)
//   30     kLiteralStep: take the literal AABB step only (test hook)
//   31     kBoxesPlain: every node box finite with min <= max, the short node step applies — set by the host for the kernels
//          (for_kernels), whatever the caller passed
namespace tune {
constexpr uint32_t kSegmentsShift = 16, kClassShift = 20, kGroupsShift = 24;
constexpr uint32_t kRefOrder = 1u << 15;
constexpr bool ref_order(uint32_t word) { return (word & kRefOrder) != 0; }
constexpr uint32_t kNoNodeTable = 1u << 28, kPassTiming = 1u << 29, kLiteralStep = 1u << 30, kBoxesPlain = 1u << 31;
constexpr uint32_t quorum(uint32_t word) { return word & 0xFFu; }
constexpr uint32_t segments(uint32_t word) { return (word >> kSegmentsShift) & 0xFu; }
constexpr uint32_t class_shift(uint32_t word) { return (word >> kClassShift) & 0xFu; }
constexpr uint32_t groups(uint32_t word) { return (word >> kGroupsShift) & 0xFu; }
constexpr bool no_node_table(uint32_t word) { return (word & kNoNodeTable) != 0; }
constexpr bool pass_timing(uint32_t word) { return (word & kPassTiming) != 0; }
constexpr bool literal_step(uint32_t word) { return (word & kLiteralStep) != 0; }
constexpr bool boxes_plain(uint32_t word) { return (word >> 31) != 0; }
// The word as the kernels get it: the scene's, with bit 31 = the host's finding about the node boxes unless bit 30 forbids it.
constexpr uint32_t for_kernels(uint32_t word, bool plain) { return (word & ~kBoxesPlain) | (plain && !literal_step(word) ? kBoxesPlain : 0u); }
// The default: fast-path quorum 18 lanes; (retired: one extra sphere test per turn, tail factor 2); pool of 8 segments per resident
// trace workgroup (4 per CU: 8192 segments = 33.5 M slots); list classes of 4 node steps; groups of segments: the library's choice (0).
constexpr uint32_t kRetiredDefault = (1u << 8) | (2u << 12);
constexpr uint32_t kDefault = 18u | kRetiredDefault | ((uint32_t)(8 * 4096 / kSlotsPerBlock > 0 ? 8 * 4096 / kSlotsPerBlock : 1) << kSegmentsShift) |
                              (2u << kClassShift) | (0u << kGroupsShift);
static_assert(kDefault == 0x00282112u, "the default tuning word");
} // namespace tune

// Traversal-stack capacities the megakernel is instantiated for (the largest, kStackLarge: rt_constants.hpp).
constexpr int kStackSmall = 22;   // 22 KiB of LDS per workgroup; the lean kernels run four workgroups per CU (VGPR-bound)
constexpr int kStackMid = 30;     // million-triangle meshes need ~26 entries; built for four workgroups per CU
constexpr int kBlock = 256;
// Vote weights of the traversal schedulers, four bits per operation label from the lowest nibble up: node, sphere, rect,
// box, medium, misc, ctx, done (publish + refill). The wave runs the label with the largest lanes x weight.
constexpr uint32_t kWfVoteWeights = 0x24444442u;      // wavefront engine: node and refill yield to the arms (the megakernel votes by plain counts)
// Node-cache variant of the traversal kernel (pt_wavefront_trace.hip): one workgroup of 1024 threads per CU, stacks of 16
// entries (64 KiB), and the first kNodeCache node records in the remaining LDS (56 bytes each: 97 440 B).
constexpr int kCacheBlock = 1024;
constexpr int kStackTiny = 16;
constexpr int kNodeCache = 1740;
// The all-in-LDS instance for small sphere-only scenes: 600 node records (33 600 B), 256 Sphere records (36 B each) and
// 512 MovingSphere records (80 B each) beside the 64 KiB of stacks.
constexpr int kPrimNodes = 600, kPrimSpheres = 256, kPrimMoving = 512;

// ---- closest-hit queries (pt_query.hip, rt_intersect*) ------------------------------
struct QueryArgs {
    const rt_query_ray *rays;          // device, 16-byte aligned
    rt_hit *hits;                      // device, 16-byte aligned
    uint64_t n_rays;
    unsigned long long *counter;       // rays handed out so far (zeroed before launch)
    StatsDev *stats;                   // counter instances only
};
hipError_t launch_query(const SceneDev &scene, const QueryArgs &args, uint32_t stack_need, bool counters, bool any_hit,
                        hipStream_t stream);

// ---- first-hit feature buffers (pt_features.hip, rt_features*) ----------------------
struct FeatureArgs {
    rt_camera cam;
    uint32_t width, height, spp;
    union {
        uint32_t n_rows;
        uint32_t ids32;                // pixel source: width * height * n_frames fits 32 bits, the ids are decoded by 32-bit divisions
    };
    double background[3];
    double t_min;
    uint64_t seed;
    uint64_t n_pixels;                 // n_rows * width; pixel source: the entries of the list; ray source: the rays
    union {                            // device (a union, and ids32 one above: the row instances' kernel arguments keep their layout)
        const uint32_t *row_ids;
        const uint64_t *pixel_ids;     // pixel source: n_pixels ids, frame * (width * height) + py * width + px, each < width * height * n_frames
        const rt_radiance_ray *rays;   // ray source: n_pixels records, 16-byte aligned, never validated (cam, width, height, seed unused)
    };
    rt_feature *out;                   // device, 16-byte aligned: n_pixels records in row_ids order (in list order, in the rays' order)
    unsigned long long *counter;       // pixels handed out so far (zeroed before launch)
    StatsDev *stats;                   // counter instances only
};
// The source of work items (the kernels' SRC): the rows of a row list (rt_features*: args.row_ids, args.n_rows), a list of (frame,
// pixel) ids (rt_features_pixels*: args.pixel_ids and args.ids32 in their place), or the caller's rays (rt_features_rays*: args.rays;
// one record per ray, in the rays' order).
constexpr int kFeatRows = 0, kFeatPixels = 1, kFeatRays = 2;
// `surfaces`: RT_FLAG_SURFACES, the instances that pop a medium leaf instead of entering it. `specular`: RT_FLAG_SPECULAR, the
// instances of pt_features_specular.hip that follow a sample through glass and mirrors (with counters they count their rays).
hipError_t launch_features(const SceneDev &scene, const FeatureArgs &args, uint32_t stack_need, int src, bool counters, bool surfaces,
                           bool specular, hipStream_t stream);

// ---- the calls on a render's buffers: where the pieces of their workspaces lie is host/post_check.hpp's to know ----
// The row kernel (pt_rows.hip) on a list of `height` ids: inv[image row] = buffer row, *bad = ids out of range or repeated.
hipError_t launch_row_list_check(const uint32_t *rows, uint32_t height, uint32_t *inv, uint32_t *bad, hipStream_t stream);

// ---- edge-avoiding denoiser (pt_denoise.hip, rt_denoise*) ----------------------------
struct DenoiseArgs {
    uint32_t width, height;
    double sp;                         // (double)spp
    double inv_n, inv_z, inv_a;        // 1 / sigma^2 of normal, depth, albedo
    double albedo_floor;
    bool demodulate;
    const double *sum;                 // device: the render's sums, buffer order
    const rt_feature *feat;            // device, 16-byte aligned, buffer order
    const uint32_t *inv;               // device: image row -> buffer row (null: the identity)
    double *out;                       // device: the filtered sums, buffer order (may be `sum`)
    char *ws;                          // the workspace, 16-byte aligned, laid out by denoise_layout
};
// prepare + n_iter a-trous passes; inv_c[k] = 1 / sigma_k^2.
hipError_t launch_denoise(const DenoiseArgs &a, uint32_t n_iter, const double *inv_c, hipStream_t stream);

// ---- variance-guided denoiser over two half-sample renders (pt_denoise.hip, rt_denoise_dual*) ----
struct DenoiseDualArgs {
    DenoiseArgs a;                     // half A's buffers; sp = (double)spp of ONE half; ws laid out by denoise_dual_layout
    const double *sum_b;               // device: half B's sums, buffer order
    const rt_feature *feat_b;          // device, 16-byte aligned, buffer order
    double *out_var;                   // device: the residual variance, buffer order (null: not wanted)
    double sp2;                        // sp + sp
    double inv_c;                      // 1 / sigma_color^2, every iteration's
    double var_floor;
};
// dual prepare + var_iter prefilter passes + n_iter variance-aware a-trous passes.
hipError_t launch_denoise_dual(const DenoiseDualArgs &a, uint32_t var_iter, uint32_t n_iter, hipStream_t stream);

// ---- temporal accumulation with reprojection (pt_temporal.hip, rt_temporal*) ------------------------------
// One kernel, one lane per pixel; the workspace holds nothing but the row kernel's map.
struct TemporalArgs {
    uint32_t width, height;
    double sp;                         // (double)spp
    double wm1, hm1;                   // (double)(width - 1), (double)(height - 1)
    double wd, hd;                     // (double)width, (double)height
    double tol_depth, tol_normal, n_max, w_min, albedo_floor;
    bool demodulate, depth_test, normal_test;      // (a tolerance of +inf switches its test off)
    bool far_misses;                   // RT_TEMPORAL_FAR_MISSES: uncovered pixels reproject as points at infinity
    double o[3], llc[3], hor[3], ver[3];           // the current camera
    double po[3], pr[3], phor[3], pver[3];         // the previous camera: origin, origin - lower_left_corner, horizontal, vertical
    const double *sum;                 // device: the render's sums, buffer order
    const rt_feature *feat;            // device, 16-byte aligned, buffer order
    const uint32_t *inv;               // device: image row -> buffer row (null: the identity)
    const rt_temporal_pixel *prev;     // device, image order (null: the first frame)
    rt_temporal_pixel *state;          // device, image order; never overlaps prev
    double *out;                       // device: the accumulated sums, buffer order (may be `sum`)
};
hipError_t launch_temporal(const TemporalArgs &a, hipStream_t stream);

// ---- adaptive sampling: planner, merge, resolve (pt_adaptive.hip, rt_adaptive_*) -----------------------
struct AdaptivePlanArgs {
    uint32_t width, height, first_frame, max_units;
    double scale;
    const double *err;                 // device, buffer order
    const uint32_t *rows;              // device: buffer row -> image row (null: the identity), already through the row kernel
    uint32_t *units;                   // device: [n]
    uint64_t *offsets;                 // device: [n + 1]
    uint64_t *entries;                 // device: [capacity] (null with capacity 0)
    uint64_t capacity;
    char *ws;                          // the workspace, 16-byte aligned, laid out by adaptive_layout
};
// The scan's three launches; the total is then at ws + totals + 8 * n_tiles. With rows, ad_emit reads the row kernel's count at ws + rows.bad.
hipError_t launch_adaptive_plan(const AdaptivePlanArgs &p, hipStream_t stream);
hipError_t launch_adaptive_merge(const double *sums, const uint32_t *units, const uint64_t *offsets, uint64_t n, uint32_t spp, double *acc,
                                 double *acc_n, hipStream_t stream);
hipError_t launch_adaptive_resolve(const double *acc, const double *acc_n, uint64_t n, uint32_t spp_out, double *out, hipStream_t stream);
// The same two for rt_feature records (16-byte aligned): all eight fields are linear; the sample count is the radiance merge's.
hipError_t launch_adaptive_merge_features(const rt_feature *entries, const uint32_t *units, const uint64_t *offsets, uint64_t n, rt_feature *acc,
                                          hipStream_t stream);
hipError_t launch_adaptive_resolve_features(const rt_feature *acc, const double *acc_n, uint64_t n, uint32_t spp_out, rt_feature *out,
                                            hipStream_t stream);

// Launchers (pt_kernel.hip). `stack_need` = entries the scene needs (host-computed).
hipError_t launch_render(const SceneDev &scene, const RenderArgs &args, uint32_t stack_need, bool counters,
                         int n_blocks_hint, hipStream_t stream);

// Streams the wavefront engine runs its groups of segments on, with their events and pinned words: all created when
// one is constructed (the caller keeps it from render to render).
constexpr int kMaxGroups = 8;
struct WfStreams {
    int n = 0;                         // groups wanted (1 = everything on the caller's stream)
    Stream stream[kMaxGroups];
    Event ev[kMaxGroups][2];
    PinnedBuf<uint32_t> h_active{2 * kMaxGroups};             // [kMaxGroups][2]
    PinnedBuf<unsigned long long> h_work{2 * kMaxGroups};     // [kMaxGroups][2]: the work counter as of the same batches (progress callback, ring mode)
    PinnedBuf<unsigned long long> h_oldest{2 * kMaxGroups};   // [kMaxGroups][2]: WfPool::oldest as of the same batches (ring mode)
    WfStreams() {
        for (int g = 0; g < kMaxGroups; g++) {
            stream[g] = Stream(hipStreamNonBlocking);
            for (int b = 0; b < 2; b++) ev[g][b] = Event(hipEventDisableTiming);
        }
    }
};
// rt_params::progress_cb as the engine sees it (host side only).
struct Progress {
    void (*cb)(void *, uint32_t, uint64_t, uint64_t) = nullptr;
    void *user = nullptr;
    uint64_t total = 0;                // camera paths of the call
    uint32_t per_item = 1;             // samples per work item
};
// Per-kernel device time of one render (RT_FLAG_KERNEL_TIMES): HIP events on the launch stream around every pass.
struct KernelTimes {
    std::vector<Event> ev;             // grown on demand, reused from call to call
    double shade_ms = 0.0, trace_ms = 0.0;
};
// Ring mode: what the engine needs to consume planes as the frame goes.
struct RingCtl {
    uint32_t planes = 0;               // 0 = off
    double *out = nullptr;             // [n_pixels * 3] the call's output: finished planes are added to it in sample order
    unsigned long long *d_limit = nullptr;   // device word behind RenderArgs::claim_limit
    uint32_t max_passes = 0;           // watchdog: more pass pairs than this is an engine error, not a long frame
};
// One render of the wavefront engine: what launch_render_wavefront is given, and what it reports.
struct WfRender {
    const SceneDev *scene = nullptr;
    const RenderArgs *args = nullptr;
    const RenderArgs *d_args = nullptr;    // the device-resident copy of *args
    const WfPool *pool = nullptr;
    uint32_t stack_need = 1;
    unsigned features = 7;
    bool counters = false;
    const WfStreams *gs = nullptr;
    hipStream_t stream = nullptr;
    Progress progress;                     // (cb null: nobody to report to)
    RingCtl ring;                          // (planes 0: off)
    double *timing = nullptr;              // null, or [5]: see rt_debug_pass_timing
    KernelTimes *kt = nullptr;             // null, or where to put the per-kernel times (three HIP events per pass pair on its group's stream)
    // out
    uint32_t passes = 0;                   // pass pairs enqueued
    uint32_t fault = 0;                    // WfPool::fault after the last pass
};
// Wavefront engine: alternates shade / trace passes over the pool until it drains.
// Blocks the calling thread (polls `n_active`).
hipError_t launch_render_wavefront(WfRender &r);
hipError_t launch_chunk_sum(const double *partial, double *out, uint64_t n_values, uint32_t n_chunks, hipStream_t stream);
hipError_t launch_tonemap(const double *rgb_sum, uint64_t n_pixels, int32_t spp, uint8_t *rgb8, hipStream_t stream);
hipError_t launch_math_probe(int op, const double *a, const double *b, double *out, uint64_t n, hipStream_t stream);
hipError_t launch_rng_probe(uint64_t state, int mode, double lo, double hi, uint64_t bound, uint64_t *out, uint64_t n, hipStream_t stream);
// Which traversal variant the wavefront engine launches for a scene without counters: {threads per workgroup, stack entries, nodes kept in LDS}.
void trace_variant(const SceneDev &scene, uint32_t stack_need, uint32_t tuning, unsigned features, uint32_t out[4]);
// {fast-path node steps that took the single-precision slab test, those it left undecided, 1 if this build counts (-DRT2022_F32_CENSUS),
// 1 (2 in a census build: the test in every whole-table instance without meshes), verdicts that differed from the double-precision
// test's (census builds make both)}; clears the counters.
hipError_t f32_slab_census(unsigned long long out[5]);
// Occupancy-derived persistent grid size for the given variant.
int render_grid_blocks(uint32_t stack_need, bool counters);

} // namespace rt2022
#endif
