/*
 * rt2022.h — C ABI of the MI355X path-tracing hot loop.
 *
 * Drop-in boundary for the per-pixel loop of Jerx2y/Raytracer-2022:
 * the body of the render-thread closure, raytracer/src/main.rs:133-159
 * (for y in rows { for x { for s { get_ray; ray_color } } } → Vec<Color>),
 * and the tone map that consumes it, main.rs:280-299.
 *
 * The reference has no FFI of its own: what crosses the seam
 * there is `cam: Camera`, `world: BvhNode`, `lights: HittableList`,
 * `background`, the shuffled row list and the image/sample constants, and what
 * comes back is one `Vec<Color>` of un-normalised f64 RGB sums per worker.
 * Here the same things cross as plain pointers and sizes:
 *
 *   reference (Rust)                          this ABI
 *   ----------------------------------------  ---------------------------------
 *   BvhNode / Arc<dyn Hittable> object graph  rt_scene_desc (flattened pools)
 *   Camera (basic/camera.rs:9-20)             rt_camera (the same 10 fields)
 *   consts + background + line_id slice       rt_params
 *   Vec<Color> sent over mpsc (main.rs:157)   double *out_rgb_sum (caller-owned)
 *   write_color (main.rs:280-299)             rt_write_color / rt_tonemap_device
 *   panic!/unwrap                             negative int + rt_last_error()
 *
 * Ownership: the caller owns every host buffer for the duration of the call
 * only; the library owns device memory behind rt_scene; output buffers are
 * caller-allocated. Threading: rt_render* are re-entrant on one rt_scene for
 * disjoint row sets (one host thread / process per GPU).
 *
 * All arithmetic is f64 like the reference. Integer outputs (pixel indices,
 * u8 colours, counters) are bit-exact against the CPU oracle in oracle/.
 */
#ifndef RT2022_H
#define RT2022_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT2022_ABI_VERSION 3

/* ---------------------------------------------------------------- refs --- */
/* A hittable reference = one `Arc<dyn Hittable>` of the reference, as a tagged
 * 32-bit id:  bit 31 = FlipFace applied to this object (hittable/mod.rs:267-292),
 * bits 30..27 = kind, bits 26..0 = index into that kind's pool. */
#define RT_REF_FLIP      0x80000000u
#define RT_REF_KIND_SHIFT 27
#define RT_REF_INDEX_MASK 0x07FFFFFFu
#define RT_MAKE_REF(kind, index) ((((uint32_t)(kind)) << RT_REF_KIND_SHIFT) | ((uint32_t)(index) & RT_REF_INDEX_MASK))
#define RT_REF_KIND(ref)  ((((uint32_t)(ref)) >> RT_REF_KIND_SHIFT) & 0xFu)
#define RT_REF_INDEX(ref) (((uint32_t)(ref)) & RT_REF_INDEX_MASK)

enum rt_kind {
    RT_KIND_NODE          = 0,  /* BvhNode            hittable/bvh/mod.rs:12-16   */
    RT_KIND_SPHERE        = 1,  /* Sphere<M>          hittable/sphere.rs:12-19    */
    RT_KIND_MOVING_SPHERE = 2,  /* MovingSphere<M>    hittable/sphere.rs:93-103   */
    RT_KIND_RECT          = 3,  /* XY/XZ/YZRect<M>    hittable/aarect.rs          */
    RT_KIND_BOX           = 4,  /* Boxes              hittable/boxes.rs:12-16     */
    RT_KIND_TRIANGLE      = 5,  /* Triangle<M>        hittable/triangle.rs:11-19  */
    RT_KIND_RING          = 6,  /* Ring<M>            hittable/ring.rs:11-20      */
    RT_KIND_MEDIUM        = 7,  /* ConstantMedium<H,T> hittable/constantmedium.rs */
    RT_KIND_TRANSLATE     = 8,  /* Translate<H>       hittable/mod.rs:135-175     */
    RT_KIND_ROTATE_Y      = 9,  /* RotateY<H>         hittable/mod.rs:177-265     */
    RT_KIND_ZOOM          = 10, /* Zoom<H>            hittable/mod.rs:294-331     */
    RT_KIND_LIST          = 11, /* HittableList       hittable/mod.rs:70-133      */
    RT_KIND_COUNT         = 12
};

/* ------------------------------------------------------------- geometry --- */
/* BvhNode flattened: aabbox + two child refs (NODE or object). 64 B. */
typedef struct rt_bvh_node {
    double   bmin[3];
    double   bmax[3];
    uint32_t left;
    uint32_t right;
    uint32_t _pad[2];                 /* one node = one 64-byte line = four 16-byte loads */
} rt_bvh_node;

typedef struct rt_sphere {            /* 40 B */
    double   center[3];
    double   radius;
    uint32_t mat;
    uint32_t _pad;
} rt_sphere;

typedef struct rt_moving_sphere {     /* 80 B */
    double   center0[3];
    double   center1[3];
    double   time0, time1;
    double   radius;
    uint32_t mat;
    uint32_t _pad;
} rt_moving_sphere;

enum rt_rect_axis { RT_RECT_XY = 0, RT_RECT_XZ = 1, RT_RECT_YZ = 2 };

/* XYRect{x0,x1,y0,y1,k} / XZRect{x0,x1,z0,z1,k} / YZRect{y0,y1,z0,z1,k}. 48 B. */
typedef struct rt_rect {
    double   a0, a1, b0, b1, k;
    uint32_t axis;
    uint32_t mat;
} rt_rect;

/* Boxes::new(p0,p1,m): six rects in the order of boxes.rs:24-66. 56 B. */
typedef struct rt_box {
    double   p0[3];
    double   p1[3];
    uint32_t mat;
    uint32_t _pad;
} rt_box;

typedef struct rt_triangle {          /* 80 B */
    double   a[3], b[3], c[3];
    uint32_t mat;
    uint32_t _pad;
} rt_triangle;

typedef struct rt_ring {              /* 40 B */
    double   r, t;
    double   dis_min, dis_max;        /* (r-t)^2, (r+t)^2   ring.rs:29-30 */
    uint32_t mat;
    uint32_t _pad;
} rt_ring;

/* ConstantMedium{boundary, phase_function: Isotropic, neg_inv_density}. 16 B.
 * `mat` must be an RT_MAT_ISOTROPIC material. The boundary may be any hittable
 * that contains no further medium (the reference's are a Sphere and
 * Translate<RotateY<Boxes>>, scene.rs:230-254, 316-329); a medium nested inside a
 * boundary is refused with RT_ERR_UNSUPPORTED. */
typedef struct rt_medium {
    uint32_t boundary;
    uint32_t mat;
    double   neg_inv_density;
} rt_medium;

/* Translate{offset} / RotateY{sin,cos} / Zoom{rate} around `child`. 32 B.
 * p = offset | {sin_theta, cos_theta, 0} | {rate, 0, 0}. */
typedef struct rt_xform {
    uint32_t kind;                    /* RT_KIND_TRANSLATE / ROTATE_Y / ZOOM */
    uint32_t child;
    double   p[3];
} rt_xform;

/* HittableList as an object: children = list_items[first .. first+count). */
typedef struct rt_list {
    uint32_t first;
    uint32_t count;
} rt_list;

#define RT_MAX_XFORM_DEPTH 4

/* ------------------------------------------------------------ shading ---- */
enum rt_material_kind {
    RT_MAT_LAMBERTIAN    = 0,  /* material/mod.rs:27-66   tex = albedo          */
    RT_MAT_METAL         = 1,  /* material/mod.rs:68-97   albedo, param = fuzz  */
    RT_MAT_DIELECTRIC    = 2,  /* material/mod.rs:99-148  param = ir            */
    RT_MAT_DIFFUSE_LIGHT = 3,  /* material/mod.rs:150-181 tex = emit            */
    RT_MAT_ISOTROPIC     = 4   /* material/mod.rs:183-214 tex = albedo          */
};

typedef struct rt_material {          /* 40 B */
    uint32_t kind;
    uint32_t tex;
    double   albedo[3];
    double   param;
} rt_material;

enum rt_texture_kind {
    RT_TEX_SOLID   = 0,        /* texture/mod.rs:14-29   color                  */
    RT_TEX_CHECKER = 1,        /* texture/mod.rs:31-60   a = odd tex, b = even  */
    RT_TEX_NOISE   = 2,        /* texture/mod.rs:62-79   a = perlin id, scale   */
    RT_TEX_IMAGE   = 3         /* texture/mod.rs:81-139  a = image id           */
};

typedef struct rt_texture {           /* 48 B */
    uint32_t kind;
    uint32_t a;
    uint32_t b;
    uint32_t _pad;
    double   color[3];
    double   scale;
} rt_texture;

/* ImageTexture: RGB8, rows stored bottom-up exactly as texture/mod.rs:94-99
 * builds `pixel_color`; texel (i,j) at image_data[offset + 3*(j*width+i)]. */
typedef struct rt_image {
    uint32_t width, height;
    uint64_t offset;
} rt_image;

/* Perlin tables, texture/perlin.rs:8-13. */
typedef struct rt_perlin {
    double  randvec[256][3];
    int32_t perm_x[256];
    int32_t perm_y[256];
    int32_t perm_z[256];
} rt_perlin;

/* ---------------------------------------------------------- the scene ---- */
typedef struct rt_scene_desc {
    uint32_t abi_version;             /* RT2022_ABI_VERSION */
    uint32_t root;                    /* world (main.rs:90), normally a NODE ref */

    uint32_t n_nodes;          const rt_bvh_node      *nodes;
    uint32_t n_spheres;        const rt_sphere        *spheres;
    uint32_t n_moving_spheres; const rt_moving_sphere *moving_spheres;
    uint32_t n_rects;          const rt_rect          *rects;
    uint32_t n_boxes;          const rt_box           *boxes;
    uint32_t n_triangles;      const rt_triangle      *triangles;
    uint32_t n_rings;          const rt_ring          *rings;
    uint32_t n_media;          const rt_medium        *media;
    uint32_t n_xforms;         const rt_xform         *xforms;
    uint32_t n_lists;          const rt_list          *lists;
    uint32_t n_list_items;     const uint32_t         *list_items;

    /* `lights: HittableList` (main.rs:89,120). n_lights == 0 selects the
     * documented cosine-only mode (the reference would panic, hittable/mod.rs:130). */
    uint32_t n_lights;         const uint32_t         *lights;

    uint32_t n_materials;      const rt_material      *materials;
    uint32_t n_textures;       const rt_texture       *textures;
    uint32_t n_images;         const rt_image         *images;
    uint64_t image_data_bytes; const uint8_t          *image_data;
    uint32_t n_perlins;        const rt_perlin        *perlins;
} rt_scene_desc;

/* Camera, the ten fields of basic/camera.rs:9-20 (built on the host by
 * Camera::new, camera.rs:24-62; consumed by get_ray, camera.rs:64-73). */
typedef struct rt_camera {
    double origin[3];
    double lower_left_corner[3];
    double horizontal[3];
    double vertical[3];
    double u[3], v[3], w[3];
    double lens_radius;
    double time0, time1;
} rt_camera;

/* Per-call constants of main.rs:33-51 + the row slice of main.rs:111-116. */
typedef struct rt_params {
    uint32_t width, height;           /* IMAGE_WIDTH / IMAGE_HEIGHT            */
    uint32_t spp;                     /* SAMPLES_PER_PIXEL                     */
    uint32_t max_depth;               /* MAX_DEPTH                             */
    double   background[3];
    double   t_min;                   /* 0.001 in main.rs:243                  */
    uint64_t seed;                    /* build-defined: the reference is unseeded */
    /* Rows to render, in output order (the reference's shuffled line ids).
     * A row id g addresses frame g / height, image row y = g % height
     * (y up, like main.rs:142); n_frames frames share scene and camera and
     * differ only in their RNG key. */
    uint32_t n_frames;                /* >= 1                                  */
    uint32_t n_rows;
    const uint32_t *row_ids;          /* host pointer (rt_render) or device pointer (rt_render_device) */
    /* 0: each pixel's samples are summed 0..spp in order (main.rs:144-151).
     * k>0: samples are summed in consecutive chunks of k, and the chunk sums
     * are then added in chunk order — same value to ~1 ulp, finer work items.
     * k=1 is the reference's order again, bit for bit (0 + L0 + L1 + ...), with
     * the finest work items: what a throughput-minded caller should pass. */
    uint32_t spp_chunk;
    uint32_t flags;                   /* RT_FLAG_* */
    /* Per-worker progress (the indicatif bars of main.rs:102-127,154-155: one per render thread, advanced as its rows
     * finish). NULL = none. Called on the thread that called rt_render* (rt_render_multi: on the device's own host
     * thread, concurrently with the other devices' — `worker` is the device's place in the set, 0 otherwise), between
     * passes — every few milliseconds of device time — with the camera paths started so far and their total
     * (n_rows * width * spp), and once more with done == total when the call's last pass has completed. It must
     * not call back into the library on the same scene; it never affects results. */
    void (*progress_cb)(void *user, uint32_t worker, uint64_t paths_done, uint64_t paths_total);
    void *progress_user;
} rt_params;

#define RT_FLAG_COUNTERS 0x1u         /* fill the counter fields of rt_stats */
#define RT_FLAG_KERNEL_TIMES 0x2u     /* fill rt_stats.trace_ms / shade_ms (HIP events around every pass of the default engine) */
#define RT_FLAG_ASYNC 0x4u            /* rt_render_device only: return as soon as the call is accepted; a host thread of the library
                                         drives the passes, rt_render_wait(scene, stream) joins it (see rt_render_device) */

typedef struct rt_stats {
    uint64_t paths;                               /* camera rays                         */
    uint64_t rays;                                /* world.hit calls from ray_color (main.rs:243) */
    uint64_t node_visits;                         /* AABB::hit calls                     */
    uint64_t prim_tests[RT_KIND_COUNT];           /* Hittable::hit calls by kind (leaf + boundary) */
    uint64_t light_pdf_tests;                     /* pdf_value re-intersections          */
    uint64_t rng_draws;                           /* 64-bit words drawn on the path      */
    double   ms;                                  /* device (or CPU) time of the call    */
    /* How the call was carried out (always filled; speed only, never results): */
    uint32_t spp_chunk;                           /* samples per work item actually used (params->spp_chunk, 0 resolved to spp) */
    uint32_t passes;                              /* shade + trace pass pairs of the wavefront engine (0: megakernel, CPU) */
    uint64_t pool_slots;                          /* path slots of the wavefront pool the call ran with */
    double   trace_ms, shade_ms;                  /* RT_FLAG_KERNEL_TIMES: device time summed over the call's traversal (wf_trace) and
                                                     shading (wf_shade) launches; 0 otherwise */
    uint64_t partial_bytes;                       /* HBM the call's per-sample partial sums took (spp_chunk > 0): 24 B x pixels x
                                                     ceil(spp / spp_chunk), or 24 B x pixels x the planes of the ring the library
                                                     switches to when that would exceed 40 % of the device's memory (same sums, bit for bit) */
} rt_stats;

typedef struct rt_scene rt_scene;     /* opaque: device-resident scene */

/* ------------------------------------------------------- entry points ---- */
/* Error codes (negative). */
#define RT_OK               0
#define RT_ERR_INVALID     -1   /* bad argument / malformed scene              */
#define RT_ERR_UNSUPPORTED -2   /* scene shape the device path does not cover  */
#define RT_ERR_DEVICE      -3   /* HIP runtime error (no GPU, OOM, launch)     */
#define RT_ERR_NOMEM       -4

/* Validates and copies the flattened scene into HBM on the current HIP device. */
int rt_scene_create(const rt_scene_desc *desc, rt_scene **out);
int rt_scene_destroy(rt_scene *scene);

/* Renders params->n_rows rows; out_rgb_sum (host) receives n_rows*width*3
 * un-normalised f64 sums in row_ids order — the Vec<Color> of main.rs:137-157.
 * Synchronous. stats may be NULL. */
int rt_render(rt_scene *scene, const rt_camera *cam, const rt_params *params,
              double *out_rgb_sum, rt_stats *stats);

/* Same, with params->row_ids and d_out_rgb_sum resident in HBM and every launch
 * issued on `hip_stream` (a hipStream_t; NULL = default stream), so it orders with
 * the caller's other work on that stream. The default engine drives its passes
 * from the host and polls a completion word, so the call returns when the frame's
 * last pass has been issued and observed (it synchronises `hip_stream`); `stats`,
 * if given, is filled by the next rt_render_wait on the same stream. One host
 * thread per (scene, stream). The device-resident row ids are checked like
 * rt_render's host ones (one small reduction kernel): an id >= height * n_frames
 * is RT_ERR_INVALID, not a silently mis-keyed frame.
 * The scene lives on the HIP device that was current at rt_scene_create; the call
 * makes that device current for its duration and restores the caller's, and
 * `hip_stream`, the row ids and the output must belong to that device.
 * RT_FLAG_ASYNC (a flag bit older callers never set: the ABI version stays 3): the call validates its arguments, copies `cam` and `params` and returns; the passes are
 * driven by a host thread of the library (one per call in flight), so the caller's thread is free — to tonemap or gather
 * the previous frame, or to start a frame on another stream of the same scene, whose passes then fill the chip while
 * this one's last rays drain. The device buffers (row ids, output) and `stats` stay the caller's until
 * rt_render_wait(scene, hip_stream), which joins the thread, returns the call's error if it had one (engine errors
 * surface there, not here) and fills `stats`; the next rt_render_device on the same (scene, stream) and
 * rt_scene_destroy wait likewise. params->progress_cb, if any, is called on the library's thread. Results are the
 * synchronous call's, bit for bit. */
int rt_render_device(rt_scene *scene, const rt_camera *cam, const rt_params *params,
                     double *d_out_rgb_sum, void *hip_stream, rt_stats *stats);
int rt_render_wait(rt_scene *scene, void *hip_stream);

/* ---- one call, several GPUs ------------------------------------------------------------------
 * The reference's main() drives all its workers from one place (main.rs:109-183: spawn, join, concatenate).
 * Two ways to do the same over GPUs:
 *   - one process per GPU (what bench.py and torch.distributed do): each process creates its own rt_scene and
 *     renders its share of the rows (film.py deals them); nothing below is needed;
 *   - ONE process, ONE call: an rt_scene_set holds a copy of the scene on every device whose bit is set in
 *     device_mask (bit d = HIP device d); rt_render_multi deals params->row_ids cyclically over those devices
 *     (entry i goes to the (i mod n)-th of them — with the reference's shuffled row list every device gets the same
 *     mix of cheap and dear rows), renders the shares concurrently, one host thread and one stream per device, and
 *     writes out_rgb_sum in row_ids order exactly as rt_render would. Results do not depend on the mask: the RNG is
 *     keyed per pixel and sample. stats, if given, carries the counters summed over the devices and the longest
 *     device time. */
typedef struct rt_scene_set rt_scene_set;
int rt_scene_set_create(const rt_scene_desc *desc, uint64_t device_mask, rt_scene_set **out);
int rt_scene_set_destroy(rt_scene_set *set);
int rt_render_multi(rt_scene_set *set, const rt_camera *cam, const rt_params *params, double *out_rgb_sum, rt_stats *stats);

/* ---- closest-hit queries ------------------------------------------------------------------------
 * `world.hit(r, t_min, t_max)` (hittable/mod.rs, bvh/mod.rs:86-101) for a batch of rays on the device scene, without
 * rendering: picking, visibility and ambient-occlusion rays, scene debugging, other integrators above this ABI.
 *
 * Closest hit, per ray: the answer is the hit of the scene's root (rt_scene_desc.root: a BvhNode, a HittableList or a
 * single object) over (t_min, t_max), with the reference's traversal order, so it is the CPU oracle's rto_hit(desc,
 * desc.root, ray, t_min, t_max, rng_state) bit for bit:
 *   - hit: t, u, v, p, normal, front_face, mat and rng_draws are the winning candidate's HitRecord, carried out through
 *     its movers and FlipFace refs; prim is the winning leaf's ref as it appears in rt_scene_desc (flip bit included);
 *   - miss: hit == 0, prim == RT_REF_NONE, rng_draws as drawn, every other field 0.
 * That holds for any ray, hostile ones included: direction components of exactly 0 (infinite slab inverses),
 * t_max <= t_min, t_max = +inf, NaN components (NaN comes out where the oracle's does).
 * Every scene rt_scene_create accepts is covered: all primitive kinds, movers up to RT_MAX_XFORM_DEPTH, lists, FlipFace
 * refs, ConstantMedium (its draws come from the ray's rng_state, constantmedium.rs:60) and moving spheres at the ray's time.
 *
 * RT_FLAG_ANY_HIT: traversal stops at the first candidate it accepts, in the reference's order. `hit` then equals the
 * closest-hit query's `hit` on every ray (the two traversals are the same up to the first acceptance); on a hit the
 * record is that candidate's: t lies in [t_closest, t_max), prim and mat are that leaf's. A scene holding a
 * ConstantMedium (n_media > 0) refuses it with RT_ERR_UNSUPPORTED: a medium's verdict depends on the draws and on the
 * closest distance so far, so an early stop has no reference meaning.
 *
 * rt_stats (may be NULL): rays = n_rays; with RT_FLAG_COUNTERS node_visits, prim_tests[] and rng_draws are the sums of
 * the oracle's counters over the same rays (0 otherwise); paths, light_pdf_tests, passes, pool_slots, partial_bytes,
 * trace_ms and shade_ms are 0; ms is the device time of the call.
 *
 * Arguments: n_rays == 0 is RT_OK with no launch. A null scene, or a null ray or hit buffer with n_rays > 0, or a flag
 * bit other than RT_FLAG_COUNTERS / RT_FLAG_ANY_HIT is RT_ERR_INVALID with rt_last_error() set; so is a device buffer of
 * rt_intersect_device that is not 16-byte aligned (records are read and written in 16-byte pieces).
 * The call makes the scene's device current and restores the caller's, like rt_render_device.
 *
 * Independence from renders: a query owns its own device scratch (a work counter and a counter block per (scene,
 * stream)) and never touches a render's pool, tape or pending stats; it may run on any stream while an RT_FLAG_ASYNC
 * render of the same scene is in flight, and both keep their serial results bit for bit. Queries are re-entrant on one
 * scene. rt_scene_destroy waits for queries still in flight before it frees anything. */
typedef struct rt_query_ray {         /* 80 B */
    double   origin[3];
    double   direction[3];
    double   time;                    /* Ray::tm (moving spheres) */
    double   t_min, t_max;            /* per ray; t_max may be +inf */
    uint64_t rng_state;               /* seeds the draws of ConstantMedium::hit, exactly as rto_hit's rng_state */
} rt_query_ray;

typedef struct rt_hit {               /* 96 B */
    double   t, u, v;
    double   p[3], normal[3];
    uint32_t hit;                     /* 1: something was hit in (t_min, t_max) */
    uint32_t front_face;
    uint32_t mat;                     /* the caller's material index */
    uint32_t prim;                    /* ref of the winning leaf as in rt_scene_desc, flip bit included; RT_REF_NONE on a miss */
    uint32_t rng_draws;               /* 64-bit words drawn from rng_state */
    uint32_t _pad;
} rt_hit;

#define RT_REF_NONE     0xFFFFFFFFu
#define RT_FLAG_ANY_HIT 0x8u          /* rt_intersect*: stop at the first accepted candidate (see above) */
#define RT_FLAG_SURFACES 0x10u        /* rt_features* / rt_features_pixels* only: look through every ConstantMedium (see there) */
#define RT_FLAG_SPECULAR 0x40u        /* rt_features* / rt_features_pixels* only: follow the sample's path through glass and mirrors
                                         (see there); 0x20 is not a flag */
#define RT_FEATURE_SPECULAR_BOUNCES 8 /* RT_FLAG_SPECULAR: specular vertices a sample follows at the most */

/* Host buffers; synchronous. stats may be NULL. */
int rt_intersect(rt_scene *scene, const rt_query_ray *rays, uint64_t n_rays, uint32_t flags,
                 rt_hit *out_hits, rt_stats *stats);
/* Device buffers, enqueued on hip_stream (NULL = default stream). With stats == NULL the call returns after the
 * enqueue, with no host synchronisation. With stats it synchronises hip_stream and fills stats. */
int rt_intersect_device(rt_scene *scene, const rt_query_ray *d_rays, uint64_t n_rays, uint32_t flags,
                        rt_hit *d_out_hits, void *hip_stream, rt_stats *stats);

/* ---- scatter: one step of ray_color between two world.hit calls -------------------------------------
 * The shading half of `ray_color` (main.rs:233-278) for a batch of hit records on the device scene: what lies between its
 * `world.hit` and its recursive call. Entry i is shaded from rays[i] (direction, time and rng_state are read), hits[i] (the
 * rt_hit of that ray, or any record the caller makes up) and the scene; the outputs are a record — weight, pdf, radiance,
 * status — and the path's next ray as a ready rt_query_ray. So rt_intersect_device -> rt_scatter_device -> rt_intersect_device
 * -> ... is a wavefront path tracer the caller drives with no kernel of their own (direct and indirect light kept apart,
 * per-bounce AOVs, Russian roulette, other estimators), and unwound in the reference's order it is rt_radiance bit for bit.
 *
 * Stream: the step draws from Rng(rays[i].rng_state advanced by hits[i].rng_draws words); the state after k words is
 * state + k * 0x9E3779B97F4A7C15 mod 2^64.
 * prev: with prev != NULL an entry whose prev[i].status is neither RT_SCATTER_SPECULAR nor RT_SCATTER_DIFFUSE is
 * RT_SCATTER_ENDED: nothing else of the entry is read but the ray's rng_state, and no word is drawn. prev == NULL: every entry
 * is live.
 * Status of a live entry:
 *   - hits[i].hit == 0: MISS, radiance = background. Any non-zero `hit` word is a hit, any non-zero `front_face` word is true.
 *   - mat >= the scene's n_materials: INVALID; the material pool is not read.
 *   - DiffuseLight: EMITTED, radiance = front_face ? the texture's value : 0 (material/mod.rs:174-180).
 *   - Metal, Dielectric, Isotropic: SPECULAR (mod.rs:85-96, 120-147, 207-213; Metal's next ray has time 0, mod.rs:91).
 *   - Lambertian: DIFFUSE. With n_lights == 0 the cosine direction and its pdf; otherwise the mixture's choice
 *     gen_range(0, 1) < 0.5, then HittableList::random over the lights or the cosine direction, and
 *     pdf = 0.5 * lights' pdf_value + 0.5 * cosine pdf (pdf.rs:94-104). weight = attenuation * scattering_pdf.
 * NaN and non-finite inputs come out where the CPU oracle's do; record contents are never validated beyond `mat`.
 * Next ray: SPECULAR, DIFFUSE: origin = the record's p, the scattered direction and time, t_min = p->t_min,
 * t_max = 1.7976931348623157e308 (f64::MAX, main.rs:243: not infinity), rng_state = the stream's state behind this step's
 * words. Every other status: all fields 0 except rng_state = the input state advanced by hits[i].rng_draws words (ENDED: the
 * input's rng_state unchanged).
 * Radiance of a path with live records r_0 .. r_{k-1}: T = the first non-live record's radiance, or (0, 0, 0) when the depth
 * ran out; L = T; for j = k-1 .. 0: L = 0 + (weight_j * L) / pdf_j, component-wise.
 * Aliasing: out_next_rays may be rays itself, and out_recs may be prev itself (an entry is read before it is written). Any
 * other overlap is the caller's error.
 *
 * rt_stats (may be NULL): with RT_FLAG_COUNTERS rng_draws = the sum of the records' rng_draws and light_pdf_tests = what the
 * oracle counts (one per Sphere or rect entry of the light list that is not a FlipFace, per DIFFUSE record of a scene with
 * lights); every other counter is 0; ms is the device time of the call. rt_scatter_device with stats == NULL is a pure
 * enqueue, like rt_intersect_device; with stats it synchronises hip_stream.
 *
 * Arguments: n == 0 is RT_OK with no launch. RT_ERR_INVALID with rt_last_error() set (prefixed by the function's name),
 * before any device call and with every output untouched: a null scene or params; a null ray, hit, record or next-ray buffer
 * with n > 0 (prev may be null); a flag bit other than RT_FLAG_COUNTERS; a device buffer of
 * rt_scatter_device that is not 16-byte aligned (prev included when given).
 * Like the queries: the call makes the scene's device current and restores the caller's, owns its scratch per (scene,
 * stream), may run beside an RT_FLAG_ASYNC render of the same scene, is awaited by rt_scene_destroy and does not depend on
 * the engine selected. New symbols only: the ABI version stays 3. */
typedef struct rt_scatter_params {    /* 40 B */
    double   background[3];           /* what a miss returns (main.rs:275-276) */
    double   t_min;                   /* copied into every next ray (0.001 in main.rs:243) */
    uint32_t flags;                   /* RT_FLAG_COUNTERS only */
    uint32_t _pad;
} rt_scatter_params;

enum rt_scatter_status { RT_SCATTER_MISS = 0, RT_SCATTER_EMITTED = 1, RT_SCATTER_SPECULAR = 2, RT_SCATTER_DIFFUSE = 3,
                         RT_SCATTER_INVALID = 4, RT_SCATTER_ENDED = 5 };

typedef struct rt_scatter_rec {       /* 64 B: four 16-byte pieces */
    double   weight[3];               /* SPECULAR: attenuation; DIFFUSE: attenuation * scattering_pdf; else 0 */
    double   pdf;                     /* SPECULAR: 1.0; DIFFUSE: the mixture pdf's value (may be 0 or NaN, as the reference's); else 0 */
    double   radiance[3];             /* MISS: background; EMITTED: Material::emitted; else 0 */
    uint32_t status;                  /* rt_scatter_status */
    uint32_t rng_draws;               /* words this step drew (the hit's own words are rt_hit.rng_draws) */
} rt_scatter_rec;

/* Host buffers; synchronous. stats and prev may be NULL. */
int rt_scatter(rt_scene *scene, const rt_query_ray *rays, const rt_hit *hits, const rt_scatter_rec *prev, uint64_t n,
               const rt_scatter_params *p, rt_scatter_rec *out_recs, rt_query_ray *out_next_rays, rt_stats *stats);
/* Device buffers, enqueued on hip_stream (NULL = default stream). */
int rt_scatter_device(rt_scene *scene, const rt_query_ray *d_rays, const rt_hit *d_hits, const rt_scatter_rec *d_prev, uint64_t n,
                      const rt_scatter_params *p, rt_scatter_rec *d_out_recs, rt_query_ray *d_out_next_rays, void *hip_stream, rt_stats *stats);

/* ---- path-traced radiance of caller rays ----------------------------------------------------------
 * `ray_color(r, background, world, lights, depth)` (main.rs:233-278) for rays the caller chooses instead of the camera's:
 * other cameras (panoramas, orthographic, stereo), light probes and irradiance baking, progressive or adaptive sampling,
 * integrators built on rt_intersect. The work runs in the render's own wavefront engine: the only difference is where a
 * new path's first ray comes from.
 *
 * Result, per ray i: out_rgb_sum[3i .. 3i+3) = 0 + L_0 + L_1 + ... + L_{spp-1}, added in sample order, where
 * L_s = ray_color(ray_i, background, t_min, max_depth) drawing from Rng(path_key(ray_i.rng_state, 0, 0, s)) — the render's
 * keying (rt_math.h) with the ray's rng_state in place of the seed. Not divided by spp, like a render's sums:
 * rt_tonemap_device / rt_write_color apply as they are. So it is the CPU oracle's rto_ray_color(desc, ray, background,
 * t_min, max_depth, rto_path_key(rng_state, 0, 0, s)) summed over s, bit for bit, on every scene rt_scene_create accepts
 * (lights or the n_lights == 0 cosine mode, media, movers, moving spheres at the ray's time, every texture kind), and
 * for rays no camera makes: zero direction components, a zero direction, +-inf or NaN components, origins inside a medium's
 * boundary or a dielectric (NaN comes out where the oracle's does). Ray contents are never validated. A ray's result does
 * not depend on the order of the rays or on the size of the batch.
 *
 * rt_stats (may be NULL): paths = n_rays * spp; with RT_FLAG_COUNTERS rays, node_visits, prim_tests[], light_pdf_tests and
 * rng_draws are the sums of the oracle's counters over the same samples (no camera draws are involved; 0 otherwise); ms,
 * passes, pool_slots, partial_bytes and (RT_FLAG_KERNEL_TIMES) trace_ms / shade_ms mean what they mean for a render;
 * spp_chunk is 1 (one sample per work item, always).
 *
 * Arguments: n_rays == 0, spp == 0 and max_depth == 0 are RT_OK (the last two write zeros, with no kernel of the engine).
 * RT_ERR_INVALID with rt_last_error() set, before anything reaches the device: a null scene or params; a null ray or
 * output buffer with n_rays > 0; a flag bit other than RT_FLAG_COUNTERS / RT_FLAG_KERNEL_TIMES (RT_FLAG_ASYNC and
 * RT_FLAG_ANY_HIT included); a device buffer of rt_radiance_device that is not 16-byte aligned; n_rays > RT_RADIANCE_MAX_RAYS
 * (a path slot keeps its ray's index in a 32-bit field) or n_rays * spp > RT_RADIANCE_MAX_ITEMS = 2^58 (the partial sums take
 * 24 B per work item and their byte counts must fit 64 bits with a margin, as must the engine's work item numbering with
 * the work counter's overshoot). Within the limits, a call whose planes do not fit the device takes the ring of planes or
 * fails with RT_ERR_DEVICE; it never writes outside what it allocated. A scene switched to the A/B megakernel engine
 * (rt_debug_set_engine) is RT_ERR_UNSUPPORTED. There is no rt_scene_set form, no progress callback and no RT_FLAG_ASYNC.
 *
 * Workspace: the call runs in the render's per-(scene, stream) workspace (path pool, partial-sum planes — the ring of
 * planes included, under the same threshold — and tape) and behaves on its stream like one more rt_render_device: an
 * RT_FLAG_ASYNC render in flight on the same (scene, stream) is joined and finished first (its stats filled, as
 * rt_render_wait would), and renders after it keep their results bit for bit. rt_radiance_device synchronises hip_stream
 * before it returns and fills stats itself. rt_radiance stages the rays and sums through device buffers the workspace
 * keeps, on the default stream. The call makes the scene's device current and restores the caller's. */
typedef struct rt_radiance_ray {      /* 64 B: the engine's own ray record {ox, oy, oz, dx, dy, dz, tm, rng} */
    double   origin[3];
    double   direction[3];
    double   time;                    /* Ray::tm (moving spheres) */
    uint64_t rng_state;               /* keys the ray's sample streams: path_key(rng_state, 0, 0, sample) */
} rt_radiance_ray;

typedef struct rt_radiance_params {   /* 48 B */
    double   background[3];
    double   t_min;                   /* 0.001 in main.rs:243, for every bounce */
    uint32_t max_depth;               /* ray_color's depth */
    uint32_t spp;                     /* samples per ray; 0 = zeros */
    uint32_t flags;                   /* rt_radiance*: RT_FLAG_COUNTERS | RT_FLAG_KERNEL_TIMES only (rt_features_rays*: see there) */
    uint32_t _pad;
} rt_radiance_params;

#define RT_RADIANCE_MAX_RAYS  0xFFFFFFFFull          /* n_rays limit */
#define RT_RADIANCE_MAX_ITEMS (1ull << 58)           /* n_rays * spp limit: 24 B of partial sums per item, in 64-bit byte counts */

/* Host buffers (n_rays records in, 3 * n_rays sums out); synchronous. stats may be NULL. */
int rt_radiance(rt_scene *scene, const rt_radiance_ray *rays, uint64_t n_rays, const rt_radiance_params *p,
                double *out_rgb_sum, rt_stats *stats);
/* Device buffers, 16-byte aligned, enqueued on hip_stream (NULL = default stream); returns once the call is complete. */
int rt_radiance_device(rt_scene *scene, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *p,
                       double *d_out_rgb_sum, void *hip_stream, rt_stats *stats);

/* ---- first-hit feature buffers of a render's view ---------------------------------------------------
 * The guide buffers of a frame — per-pixel albedo, shading normal, depth and coverage — for exactly the camera rays
 * rt_render shoots with the same rt_camera and rt_params: what a denoiser, an adaptive sampler, an edge-aware upscaler or
 * a compositor reads beside the radiance sums. Only the first segment of every path is traced; nothing bounces.
 *
 * For each entry g of params->row_ids (frame g / height, image row py = g % height, as for a render), each px in
 * [0, width) and each sample s in [0, spp): rng = Rng(path_key(seed, frame, py * width + px, s)); rand_u, rand_v =
 * rng.gen_f64() twice; r = get_ray(cam, (px + rand_u) / (width - 1), (py + rand_v) / (height - 1), rng) — the render's
 * own code (main.rs:144-149) — and rec = world.hit(r, t_min, f64::MAX) on the scene's root with the SAME rng continuing,
 * so a ConstantMedium draws the words the render's first ray draws. The sample's features:
 *
 *   field      hit                                                                             miss
 *   albedo[3]  by the kind of rec.mat — LAMBERTIAN / ISOTROPIC: texture_value(tex, rec.u,      params->background
 *              rec.v, rec.p); METAL: its albedo; DIELECTRIC: (1, 1, 1); DIFFUSE_LIGHT:
 *              texture_value(tex, u, v, p) on the front face, (0, 0, 0) on the back — scatter's
 *              attenuation where the material scatters, emitted where it does not (material/mod.rs)
 *   normal[3]  rec.normal: face-oriented, carried out through movers and FlipFace refs;          0
 *              a medium's (1, 0, 0) as it is
 *   depth      rec.t                                                                            0
 *   hits       1                                                                                0
 *
 * RT_FLAG_SURFACES (a flag bit older callers never set: the ABI version stays 3; all four feature calls take it): the
 * records of the first SURFACE behind every participating medium. The sample is the one above with one change:
 * ConstantMedium::hit returns None at once — it does not query its boundary and draws no word. Everything else stays:
 * world.hit's order, the winner's record, the albedo rule, the sums and their order. Fog in front of nothing gives the miss
 * record (background, zeros, hits 0); an object that is both in the world and some medium's boundary is still hit through
 * its own reference; a scene whose root is a medium gives miss records only. On a scene without a medium the flag changes
 * nothing, counters included. With RT_FLAG_COUNTERS rt_stats counts what this definition does: prim_tests[RT_KIND_MEDIUM]
 * is 0, no boundary is tested, and rng_draws is the camera's words only (2 + what rto_get_ray returns). The CPU oracle
 * gives the same records on a copy of the scene whose media all have neg_inv_density = -inf (hit_distance is then +inf
 * and a medium never answers) as long as every distance_inside_boundary is finite. What it is for: rt_temporal* and the
 * denoisers read these records, and a medium's drawn depth and (1, 0, 0) normal are noise to them. Participating media are
 * then reprojected and filtered by the surface behind them — wrong for dense smoke with parallax of its own.
 *
 * RT_FLAG_SPECULAR (a flag bit older callers never set: the ABI version stays 3; all four feature calls take it, alone, with
 * RT_FLAG_COUNTERS, with RT_FLAG_SURFACES or with both; every other call refuses it): the records of the first NON-SPECULAR
 * vertex of the sample's own path, behind glass and mirrors. The sample is aimed as above (rng, two jitter draws, r_0 =
 * get_ray(...)). Then, for k = 0, 1, ...: rec_k = world.hit(r_k, t_min, f64::MAX) on the root with the same rng continuing.
 *   - A miss at k = 0 is the miss record above (background, zeros, hits 0). A miss at k > 0 ends the chain with the
 *     terminal colour c = background and the normal rec_{k-1}.normal.
 *   - A hit is FOLLOWED iff k < RT_FEATURE_SPECULAR_BOUNCES and its material is DIELECTRIC, or METAL with param == 0.0.
 *     Then a_k is Material::scatter's attenuation — (1, 1, 1) for a Dielectric, the albedo for a Metal — and r_{k+1} is
 *     scatter's specular ray with rng continuing (material/mod.rs:85-147): a Dielectric draws its one gen_range word and
 *     keeps r_k.tm; a Metal draws random_in_unit_sphere although it is multiplied by a fuzz of 0, and its ray has tm = 0.0.
 *   - Any other hit is the terminal vertex j: Lambertian, Isotropic, DiffuseLight, Metal with fuzz > 0, and whatever is
 *     hit at k == RT_FEATURE_SPECULAR_BOUNCES. Its colour c is the albedo rule above on rec_j, the normal is rec_j.normal.
 * The record: albedo = a_0 * (a_1 * ( ... * (a_{j-1} * c))), component-wise and innermost first — ray_color's own order,
 * attenuation * ray_color(...), which matters for the bits once two metals are in a chain (a Dielectric's factor is exactly
 * 1); normal as said; depth = rec_0.t and hits = 1, the primary-visibility values as without the flag, so coverage and the
 * silhouette of the specular object stay what they were. Sums per pixel are 0 + f_0 + f_1 + ... in sample order as above; NaN
 * where IEEE gives NaN. On a scene with no Dielectric and no fuzz-0 Metal the flag changes nothing, counters included. With
 * RT_FLAG_SURFACES as well a ConstantMedium answers None on EVERY segment (the oracle's reference is then the same
 * composition on the looked-through copy). The guides describe the path prefix the pixel's radiance came from, each sample's
 * reflect / refract choice at a Dielectric included: on a scene that holds only specular surfaces, lights and background the
 * flagged albedo of a sample whose chain ends within the cap IS ray_color of that sample, bit for bit. rt_stats under the
 * flag: paths = n * spp; rays is the number of world.hit calls, counted on the device and filled only with
 * RT_FLAG_COUNTERS (0 without); with counters node_visits and prim_tests[] sum over all segments and rng_draws is the
 * camera's words plus every hit's plus every followed vertex's scatter words. What it is for: the denoisers (rt_denoise*,
 * rt_denoise_dual*, render_adaptive's guides) — demodulation then divides by the albedo the radiance actually carries, and
 * the edge-stopping terms see edges inside a reflection or a refraction. What it is NOT for: rt_temporal*. A mirror image
 * does not reproject by the mirror's depth, and the normals now change with each sample's reflect / refract choice: the
 * accumulation stays better served by first-hit or RT_FLAG_SURFACES records.
 *
 * Each field of a pixel's record is 0 + f_0 + f_1 + ... + f_{spp-1}, added in sample order and NOT divided by spp, like a
 * render's sums (rt_tonemap_device / rt_write_color do not apply): hits / spp is coverage, depth / hits the mean depth over
 * the hits. Records come in row_ids order, n_rows * width of them. Every sum is the CPU oracle's composition rto_path_key
 * -> rto_get_ray -> rto_hit -> rto_texture_value bit for bit (NaN where the oracle gives NaN — width == 1 or height == 1
 * divide by zero as the render does) on every scene rt_scene_create accepts.
 *
 * rt_params: the render's struct, so one struct describes both calls of a frame. Used: width, height, spp, background,
 * t_min, seed, n_frames, n_rows, row_ids, flags. IGNORED: max_depth (features are defined for a depth-0 render too),
 * spp_chunk, progress_cb / progress_user. row_ids is host memory for rt_features, device memory for rt_features_device.
 *
 * Arguments: spp == 0 or n_rows == 0 is RT_OK (zeros or nothing written, no kernel). RT_ERR_INVALID with rt_last_error()
 * set, before any kernel: a null scene, cam or params; null rows or output with work to do; a flag bit other than
 * RT_FLAG_COUNTERS / RT_FLAG_SURFACES / RT_FLAG_SPECULAR; a device output that is not 16-byte aligned or device rows that are not 4-byte aligned; width, height
 * or n_frames equal to 0 (or cam->time0 >= cam->time1, as for a render); a row id >= height * n_frames (device rows are
 * checked by the small reduction kernel rt_render_device uses, behind one synchronisation of hip_stream before the
 * feature kernel is enqueued).
 *
 * rt_stats (may be NULL): paths = rays = n_rows * width * spp; with RT_FLAG_COUNTERS node_visits and prim_tests[] are the
 * sums of rto_hit's counters and rng_draws the camera's words (2 + what rto_get_ray returns) plus the hit's; ms is the
 * device time of the call; everything else is 0. (RT_FLAG_SPECULAR: see there — rays counts every segment.)
 *
 * Independence: a call owns its scratch per (scene, stream) — a work counter, a counter block, two events — and uses
 * neither engine, so it works whichever is selected, never touches a render's pool, tape or pending stats, and may run on
 * another stream beside an RT_FLAG_ASYNC render or a query of the same scene; all of them keep their serial results bit
 * for bit. rt_scene_destroy waits for it. The call makes the scene's device current and restores the caller's. There is
 * no rt_scene_set form. One lane works one pixel through all its samples: a job of a few pixels at a huge spp balances
 * poorly — the intended use is a whole frame at modest spp. */
typedef struct rt_feature {           /* 64 B: four 16-byte pieces */
    double   albedo[3];
    double   normal[3];
    double   depth;
    double   hits;
} rt_feature;

/* Host buffers (n_rows * width records out); synchronous. stats may be NULL. */
int rt_features(rt_scene *scene, const rt_camera *cam, const rt_params *params,
                rt_feature *out_features, rt_stats *stats);
/* Device buffers, enqueued on hip_stream (NULL = default stream). With stats == NULL the call returns once the kernel is
 * enqueued; with stats it synchronises hip_stream and fills stats, like rt_intersect_device. */
int rt_features_device(rt_scene *scene, const rt_camera *cam, const rt_params *params,
                       rt_feature *d_out_features, void *hip_stream, rt_stats *stats);

/* The pixel-list form: the feature records of a LIST of (frame, pixel) ids instead of whole rows — rt_render_pixels' ids,
 *   id = frame * (width * height) + py * width + px.
 * Record e of the output is exactly the record rt_features writes for column px of row id frame * height + py with the same
 * rt_camera and rt_params (n_frames > frame): the same composition summed over spp samples in sample order, bit for bit,
 * NaN where the oracle has NaN. Repeated ids are allowed and give equal records; the order and the length of the list
 * never change an entry's record. The kernel is rt_features' own with another source of work items: one lane works one
 * ENTRY through all its samples, and decodes the id by two 32-bit divisions where width * height * n_frames fits 32 bits,
 * by 64-bit ones otherwise.
 *
 * rt_params: used — width, height, spp, background, t_min, seed, n_frames, flags (RT_FLAG_SURFACES and RT_FLAG_SPECULAR as for rt_features); IGNORED — n_rows, row_ids, max_depth,
 * spp_chunk, progress_cb / progress_user.
 *
 * Arguments: n_entries == 0 is RT_OK; spp == 0 is RT_OK and writes zeros with no feature kernel. RT_ERR_INVALID with
 * rt_last_error() set, before any feature kernel: a null scene, cam or params; null ids or output with n_entries > 0;
 * width, height or n_frames equal to 0 (or height * n_frames above 2^32 - 1: the matching row id must exist);
 * cam->time0 >= cam->time1; a flag bit other than RT_FLAG_COUNTERS / RT_FLAG_SURFACES / RT_FLAG_SPECULAR; device ids that are not 8-byte aligned or a device
 * output that is not 16-byte aligned; n_entries > 2^40; an id >= width * height * n_frames — host ids are checked on the
 * host, device ids by the counting kernel rt_render_pixels_device uses, behind one synchronisation of hip_stream BEFORE
 * the feature kernel is enqueued: a refused call leaves the output untouched.
 *
 * rt_stats (may be NULL): paths = rays = n_entries * spp; with RT_FLAG_COUNTERS node_visits, prim_tests[] and rng_draws
 * are the oracle's sums as for rt_features; ms is the device time; everything else is 0. Scratch and independence are
 * rt_features*' own: the same per-(scene, stream) scratch, neither engine, no pool. No RT_FLAG_ASYNC, no rt_scene_set
 * form. With stats == NULL the device form returns after the enqueue, apart from the id check's synchronisation. */
int rt_features_pixels(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *pixel_ids, uint64_t n_entries,
                       rt_feature *out_features, rt_stats *stats);
int rt_features_pixels_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *d_pixel_ids, uint64_t n_entries,
                              rt_feature *d_out_features, void *hip_stream, rt_stats *stats);

/* The ray form: the feature records of rays the CALLER chooses instead of the camera's — rt_radiance's ray records and
 * rt_radiance's params, so that one ray buffer and one rt_radiance_params serve rt_radiance_device and this call, as
 * rt_params serves a render and rt_features. What the denoisers (rt_denoise*, rt_denoise_dual*) and rt_temporal* need beside
 * the sums of other cameras (panoramas, orthographic, stereo), light probes, baking, integrators built on rt_intersect: they
 * take no scene, only rt_feature records. New symbols only: the ABI version stays 3.
 *
 * For ray i and each sample s in [0, p->spp): rng = Rng(path_key(rays[i].rng_state, 0, 0, s)) — rt_radiance's keying; no
 * camera word is drawn. r_0 = Ray(origin, direction, time), and rec = world.hit(r_0, p->t_min, f64::MAX) on the scene's root
 * with that rng, so a ConstantMedium draws exactly the words the first segment of rt_radiance's sample s draws. The sample's
 * features are rt_features' table above unchanged: the albedo rule by material kind, rec.normal, rec.t and 1 for a hit;
 * p->background, zeros and 0 for a miss. RT_FLAG_SURFACES and RT_FLAG_SPECULAR mean what they mean for the other four
 * feature calls with r_0 as here in place of the aimed ray (a followed Metal's ray has tm = 0.0, a Dielectric keeps r_k.tm).
 * Record i is 0 + f_0 + ... + f_{spp-1} per field, added in sample order and not divided; the kernel makes these spp
 * additions (on a scene without media and without RT_FLAG_SPECULAR all samples of a ray are equal, but spp * f is not the
 * same bits as the sum). A ray's record does not depend on the batch or on its order. Ray contents are never validated: zero
 * directions, zero, +-inf or NaN components, origins inside a medium's boundary or a dielectric, huge origins — NaN comes out
 * where the oracle gives NaN. Every sum is the oracle's composition rto_path_key -> rto_hit -> rto_texture_value bit for bit.
 * Two consequences make the call usable with the rest:
 *   (a) with RT_FLAG_SPECULAR, albedo of ray i equals rt_radiance's out_rgb_sum of ray i bit for bit if the scene holds only
 *       specular surfaces, lights and background, max_depth is at least 10 on the radiance side and no sample's chain reaches
 *       the cap (RT_FEATURE_SPECULAR_BOUNCES vertices followed);
 *   (b) with no flag, spp = 1 and a scene without media, the record of the ray that rt_features aims for a pixel's sample 0
 *       (whatever its rng_state: nothing draws) equals that pixel's rt_features record at spp = 1.
 *
 * rt_radiance_params: used — background, t_min, spp, flags; IGNORED — max_depth. Flags: RT_FLAG_COUNTERS, RT_FLAG_SURFACES and
 * RT_FLAG_SPECULAR in any combination; every other bit is RT_ERR_INVALID (RT_FLAG_KERNEL_TIMES, RT_FLAG_ASYNC and
 * RT_FLAG_ANY_HIT included). rt_radiance* keeps refusing the two feature flags.
 *
 * Arguments: n_rays == 0 is RT_OK with nothing written and no device call; spp == 0 is RT_OK and writes zeros with no feature
 * kernel. RT_ERR_INVALID with rt_last_error() set (prefixed by the function's name), before any device call: a null scene or
 * params; a null ray or output buffer with n_rays > 0; n_rays > 2^40 (the entry index lives in the lane's two 32-bit words,
 * like a pixel-list entry); a device ray buffer or device output that is not 16-byte aligned. There is no id list, so there
 * is no checking kernel: with stats == NULL the device form is a pure enqueue with no host synchronisation; with stats it
 * synchronises hip_stream like rt_features_device.
 *
 * rt_stats (may be NULL): paths = rays = n_rays * spp (RT_FLAG_SPECULAR: rays counts segments and is filled only with
 * counters, as documented there); with RT_FLAG_COUNTERS node_visits, prim_tests[] and rng_draws are the oracle's sums — there
 * are no camera words: rng_draws is the hits' words plus the followed vertices' scatter words; ms is the device time;
 * everything else is 0. Scratch and independence are the feature calls' own: the same per-(scene, stream) scratch, neither
 * engine, no pool; the call may run beside an RT_FLAG_ASYNC render or a query of the same scene, and rt_scene_destroy waits
 * for it. No rt_scene_set form. One lane works one RAY through all its samples. */
int rt_features_rays(rt_scene *scene, const rt_radiance_ray *rays, uint64_t n_rays, const rt_radiance_params *p,
                     rt_feature *out_features, rt_stats *stats);
int rt_features_rays_device(rt_scene *scene, const rt_radiance_ray *d_rays, uint64_t n_rays, const rt_radiance_params *p,
                            rt_feature *d_out_features, void *hip_stream, rt_stats *stats);

/* ---- edge-avoiding denoiser over the feature buffers ----------------------------------------------------
 * The consumer of rt_features*: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) on albedo-demodulated
 * radiance, guided by the frame's first-hit albedo, normal and depth — the step between a render and its tone map,
 *   rt_render_device -> rt_features_device -> rt_denoise_device -> rt_tonemap_device,
 * all in HBM on one stream. It needs no variance estimate and no rt_scene, and never touches a render's sums or RNG.
 * The edge-stopping function is rational, 1 / (1 + d / sigma^2), not exp: every operation below is an IEEE + - * / of
 * doubles in the stated order, with no contraction, so the result is defined bit for bit.
 *
 * The image has width x height pixels. Per pixel p the inputs are S[3], a render's sums, and F, its rt_feature record,
 * both sums of `spp` samples. With sp = (double)spp:
 *   c_j = (S_j is NaN ? 0 : S_j) / sp          (write_color's rule for NaN)
 *   a_j = F.albedo_j / sp,  n_j = F.normal_j / sp,  z = F.depth / sp      (F.hits is unused: misses count as depth 0)
 *   m_j = a_j > albedo_floor ? a_j : albedo_floor   (a NaN albedo gives the floor); RT_DENOISE_NO_DEMODULATE: m_j = 1.0
 *   e0_j = c_j / m_j
 * On the host, in doubles: inv_n = 1.0 / (sigma_normal * sigma_normal), inv_z and inv_a likewise from sigma_depth and
 * sigma_albedo; a sigma of +inf gives 0 and switches its term off.
 * Iteration k = 0 .. n_iter-1: step s = 2^k, sigma_k = sigma_color * 2^-k (an exact scaling), inv_c = 1.0 / (sigma_k *
 * sigma_k), h = {1/16, 1/4, 3/8, 1/4, 1/16}:
 *   sw = 0.0; sv = (0, 0, 0)
 *   for j = -2 .. 2 (rows), for i = -2 .. 2 (columns), in that order:
 *       q = (x + i*s, y + j*s); a tap outside the image is skipped (it adds nothing)
 *       dc = (d0*d0 + d1*d1) + d2*d2      with d = ek(p) - ek(q);   dn, da the same on n and a;   dz = z(p) - z(q)
 *       den = (((1.0 + dc*inv_c) * (1.0 + dn*inv_n)) * (1.0 + (dz*dz)*inv_z)) * (1.0 + da*inv_a)
 *       w = (h[j+2] * h[i+2]) / den
 *       sw = sw + w;  sv_c = sv_c + w * ek_c(q)
 *   e(k+1)_c(p) = sv_c / sw               (the centre tap makes sw >= 9/64)
 * Output: out_c = (e(n_iter)_c * m_c) * sp — sums like a render's, so rt_tonemap_device and rt_write_color apply as they
 * are. NaN or inf in a guide field propagates where IEEE arithmetic carries it; buffer contents are never validated.
 * (x, y) are the column and the image row; tap offsets i * 2^k are computed in 64 bits.
 *
 * Row order: row_ids == NULL means buffer row i is image row i. Otherwise row_ids holds `height` entries and buffer row i
 * is image row row_ids[i], as rt_render / rt_features wrote it for ONE frame; the output comes in the same order. A list
 * that is not a permutation of [0, height) is RT_ERR_INVALID with the output untouched: rt_denoise checks it on the host;
 * rt_denoise_device builds the inverse map in the workspace with one small kernel that counts bad and repeated ids, and
 * reads the count behind one synchronisation of hip_stream before anything else is enqueued. With NULL rows
 * rt_denoise_device is a pure enqueue with no host synchronisation.
 *
 * Workspace: rt_denoise_device allocates nothing. The caller gives it rt_denoise_workspace_bytes(p) bytes of device memory
 * (the packed guides, two colour planes, the inverse row map), whose contents before the call mean nothing and which may
 * be reused by the next call on the stream. d_out_rgb_sum may alias d_rgb_sum: every sum is read before any output is
 * written. d_rgb_sum, d_features, d_out_rgb_sum and the workspace must be 16-byte aligned, device rows 4-byte aligned.
 * rt_denoise stages host buffers through device memory of its own on the current device's default stream (out_rgb_sum may
 * be rgb_sum) and reports the device time of the filter in *ms.
 *
 * RT_ERR_INVALID with rt_last_error() set, before any device call: a null params, buffer or workspace; width, height or
 * spp equal to 0; n_iter > RT_DENOISE_MAX_ITER; a sigma or floor that is <= 0 or NaN, or an infinite floor; a flag bit
 * other than RT_DENOISE_NO_DEMODULATE; a misaligned device pointer; width * height > RT_DENOISE_MAX_PIXELS. */
typedef struct rt_denoise_params {    /* 64 B */
    uint32_t width, height;
    uint32_t spp;                     /* divisor of the sums, >= 1 */
    uint32_t n_iter;                  /* 0 .. RT_DENOISE_MAX_ITER */
    double   sigma_color, sigma_normal, sigma_depth, sigma_albedo;   /* > 0; +inf = term off */
    double   albedo_floor;            /* > 0, finite */
    uint32_t flags;                   /* RT_DENOISE_NO_DEMODULATE */
    uint32_t _pad;
} rt_denoise_params;

#define RT_DENOISE_MAX_ITER      16
#define RT_DENOISE_NO_DEMODULATE 0x1u                /* filter the radiance itself: m = 1 */
#define RT_DENOISE_MAX_PIXELS    (1ull << 36)        /* width * height limit (a 1-D grid of 256-pixel workgroups) */

/* Bytes of device workspace rt_denoise_device needs for p's image; 0 on invalid params. */
uint64_t rt_denoise_workspace_bytes(const rt_denoise_params *p);
/* Device buffers (width * height * 3 sums in and out, width * height records, NULL or `height` row ids), enqueued on
 * hip_stream (NULL = default stream). */
int rt_denoise_device(const double *d_rgb_sum, const rt_feature *d_features, const uint32_t *d_row_ids,
                      const rt_denoise_params *p, double *d_out_rgb_sum, void *d_workspace, void *hip_stream);
/* Host buffers; synchronous. ms may be NULL. */
int rt_denoise(const double *rgb_sum, const rt_feature *features, const uint32_t *row_ids,
               const rt_denoise_params *p, double *out_rgb_sum, double *ms);

/* ---- variance-guided denoising from two half-sample renders ------------------------------------------------
 * rt_denoise's colour term cannot tell noise from detail. rt_params.n_frames already renders frames that share scene and
 * camera and differ only in their RNG key: two frames of `spp` samples each are two independent estimates A and B of one
 * image, (A + B) / 2 is the frame and ((A - B) / 2)^2 an unbiased estimate of that frame's variance. This filter is
 * rt_denoise's with the colour distance measured in units of that variance, which it propagates through the iterations.
 * A caller produces the halves with ONE render and ONE feature call, both with n_frames = 2 and the row list
 * rows ++ (rows + height): the two halves of each output buffer are A and B. The engine is not touched.
 *
 * p is rt_denoise's block: spp is the samples in EACH half; width, height, n_iter, sigma_normal / depth / albedo,
 * albedo_floor and RT_DENOISE_NO_DEMODULATE mean what they mean there; sigma_color is in units of the estimated standard
 * deviation and is NOT halved per iteration — the propagated variance shrinks instead.
 *
 * Definition: IEEE + - * / on doubles in the stated order, no contraction. Per pixel, with sp = (double)spp, sp2 = sp + sp
 * and nan0(x) = x is NaN ? 0 : x:
 *   cA_j = nan0(A_j) / sp;  cB_j = nan0(B_j) / sp;  c_j = (cA_j + cB_j) * 0.5
 *   a_j = (FA.albedo_j + FB.albedo_j) / sp2;  n_j and z likewise from normal and depth (hits is unused)
 *   m_j = rt_denoise's rule on a_j (floor; NaN albedo -> floor; RT_DENOISE_NO_DEMODULATE -> 1.0)
 *   e0_j = c_j / m_j
 *   h_j  = ((cA_j - cB_j) * 0.5) / m_j
 *   v0   = (h_0*h_0 + h_1*h_1) + h_2*h_2
 * On the host: inv_n, inv_z, inv_a as for rt_denoise; inv_c = 1.0 / (sigma_color * sigma_color); +inf gives 0 (term off).
 * Taps run over j = -2 .. 2 (rows), then i = -2 .. 2, offsets i*step and j*step in 64 bits, taps outside the image
 * skipped, hh = h[j+2] * h[i+2], dn / da / dz as for rt_denoise on the averaged guides.
 * Variance prefilter, t = 0 .. var_iter-1, step 2^t (sw = sx = 0.0 before the taps):
 *   g = ((1.0 + dn*inv_n) * (1.0 + (dz*dz)*inv_z)) * (1.0 + da*inv_a);  w = hh / g
 *   sw = sw + w;  sx = sx + w * v_t(q);          v_{t+1}(p) = sx / sw
 * u_0 = v_{var_iter}. Colour iteration k = 0 .. n_iter-1, step 2^k (sw = su = sv_c = 0.0 before the taps):
 *   dc  = rt_denoise's squared distance on e_k(p), e_k(q)
 *   r   = (dc * inv_c) / ((u_k(p) + u_k(q)) + var_floor)
 *   den = (((1.0 + r) * (1.0 + dn*inv_n)) * (1.0 + (dz*dz)*inv_z)) * (1.0 + da*inv_a);  w = hh / den
 *   sw = sw + w;  sv_c = sv_c + w * e_k,c(q);  su = su + (w*w) * u_k(q)
 *   e_{k+1},c(p) = sv_c / sw;   u_{k+1}(p) = su / (sw*sw)
 * Outputs: out_c = (e_{n_iter},c * m_c) * sp2 — sums of 2*spp samples, so rt_tonemap_device(.., 2*spp, ..) applies as it
 * is; out_variance[p] = u_{n_iter}(p), the residual variance of the demodulated mean, one double per pixel in buffer order
 * (with n_iter = 0 the prefiltered input variance): what an adaptive sampler ranks pixels by. Buffer contents are never
 * validated; NaN and inf in guides propagate as IEEE carries them.
 *
 * Row order: rt_denoise's rules. NULL, or `height` entries that are a permutation of [0, height); one list serves both
 * halves and both outputs. rt_denoise_dual checks it on the host, rt_denoise_dual_device with rt_denoise_device's kernel
 * behind one synchronisation of hip_stream, before anything writes an output; with NULL rows it is a pure enqueue.
 *
 * Workspace: rt_denoise_dual_device allocates nothing; the caller gives rt_denoise_dual_workspace_bytes(p) bytes (the
 * packed guides, the ping-pong planes of colour and variance, the row map), contents meaningless before and reusable
 * after. d_out_rgb_sum may alias either sum input (every input is read before any output is written); d_out_variance
 * (may be NULL: not wanted) must not overlap any other buffer. All device buffers and the workspace are 16-byte aligned,
 * device rows 4-byte aligned.
 *
 * RT_ERR_INVALID with rt_last_error() set, before any device call: everything rt_denoise* refuses; a null q, sum_b or
 * feat_b; var_iter > RT_DENOISE_MAX_VAR_ITER; a var_floor that is <= 0, NaN or infinite; q->flags != 0; a misaligned
 * d_out_variance. */
typedef struct rt_denoise_dual_params {   /* 16 B */
    uint32_t var_iter;                /* 0 .. RT_DENOISE_MAX_VAR_ITER: prefilter passes over the variance estimate */
    uint32_t flags;                   /* must be 0 */
    double   var_floor;               /* > 0, finite: added to the variance sum under the colour distance */
} rt_denoise_dual_params;
#define RT_DENOISE_MAX_VAR_ITER 8

/* Bytes of device workspace rt_denoise_dual_device needs for p's image; 0 on invalid params. */
uint64_t rt_denoise_dual_workspace_bytes(const rt_denoise_params *p);
/* Device buffers (per half width * height * 3 sums and width * height records; NULL or `height` row ids; width * height
 * * 3 sums and, if wanted, width * height variances out), enqueued on hip_stream (NULL = default stream). */
int rt_denoise_dual_device(const double *d_sum_a, const double *d_sum_b,
                           const rt_feature *d_feat_a, const rt_feature *d_feat_b,
                           const uint32_t *d_row_ids, const rt_denoise_params *p, const rt_denoise_dual_params *q,
                           double *d_out_rgb_sum, double *d_out_variance, void *d_workspace, void *hip_stream);
/* Host buffers; synchronous. out_variance and ms may be NULL. */
int rt_denoise_dual(const double *sum_a, const double *sum_b,
                    const rt_feature *feat_a, const rt_feature *feat_b,
                    const uint32_t *row_ids, const rt_denoise_params *p, const rt_denoise_dual_params *q,
                    double *out_rgb_sum, double *out_variance, double *ms);

/* ---- temporal accumulation with reprojection for moving-camera frames ------------------------------------
 * A caller who renders a camera path reuses the earlier frames' samples: each pixel's first-hit point is found from the
 * frame's own feature record, projected into the previous camera, and the previous frame's accumulated radiance is
 * gathered there by bilinear taps that pass a depth and a normal test. It sits between the feature call and the denoiser,
 *   rt_render_device -> rt_features_device -> rt_temporal_device -> rt_denoise*_device -> rt_tonemap_device,
 * all in HBM on one stream, needs no rt_scene and changes nothing of a render. The scene is taken to be static: the camera
 * moves, objects do not. The mean first-hit point of a pixel comes from F.depth / F.hits alone: get_ray's direction is
 * lower_left + s*horizontal + t*vertical - origin - offset, so a hit at ray parameter z lies at origin + z*(G - origin) +
 * (1 - z)*offset with G the point of the focus plane, and the lens offset averages to zero over a pixel's samples.
 *
 * State: one rt_temporal_pixel per pixel in IMAGE order (index y * width + x, y the image row of a row id, whatever the
 * order of the sums): the accumulated demodulated mean radiance e, the history length n, and this frame's mean first-hit
 * depth and normal, which the NEXT frame's taps are tested against. The caller keeps two states and swaps them.
 *
 * Definition: IEEE + - * / on doubles in the stated order, no contraction; floor() is exact. Per pixel p = (x, y), with
 * sp = (double)spp, S the pixel's sums, F its rt_feature record (both sums of `spp` samples) and nan0(v) = v is NaN ? 0 : v:
 *   c_j = nan0(S_j) / sp;  a_j = F.albedo_j / sp
 *   m_j = a_j > albedo_floor ? a_j : albedo_floor  (rt_denoise's rule; RT_TEMPORAL_NO_DEMODULATE: m_j = 1.0);  e_j = c_j / m_j
 *   covered = F.hits > 0;  zb = covered ? F.depth / F.hits : 0;  nb_j = covered ? F.normal_j / F.hits : 0
 * Restart: e_out = e, n_out = 1. A pixel restarts with no d_prev, when it is not covered (but see RT_TEMPORAL_FAR_MISSES below), and wherever stated below.
 * Otherwise, with cross(u, v) = (u1*v2 - u2*v1, u2*v0 - u0*v2, u0*v1 - u1*v0) and dot(u, v) = (u0*v0 + u1*v1) + u2*v2,
 * o / llc / hor / ver the current camera's origin, lower_left_corner, horizontal, vertical and o' / llc' / hor' / ver' the
 * previous camera's:
 *   sc = ((double)x + 0.5) / (double)(width - 1);  tc = ((double)y + 0.5) / (double)(height - 1)
 *   G_k = (llc_k + sc*hor_k) + tc*ver_k;   P_k = o_k + zb*(G_k - o_k)                    the mean first-hit point
 *   D_k = P_k - o'_k;  r_k = o'_k - llc'_k;  c_k = -D_k                                   solve s'*hor' + t'*ver' + lam*c = r
 *   bc = cross(ver', c);  rc = cross(r, c);  br = cross(ver', r);  det = dot(hor', bc)
 *   s' = dot(r, bc) / det;  t' = dot(hor', rc) / det;  lam = dot(hor', br) / det
 *   fx = s' * (double)(width - 1) - 0.5;  fy = t' * (double)(height - 1) - 0.5;  ze = 1.0 / lam
 * ze is the ray parameter at which the previous camera's ray through (fx, fy) reaches P: what its depth records hold.
 * History exists only if lam > 0, fx and fy are finite, -1 <= fx < (double)width and -1 <= fy < (double)height; otherwise
 * the pixel restarts (every pixel of an image one pixel wide or high does: sc or tc is infinite). Only then are fx and fy
 * converted to integers: x0 = floor(fx), wx = fx - x0, y0 = floor(fy), wy = fy - y0. The taps q_0 .. q_3 are (x0, y0),
 * (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with bw_0 = (1.0 - wx)*(1.0 - wy), bw_1 = wx*(1.0 - wy), bw_2 = (1.0 - wx)*wy,
 * bw_3 = wx*wy. A tap q counts if it is inside the image, prev(q).depth > 0, |prev(q).depth - ze| <= tol_depth * ze and
 * d <= tol_normal with d = (d0*d0 + d1*d1) + d2*d2, d_k = nb_k - prev(q).normal_k; a tolerance of +inf skips its test (a
 * NaN then passes it). Over the counting taps in tap order, from sw = sn = se_j = 0.0:
 *   sw = sw + bw;  se_j = se_j + bw * prev(q).e_j;  sn = sn + bw * prev(q).n
 * If sw >= w_min:  eh_j = se_j / sw;  nh = sn / sw;  t = nh + 1.0;  n_out = t < n_max ? t : n_max;
 *                  e_out_j = eh_j + (e_j - eh_j) / n_out;       otherwise the pixel restarts.
 * Outputs: state_out(p) = {e_out, n_out, zb, nb}; out_j = (e_out_j * m_j) * sp at the pixel's place in the sums' order —
 * sums of `spp` samples again, so rt_tonemap_device, rt_denoise*, rt_write_color apply as they are. Buffer contents are
 * never validated: NaN and inf propagate as IEEE carries them. n_max = 1 makes e_out = eh + (e - eh), which is e to rounding: no history is kept.
 *
 * RT_TEMPORAL_FAR_MISSES (a flag bit older callers never set: the ABI version stays 3): history for pixels that miss. It
 * applies when d_prev is given and the pixel is not covered (F.hits > 0 is false); covered pixels are untouched. Then
 *   D_k = G_k - o_k  with G from sc, tc as above: the pixel centre's direction, a point at infinity
 *   c_k = -D_k;  r_k = o'_k - llc'_k
 *   bc, rc, br, det, s', t', lam, fx, fy by the same expressions in the same order; no ze is formed.
 * History exists only if lam > 0 and the same range tests hold; only then are fx and fy converted to integers, and the taps
 * and their weights are the same four. A tap q counts if it is inside the image and prev(q).depth == 0.0 — an uncovered
 * pixel of the previous state (a NaN depth does not count); there is no depth test and no normal test. The sums, the w_min
 * rule, n_out and e_out are as above; state_out(p) = {e_out, n_out, 0, 0}. A covered pixel's taps need depth > 0, so the
 * two kinds never mix. An image one pixel wide or high still restarts everywhere. Sky, a black backdrop and — with
 * RT_FLAG_SURFACES records — fog in front of nothing then keep their history under a turning camera.
 *
 * Two halves for rt_denoise_dual need nothing more: call once per half, each with that half's own sums, features and
 * states, so that A and B stay independent estimates; then rt_denoise_dual_device on the two outputs with the current
 * frame's features.
 *
 * Row order: d_rgb_sum, d_features and d_out_rgb_sum are in row_ids order under rt_denoise's rules — NULL, or `height`
 * entries that are a permutation of [0, height), checked on the host by rt_temporal and by rt_denoise_device's row kernel
 * behind one synchronisation of hip_stream by rt_temporal_device, before anything writes an output: a refused list leaves
 * both outputs untouched. With NULL rows rt_temporal_device is a pure enqueue. Both states are always in image order.
 *
 * Buffers: d_prev == NULL means the first frame (prev_cam may then be NULL too). d_out_rgb_sum may alias d_rgb_sum.
 * d_state_out must not overlap d_prev — the kernel gathers from d_prev — which is checked on the address ranges. The
 * workspace (rt_temporal_workspace_bytes(p) bytes: the inverse row map, height x uint32 rounded up to 16 bytes, and 16
 * bytes for its bad-id count) means nothing before the call and may be reused. All buffers and the workspace are 16-byte
 * aligned, device rows 4-byte aligned. rt_temporal stages host buffers through device memory of its own on the current
 * device's default stream and reports the device time of the kernel in *ms.
 *
 * RT_ERR_INVALID with rt_last_error() set, before any device call: a null params, cam, sums, features, output, state or
 * workspace; width, height or spp equal to 0; width * height > RT_DENOISE_MAX_PIXELS; a tolerance that is <= 0 or NaN;
 * n_max < 1, NaN or infinite; w_min outside (0, 1]; a floor that is <= 0, NaN or infinite; a flag bit other than
 * RT_TEMPORAL_NO_DEMODULATE / RT_TEMPORAL_FAR_MISSES; a misaligned pointer; d_prev without prev_cam; overlapping states.
 *
 * Limits: static scenes only. Under first-hit records a ConstantMedium's hit has a drawn depth and the normal (1, 0, 0):
 * pixels seen through a medium mostly fail the depth test and restart. RT_FLAG_SURFACES records reproject a medium by the
 * surface behind it instead, which is wrong for dense smoke with parallax of its own. Without RT_TEMPORAL_FAR_MISSES a pixel
 * that is not covered never takes history. Edge pixels whose samples straddle two surfaces have a mean depth on
 * neither and restart. Neither state can be given as a strip of rows; there is no rt_scene_set form. */
typedef struct rt_temporal_pixel {    /* 64 B: four 16-byte pieces */
    double   e[3];                    /* accumulated demodulated mean radiance */
    double   n;                       /* history length, >= 1 (a double: bilinear taps mix lengths) */
    double   depth;                   /* this frame's mean first-hit depth F.depth / F.hits; 0 = not covered */
    double   normal[3];               /* F.normal / F.hits; 0 when not covered */
} rt_temporal_pixel;

typedef struct rt_temporal_params {   /* 64 B */
    uint32_t width, height, spp, flags;   /* flags: RT_TEMPORAL_NO_DEMODULATE | RT_TEMPORAL_FAR_MISSES */
    double   tol_depth, tol_normal;   /* > 0; +inf = test off */
    double   n_max;                   /* >= 1, finite: cap of the history length */
    double   w_min;                   /* in (0, 1]: least valid bilinear weight that still counts as history */
    double   albedo_floor;            /* > 0, finite: rt_denoise's rule */
    double   _pad;
} rt_temporal_params;
#define RT_TEMPORAL_NO_DEMODULATE 0x1u               /* accumulate the radiance itself: m = 1 */
#define RT_TEMPORAL_FAR_MISSES 0x4u                  /* uncovered pixels reproject as points at infinity (see above); 0x2 is not a flag */

/* Bytes of device workspace rt_temporal_device needs for p's image; 0 on invalid params. */
uint64_t rt_temporal_workspace_bytes(const rt_temporal_params *p);
/* Device buffers (width * height * 3 sums in and out, width * height feature records, NULL or `height` row ids, width *
 * height state records in — or NULL — and out), enqueued on hip_stream (NULL = default stream). */
int rt_temporal_device(const double *d_rgb_sum, const rt_feature *d_features, const uint32_t *d_row_ids,
                       const rt_camera *cam, const rt_temporal_pixel *d_prev, const rt_camera *prev_cam,
                       const rt_temporal_params *p, rt_temporal_pixel *d_state_out, double *d_out_rgb_sum,
                       void *d_workspace, void *hip_stream);
/* Host buffers; synchronous. prev, prev_cam and ms may be NULL. */
int rt_temporal(const double *rgb_sum, const rt_feature *features, const uint32_t *row_ids,
                const rt_camera *cam, const rt_temporal_pixel *prev, const rt_camera *prev_cam,
                const rt_temporal_params *p, rt_temporal_pixel *state_out, double *out_rgb_sum, double *ms);

/* ---- per-pixel adaptive sampling: pixel-list renders and a sample planner -------------------------------------
 * The consumer of rt_denoise_dual's variance: more samples where the frame needs them, none where it does not,
 *   render -> features -> denoise_dual -> plan -> render_pixels -> merge -> ... -> resolve,
 * all in HBM. The unit of extra work is one FRAME's worth of samples of one pixel: rt_params.n_frames already gives every
 * (frame, pixel) an independent, reproducible set of `spp` samples, so "k more units for pixel b" is "pixel b of k frames
 * nobody has rendered yet" — and a per-pixel sample count is a multiple of spp.
 *
 * rt_render_pixels*: a render of a LIST of (frame, pixel) ids instead of whole rows. An entry is
 *   id = frame * (width * height) + py * width + px,     py counted upwards as in a render,
 * and out_rgb_sum[3e .. 3e+3) of entry e is exactly what rt_render writes for column px of row id frame * height + py with
 * the same rt_camera and rt_params (n_frames > frame), spp_chunk included: Rng(path_key(seed, frame, py * width + px, s)),
 * the camera's draws, ray_color on the same generator, summed in the render's order — the oracle's rt_render_cpu bit for
 * bit, NaN where it has NaN. Repeated ids are allowed and give equal sums; the order and the size of the list never change
 * an entry's result. The work runs in the render's wavefront engine: the only difference is where a new path's px, py and
 * frame come from.
 *
 * rt_params: used — width, height, spp, max_depth, background, t_min, seed, n_frames, spp_chunk, flags; IGNORED — n_rows,
 * row_ids, progress_cb, progress_user.
 *
 * Arguments: n_entries == 0, spp == 0 and max_depth == 0 are RT_OK, as for rt_radiance (zeros are written where there is
 * output, with no kernel of the engine). RT_ERR_INVALID with rt_last_error() set, before any engine kernel: a null scene,
 * cam or params; a null id or output buffer with n_entries > 0; width, height or n_frames equal to 0, or height * n_frames
 * above 2^32 - 1 (the matching row id must exist); cam->time0 >= cam->time1; a flag bit other than RT_FLAG_COUNTERS /
 * RT_FLAG_KERNEL_TIMES; a device id buffer that is not 8-byte aligned or a device output that is not 16-byte aligned;
 * n_entries > RT_RADIANCE_MAX_RAYS or n_entries * ceil(spp / chunk) > RT_RADIANCE_MAX_ITEMS; an id >= width * height *
 * n_frames — host ids are checked on the host, device ids by a small counting kernel whose count is read behind the one
 * synchronisation of hip_stream the engine makes anyway before its first pass (the output is untouched). A scene switched
 * to the A/B megakernel engine is RT_ERR_UNSUPPORTED. There is no RT_FLAG_ASYNC and no rt_scene_set form.
 *
 * Workspace and stats: like rt_radiance*, the call runs in the render's per-(scene, stream) workspace — pool, planes (the
 * ring of planes under the same rule) and tape; an RT_FLAG_ASYNC render in flight on that (scene, stream) is joined and
 * finished first; renders after it keep their bits. rt_render_pixels_device returns once the call is complete.
 * rt_render_pixels stages ids and sums through buffers the workspace keeps, on the default stream. rt_stats (may be NULL)
 * means what it means for a render of those pixels: paths = n_entries * spp, and with RT_FLAG_COUNTERS the counters are
 * the oracle's sums over the same samples, camera draws included. */
int rt_render_pixels(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *pixel_ids, uint64_t n_entries,
                     double *out_rgb_sum, rt_stats *stats);
int rt_render_pixels_device(rt_scene *scene, const rt_camera *cam, const rt_params *params, const uint64_t *d_pixel_ids, uint64_t n_entries,
                            double *d_out_rgb_sum, void *hip_stream, rt_stats *stats);

/* The planner, the merge and the resolve: no rt_scene, nothing of a render's state. All are defined bit for bit: IEEE * / +
 * on doubles in the stated order with no contraction, integers otherwise. Buffers are in BUFFER order: row r of a buffer is
 * image row row_ids[r]; row_ids is NULL (the identity) or `height` entries that are a permutation of [0, height), under
 * rt_denoise's rules and checked by its row kernel.
 *
 * Plan — an error map to a list of entries. Per buffer pixel b = r * width + x (n = width * height of them):
 *   t = err[b] * scale
 *   units[b] = !(t >= 1.0) ? 0 : (t >= (double)max_units ? max_units : (uint32_t)t)       NaN and negatives: 0; +inf: max_units
 *   offsets[0 .. n] = the exclusive prefix sum of units in 64 bits; offsets[n] = total, also stored to *out_total
 *   only if total <= capacity: for k < units[b]:
 *       entries[offsets[b] + k] = (uint64_t)(first_frame + k) * (width * height) + row_ids[r] * width + x
 *   otherwise no entry is written, units and offsets are still valid and the call is RT_OK: capacity == 0 with NULL entries
 *   counts only, so a caller can lower scale or grow the buffer and call again.
 * rt_adaptive_plan_device allocates nothing: the caller gives it rt_adaptive_workspace_bytes(p) bytes (the scan's tile
 * totals, the row kernel's map and count). It synchronises hip_stream ONCE, reading the total and the bad-row count
 * together; a bad row list is RT_ERR_INVALID with units, offsets and entries untouched. The prefix sum is a scan in three
 * launches — tile totals, a scan of the totals, emit — in which no workgroup ever waits on another.
 * RT_ERR_INVALID with rt_last_error() set, before any device call: a null params, error map, units, offsets or workspace,
 * null entries with capacity > 0; width or height 0; width * height > RT_DENOISE_MAX_PIXELS; max_units == 0 or first_frame
 * + max_units > 2^32 - 1; a scale that is <= 0, NaN or infinite; flags or _pad != 0; misalignment — 16 bytes for the error
 * map and the workspace, 8 for offsets and entries, 4 for units and rows. rt_adaptive_plan (host buffers) checks the row
 * list on the host and stages through device memory of its own on the current device's default stream.
 *
 * Merge — the sums rt_render_pixels* wrote for a plan's entries (E, three doubles per entry), into per-pixel accumulators.
 * One lane per pixel b, for k = 0 .. units[b]-1 in order: acc_c = acc_c + E[(offsets[b] + k) * 3 + c]; then
 * acc_n[b] = acc_n[b] + (double)((uint64_t)units[b] * spp). Pixels with 0 units are not written. A pure enqueue.
 * Resolve — out_c = (acc_c / acc_n[b]) * (double)spp_out: sums "of spp_out samples", so rt_tonemap_device, rt_write_color
 * and both denoisers apply as they are; acc_n == 0 gives NaN, which the tone map turns to 0. d_out may alias d_acc_sum. A
 * pure enqueue. Both take buffers that are 8-byte aligned (units 4); n_pixels == 0 is RT_OK with no launch; a null buffer
 * or n_pixels > RT_DENOISE_MAX_PIXELS is RT_ERR_INVALID.
 *
 * Feature records go through the same accumulators, so that an adaptive frame's guides come from every sample it took:
 * rt_adaptive_merge_features_device — E the records rt_features_pixels* wrote for a plan's entries; one lane per pixel b,
 * for k = 0 .. units[b]-1 in order, each of the record's eight doubles f: acc_f = acc_f + E[offsets[b] + k].f. Pixels with
 * 0 units are not written. It touches no sample count: the radiance merge's acc_n counts both.
 * rt_adaptive_resolve_features_device — out_f = (acc_f / acc_n[b]) * (double)spp_out on all eight fields: records "of
 * spp_out samples", which both denoisers take as they are (they divide albedo, normal and depth by the sample count and
 * ignore hits, so every field is linear). acc_n == 0 gives NaN; d_out may alias d_acc. Both are pure enqueues; records are
 * 16-byte aligned and moved as four 16-byte pieces, units 4-byte, offsets and acc_n 8-byte aligned; n_pixels == 0 is RT_OK
 * with no launch; a null buffer, a misaligned buffer or n_pixels > RT_DENOISE_MAX_PIXELS is RT_ERR_INVALID.
 *
 * Two independent halves for rt_denoise_dual need nothing more: plan twice with first_frame = f and f + max_units (the
 * units are the same), writing at d_entries and d_entries + total; render both lists in ONE rt_render_pixels_device; merge
 * each half of the sums into its own accumulator. */
typedef struct rt_adaptive_params {   /* 32 B */
    uint32_t width, height;
    uint32_t first_frame;             /* frame of a pixel's first new unit */
    uint32_t max_units;               /* >= 1; first_frame + max_units <= 2^32 - 1 */
    double   scale;                   /* > 0, finite */
    uint32_t flags, _pad;             /* 0 */
} rt_adaptive_params;

/* Bytes of device workspace rt_adaptive_plan_device needs for p's image; 0 on invalid params. */
uint64_t rt_adaptive_workspace_bytes(const rt_adaptive_params *p);
int rt_adaptive_plan_device(const double *d_err, const uint32_t *d_row_ids, const rt_adaptive_params *p, uint32_t *d_units, uint64_t *d_offsets,
                            uint64_t *d_entries, uint64_t capacity, void *d_workspace, void *hip_stream, uint64_t *out_total);
/* Host buffers (entries may be NULL with capacity 0; out_total may be NULL); synchronous. */
int rt_adaptive_plan(const double *err, const uint32_t *row_ids, const rt_adaptive_params *p, uint32_t *units, uint64_t *offsets,
                     uint64_t *entries, uint64_t capacity, uint64_t *out_total);
int rt_adaptive_merge_device(const double *d_entry_sums, const uint32_t *d_units, const uint64_t *d_offsets, uint64_t n_pixels, uint32_t spp,
                             double *d_acc_sum, double *d_acc_n, void *hip_stream);
int rt_adaptive_resolve_device(const double *d_acc_sum, const double *d_acc_n, uint64_t n_pixels, uint32_t spp_out, double *d_out, void *hip_stream);
int rt_adaptive_merge_features_device(const rt_feature *d_entry_features, const uint32_t *d_units, const uint64_t *d_offsets,
                                      uint64_t n_pixels, rt_feature *d_acc, void *hip_stream);
int rt_adaptive_resolve_features_device(const rt_feature *d_acc, const double *d_acc_n, uint64_t n_pixels, uint32_t spp_out,
                                        rt_feature *d_out, void *hip_stream);

/* ---- a BVH over caller geometry, built on the device -------------------------------------------------------
 * Everything above needs only a valid rt_scene_desc; this makes its rt_bvh_node records from the caller's own leaves — a
 * mesh, a million spheres — instead of the nine scene builders' (rt2022_host.h). A linear BVH: Morton order of the leaf
 * boxes' centres, Karras' radix tree over the sorted keys, one bottom-up pass. The definition is exact (f64, no contraction),
 * so the records are defined bit for bit (tests/bvh_ref.py restates them in numpy); DESIGN.md §4.15 has the reasoning.
 *
 * Input: n_leaves refs and boxes6[i] = {min[3], max[3]} of leaf i (rtb_ref_boxes computes them for the refs of a description).
 * A ref goes into the tree exactly as given, flip bit included; a ref of kind RT_KIND_NODE is allowed (a subtree as a leaf).
 * Output: max(1, n_leaves - 1) records; record j is the ref RT_MAKE_REF(RT_KIND_NODE, node_base + j) and the root is record
 * 0, so the result can be appended to a pool that already holds node_base nodes. _pad is 0.
 *
 *   1. Scene box: lo[a] = min_i bmin_i[a], hi[a] = max_i bmax_i[a] (a two-stage reduction).
 *   2. Key of leaf i, per axis: c = 0.5 * (bmin + bmax); e = hi - lo; q = e > 0 ? (c - lo) / e : 0;
 *      k = (uint32) min(q * 2097152.0, 2097151.0) — 21 bits. The 63-bit Morton key has bit b of k_x at 3b + 2, of k_y at
 *      3b + 1, of k_z at 3b.
 *   3. Order: by (key, i) — a stable radix sort of (key, index) pairs.
 *   4. Tree: Karras' radix tree over the n distinct 95-bit keys (key << 32) | i in that order. The range [a, b] of sorted
 *      positions splits at g, the last position whose key shares more than the range's common prefix with key a; the children
 *      are [a, g] and [g + 1, b]. A child of one position is that leaf's ref; otherwise the left child is internal node g and
 *      the right one internal node g + 1. The root, [0, n - 1], is node 0. Built in parallel, one thread per internal node.
 *   5. Bottom-up: a node's box is the component-wise min and max of its children's (exact, order-free). Stack need: a leaf
 *      needs 1, a node with children needing l and r needs max(1 + l, r) — what rt_scene_create counts (a leaf that is itself a
 *      subtree, a mover, a list or a medium counts as 1 here). If need(left) > need(right) the children are swapped before the
 *      node's need is computed, which gives need(root) <= 1 + floor(log2 n): a need of k takes at least 2^(k-1) leaves. So a
 *      million primitive leaves stay on the 22-entry stack however deep the radix tree is (clustered geometry makes it deep).
 *      Record j stays node j whichever way its children are ordered.
 *   6. n_leaves == 1: one record with left == right == the leaf and the leaf's box (the reference's span-1 node; its need is 2).
 *
 * RT_ERR_INVALID with rt_last_error() set and the output untouched: a null pointer; n_leaves == 0; node_base + max(1, n - 1)
 * > 2^27; (device form) a workspace that is null, not 16-byte aligned or smaller than rt_bvh_workspace_bytes(n_leaves), node
 * or box buffers that are not 16-byte aligned, refs that are not 4-byte aligned — all before any device call; and any box
 * with a non-finite coordinate, a coordinate beyond 1e300 in magnitude or min > max — counted on the device by the reduction
 * of step 1, before anything but workspace is written. Without a device rt_bvh_build then returns RT_ERR_DEVICE.
 *
 * rt_bvh_build_device is ordered on hip_stream (NULL = default stream) on the current device. It synchronises that stream
 * once, to read the count of refused boxes, and makes no other host round trip. It allocates nothing: the caller gives it
 * rt_bvh_workspace_bytes(n_leaves) bytes of 16-byte aligned device memory, whose contents before the call mean nothing and
 * which the next build on the stream may reuse (a larger workspace serves a smaller build). rt_bvh_build stages host
 * buffers through device memory of its own on the default stream. Out of scope: no SAH, no refit, no treelet optimisation. */
uint64_t rt_bvh_workspace_bytes(uint32_t n_leaves);
int rt_bvh_build_device(const uint32_t *d_leaf_refs, const double *d_boxes6, uint32_t n_leaves, uint32_t node_base,
                        rt_bvh_node *d_out_nodes, void *d_workspace, uint64_t workspace_bytes, void *hip_stream);
int rt_bvh_build(const uint32_t *leaf_refs, const double *boxes6, uint32_t n_leaves, uint32_t node_base, rt_bvh_node *out_nodes);

/* ---- a coherence order for a batch of rays, and queries worked in a given order ---------------------------------
 * rt_intersect* works its rays in the caller's order, and a wave of 64 neighbouring rays that start far apart or point
 * apart walks the tree with most lanes idle. rt_ray_order* computes, on the device and without a scene, an order that puts
 * rays of like origin and direction next to each other; rt_intersect_ordered* does rt_intersect's work in a given order.
 * DESIGN.md §4.16 has the reasoning and what it buys; tests/ray_order_ref.py restates the definition in numpy.
 *
 * order[w] is the index of the ray to work on w-th: the permutation that sorts (key, index) ascending (a stable radix sort
 * of (key, index) pairs, indices going in ascending). Only origin[3] at byte 0 and direction[3] at byte 24 of each record
 * are read, ray_stride bytes apart: 80 for rt_query_ray, 64 for rt_radiance_ray. All arithmetic is f64, no contraction:
 *
 *   Straggler: a ray with an origin or direction component that is not finite, an origin component beyond 1e300 in
 *     magnitude, or all three direction components zero. Its key is 1 << 63: stragglers come last, in index order. They are
 *     not refused (hostile rays are valid input to rt_intersect).
 *   Origin box: lo, hi = component-wise min and max of the non-stragglers' origins (a two-stage reduction).
 *   Origin word O, 3 * origin_bits bits. Per axis: e = hi - lo; q = e > 0 ? (o - lo) / e : 0;
 *     k = (uint32) min(q * 2^origin_bits, 2^origin_bits - 1). Morton-interleaved: bit b of k_x at 3b + 2, of k_y at 3b + 1,
 *     of k_z at 3b. origin_bits == 0 gives O = 0.
 *   Direction word D, 3 + 2 * dir_bits bits. a = the first axis of largest |d|; m = |d_a|; s = d_a < 0; face = 2a + s.
 *     For j = (a + 1) % 3, then (a + 2) % 3: r = d_j / m; k = (uint32) min((r + 1.0) * (0.5 * 2^dir_bits), 2^dir_bits - 1).
 *     uv has bit b of the first k at 2b + 1 and of the second at 2b. D = face << (2 * dir_bits) | uv.
 *   Key: RT_ORDER_ORIGIN_FIRST     O << (3 + 2 * dir_bits) | D
 *        RT_ORDER_DIRECTION_FIRST  D << (3 * origin_bits) | O
 *        RT_ORDER_FACE_ORIGIN_UV   face << (3 * origin_bits + 2 * dir_bits) | O << (2 * dir_bits) | uv
 *     — at most 63 bits, so none reaches bit 63.
 *
 * rt_ray_order_device is a pure enqueue on hip_stream (NULL = default stream) on the current device, with no host
 * synchronisation: nothing is refused on the device. It allocates nothing: the caller gives it
 * rt_ray_order_workspace_bytes(n_rays) bytes of 16-byte aligned device memory, whose contents before the call mean nothing and
 * which the next call on the stream may reuse (a larger workspace serves a smaller call). rt_ray_order stages host buffers
 * through device memory of its own on the default stream. n_rays == 0 is RT_OK with no launch.
 * RT_ERR_INVALID with rt_last_error() set and nothing written, before any device call: a null pointer with n_rays > 0;
 * n_rays >= 2^32; origin_bits > 16, dir_bits > 6, an unknown layout; a ray_stride that is not a multiple of 16 or is below
 * 48; (device form) a workspace that is null, not 16-byte aligned or too short, rays that are not 16-byte aligned, an order
 * buffer that is not 4-byte aligned. */
#define RT_ORDER_ORIGIN_FIRST    0u
#define RT_ORDER_DIRECTION_FIRST 1u
#define RT_ORDER_FACE_ORIGIN_UV  2u
typedef struct rt_ray_order_params {  /* 16 B */
    uint32_t origin_bits;             /* per axis, 0..16 */
    uint32_t dir_bits;                /* per face axis, 0..6 */
    uint32_t layout;                  /* RT_ORDER_* */
    uint32_t ray_stride;              /* bytes from one ray record to the next: a multiple of 16, >= 48 */
} rt_ray_order_params;
uint64_t rt_ray_order_workspace_bytes(uint64_t n_rays);
int rt_ray_order_device(const void *d_rays, uint64_t n_rays, const rt_ray_order_params *p, uint32_t *d_order,
                        void *d_workspace, uint64_t workspace_bytes, void *hip_stream);
int rt_ray_order(const void *rays, uint64_t n_rays, const rt_ray_order_params *p, uint32_t *order);

/* rt_intersect's work in a given order: work item w is ray order[w], and its record goes to out_hits[order[w]] — the
 * record rt_intersect_device writes for that ray, every byte of it. The rays are gathered into the workspace in working
 * order, the query kernel runs on the gathered buffer as it does on a caller's, and the records are scattered back.
 * Any order list is safe: an entry >= n_rays is never used as an address (its work item is an inert ray whose record goes
 * nowhere); the record of a ray that no entry names stays untouched; a ray named twice is computed twice and gets the same
 * record both times.
 * rt_stats as for rt_intersect_device, except that rays counts the entries < n_rays and ms covers the gather, the query
 * and the scatter; the sums of the counters do not depend on the order (an inert ray may add node visits of its own).
 * rt_intersect_ordered_device: rt_intersect_device's arguments, refusals and synchronisation (none without stats), and
 * rt_ray_order_device's for n_rays, the order buffer and the workspace, of rt_intersect_ordered_workspace_bytes(n_rays)
 * bytes. rt_intersect_ordered: host buffers; order == NULL computes the order of the rays with p (then p must not be NULL,
 * and its ray_stride must be 80; with an order, p is ignored). */
uint64_t rt_intersect_ordered_workspace_bytes(uint64_t n_rays);
int rt_intersect_ordered_device(rt_scene *scene, const rt_query_ray *d_rays, const uint32_t *d_order, uint64_t n_rays, uint32_t flags,
                                rt_hit *d_out_hits, void *d_workspace, uint64_t workspace_bytes, void *hip_stream, rt_stats *stats);
int rt_intersect_ordered(rt_scene *scene, const rt_query_ray *rays, const uint32_t *order, const rt_ray_order_params *p,
                         uint64_t n_rays, uint32_t flags, rt_hit *out_hits, rt_stats *stats);

/* write_color (main.rs:280-299): NaN→0, sqrt(c/spp), clamp [0,0.999], *255.999, floor. */
void rt_write_color(const double rgb_sum[3], int32_t spp, uint8_t out_rgb[3]);
/* Device form over n_pixels sums → n_pixels*3 bytes, on hip_stream. */
int rt_tonemap_device(const double *d_rgb_sum, uint64_t n_pixels, int32_t spp,
                      uint8_t *d_rgb8, void *hip_stream);

/* Last error message of the calling thread ("" if none). */
const char *rt_last_error(void);
/* ABI version the library was built with. */
uint32_t rt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT2022_H */
