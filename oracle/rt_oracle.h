/* rt_oracle.h — entry points of the CPU oracle (test infrastructure only; see
 * rt_oracle.cpp). Same POD types as include/rt2022.h. */
#ifndef RT_ORACLE_H
#define RT_ORACLE_H
#include "../include/rt2022.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct rto_hit_record {       /* HitRecord, hittable/mod.rs:18-26 */
    int32_t  hit;
    int32_t  front_face;
    double   p[3];
    double   normal[3];
    double   t, u, v;
    uint32_t mat;
    uint32_t rng_draws;
} rto_hit_record;

enum rto_math_op { RTO_SIN = 0, RTO_COS = 1, RTO_ACOS = 2, RTO_ATAN2 = 3, RTO_LOG = 4, RTO_SQRT = 5, RTO_DIV = 6 };

/* The shade census: what rto_ray_color did on the paths of rt_render_cpu / rto_ray_color calls made while it was on.
 * Off by default; rt_stats, results and every other counter are the same with it on or off. Indices are the enums of
 * rt2022.h (rt_material_kind, rt_texture_kind) and the ones below; a [2] is [0] = no / back face, [1] = yes / front face. */
enum rto_light_arm { RTO_ARM_SPHERE = 0, RTO_ARM_RECT_XY = 1, RTO_ARM_RECT_XZ = 2, RTO_ARM_RECT_YZ = 3, RTO_ARM_FLIPPED = 4, RTO_ARM_OTHER = 5 };
enum rto_tex_none { RTO_TEX_NONE = 4 };                      /* the material reads no texture (Metal, Dielectric) */
enum rto_mixture_choice { RTO_MIX_LIGHT = 0, RTO_MIX_COSINE = 1, RTO_MIX_COSINE_ONLY = 2 /* n_lights == 0: no choice is drawn */ };
enum rto_dielectric_outcome { RTO_DIEL_CANNOT_REFRACT = 0, RTO_DIEL_SCHLICK = 1, RTO_DIEL_REFRACT = 2 };
enum rto_path_end { RTO_END_MISS = 0, RTO_END_LIGHT_FRONT = 1, RTO_END_LIGHT_BACK = 2, RTO_END_DEPTH = 3 };
typedef struct rto_shade_census {
    uint64_t scatter[5][5][5][2];   /* Material::scatter -> Some: [material kind][leaf texture kind, checkers resolved][top texture kind][front_face] */
    uint64_t emitted[4][2];         /* a DiffuseLight was hit: [leaf texture kind][front_face] */
    uint64_t light_draw[6];         /* HittableList::random, by the arm of the entry drawn */
    uint64_t mixture_choice[3];     /* MixturePdf::generate: light half, cosine half; cosine-only mode */
    uint64_t light_pdf[6][2];       /* Hittable::pdf_value of one entry: [arm][the ray hit it] */
    uint64_t dielectric[3][2];      /* [outcome][front_face] */
    uint64_t metal[2];              /* fuzz == 0, fuzz > 0 */
    uint64_t path_end[4][2][2];     /* [cause][tainted: a record with pdf 0 / NaN or a non-finite weight][terminal radiance == (0, 0, 0)] */
} rto_shade_census;
void rto_census_enable(int on);     /* on != 0: zero the census and start counting; 0: stop (the counts stay readable) */
void rto_census_read(rto_shade_census *out);

/* CPU twin of rt_render (main.rs:109-162 threading scheme with n_threads workers). */
int rt_render_cpu(const rt_scene_desc *scene, const rt_camera *cam, const rt_params *params,
                  double *out_rgb_sum, rt_stats *stats, int n_threads);
void rto_write_color(const double rgb_sum[3], int32_t spp, uint8_t out[3]);
const char *rto_last_error(void);

int rto_hit(const rt_scene_desc *scene, uint32_t ref, const double ray[7], double t_min, double t_max,
            uint64_t rng_state, rto_hit_record *out, rt_stats *stats);
int rto_ray_color(const rt_scene_desc *scene, const double ray[7], const double background[3], double t_min,
                  int depth, uint64_t rng_state, double out_rgb[3], rt_stats *stats);
/* CPU twin of rt_radiance: out_rgb_sum[3 i ..] = 0 + L_0 + L_1 + ... over spp samples of ray i, sample s drawing from
 * path_key(rays[i].rng_state, 0, 0, s), each L one ray_color call; n_threads workers over contiguous sections of the rays.
 * stats (may be NULL): paths = n * spp and the summed counters of the calls. */
int rto_radiance(const rt_scene_desc *scene, const rt_radiance_ray *rays, uint64_t n, uint32_t spp, const double background[3],
                 double t_min, int depth, double *out_rgb_sum, rt_stats *stats, int n_threads);
int rto_get_ray(const rt_camera *cam, double s, double t, uint64_t rng_state, double out_ray[7]);
int rto_texture_value(const rt_scene_desc *scene, uint32_t tex, double u, double v, const double p[3], double out_rgb[3]);
double rto_perlin_noise(const rt_perlin *pl, const double p[3]);
double rto_perlin_turb(const rt_perlin *pl, const double p[3], int depth);
double rto_lights_pdf_value(const rt_scene_desc *scene, const double o[3], const double v[3]);
int rto_lights_random(const rt_scene_desc *scene, const double o[3], uint64_t rng_state, double out_dir[3]);
int rto_scatter(const rt_scene_desc *scene, uint32_t mat, const double ray_in[7], const rto_hit_record *rec_in,
                uint64_t rng_state, double out_ray[7], double out_attenuation[3], double out_emitted[3]);
double rto_math(int op, double a, double b);
/* 1 if this library was built with -DRTO_LIBM (`make libm`: the render path calls the platform libm). */
int rto_uses_libm(void);
/* 1 if this library was built with -DRTO_OWN_MATH (`make own`: oracle/rto_math.h instead of the product's rt_math.h). */
int rto_uses_own_math(void);
/* The transcendental as the render path of THIS build calls it (rt_math.h, or the platform libm under -DRTO_LIBM). */
double rto_path_math(int op, double a, double b);
void rto_math_array(int op, const double *a, const double *b, double *out, uint64_t n);
void rto_rng_u64(uint64_t state, uint64_t *out, uint64_t n);
void rto_rng_f64(uint64_t state, double *out, uint64_t n);
void rto_rng_range(uint64_t state, double lo, double hi, double *out, uint64_t n);
void rto_rng_index(uint64_t state, uint64_t bound, uint64_t *out, uint64_t n);
uint64_t rto_path_key(uint64_t seed, uint32_t frame, uint64_t pixel, uint32_t sample);

#ifdef __cplusplus
}
#endif
#endif
