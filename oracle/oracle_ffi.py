"""ctypes binding of the CPU oracle (oracle/librt_oracle.so).

TEST INFRASTRUCTURE: import this only from tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg. The product package never imports it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from raytracer_2022_amd import _ffi as F

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librt_oracle.so")

RTO_SIN, RTO_COS, RTO_ACOS, RTO_ATAN2, RTO_LOG, RTO_SQRT, RTO_DIV = range(7)


class rto_hit_record(C.Structure):
    _fields_ = [("hit", C.c_int32), ("front_face", C.c_int32), ("p", C.c_double * 3), ("normal", C.c_double * 3),
                ("t", C.c_double), ("u", C.c_double), ("v", C.c_double), ("mat", C.c_uint32), ("rng_draws", C.c_uint32)]


class rto_shade_census(C.Structure):
    """rt_oracle.h: the shade census. Indices: ARMS, MIX, DIEL, END below; a trailing [2] is (no / back face, yes / front face)."""
    _fields_ = [("scatter", C.c_uint64 * 2 * 5 * 5 * 5), ("emitted", C.c_uint64 * 2 * 4), ("light_draw", C.c_uint64 * 6),
                ("mixture_choice", C.c_uint64 * 3), ("light_pdf", C.c_uint64 * 2 * 6), ("dielectric", C.c_uint64 * 2 * 3),
                ("metal", C.c_uint64 * 2), ("path_end", C.c_uint64 * 2 * 2 * 4)]


ARM_SPHERE, ARM_RECT_XY, ARM_RECT_XZ, ARM_RECT_YZ, ARM_FLIPPED, ARM_OTHER = range(6)
TEX_NONE = 4
MIX_LIGHT, MIX_COSINE, MIX_COSINE_ONLY = range(3)
DIEL_CANNOT_REFRACT, DIEL_SCHLICK, DIEL_REFRACT = range(3)
END_MISS, END_LIGHT_FRONT, END_LIGHT_BACK, END_DEPTH = range(4)


LIBM_LIB_PATH = os.path.join(_HERE, "librt_oracle_libm.so")


def build(target=None):
    subprocess.check_call(["make", "-s", "-C", _HERE] + ([target] if target else []))


_lib = None
_lib_libm = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build()
    _lib = _bind(C.CDLL(LIB_PATH))
    return _lib


def lib_libm():
    """The -DRTO_LIBM build of the same restatement: the render path's sin / cos / acos / atan2 / log are the
    platform libm's (what the Rust reference links), not rt_math.h's. For tools/libm_sensitivity.py only."""
    global _lib_libm
    if _lib_libm is not None:
        return _lib_libm
    if not os.path.exists(LIBM_LIB_PATH):
        build("libm")
    _lib_libm = _bind(C.CDLL(LIBM_LIB_PATH))
    assert _lib_libm.rto_uses_libm() == 1 and lib().rto_uses_libm() == 0
    return _lib_libm


OWN_LIB_PATH = os.path.join(_HERE, "librt_oracle_own.so")
_lib_own = None


def lib_own():
    """The -DRTO_OWN_MATH build: rt_oracle.cpp against oracle/rto_math.h (the oracle's own vectors, RNG conversions and casts) and
    the platform libm — no arithmetic shared with the product. For tests/test_oracle_own_math.py only."""
    global _lib_own
    if _lib_own is not None:
        return _lib_own
    if not os.path.exists(OWN_LIB_PATH):
        build("own")
    _lib_own = _bind(C.CDLL(OWN_LIB_PATH))
    assert _lib_own.rto_uses_own_math() == 1 and _lib_own.rto_uses_libm() == 1 and lib().rto_uses_own_math() == 0
    return _lib_own


def _bind(L):
    P, dbl, u64, u32 = C.POINTER, C.c_double, C.c_uint64, C.c_uint32
    L.rt_render_cpu.argtypes = [P(F.rt_scene_desc), P(F.rt_camera), P(F.rt_params), P(dbl), P(F.rt_stats), C.c_int]
    L.rto_write_color.argtypes = [P(dbl), C.c_int32, P(C.c_uint8)]
    L.rto_write_color.restype = None
    L.rto_last_error.restype = C.c_char_p
    L.rto_hit.argtypes = [P(F.rt_scene_desc), u32, P(dbl), dbl, dbl, u64, P(rto_hit_record), P(F.rt_stats)]
    L.rto_ray_color.argtypes = [P(F.rt_scene_desc), P(dbl), P(dbl), dbl, C.c_int, u64, P(dbl), P(F.rt_stats)]
    L.rto_radiance.argtypes = [P(F.rt_scene_desc), C.c_void_p, u64, u32, P(dbl), dbl, C.c_int, C.c_void_p, P(F.rt_stats), C.c_int]
    L.rto_get_ray.argtypes = [P(F.rt_camera), dbl, dbl, u64, P(dbl)]
    L.rto_texture_value.argtypes = [P(F.rt_scene_desc), u32, dbl, dbl, P(dbl), P(dbl)]
    L.rto_perlin_noise.argtypes = [P(F.rt_perlin), P(dbl)]
    L.rto_perlin_noise.restype = dbl
    L.rto_perlin_turb.argtypes = [P(F.rt_perlin), P(dbl), C.c_int]
    L.rto_perlin_turb.restype = dbl
    L.rto_lights_pdf_value.argtypes = [P(F.rt_scene_desc), P(dbl), P(dbl)]
    L.rto_lights_pdf_value.restype = dbl
    L.rto_lights_random.argtypes = [P(F.rt_scene_desc), P(dbl), u64, P(dbl)]
    L.rto_scatter.argtypes = [P(F.rt_scene_desc), u32, P(dbl), P(rto_hit_record), u64, P(dbl), P(dbl), P(dbl)]
    L.rto_math.argtypes = [C.c_int, dbl, dbl]
    L.rto_math.restype = dbl
    L.rto_math_array.argtypes = [C.c_int, P(dbl), P(dbl), P(dbl), u64]
    L.rto_math_array.restype = None
    L.rto_rng_u64.argtypes = [u64, P(u64), u64]
    L.rto_rng_f64.argtypes = [u64, P(dbl), u64]
    L.rto_rng_range.argtypes = [u64, dbl, dbl, P(dbl), u64]
    L.rto_rng_index.argtypes = [u64, u64, P(u64), u64]
    for f in (L.rto_rng_u64, L.rto_rng_f64, L.rto_rng_range, L.rto_rng_index):
        f.restype = None
    L.rto_path_key.argtypes = [u64, u32, u64, u32]
    L.rto_path_key.restype = u64
    L.rto_uses_libm.restype = C.c_int
    L.rto_uses_own_math.restype = C.c_int
    L.rto_path_math.argtypes = [C.c_int, dbl, dbl]
    L.rto_path_math.restype = dbl
    L.rto_census_enable.argtypes = [C.c_int]
    L.rto_census_enable.restype = None
    L.rto_census_read.argtypes = [P(rto_shade_census)]
    L.rto_census_read.restype = None
    return L


def _d(v):
    return (C.c_double * len(v))(*[float(x) for x in v])


def render_cpu(desc, cam, params, row_ids, n_threads=1, want_stats=False, libm=False, own=False):
    """rt_render_cpu → (n_rows, width, 3) float64 sums [, rt_stats]. libm=True: the -DRTO_LIBM build (lib_libm); own=True: the
    -DRTO_OWN_MATH build (lib_own)."""
    L = lib_own() if own else lib_libm() if libm else lib()
    rows = np.ascontiguousarray(row_ids, dtype=np.uint32)
    p = F.rt_params.from_buffer_copy(params)
    p.n_rows = len(rows)
    p.row_ids = rows.ctypes.data
    out = np.empty((len(rows), p.width, 3), dtype=np.float64)
    st = F.rt_stats()
    rc = L.rt_render_cpu(C.byref(desc), C.byref(cam), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)),
                         C.byref(st), n_threads)
    if rc < 0:
        raise RuntimeError("oracle error %d: %s" % (rc, L.rto_last_error().decode()))
    return (out, st) if want_stats else out


def census_begin():
    """Zero the shade census and switch it on: render_cpu and ray_color calls count into it until census_end()."""
    lib().rto_census_enable(1)


def census_end():
    """Switch the shade census off → {field: uint64 array} of rto_shade_census (scatter[mat][leaf][top][front], ...)."""
    lib().rto_census_enable(0)
    c = rto_shade_census()
    lib().rto_census_read(C.byref(c))
    return {name: np.ctypeslib.as_array(getattr(c, name)).astype(np.uint64) for name, _ in rto_shade_census._fields_}


def write_color(rgb_sum, spp):
    sums = np.ascontiguousarray(rgb_sum, dtype=np.float64).reshape(-1, 3)
    out = np.zeros((sums.shape[0], 3), dtype=np.uint8)
    for i in range(sums.shape[0]):
        lib().rto_write_color(sums[i].ctypes.data_as(C.POINTER(C.c_double)), spp, out[i].ctypes.data_as(C.POINTER(C.c_uint8)))
    return out.reshape(np.shape(rgb_sum))


def hit(desc, ref, orig, direction, tm=0.0, t_min=0.001, t_max=float("inf"), rng_state=1, stats=None):
    rec = rto_hit_record()
    ray = _d(list(orig) + list(direction) + [tm])
    lib().rto_hit(C.byref(desc), ref, ray, t_min, t_max, rng_state, C.byref(rec), C.byref(stats) if stats is not None else None)
    return rec


def ray_color(desc, orig, direction, tm=0.0, background=(0, 0, 0), t_min=0.001, depth=50, rng_state=1, stats=None):
    out = (C.c_double * 3)()
    ray = _d(list(orig) + list(direction) + [tm])
    lib().rto_ray_color(C.byref(desc), ray, _d(background), t_min, depth, rng_state, out,
                        C.byref(stats) if stats is not None else None)
    return np.array(out[:])


def radiance(desc, rays, spp=1, background=(0, 0, 0), t_min=0.001, depth=50, n_threads=1, want_stats=False):
    """rto_radiance, the CPU twin of rt_radiance: `rays` an array of RADIANCE_RAY_DTYPE records → (n, 3) float64 sums over
    spp samples, sample s of ray i drawing from path_key(rng_state_i, 0, 0, s) [, rt_stats with the summed counters]."""
    r = np.ascontiguousarray(rays, dtype=F.RADIANCE_RAY_DTYPE)
    out = np.zeros((len(r), 3), dtype=np.float64)
    st = F.rt_stats()
    rc = lib().rto_radiance(C.byref(desc), r.ctypes.data if len(r) else None, len(r), spp, _d(background), t_min, depth,
                            out.ctypes.data if len(r) else None, C.byref(st), n_threads)
    if rc < 0:
        raise RuntimeError("oracle error %d: %s" % (rc, lib().rto_last_error().decode()))
    return (out, st) if want_stats else out


def texture_value(desc, tex, u, v, p):
    """Texture::value(u, v, p) of texture `tex` (texture/mod.rs:25-139) → (r, g, b)."""
    out = (C.c_double * 3)()
    rc = lib().rto_texture_value(C.byref(desc), tex, float(u), float(v), _d(p), out)
    if rc != 0:
        raise RuntimeError("rto_texture_value: %s" % lib().rto_last_error().decode())
    return np.array(out[:])


def math_array(op, a, b=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64)
        bp = b.ctypes.data_as(C.POINTER(C.c_double))
    lib().rto_math_array(op, a.ctypes.data_as(C.POINTER(C.c_double)), bp, out.ctypes.data_as(C.POINTER(C.c_double)), a.size)
    return out
