"""The reference of RT_FLAG_SURFACES (include/rt2022.h): the oracle's feature composition on a copy of the scene whose media
never answer. No GPU is needed.

The copy: every desc.media[i].neg_inv_density set to -inf. ConstantMedium::hit then still queries its boundary, but
hit_distance = -inf * (ln(rnd) / ln(e)) is +inf (ln(rnd) < 0 for every rnd the generator gives), `hit_distance >
distance_inside_boundary` holds and the medium returns None — which is the flag's definition, up to what the boundary queries
count and the one word the medium draws, neither of which reaches a record: the stream behind world.hit is not used again.

The copy equals the definition ONLY while every distance_inside_boundary is finite: against +inf the comparison inf > inf is
false and the copy's medium would answer. So use it on well-formed views only (width, height >= 2, finite cameras). All
depths are finite on final_scene and cornell_smoke along the grid's paths (checked on the CPU)."""
import contextlib
import math

from test_features import oracle_features


@contextlib.contextmanager
def media_looked_through(desc):
    """Inside: every medium of `desc` has neg_inv_density = -inf. The values come back on exit, whatever happened."""
    saved = [desc.media[i].neg_inv_density for i in range(desc.n_media)]
    try:
        for i in range(desc.n_media):
            desc.media[i].neg_inv_density = -math.inf
        yield desc
    finally:
        for i, v in enumerate(saved):
            desc.media[i].neg_inv_density = v


def camera_words(seen):
    """The words the cameras drew in an oracle_features run: 2 + what rto_get_ray returned, summed over the samples."""
    return seen.draws - seen.medium_draws


def oracle_surface_features(O, desc, cam, params, rows, pixels=None):
    """oracle_features on the looked-through copy -> (records, the copy's summed rt_stats, Seen, the cameras' word count: what
    rng_draws must be under RT_FLAG_SURFACES)."""
    with media_looked_through(desc):
        out, st, seen = oracle_features(O, desc, cam, params, rows, pixels)
    return out, st, seen, camera_words(seen)
