#!/usr/bin/env python3
"""One line per scene and ray family of the oracle's hit records (rto_hit, and the albedo rule by rto_texture_value) — and, with
--gpu, of rt_intersect's rt_hit — against the BVH-free record reference of tests/brute_records.py: rays, records compared, media
records, the worst error / tolerance of p, normal, u, v and the texture value, and the rays in each of the new classes. Then the
worst ratio per field and scene. profiles/brute_records.log is this tool's output with --gpu.

    python tools/brute_records_report.py [--gpu] [scene ...]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import brute_hits as B          # noqa: E402
import brute_records as BR      # noqa: E402
import brute_scenes as S        # noqa: E402

SCENES = ["every_kind", "cornell_box", "cornell_smoke", "final_scene", "earth", "two_perlin_spheres", "wwscene", "mover_records"]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gpu", action="store_true", help="also run rt_intersect on the current HIP device")
    ap.add_argument("scenes", nargs="*", default=SCENES)
    a = ap.parse_args()
    import raytracer_2022_amd as rt
    from raytracer_2022_amd import _ffi as F
    from oracle import oracle_ffi as O
    if a.gpu:
        import torch
        torch.zeros(1, device="cuda")
    failures, table = 0, {}
    for name in a.scenes:
        d, cam = S.mover_records() if name == "mover_records" else S.make(name)
        sc, sh = B.Scene(d), BR.Shading(d)
        dev = rt.DeviceScene(d) if a.gpu else None
        seed = 700 + len(name)
        for family, rays in S.families(B, sc, cam, seed).items():
            ans = B.solve(sc, rays["origin"], rays["direction"], rays["time"], rays["t_min"], rays["t_max"])
            R = BR.records(sc, rays, ans)
            want = BR.albedo_ref(sh, R.mat, R.front, R.u, R.v, R.p)
            want.skip = want.skip | R.face_ambiguous
            results = [("oracle", S.oracle_records(O, d, rays))]
            if dev is not None:
                got = dev.intersect(np.ascontiguousarray(rays, dtype=F.QUERY_RAY_DTYPE))
                results.append(("hip", {k: got[k] for k in S.RECORD_FIELDS}))
            for who, got in results:
                ta = BR.compare(sc, rays, ans, R, got, got_value=S.oracle_albedo(O, d, got), want_value=want)
                print(ta.line(name, family, who), flush=True)
                for i, what in ta.failures[:3]:
                    print("    ray %d: %s" % (i, what))
                failures += len(ta.failures)
                row = table.setdefault((name, who), {f: 0.0 for f in BR.FIELDS})
                for f in BR.FIELDS:
                    row[f] = max(row[f], ta.worst[f])
    print("\nworst error / tolerance per scene (front and mat: 1 = a mismatch)")
    for (name, who), row in table.items():
        print("%-22s %-6s %s" % (name, who, " ".join("%s %.3e" % (f, row[f]) for f in BR.FIELDS)))
    print("worst ratio overall %.3e; failures %d" % (max(max(r.values()) for r in table.values()), failures))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
