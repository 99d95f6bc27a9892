"""The redraw loops of the path RNG cost ONE draw where the first try is accepted (CPU test; needs hipcc, not a GPU).

The generator is counter based (rt_math.h: draw i = mix64(s + i * gamma)), so the device compiler turns a plain
`for (tries < RT_MAX_REJECT) { draw; if (accepted) return; }` into a block of four draws side by side followed by a
pick of the first accepted one: every gen_range / gen_index then pays four draws although the redraw (almost) never
fires. rt_math.h therefore peels the first draw out of the loop. This test compiles three tiny kernels with the
library's flags to gfx950 assembly and walks each from its entry: every stretch up to the next conditional branch
that belongs to a call site must hold exactly one draw (one mix64: one 64-bit `>> 30`, one `>> 27`, two 64-bit
multiplications by the mixer's constants). tools/isa_draws.py is the same census over the real kernels.
"""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raytracer_2022_amd", "csrc")

_spec = importlib.util.spec_from_file_location("isa_draws", os.path.join(ROOT, "tools", "isa_draws.py"))
isa_draws = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_draws)

pytestmark = pytest.mark.skipif(not (os.path.exists(isa_draws.HIPCC) or shutil.which("hipcc")), reason="needs hipcc (no GPU)")

SOURCE = r"""
#include "hip/pt_common.hpp"
using namespace rt2022;
extern "C" __global__ void k_range(uint64_t *st, double *out) {
    Rng r(st[threadIdx.x]);
    out[threadIdx.x] = r.gen_range(-1.0, 1.0);
    st[threadIdx.x] = r.s + r.draws;
}
extern "C" __global__ void k_index(uint64_t *st, uint64_t n, uint64_t *out) {
    Rng r(st[threadIdx.x]);
    out[threadIdx.x] = r.gen_index(n);
    st[threadIdx.x] = r.s + r.draws;
}
extern "C" __global__ void k_sphere(uint64_t *st, double *out) {
    Rng r(st[threadIdx.x]);
    Vec3 p = random_in_unit_sphere(r);
    out[3 * threadIdx.x] = p.x; out[3 * threadIdx.x + 1] = p.y; out[3 * threadIdx.x + 2] = p.z;
    st[threadIdx.x] = r.s + r.draws;
}
"""

SHR30 = re.compile(r"^v_lshrrev_b64\s+v\[\d+:\d+\],\s*30,")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rng_isa")
    src = tmp / "rng_sites.hip"
    src.write_text(SOURCE)
    hipcc = isa_draws.HIPCC if os.path.exists(isa_draws.HIPCC) else shutil.which("hipcc")
    p = subprocess.run([hipcc] + isa_draws.FLAGS + ["-I", CSRC, "-o", str(tmp / "rng_sites.s"), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return isa_draws.kernels((tmp / "rng_sites.s").read_text())


def stretches(body):
    """The kernel's instructions in layout order from its entry, cut after every conditional branch."""
    out = [[]]
    for _, _, insns in isa_draws.blocks(body):
        for i in insns:
            out[-1].append(i)
            if i.startswith("s_cbranch"):
                out.append([])
    return out


@pytest.mark.parametrize("name,sites,mantissa", [("k_range", 1, 1), ("k_index", 1, 0), ("k_sphere", 3, 1)])
def test_accepted_first_try_path_holds_one_draw_per_call(kernels, name, sites, mantissa):
    st = stretches(kernels[name])
    assert len(st) > sites, "no conditional branch after the first draw: the redraw loop has gone missing"
    for n in range(sites):
        c = isa_draws.census(st[n])
        first_steps = sum(1 for i in st[n] if SHR30.match(i))
        print("%s call site %d: %d instructions, %d vector, draws %d, first mixer steps %d, v_mad_u64_u32 %d, mantissa ors %d"
              % (name, n, c["all"], c["valu"], c["draws"], first_steps, c["mad"], c["or3ff"]))
        assert c["draws"] == 1 and first_steps == 1, "call site %d of %s computes %d draws before it looks at the first" % (n, name, max(c["draws"], first_steps))
        assert c["or3ff"] == mantissa
        # two 64-bit multiplications per mix64; gen_index adds its widening multiply (at most one v_mad_u64_u32 per 32-bit partial product)
        assert 2 <= c["mad"] <= (2 if mantissa else 2 + 4)
    # no call, no scratch: the redraws stay in the function (a call would force the generator's state through memory)
    text = "\n".join(kernels[name])
    assert "s_swappc" not in text and "scratch_" not in text
