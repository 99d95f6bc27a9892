"""numpy restatement of the feature merge and resolve (include/rt2022.h, rt_adaptive_merge_features_device /
rt_adaptive_resolve_features_device). Not a test: the reference the tests compare the kernels with, bit for bit. A record is
eight float64 (albedo 3, normal 3, depth, hits); every operation is a single IEEE + / * of numpy float64 in the header's order."""
import numpy as np


def merge(entry_features, units, offsets, acc):
    """In place on acc [n, 8] (float64): acc_f = acc_f + E[offsets[b] + k].f for k < units[b], in order. Pixels with 0 units
    are not touched; no sample count is."""
    E = np.asarray(entry_features).view(np.float64).reshape(-1, 8)
    off = np.asarray(offsets, dtype=np.uint64)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in np.nonzero(np.asarray(units))[0]:
            for k in range(int(units[b])):
                acc[b] = acc[b] + E[int(off[b]) + k]              # (elementwise: eight independent adds)


def resolve(acc, acc_n, spp_out):
    """-> [n, 8]: (acc_f / acc_n[b]) * spp_out on all eight fields; acc_n == 0 gives NaN (or inf * spp_out where acc_f != 0:
    IEEE's own answers)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (np.asarray(acc, dtype=np.float64).reshape(-1, 8) / np.asarray(acc_n, dtype=np.float64).reshape(-1)[:, None]) * np.float64(spp_out)
