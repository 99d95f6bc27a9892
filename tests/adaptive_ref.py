"""numpy restatement of the adaptive planner, merge and resolve (include/rt2022.h, rt_adaptive_*). Not a test: the reference
the tests compare the kernels with, bit for bit. Every double operation is a single IEEE * / + of numpy float64 in the
header's order; integers are uint32 / uint64 with wrap-around."""
import numpy as np


def plan(err, width, height, scale, max_units, first_frame=0, row_ids=None, capacity=None):
    """-> (units uint32 [n], offsets uint64 [n + 1], entries uint64 [total] or None when total > capacity, total)."""
    e = np.asarray(err, dtype=np.float64).reshape(-1)
    n = width * height
    assert e.size == n
    units = np.zeros(n, dtype=np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = e * np.float64(scale)
    for b in range(n):
        tb = t[b]
        if not (tb >= 1.0):
            units[b] = 0
        elif tb >= np.float64(max_units):
            units[b] = max_units
        else:
            units[b] = np.uint32(int(tb))                     # (truncation: tb is finite and below 2^32 here)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(units.astype(np.uint64), dtype=np.uint64)
    total = int(offsets[n])
    if capacity is not None and total > capacity:
        return units, offsets, None, total
    rows = np.arange(height, dtype=np.uint64) if row_ids is None else np.asarray(row_ids, dtype=np.uint64)
    entries = np.zeros(total, dtype=np.uint64)
    mask = (1 << 64) - 1
    for b in range(n):
        r, x = divmod(b, width)
        pixel = int(rows[r]) * width + x
        for k in range(int(units[b])):
            entries[int(offsets[b]) + k] = ((first_frame + k) * (width * height) + pixel) & mask
    return units, offsets, entries, total


def merge(entry_sums, units, offsets, spp, acc_sum, acc_n):
    """In place on acc_sum [n, 3] and acc_n [n] (float64)."""
    E = np.asarray(entry_sums, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(len(units)):
            u = int(units[b])
            if u == 0:
                continue
            for k in range(u):
                for c in range(3):
                    acc_sum[b, c] = acc_sum[b, c] + E[int(offsets[b]) + k, c]
            acc_n[b] = acc_n[b] + np.float64(u * spp)


def resolve(acc_sum, acc_n, spp_out):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (np.asarray(acc_sum, dtype=np.float64) / np.asarray(acc_n, dtype=np.float64)[:, None]) * np.float64(spp_out)
