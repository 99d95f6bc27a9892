"""The six feature calls name the same fault of every pair of faulty arguments as the build on which each call still had its
own argument check (tests/features_fault_pairs.py: the table; tests/golden/features_fault_pairs.json: that build's answers).
No compute calls: runs without a GPU."""
import json

import pytest

import features_fault_pairs as T


@pytest.fixture(scope="module")
def recorded():
    with open(T.GOLDEN) as f:
        return json.load(f)


def test_the_record_covers_the_table(recorded):
    """Every entry point, every pair of faults it can show — and every fault but the null scene is the one named for some pair, so
    that none of the table's faults has gone dead (a fault no call ever names would pin nothing)."""
    assert sorted(recorded) == sorted(T.ENTRIES)
    for entry in T.ENTRIES:
        assert sorted(recorded[entry]) == sorted("+".join(p) for p in T.pairs(entry)), entry
        assert len(T.pairs(entry)) >= 15, entry                                 # (rt_features_rays: 6 faults, 15 pairs; rt_features_device: 9, 34)
    said = " ".join(msg for entry in T.ENTRIES for _, msg in recorded[entry].values())
    assert "null scene" not in said                                             # (the scene comes last: beside any other fault it is never named)
    for words in ("the ray buffer must be 16-byte aligned", "the output must be 16-byte aligned", "4-byte aligned", "8-byte aligned", "too large", "null output", "null row_ids",
                  "null id or output buffer", "null ray or output buffer", "flag bits", "null camera", "null params"):
        assert words in said, words


@pytest.mark.parametrize("entry", T.ENTRIES)
def test_each_pair_of_faults_names_the_fault_it_always_named(rt, recorded, entry):
    from raytracer_2022_amd import _ffi as F
    for pair in T.pairs(entry):
        rc, msg = T.call(rt, entry, pair)
        want_rc, want_msg = recorded[entry]["+".join(pair)]
        assert want_rc == F.RT_ERR_INVALID and want_msg.startswith(entry + ": "), (pair, want_msg)     # (the record itself)
        assert (rc, msg) == (want_rc, want_msg), pair
