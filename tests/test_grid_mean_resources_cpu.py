"""The tabulated mean went inside the two out-of-line mean functions of csrc/gpis_sdf.hpp and adds no kernel.  So every kernel of
the commit before the feature, except k_mean (the test surface of gpis_mean_batch, which learns the new type), must have kept its
VGPR count, VGPR spill count, scratch and LDS: profiles/r15_grid_mean_resources.json holds the table of the commit before the
feature ("before": every kernel) and of the feature ("after": every kernel too), both read from the built library the way
tests/test_kernel_resources.py reads it.

What is checked against the built library: (1) each kernel listed in "before", k_mean aside, is present with the figures of
"before"; (2) none of the feature's own names (grid_mean, tabulated, set_mean_grid) is a kernel symbol, and the record's "after"
lists exactly the kernels of "before".  A kernel a LATER change adds is in neither list and is none of this file's business.

    python tests/test_grid_mean_resources_cpu.py before|after path/to/libgpis_hip.so     # rewrites that half of the table
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TABLE = os.path.join(ROOT, "profiles", "r15_grid_mean_resources.json")
KEYS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
FREE = "k_mean"                    # the one kernel the feature changes
FEATURE_NAMES = ("grid_mean", "tabulated", "set_mean_grid")


def _is_free(name):
    return ("%d%s" % (len(FREE), FREE)) in name and "k_mean_color" not in name


def _table(lib):
    sys.path.insert(0, HERE)
    import test_kernel_resources as tkr
    return {name: {k: int(res[k]) for k in KEYS} for name, res in sorted(tkr._kernels(lib).items())}


@pytest.fixture(scope="module")
def tables(pkg):
    import test_kernel_resources as tkr
    if not os.path.exists(os.path.join(tkr.LLVM, "clang-offload-bundler")):
        pytest.skip("LLVM tools of the ROCm image")
    return json.load(open(TABLE)), _table(pkg.library_path())


def test_the_record_adds_no_kernel(tables):
    rec, _ = tables
    assert sorted(rec["after"]) == sorted(rec["before"]) and len(rec["before"]) >= 45
    assert sum(_is_free(n) for n in rec["before"]) == 1
    for name, res in rec["before"].items():
        if not _is_free(name):
            assert rec["after"][name] == res, (name, res, rec["after"][name])


def test_every_kernel_of_the_parent_keeps_its_resources(tables):
    rec, now = tables
    checked = 0
    for name, res in rec["before"].items():
        assert name in now, "a kernel of the parent is gone: %s" % name
        if _is_free(name):
            continue
        assert now[name] == res, (name, res, now[name])
        checked += 1
    assert checked >= 45


def test_the_feature_has_no_kernel_of_its_own(tables):
    _, now = tables
    own = [n for n in now if any(k in n for k in FEATURE_NAMES)]
    assert not own, own


if __name__ == "__main__":
    which, lib = sys.argv[1], sys.argv[2]
    assert which in ("before", "after")
    rec = json.load(open(TABLE)) if os.path.exists(TABLE) else {}
    rec[which] = _table(lib)
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    json.dump(rec, open(TABLE, "w"), indent=1, sort_keys=True)
    print("%s: %d kernels" % (which, len(rec[which])))
