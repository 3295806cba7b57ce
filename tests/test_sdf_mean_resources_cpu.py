"""The procedural SDF mean went into the all-features (`generic`) instance of the path section only.  Every other kernel must have
kept its register, spill, scratch and LDS figures: profiles/r14_sdf_mean_resources.json holds the table of the commit before the
feature ("before") and of the feature ("after"), both read from the built library the way tests/test_kernel_resources.py reads it.

    python tests/test_sdf_mean_resources_cpu.py before|after path/to/libgpis_hip.so     # rewrites that half of the table
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TABLE = os.path.join(ROOT, "profiles", "r14_sdf_mean_resources.json")
KEYS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
NEW_KERNELS = ("k_mean",)          # kernels the feature adds (substring of the mangled name, followed by its parameter list)


def _is_generic(name):
    return "7generic" in name          # an instance of namespace gpis::generic (Itanium mangling: <length><name>)


def _is_new(name):
    return any(("%d%s" % (len(k), k)) in name and "k_mean_color" not in name for k in NEW_KERNELS)


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


def test_other_kernels_keep_their_resources(tables):
    rec, now = tables
    before = rec["before"]
    checked = 0
    for name, res in now.items():
        if _is_generic(name) or _is_new(name):
            continue
        assert name in before, "a kernel the table of the parent does not know: %s" % name
        assert res == before[name], (name, before[name], res)
        checked += 1
    assert checked >= 40
    gone = [n for n in before if n not in now]
    assert not gone, gone


def test_generic_kernels_recorded_and_resident(tables):
    """The all-features instances are listed before and after; their scratch may rise (written down in the table), but each must
    still fit one wave per SIMD: at most 512 VGPRs (arch + accumulation) and the 64 KiB of LDS a workgroup can address."""
    rec, now = tables
    generic = {n: r for n, r in now.items() if _is_generic(n)}
    assert len(generic) >= 5
    for name, res in generic.items():
        assert name in rec["before"] and name in rec["after"], name
        assert res == rec["after"][name], (name, rec["after"][name], res)
        assert res["vgpr_count"] <= 512 and res["group_segment_fixed_size"] <= 64 * 1024, (name, res)


def test_new_kernels_are_the_listed_ones(tables):
    rec, now = tables
    added = sorted(n for n in now if n not in rec["before"])
    assert added and all(_is_new(n) for n in added), added


if __name__ == "__main__":
    which, lib = sys.argv[1], sys.argv[2]
    assert which in ("before", "after")
    rec = json.load(open(TABLE)) if os.path.exists(TABLE) else {}
    t = _table(lib)
    rec[which] = t if which == "before" else {n: r for n, r in t.items() if _is_generic(n) or _is_new(n)}
    if "before" in rec and "after" in rec:
        rec["generic_scratch_change"] = {n: [rec["before"][n]["private_segment_fixed_size"], r["private_segment_fixed_size"]]
                                         for n, r in rec["after"].items() if n in rec["before"]}
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    json.dump(rec, open(TABLE, "w"), indent=1, sort_keys=True)
    print("%s: %d kernels" % (which, len(rec[which])))
