"""The neural SDF mean adds kernels and touches none: its evaluator is in csrc/gpis_nn_mean.hpp, which only gpis_hip.hip includes, and
the march reads the baked voxels through the tabulated mean that was there before.  profiles/r16_nn_mean_resources.json holds the
table of the commit before the feature ("before": every kernel) and the feature's own kernels ("new"), both read from the built
library the way tests/test_kernel_resources.py reads it.

Checked against the built library: (1) every kernel of "before" is present with the figures of "before", the older k_mean included;
(2) the kernels "before" lacks are forms of k_mean ("the mean at n points" over a network: points or lattice, by activation
storage), exactly the recorded ones, with the recorded figures; (3) each fits one workgroup: at most 64 KiB of LDS, at most 512
VGPRs, and the forms that keep activations in LDS spill nothing.

    python tests/test_nn_mean_resources_cpu.py before|new path/to/libgpis_hip.so     # rewrites that half of the table
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TABLE = os.path.join(ROOT, "profiles", "r16_nn_mean_resources.json")
KEYS = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
NETWORK_ARG = "N4gpis2nn3NetE"         # gpis::nn::Net, the first parameter of every network kernel (Itanium mangling)


def _is_network_kernel(name):
    return "6k_mean" in name and "k_mean_color" not in name and NETWORK_ARG in name


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


def test_every_kernel_of_the_parent_keeps_its_resources(tables):
    rec, now = tables
    assert len(rec["before"]) >= 45 and not any(_is_network_kernel(n) for n in rec["before"])
    for name, res in rec["before"].items():
        assert name in now, "a kernel of the parent is gone: %s" % name
        assert now[name] == res, (name, res, now[name])


def test_the_new_kernels_are_the_recorded_k_mean_forms(tables):
    rec, now = tables
    added = sorted(n for n in now if n not in rec["before"] and _is_network_kernel(n))
    assert added == sorted(rec["new"]) and len(added) == 6, added          # points and lattice x LDS 32, LDS 64, global workspace
    other = [n for n in now if n not in rec["before"] and "6k_mean" in n and not _is_network_kernel(n)]
    assert not other, other
    for name in added:
        assert now[name] == rec["new"][name], (name, rec["new"][name], now[name])


def test_the_new_kernels_fit_one_workgroup(tables):
    _, now = tables
    lds = {}
    for name, res in now.items():
        if not _is_network_kernel(name):
            continue
        assert res["group_segment_fixed_size"] <= 64 * 1024 and res["vgpr_count"] <= 512, (name, res)
        if res["group_segment_fixed_size"]:
            assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, (name, res)
        lds.setdefault(res["group_segment_fixed_size"], []).append(name)
    # two activation buffers of 32 / 64 doubles per lane of a 64-lane workgroup, or none (the global workspace): two kernels each
    assert sorted(lds) == [0, 2 * 32 * 64 * 8, 2 * 64 * 64 * 8] and all(len(v) == 2 for v in lds.values()), lds


if __name__ == "__main__":
    which, lib = sys.argv[1], sys.argv[2]
    assert which in ("before", "new")
    rec = json.load(open(TABLE)) if os.path.exists(TABLE) else {}
    t = _table(lib)
    rec[which] = {n: r for n, r in t.items() if _is_network_kernel(n) == (which == "new")}
    os.makedirs(os.path.dirname(TABLE), exist_ok=True)
    json.dump(rec, open(TABLE, "w"), indent=1, sort_keys=True)
    print("%s: %d kernels" % (which, len(rec[which])))
