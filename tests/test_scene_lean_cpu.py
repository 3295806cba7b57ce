"""Host-only checks of the Lambert frame driver's option (no GPU needed)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_option_ids_match_header(pkg):
    header = open(os.path.join(ROOT, "include", "gpis.h")).read()
    ids = {n.lower(): int(v) for n, v in re.findall(r"GPIS_OPT_([A-Z0-9_]+) = (\d+)", header)}
    assert ids["scene_exit_state"] == 9
    assert pkg.Medium.OPTIONS == ids
