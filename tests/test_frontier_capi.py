"""include/smj_frontier.h (the frontier entry; smj_navigation.h includes it, smj_distance.h that one, smj_occupancy.h that one and smj.h
that one) and the loader agree, as tests/test_navigation_capi.py checks for smj_navigation.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

NAME, ENTRY = "smj_frontier.h", "smj_occupancy_to_frontiers"


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(NAME, lib.FRONTIER_EXPORTS, ENTRY)
    text = capi_check.header(NAME)
    assert len(re.findall(r"^#define\s+SMJ_", text, flags=re.M)) == 1      # the include guard
    assert "65536 * 4095 < 2^28" in text and 65536 * 4095 < 1 << 28      # the header states the largest coordinate sum


def test_smj_navigation_h_includes_it_after_its_declarations():
    text = capi_check.header(NAME)
    first_include = re.search(r"^#include.*$", text, flags=re.M).group(0)
    assert first_include == '#include "smj.h"'
    lines = capi_check.header("smj_navigation.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_frontier.h"')]
    assert len(inc) == 1
    closing = max(k for k, line in enumerate(lines) if line.strip() == "}")      # the end of extern "C"
    assert closing < inc[0] and lines[inc[0] + 1:] == ["#endif"] and lines[inc[0] - 1] == "#endif"
    assert NAME not in capi_check.smj_h_includes()[1]
    assert NAME not in capi_check.header("smj_occupancy.h") and NAME not in capi_check.header("smj_distance.h")


def test_constants_of_the_kernel_header():
    text = capi_check.kernel_header("smj_front.h")
    nav = capi_check.kernel_header("smj_nav.h")
    for name, value in (("MAX_CELLS", 65536), ("MAX_SIDE", 4096)):      # the navigation entry's limits: its goal_dev is fed from here
        assert int(re.search(rf"SMJ_FRONT_{name}\s*=\s*(\d+)", text).group(1)) == value == int(re.search(rf"SMJ_NAV_{name}\s*=\s*(\d+)", nav).group(1))
    assert int(re.search(r"SMJ_FRONT_MAX_REGIONS\s*=\s*(\d+)", text).group(1)) == 64 == int(re.search(r"SMJ_NAV_MAX_GOALS\s*=\s*(\d+)", nav).group(1))
    lds = int(re.search(r"SMJ_FRONT_LDS_CELLS\s*=\s*(\d+)", text).group(1))
    assert lds == 16384 and 2 * (4 * lds + 4096) <= 160 * 1024      # int32 labels: two workgroups per CU; tests/test_gpu_frontier.py straddles it
    assert re.search(r"SMJ_FRONT_CHOSEN\s*=\s*-\(1 << 20\)", text) and 1 << 20 > 65536 + 1      # row codes lie below every size code


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(NAME, lib.FRONTIER_EXPORTS, ENTRY, 15)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry; so does one that includes smj_navigation.h or smj_frontier.h
    first."""
    body = ("int f(smj_ctx* c, const void* h, const void* m, void* l, void* g) { return smj_occupancy_to_frontiers(c, h, m, 0, 128, 128, 1, 253, 4, 16, "
            "l, g, 0, 0, 0) + smj_costmap_to_navigation(c, 0, g, 16, 128, 128, 253, 50, l, 0, 0); }\n")
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_navigation.h", "smj_frontier.h"))
