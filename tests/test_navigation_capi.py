"""include/smj_navigation.h (the navigation-field entry; smj_distance.h includes it, smj_occupancy.h that one and smj.h that one) and
the loader agree, as tests/test_distance_capi.py checks for smj_distance.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

NAME, ENTRY = "smj_navigation.h", "smj_costmap_to_navigation"


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(NAME, lib.NAVIGATION_EXPORTS, ENTRY)
    text = capi_check.header(NAME)
    assert int(re.search(r"#define\s+SMJ_NAV_NONE\s+\(1 << (\d+)\)", text).group(1)) == 30 and lib.NAV_NONE == 1 << 30
    assert len(re.findall(r"^#define\s+SMJ_", text, flags=re.M)) == 2      # the include guard and SMJ_NAV_NONE
    assert "467 919 900" in text and 65535 * 7 * 1020 == 467919900 < 1 << 30      # the header states the largest finite potential


def test_smj_distance_h_includes_it_after_its_declarations():
    text = capi_check.header(NAME)
    first_include = re.search(r"^#include.*$", text, flags=re.M).group(0)
    assert first_include == '#include "smj.h"'
    lines = capi_check.header("smj_distance.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_navigation.h"')]
    assert len(inc) == 1
    closing = max(k for k, line in enumerate(lines) if line.strip() == "}")      # the end of extern "C"
    assert closing < inc[0] and lines[inc[0] + 1:] == ["#endif"] and lines[inc[0] - 1] == "#endif"
    assert NAME not in capi_check.smj_h_includes()[1] and NAME not in capi_check.header("smj_occupancy.h")


def test_constants_of_the_kernel_header():
    text = capi_check.kernel_header("smj_nav.h")
    assert re.search(r"#define\s+SMJ_NAV_NONE\s+\(1 << 30\)", text)
    assert int(re.search(r"SMJ_NAV_MAX_CELLS\s*=\s*(\d+)", text).group(1)) == 65536
    assert int(re.search(r"SMJ_NAV_MAX_SIDE\s*=\s*(\d+)", text).group(1)) == 4096
    assert int(re.search(r"SMJ_NAV_MAX_GOALS\s*=\s*(\d+)", text).group(1)) == 64
    assert int(re.search(r"SMJ_NAV_LDS_CELLS\s*=\s*(\d+)", text).group(1)) == 16384      # int32 potentials: 64 KiB of LDS; tests/test_gpu_navigation.py straddles it


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(NAME, lib.NAVIGATION_EXPORTS, ENTRY, 11)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry and SMJ_NAV_NONE; so does one that includes smj_distance.h or
    smj_navigation.h first."""
    body = ("int f(smj_ctx* c, const void* k, const void* g, void* p, void* n) { return smj_costmap_to_navigation(c, k, g, 1, 128, 128, 253, 50, p, n, 0) "
            "+ (SMJ_NAV_NONE == 1073741824 ? 0 : 1) + (SMJ_DIST_NONE == SMJ_NAV_NONE ? 0 : 1); }\n")
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_distance.h", "smj_navigation.h"))
