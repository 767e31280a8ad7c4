"""include/smj_mapping.h (the mapping entry; smj_scanmatch.h includes it, smj_drive.h that one and so on up to smj.h) and the loader
agree, as tests/test_scanmatch_capi.py checks for smj_scanmatch.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

NAME, ENTRY = "smj_mapping.h", "smj_scan_to_map"


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(NAME, lib.MAPPING_EXPORTS, ENTRY)
    text = capi_check.header(NAME)
    macros = dict(re.findall(r"^#define\s+(SMJ_\w+)[ \t]*(\S*)$", text, flags=re.M))
    assert macros == {"SMJ_MAPPING_H": "", "SMJ_MAP_OK": "0", "SMJ_MAP_GATED": "1", "SMJ_MAP_OFF": "2", "SMJ_MAP_NO_CELL": "(-1073741824)"}
    assert "AN ENV IS INTEGRATED IFF ITS WORD IS 0" in text      # the header states the gate's rule


def test_smj_scanmatch_h_includes_it_once_after_its_declarations():
    text = capi_check.header(NAME)
    first_include = re.search(r"^#include.*$", text, flags=re.M).group(0)
    assert first_include == '#include "smj.h"'
    lines = capi_check.header("smj_scanmatch.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_mapping.h"')]
    assert len(inc) == 1
    closing = max(k for k, line in enumerate(lines) if line.strip() == "}")      # the end of extern "C"
    assert closing < inc[0] and lines[inc[0] + 1:] == ["#endif"] and lines[inc[0] - 1] == "#endif"
    includes = [line for line in lines if line.startswith("#include")]
    assert includes == ['#include "smj.h"', '#include "smj_mapping.h"']      # smj.h stays its first include
    others = ("smj_occupancy.h", "smj_distance.h", "smj_navigation.h", "smj_frontier.h", "smj_drive.h", "smj_pointcloud.h", "smj_heightmap.h", "smj_build.h")
    assert all(NAME not in capi_check.header(h) for h in others)


def test_smj_h_includes_are_unchanged():
    """A caller includes smj.h alone: the list of entry headers smj.h itself includes is what it was."""
    assert capi_check.smj_h_includes()[1] == ["smj_pointcloud.h", "smj_heightmap.h", "smj_occupancy.h"]


def test_constants_of_the_kernel_header():
    text = capi_check.kernel_header("smj_map.h")
    public = capi_check.header(NAME)
    found = re.findall(r"^#define\s+SMJ_MAP_(?:OK|GATED|OFF|NO_CELL)\s.*$", public, flags=re.M)
    assert len(found) == 4
    for m in found:      # token for token
        assert m in text, m
    assert "SMJ_MAP_MAX_RAYS = SMJ_MATCH_MAX_POINTS" in text and re.search(r"SMJ_MATCH_MAX_POINTS\s*=\s*1024", capi_check.kernel_header("smj_match.h"))
    occ = capi_check.kernel_header("smj_occ.h")
    assert re.search(r"SMJ_OCC_MAX_CELLS\s*=\s*65536", occ) and re.search(r"SMJ_OCC_MAX_STEPS\s*=\s*8192", occ)
    assert -(1 << 30) < -(1 << 21)      # SMJ_MAP_NO_CELL lies outside what a cell can take
    # the limits the public header states in words
    for phrase in ("nlidar <= 1024", "nx, ny >= 1 and nx ny <= 65536", "r_max / cell <= 8192", "gate_ld >= 1", "|fax|, |fay| <= 2^20", "|fbx - fax|, |fby - fay| <= 16384",
                   "cell finite and > 0", "0 <= r_min <= r_max"):
        assert phrase in public, phrase


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(NAME, lib.MAPPING_EXPORTS, ENTRY, 21)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry and its macros, and the matcher's beside them; so does one that
    includes smj_scanmatch.h or smj_mapping.h first."""
    body = ("int none = SMJ_MAP_NO_CELL;\n"
            "int f(smj_ctx* c, const void* scan, const void* pose, const int* best, void* hit, void* miss, void* info) {\n"
            "  return smj_scan_to_map(c, scan, 4096, 1, 0.2f, 5.0f, pose, best + 3, 4, -3.2f, -3.2f, 0.05f, 128, 128, 1, 1, hit, miss, info, 0, 0)\n"
            "         + SMJ_MAP_OK + SMJ_MAP_GATED + SMJ_MAP_OFF + SMJ_MATCH_OK; }\n")
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_scanmatch.h", "smj_mapping.h"))
