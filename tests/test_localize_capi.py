"""include/smj_localize.h (the particle-filter entry; smj_mapping.h includes it, smj_scanmatch.h that one and so on up to smj.h) and
the loader agree, as tests/test_mapping_capi.py checks for smj_mapping.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

NAME, ENTRY = "smj_localize.h", "smj_scan_to_particles"


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(NAME, lib.LOCALIZE_EXPORTS, ENTRY)
    text = capi_check.header(NAME)
    macros = dict(re.findall(r"^#define\s+(SMJ_\w+)[ \t]*(\S*)$", text, flags=re.M))
    assert macros == {"SMJ_LOCALIZE_H": "", "SMJ_MCL_OK": "0", "SMJ_MCL_FEW": "1", "SMJ_MCL_LOST": "2"}
    for phrase in ("AMONG EQUAL S THE SMALLEST j WINS", "THE ANCESTOR OF SLOT k IS THE SMALLEST j WITH C_j > u_k", "EVERYTHING BELOW IS INTEGERS"):
        assert phrase in text, phrase      # the header states the rules


def test_smj_mapping_h_includes_it_once_after_its_declarations():
    text = capi_check.header(NAME)
    first_include = re.search(r"^#include.*$", text, flags=re.M).group(0)
    assert first_include == '#include "smj.h"' and len(re.findall(r"^#include", text, flags=re.M)) == 1
    lines = capi_check.header("smj_mapping.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_localize.h"')]
    assert len(inc) == 1
    closing = max(k for k, line in enumerate(lines) if line.strip() == "}")      # the end of extern "C"
    assert closing < inc[0] and lines[inc[0] + 1:] == ["#endif"] and lines[inc[0] - 1] == "#endif"
    includes = [line for line in lines if line.startswith("#include")]
    assert includes == ['#include "smj.h"', '#include "smj_localize.h"']      # smj.h stays its first include
    others = ("smj_occupancy.h", "smj_distance.h", "smj_navigation.h", "smj_frontier.h", "smj_drive.h", "smj_scanmatch.h", "smj_pointcloud.h", "smj_heightmap.h",
              "smj_build.h", "smj.h")
    assert all(NAME not in capi_check.header(h) for h in others)


def test_smj_h_includes_are_unchanged():
    """A caller includes smj.h alone: the list of entry headers smj.h itself includes is what it was."""
    assert capi_check.smj_h_includes()[1] == ["smj_pointcloud.h", "smj_heightmap.h", "smj_occupancy.h"]


def test_constants_of_the_kernel_header():
    text = capi_check.kernel_header("smj_mcl.h")
    public = capi_check.header(NAME)
    found = re.findall(r"^#define\s+SMJ_MCL_(?:OK|FEW|LOST)\s.*$", public, flags=re.M)
    assert len(found) == 3
    for m in found:      # token for token
        assert m in text, m
    assert re.search(r"SMJ_MCL_MAX_PARTICLES\s*=\s*4096", text) and re.search(r"SMJ_MCL_MAX_SPAN\s*=\s*1 << 18", text) and re.search(r"SMJ_MCL_STAT_WORDS\s*=\s*8", text)
    assert "SMJ_MCL_MAX_POINTS = SMJ_MATCH_MAX_POINTS" in text and re.search(r"SMJ_MATCH_MAX_POINTS\s*=\s*1024", capi_check.kernel_header("smj_match.h"))
    assert re.search(r"SMJ_MCL_STAT_STATUS\s*=\s*3", text)      # where smj_scan_to_map's gate reads it
    # it reuses the matcher's functions and does not restate them
    for name in ("smj_match_point", "smj_match_cell", "smj_match_shifted", "smj_match_before"):
        assert not re.search(rf"SMJ_GRID_HD\s+\w+\s+{name}\b", text), name
    # the limits the public header states in words
    for phrase in ("nlidar <= 1024", "nx ny <= 65536", "r_max / cell <= 8192", "P = num_particles in [1, 4096]", "span in [1, 262144]", "min_points in [1, 1024]",
                   "resample in {0, 1}", "cell finite and > 0", "0 <= r_min <= r_max", "0x7FC00000", "gate_ld = 8"):
        assert phrase in public, phrase


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(NAME, lib.LOCALIZE_EXPORTS, ENTRY, 25)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry and its macros, and hands its status column to smj_scan_to_map
    as the gate, where it lies; so does one that includes smj_scanmatch.h, smj_mapping.h or smj_localize.h first."""
    body = ("int f(smj_ctx* c, const void* scan, const void* field, const void* part, const void* noise, const unsigned* draw, void* out, void* weight, int* stat,\n"
            "      void* pose, void* hit, void* miss, void* info) {\n"
            "  int rc = smj_scan_to_particles(c, scan, 4096, 1, 0.2f, 5.0f, field, 128, 128, -3.2f, -3.2f, 0.05f, part, 1024, noise, draw, 4096, 30, 1, out, weight, 0,\n"
            "                                 stat, pose, 0);\n"
            "  return rc + smj_scan_to_map(c, scan, 4096, 1, 0.2f, 5.0f, pose, stat + 3, 8, -3.2f, -3.2f, 0.05f, 128, 128, 1, 1, hit, miss, info, 0, 0)\n"
            "         + SMJ_MCL_OK + SMJ_MCL_FEW + SMJ_MCL_LOST + SMJ_MAP_OK + SMJ_MATCH_OK; }\n")
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_scanmatch.h", "smj_mapping.h", "smj_localize.h"))
