"""include/smj_scanmatch.h (the scan-matching entry; smj_drive.h includes it, smj_frontier.h that one and so on up to smj.h) and the
loader agree, as tests/test_drive_capi.py checks for smj_drive.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

NAME, ENTRY = "smj_scanmatch.h", "smj_scan_to_pose"


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(NAME, lib.SCANMATCH_EXPORTS, ENTRY)
    text = capi_check.header(NAME)
    macros = dict(re.findall(r"^#define\s+(SMJ_\w+)[ \t]*(\S*)$", text, flags=re.M))
    assert macros == {"SMJ_SCANMATCH_H": "", "SMJ_MATCH_OK": "0", "SMJ_MATCH_FEW": "1", "SMJ_MATCH_OFF": "2", "SMJ_MATCH_NO_CELL": "(-32768)"}
    assert "THE LARGEST J WINS; AMONG EQUAL J THE SMALLEST i WINS" in text      # the header states the tie-break


def test_smj_drive_h_includes_it_after_its_declarations():
    text = capi_check.header(NAME)
    first_include = re.search(r"^#include.*$", text, flags=re.M).group(0)
    assert first_include == '#include "smj.h"'
    lines = capi_check.header("smj_drive.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_scanmatch.h"')]
    assert len(inc) == 1
    closing = max(k for k, line in enumerate(lines) if line.strip() == "}")      # the end of extern "C"
    assert closing < inc[0] and lines[inc[0] + 1:] == ["#endif"] and lines[inc[0] - 1] == "#endif"
    assert NAME not in capi_check.smj_h_includes()[1]
    assert all(NAME not in capi_check.header(h) for h in ("smj_occupancy.h", "smj_distance.h", "smj_navigation.h", "smj_frontier.h"))


def test_constants_of_the_kernel_header():
    text = capi_check.kernel_header("smj_match.h")
    get = lambda name: int(re.search(rf"SMJ_MATCH_{name}\s*=\s*(\d+)", text).group(1))
    for name, value, other, theirs in (("MAX_CELLS", 65536, "smj_occ.h", "SMJ_OCC_MAX_CELLS"), ("MAX_CELLS", 65536, "smj_edt.h", "SMJ_EDT_MAX_CELLS"),
                                       ("MAX_SIDE", 4096, "smj_edt.h", "SMJ_EDT_MAX_SIDE"), ("MAX_CELLS", 65536, "smj_drive.h", "SMJ_DRIVE_MAX_CELLS"),
                                       ("MAX_SIDE", 4096, "smj_drive.h", "SMJ_DRIVE_MAX_SIDE")):      # the entries whose maps are matched, and the pose's consumer
        assert get(name) == value == int(re.search(rf"{theirs}\s*=\s*(\d+)", capi_check.kernel_header(other)).group(1)), (name, other)
    assert (get("MAX_ANGLES"), get("MAX_WINDOW"), get("MAX_SHIFT_WEIGHT"), get("MAX_POINTS")) == (64, 32, 1024, 1024)
    assert re.search(r"SMJ_MATCH_MAX_BIAS\s*=\s*1 << 20", text)
    # the header's bounds: S < 2^18 and J > -2^22, and a cell of the band fits the 16 bits it is packed into
    assert get("MAX_POINTS") * 255 < 1 << 18 and (1 << 20) + get("MAX_SHIFT_WEIGHT") * 2 * get("MAX_WINDOW") ** 2 < 1 << 22
    assert get("MAX_SIDE") + get("MAX_WINDOW") < 1 << 15
    public = capi_check.header(NAME)
    found = re.findall(r"^#define\s+SMJ_MATCH_(?:OK|FEW|OFF|NO_CELL)\s.*$", public, flags=re.M)
    assert len(found) == 4
    for m in found:      # token for token
        assert m in text, m
    # the limits the public header states in words
    for phrase in ("num_angles in [1, 64]", "wx, wy in [0, 32]", "shift_weight in [0, 1024]", "min_points in [1, 1024]", "nlidar <= 1024",
                   "nx, ny in [1, 4096] and nx ny <= 65536", "min(max(b, 0), 1 << 20)"):
        assert phrase in public, phrase


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(NAME, lib.SCANMATCH_EXPORTS, ENTRY, 25)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry and its macros; so does one that includes smj_drive.h or
    smj_scanmatch.h first."""
    body = ("int none = SMJ_MATCH_NO_CELL;\n"
            "int f(smj_ctx* c, const void* scan, const void* field, const void* prior, const void* angles, void* pose, void* best) {\n"
            "  return smj_scan_to_pose(c, scan, 4096, 1, 0.2f, 5.0f, field, 128, 128, -3.2f, -3.2f, 0.05f, prior, angles, 0, 21, 10, 10, 0, 30, pose, best, 0, 0, 0)\n"
            "         + SMJ_MATCH_OK + SMJ_MATCH_FEW + SMJ_MATCH_OFF; }\n")
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_drive.h", "smj_scanmatch.h"))
