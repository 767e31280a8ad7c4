"""include/smj_drive.h (the base-command entry; smj_frontier.h includes it, smj_navigation.h that one and so on up to smj.h) and the
loader agree, as tests/test_frontier_capi.py checks for smj_frontier.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

NAME, ENTRY = "smj_drive.h", "smj_navigation_to_velocity"


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(NAME, lib.DRIVE_EXPORTS, ENTRY)
    text = capi_check.header(NAME)
    macros = dict(re.findall(r"^#define\s+(SMJ_\w+)[ \t]*(\S*)$", text, flags=re.M))
    assert macros == {"SMJ_DRIVE_H": "", "SMJ_DRIVE_OK": "0", "SMJ_DRIVE_ARRIVED": "1", "SMJ_DRIVE_BLOCKED": "2", "SMJ_DRIVE_OFF_GRID": "3",
                      "SMJ_DRIVE_NO_SCORE": "0x7fffffffffffffffLL"}
    assert int(macros["SMJ_DRIVE_NO_SCORE"][:-2], 16) == 2 ** 63 - 1
    assert "THE SMALLEST SCORE WINS; AMONG EQUAL SCORES THE SMALLEST k WINS" in text      # the header states the tie-break


def test_smj_frontier_h_includes_it_after_its_declarations():
    text = capi_check.header(NAME)
    first_include = re.search(r"^#include.*$", text, flags=re.M).group(0)
    assert first_include == '#include "smj.h"'
    lines = capi_check.header("smj_frontier.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_drive.h"')]
    assert len(inc) == 1
    closing = max(k for k, line in enumerate(lines) if line.strip() == "}")      # the end of extern "C"
    assert closing < inc[0] and lines[inc[0] + 1:] == ["#endif"] and lines[inc[0] - 1] == "#endif"
    assert NAME not in capi_check.smj_h_includes()[1]
    assert all(NAME not in capi_check.header(h) for h in ("smj_occupancy.h", "smj_distance.h", "smj_navigation.h"))


def test_constants_of_the_kernel_header():
    text = capi_check.kernel_header("smj_drive.h")
    nav = capi_check.kernel_header("smj_nav.h")
    get = lambda name: int(re.search(rf"SMJ_DRIVE_{name}\s*=\s*(\d+)", text).group(1))
    for name, value in (("MAX_CELLS", 65536), ("MAX_SIDE", 4096)):      # the navigation entry's limits: its potential is read here
        assert get(name) == value == int(re.search(rf"SMJ_NAV_{name}\s*=\s*(\d+)", nav).group(1))
    assert (get("MAX_CANDIDATES"), get("MAX_POINTS"), get("MAX_TABLE"), get("MAX_WEIGHT"), get("SWEPT_BLOCKS")) == (1024, 256, 32768, 65535, 256)
    assert re.search(r"SMJ_DRIVE_NAV_NONE\s*=\s*1 << 30", text) and lib.NAV_NONE == 1 << 30
    assert get("MAX_WEIGHT") * (1 << 30) + get("MAX_WEIGHT") * 255 + (1 << 31) < 1 << 47      # the header's bound on a score
    public = capi_check.header(NAME)
    for m in re.findall(r"^#define\s+SMJ_DRIVE_(?:OK|ARRIVED|BLOCKED|OFF_GRID|NO_SCORE)\s.*$", public, flags=re.M):      # token for token
        assert m in text, m


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(NAME, lib.DRIVE_EXPORTS, ENTRY, 27)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry and its macros; so does one that includes smj_frontier.h or
    smj_drive.h first."""
    body = ("long long none = SMJ_DRIVE_NO_SCORE;\n"
            "int f(smj_ctx* c, const void* pose, const void* pot, const void* cmd, const void* pts, void* out, void* best) {\n"
            "  return smj_navigation_to_velocity(c, pose, 0, 0, pot, 128, 128, -3.2f, -3.2f, 0.05f, cmd, pts, 0, 35, 13, 253, 0, 1, 20, 1000, 0.1f, 0.5f, out, best, 0, 0, 0)\n"
            "         + SMJ_DRIVE_OK + SMJ_DRIVE_ARRIVED + SMJ_DRIVE_BLOCKED + SMJ_DRIVE_OFF_GRID; }\n")
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_frontier.h", "smj_drive.h"))
