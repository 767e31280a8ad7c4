"""include/smj_distance.h (the distance-field entry; smj_occupancy.h includes it, so smj.h does) and the loader agree, as
tests/test_occupancy_capi.py checks for smj_occupancy.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

ENTRY = ("smj_distance.h", lib.DISTANCE_EXPORTS, "smj_occupancy_to_distance")


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(*ENTRY)
    assert int(re.search(r"#define\s+SMJ_DIST_NONE\s+\(1 << (\d+)\)", capi_check.header("smj_distance.h")).group(1)) == 30 and lib.DIST_NONE == 1 << 30


def test_smj_occupancy_h_includes_it_after_its_declarations():
    lines = capi_check.header("smj_occupancy.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_distance.h"')]
    assert len(inc) == 1
    closing = max(k for k, line in enumerate(lines) if line.strip() == "}")      # the end of extern "C"
    assert closing < inc[0] and lines[inc[0] + 1:] == ["#endif"] and lines[inc[0] - 1] == "#endif"
    assert "smj_distance.h" not in capi_check.smj_h_includes()[1]


def test_constants_of_the_kernel_header():
    text = capi_check.kernel_header("smj_edt.h")
    assert re.search(r"SMJ_EDT_NONE\s*=\s*1 << 30", text)
    assert int(re.search(r"SMJ_EDT_MAX_CELLS\s*=\s*(\d+)", text).group(1)) == 65536
    assert int(re.search(r"SMJ_EDT_MAX_SIDE\s*=\s*(\d+)", text).group(1)) == 4096
    assert int(re.search(r"SMJ_EDT_STRIP_CELLS\s*=\s*(\d+)", text).group(1)) == 16384      # int16 offsets: 32 KiB of LDS


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(*ENTRY, 11)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry and SMJ_DIST_NONE; so does one that includes smj_distance.h or
    smj_occupancy.h first."""
    body = ("int f(smj_ctx* c, const void* h, const void* m, void* d, void* n) { return smj_occupancy_to_distance(c, h, m, 128, 128, 1, 0, 20, d, n, 0) "
            "+ (SMJ_DIST_NONE == 1073741824 ? 0 : 1); }\n")
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_distance.h", "smj_occupancy.h"))
