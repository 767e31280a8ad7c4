"""include/smj_pointcloud.h (the point-cloud entry, included by smj.h) and the loader agree, as tests/test_capi.py checks for smj.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

ENTRY = ("smj_pointcloud.h", lib.POINT_EXPORTS, "smj_depth_to_points")


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(*ENTRY)
    assert "smj_pointcloud.h" in capi_check.smj_h_includes()[1]   # a caller includes smj.h alone


def test_frame_constants_match_header():
    text = capi_check.header("smj_pointcloud.h")
    for name, val in (("CAMERA", lib.FRAME_CAMERA), ("WORLD", lib.FRAME_WORLD)):
        assert re.search(rf"SMJ_FRAME_{name}\s*=\s*{val}\b", text), name
    assert lib.FRAME_CAMERA < 0 and lib.FRAME_WORLD < 0      # frame >= 0 is a body id


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(*ENTRY, 10)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C translation unit that includes only smj.h sees the entry and its frame constants; so does one that includes
    smj_pointcloud.h first (the two headers include each other behind their guards)."""
    body = "int f(smj_ctx* c, void* d, void* p) { return smj_depth_to_points(c, 1, 4, 4, 60.f, d, 1, SMJ_FRAME_WORLD, p, 0); }\n"
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_pointcloud.h"))
