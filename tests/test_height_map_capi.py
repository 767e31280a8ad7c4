"""include/smj_heightmap.h (the height-map entry, included by smj.h) and the loader agree, as tests/test_point_cloud_capi.py checks for
smj_pointcloud.h."""
import re

import capi_check
from stretch_mujoco_amd import lib

ENTRY = ("smj_heightmap.h", lib.HEIGHTMAP_EXPORTS, "smj_depth_to_heightmap")


def test_header_and_loader_agree():
    capi_check.header_and_loader_agree(*ENTRY)
    assert "smj_heightmap.h" in capi_check.smj_h_includes()[1]   # a caller includes smj.h alone


def test_band_constant_of_the_kernel_header():
    """A 64 x 64 grid is one band; the largest grid the entry takes is 65536 cells."""
    text = capi_check.kernel_header("smj_hmap.h")
    band = int(re.search(r"SMJ_HMAP_BAND_CELLS\s*=\s*(\d+)", text).group(1))
    assert band >= 64 * 64 and 8 * band <= 160 * 1024
    assert int(re.search(r"SMJ_HMAP_MAX_CELLS\s*=\s*(\d+)", text).group(1)) == 65536


def test_library_exports_the_entry_with_its_signature():
    capi_check.library_exports(*ENTRY, 19)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry; so does one that includes smj_heightmap.h first."""
    body = ("int f(smj_ctx* c, void* d, void* z, void* n) { return smj_depth_to_heightmap(c, 1, 4, 4, 60.f, d, 1, SMJ_FRAME_WORLD, -1.6f, -1.6f, 0.05f, "
            "64, 64, -0.05f, 2.f, 0, z, n, 0); }\n")
    capi_check.c_caller_compiles(tmp_path, body, ("smj.h", "smj_heightmap.h"))
