"""include/smj_occupancy.h (the occupancy entry, included by smj.h) and the loader agree, as tests/test_height_map_capi.py checks for
smj_heightmap.h."""
import os
import re

import pytest

from conftest import ROOT
from stretch_mujoco_amd import lib


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def _declared(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(smj_[a-z_]+)\s*\(", text)))


def test_header_and_loader_agree():
    assert _declared(_header("smj_occupancy.h")) == sorted(lib.OCCUPANCY_EXPORTS) == ["smj_lidar_to_occupancy"]
    groups = [lib.EXPORTS, lib.POINT_EXPORTS, lib.HEIGHTMAP_EXPORTS, lib.OCCUPANCY_EXPORTS]
    for i, a in enumerate(groups):      # disjoint export tuples
        for b in groups[i + 1:]:
            assert not set(a) & set(b), (a, b)
    lines = _header("smj.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_')]
    assert [lines[k].split('"')[1] for k in inc] == ["smj_pointcloud.h", "smj_heightmap.h", "smj_occupancy.h"]      # a caller includes smj.h alone
    assert inc[2] == inc[1] + 1
    assert "smj_lidar_to_occupancy" not in _declared(_header("smj.h")) + _declared(_header("smj_pointcloud.h")) + _declared(_header("smj_heightmap.h"))


def test_constants_of_the_kernel_header():
    """The bands are those of the height map (a 64 x 64 grid is one band), the largest grid is 65536 cells, the longest ray 8192 cells."""
    with open(os.path.join(ROOT, "stretch_mujoco_amd", "csrc", "smj_occ.h")) as f:
        text = f.read()
    assert re.search(r"SMJ_OCC_BAND_CELLS\s*=\s*SMJ_HMAP_BAND_CELLS", text)
    assert int(re.search(r"SMJ_OCC_MAX_CELLS\s*=\s*(\d+)", text).group(1)) == 65536
    assert int(re.search(r"SMJ_OCC_MAX_STEPS\s*=\s*(\d+)", text).group(1)) == 8192
    assert "smj_hmap_band(" not in re.sub(r"//.*", "", text) and '#include "smj_hmap.h"' in text      # the cut into bands is reused, not copied


def test_library_exports_the_entry_with_its_signature():
    if not os.path.exists(lib.LIB_PATH):
        pytest.fail(f"{lib.LIB_PATH} not built: run __graft_entry__.build()")
    L = lib.load()
    for sym in lib.OCCUPANCY_EXPORTS:
        assert hasattr(L, sym), sym
    decl = re.search(r"int smj_lidar_to_occupancy\((.*?)\);", _header("smj_occupancy.h"), flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == len(L.smj_lidar_to_occupancy.argtypes) == 16
    import ctypes
    kinds = {"float": ctypes.c_float, "int": ctypes.c_int, "long": ctypes.c_long}
    for a, t in zip(args, L.smj_lidar_to_occupancy.argtypes):      # floats where the header has floats: a wrong slot would pass garbage
        want = ctypes.c_void_p if "*" in a else kinds[a.split()[0]]
        assert t is want, (a, t)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry; so does one that includes smj_occupancy.h first."""
    import shutil
    import subprocess

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler on this box")
    body = ("int f(smj_ctx* c, const void* scan, void* h, void* m) { return smj_lidar_to_occupancy(c, scan, 4096L, SMJ_FRAME_WORLD, -3.2f, -3.2f, 0.05f, "
            "128, 128, 0.2f, 5.f, 1, 0, h, m, 0); }\n")
    for first in ("smj.h", "smj_occupancy.h"):
        src = tmp_path / f"use_{first[:-2]}.c"
        src.write_text(f'#include "{first}"\n' + body)
        subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                               str(tmp_path / "use.o")])
