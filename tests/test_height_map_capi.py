"""include/smj_heightmap.h (the height-map entry, included by smj.h) and the loader agree, as tests/test_point_cloud_capi.py checks for
smj_pointcloud.h."""
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
    assert _declared(_header("smj_heightmap.h")) == sorted(lib.HEIGHTMAP_EXPORTS) == ["smj_depth_to_heightmap"]
    assert not set(lib.HEIGHTMAP_EXPORTS) & set(lib.EXPORTS)
    assert not set(lib.HEIGHTMAP_EXPORTS) & set(lib.POINT_EXPORTS)
    assert not set(lib.POINT_EXPORTS) & set(lib.EXPORTS)
    assert re.search(r'^#include "smj_heightmap.h"', _header("smj.h"), flags=re.M)   # a caller includes smj.h alone
    assert "smj_depth_to_heightmap" not in _declared(_header("smj.h")) + _declared(_header("smj_pointcloud.h"))


def test_band_constant_of_the_kernel_header():
    """A 64 x 64 grid is one band; the largest grid the entry takes is 65536 cells."""
    with open(os.path.join(ROOT, "stretch_mujoco_amd", "csrc", "smj_hmap.h")) as f:
        text = f.read()
    band = int(re.search(r"SMJ_HMAP_BAND_CELLS\s*=\s*(\d+)", text).group(1))
    assert band >= 64 * 64 and 8 * band <= 160 * 1024
    assert int(re.search(r"SMJ_HMAP_MAX_CELLS\s*=\s*(\d+)", text).group(1)) == 65536


def test_library_exports_the_entry_with_its_signature():
    if not os.path.exists(lib.LIB_PATH):
        pytest.fail(f"{lib.LIB_PATH} not built: run __graft_entry__.build()")
    L = lib.load()
    for sym in lib.HEIGHTMAP_EXPORTS:
        assert hasattr(L, sym), sym
    decl = re.search(r"int smj_depth_to_heightmap\((.*?)\);", _header("smj_heightmap.h"), flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert len(args) == len(L.smj_depth_to_heightmap.argtypes) == 19
    import ctypes
    kinds = {"float": ctypes.c_float, "int": ctypes.c_int}
    for a, t in zip(args, L.smj_depth_to_heightmap.argtypes):      # floats where the header has floats: a wrong slot would pass garbage
        want = ctypes.c_void_p if "*" in a else kinds[a.split()[0]]
        assert t is want, (a, t)


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C99 translation unit that includes only smj.h sees the entry; so does one that includes smj_heightmap.h first."""
    import shutil
    import subprocess

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler on this box")
    body = ("int f(smj_ctx* c, void* d, void* z, void* n) { return smj_depth_to_heightmap(c, 1, 4, 4, 60.f, d, 1, SMJ_FRAME_WORLD, -1.6f, -1.6f, 0.05f, "
            "64, 64, -0.05f, 2.f, 0, z, n, 0); }\n")
    for first in ("smj.h", "smj_heightmap.h"):
        src = tmp_path / f"use_{first[:-2]}.c"
        src.write_text(f'#include "{first}"\n' + body)
        subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                               str(tmp_path / "use.o")])
