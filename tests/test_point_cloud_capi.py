"""include/smj_pointcloud.h (the point-cloud entry, included by smj.h) and the loader agree, as tests/test_capi.py checks for smj.h."""
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
    assert _declared(_header("smj_pointcloud.h")) == sorted(lib.POINT_EXPORTS) == ["smj_depth_to_points"]
    assert not set(lib.POINT_EXPORTS) & set(lib.EXPORTS)
    assert re.search(r'^#include "smj_pointcloud.h"', _header("smj.h"), flags=re.M)   # a caller includes smj.h alone


def test_frame_constants_match_header():
    text = _header("smj_pointcloud.h")
    for name, val in (("CAMERA", lib.FRAME_CAMERA), ("WORLD", lib.FRAME_WORLD)):
        assert re.search(rf"SMJ_FRAME_{name}\s*=\s*{val}\b", text), name
    assert lib.FRAME_CAMERA < 0 and lib.FRAME_WORLD < 0      # frame >= 0 is a body id


def test_library_exports_the_entry_with_its_signature():
    if not os.path.exists(lib.LIB_PATH):
        pytest.fail(f"{lib.LIB_PATH} not built: run __graft_entry__.build()")
    L = lib.load()
    for sym in lib.POINT_EXPORTS:
        assert hasattr(L, sym), sym
    decl = re.search(r"int smj_depth_to_points\((.*?)\);", _header("smj_pointcloud.h"), flags=re.S).group(1)
    assert len(decl.split(",")) == len(L.smj_depth_to_points.argtypes) == 10


def test_c_caller_compiles_against_smj_h_alone(tmp_path):
    """A C translation unit that includes only smj.h sees the entry and its frame constants; so does one that includes
    smj_pointcloud.h first (the two headers include each other behind their guards)."""
    import shutil
    import subprocess

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler on this box")
    body = "int f(smj_ctx* c, void* d, void* p) { return smj_depth_to_points(c, 1, 4, 4, 60.f, d, 1, SMJ_FRAME_WORLD, p, 0); }\n"
    for first in ("smj.h", "smj_pointcloud.h"):
        src = tmp_path / f"use_{first[:-2]}.c"
        src.write_text(f'#include "{first}"\n' + body)
        subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                               str(tmp_path / "use.o")])
