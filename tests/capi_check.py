"""What the C-API tests of the perception entries share (tests/test_{point_cloud,height_map,occupancy,distance,navigation}_capi.py): reading the
headers of include/ and csrc/, and the assertions that hold a header, the loader (stretch_mujoco_amd/lib.py) and the library together."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from stretch_mujoco_amd import lib


def header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def kernel_header(name):
    with open(os.path.join(ROOT, "stretch_mujoco_amd", "csrc", name)) as f:
        return f.read()


def declared(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(smj_[a-z_]+)\s*\(", text)))


def header_and_loader_agree(name, exports, entry):
    """The header declares the entry and nothing else, the loader lists it, no other header declares it, and the export tuples of
    lib.py -- every module attribute named *EXPORTS, so that a new one cannot be left out -- are disjoint."""
    assert declared(header(name)) == sorted(exports) == [entry]
    others = [n for n in sorted(os.listdir(os.path.join(ROOT, "include"))) if n != name]
    assert entry not in sum((declared(header(n)) for n in others), [])
    groups = [getattr(lib, a) for a in sorted(dir(lib)) if a.endswith("EXPORTS")]
    assert len(groups) >= 7 and any(g is exports for g in groups)
    for i, a in enumerate(groups):
        for b in groups[i + 1:]:
            assert not set(a) & set(b), (a, b)


def smj_h_includes():
    """(line numbers, names) of the entry headers smj.h includes: a caller includes smj.h alone."""
    lines = header("smj.h").splitlines()
    inc = [k for k, line in enumerate(lines) if line.startswith('#include "smj_')]
    return inc, [lines[k].split('"')[1] for k in inc]


def library_exports(name, exports, entry, nargs):
    """The built library has the entry, and the loader's argtypes follow the header's declaration slot by slot: floats where the
    header has floats -- a wrong slot would pass garbage."""
    if not os.path.exists(lib.LIB_PATH):
        pytest.fail(f"{lib.LIB_PATH} not built: run __graft_entry__.build()")
    L = lib.load()
    for sym in exports:
        assert hasattr(L, sym), sym
    decl = re.search(rf"int {entry}\((.*?)\);", header(name), flags=re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    argtypes = getattr(L, entry).argtypes
    assert len(args) == len(argtypes) == nargs
    kinds = {"float": ctypes.c_float, "int": ctypes.c_int, "long": ctypes.c_long}
    for a, t in zip(args, argtypes):
        want = ctypes.c_void_p if "*" in a else kinds[a.split()[0]]
        assert t is want, (a, t)


def c_caller_compiles(tmp_path, body, first_headers):
    """A C99 translation unit with `body` compiles after including any one of first_headers alone."""
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler on this box")
    for first in first_headers:
        src = tmp_path / f"use_{first[:-2]}.c"
        src.write_text(f'#include "{first}"\n' + body)
        subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                               str(tmp_path / "use.o")])
