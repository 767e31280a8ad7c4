"""The distance-field arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_edt.h: the obstacle predicate, the row rule on the
bit mask, the column rule with its tie order and stop condition, the cut into column strips, the store's groups) compiled for the host
by g++ -Wall -Wextra -Werror and checked by a small C++ harness (tests/edt/edt_check.cpp), which emulates the kernel's three phases
serially for every strip and holds them against its own brute force on seeded grids and grids full of ties; once more under
AddressSanitizer / UBSan where their runtime links.  CPU only: stand-alone programs, nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build(exe, extra=()):
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-I", os.path.join(ROOT, "stretch_mujoco_amd", "csrc"),
                           os.path.join(ROOT, "tests", "edt", "edt_check.cpp"), "-o", str(exe)])


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    return out.stdout


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "smj_edt.h"\nint main() { unsigned long long m[1] = {1ull << 5}; return smj_edt_row_offset(m, 9, 0, 7, 0) != -2; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "stretch_mujoco_amd", "csrc"), str(src), "-o",
                           str(tmp_path / "alone")])
    subprocess.check_call([str(tmp_path / "alone")])


def test_three_phases_against_brute_force(tmp_path):
    exe = tmp_path / "edt_check"
    _build(exe)
    print(_run(exe))


def test_the_same_under_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("the sanitizer runtime is absent here: an empty main does not link with -fsanitize=address,undefined")
    exe = tmp_path / "edt_check_san"
    _build(exe, SAN)
    print(_run(exe))
