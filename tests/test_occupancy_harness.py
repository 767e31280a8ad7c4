"""The occupancy arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_occ.h: the classification of a range, the ray in the
requested frame, the cells of its ends with their guards, the closed-form line) compiled for the host by g++ -Wall -Werror and
checked by a small C++ harness (tests/occ/occ_check.cpp), which also emulates the kernel's scatter serially on a seeded scan and
holds it against long-hand fp64 by the comparison rule of tests/occupancy_ref.py; once more under AddressSanitizer / UBSan where
their runtime links.  CPU only: stand-alone programs, nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build(exe, extra=()):
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "stretch_mujoco_amd", "csrc"),
                           os.path.join(ROOT, "tests", "occ", "occ_check.cpp"), "-o", str(exe)])


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    return out.stdout


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    src = tmp_path / "alone.cpp"
    src.write_text('#include "smj_occ.h"\nint main() { float len; return smj_occ_classify(1.f, 0.2f, 5.f, 1, &len) != SMJ_OCC_RETURN; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "stretch_mujoco_amd", "csrc"), str(src), "-o",
                           str(tmp_path / "alone")])
    subprocess.check_call([str(tmp_path / "alone")])


def test_classification_line_guards_and_scatter(tmp_path):
    exe = tmp_path / "occ_check"
    _build(exe)
    print(_run(exe))


def test_the_same_under_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("the sanitizer runtime is absent here: an empty main does not link with -fsanitize=address,undefined")
    exe = tmp_path / "occ_check_san"
    _build(exe, SAN)
    print(_run(exe))
