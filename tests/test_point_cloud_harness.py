"""The point-cloud arithmetic the HIP kernels run (stretch_mujoco_amd/csrc/smj_points.h: index mapping, per-pixel point in the three
frame kinds, NaN rule) compiled for the host and checked against long-hand fp64 by a small C++ harness
(tests/points/points_check.cpp); once more under AddressSanitizer / UBSan where their runtime links.  CPU only: stand-alone
programs, nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _build(exe, extra=()):
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "stretch_mujoco_amd", "csrc"),
                           os.path.join(ROOT, "tests", "points", "points_check.cpp"), "-o", str(exe)])


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    return out.stdout


def test_point_arithmetic_and_index_mapping(tmp_path):
    exe = tmp_path / "points_check"
    _build(exe)
    print(_run(exe))


def test_point_arithmetic_under_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("the sanitizer runtime is absent here: an empty main does not link with -fsanitize=address,undefined")
    exe = tmp_path / "points_check_san"
    _build(exe, SAN)
    print(_run(exe))
