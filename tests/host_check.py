"""Host-compiler checks of the device headers in stretch_mujoco_amd/csrc: build a stand-alone check program with g++, run it, run it
again under AddressSanitizer / UBSan where their runtime links, and compile a header on its own.  Plain helpers for
tests/test_{point_cloud,height_map,occupancy,distance,navigation}_harness.py; nothing here is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = ["-I", os.path.join(ROOT, "stretch_mujoco_amd", "csrc"), "-I", os.path.join(ROOT, "tests")]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def build(source, exe, flags=()):
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, *INCLUDE, str(source), "-o", str(exe)])


def run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
    return out.stdout


def check_program(tmp_path, name, sanitizers=False):
    """Build tests/<name>/<name>_check.cpp with -Wall -Wextra -Werror (under the sanitizers too, or skip where they do not link), run
    it and return what it printed."""
    flags = ["-Wextra"] + (sanitizers_or_skip(tmp_path) if sanitizers else [])
    exe = tmp_path / (name + ("_check_san" if sanitizers else "_check"))
    build(os.path.join(ROOT, "tests", name, name + "_check.cpp"), exe, flags)
    return run(exe)


def sanitizers_or_skip(tmp_path):
    """SAN where an empty main links with it; the test skips where the sanitizer runtime is absent."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if p.returncode != 0:
        pytest.skip("the sanitizer runtime is absent here: an empty main does not link with -fsanitize=address,undefined")
    return SAN


def header_alone(tmp_path, header, main_body):
    """`header` is the only include of a program whose main returns 0; built with -Wall -Wextra -Werror and run."""
    src = tmp_path / "alone.cpp"
    src.write_text(f'#include "{header}"\nint main() {{ {main_body} }}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *INCLUDE, str(src), "-o", str(tmp_path / "alone")])
    subprocess.check_call([str(tmp_path / "alone")])
