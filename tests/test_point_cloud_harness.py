"""The point-cloud arithmetic the HIP kernels run (stretch_mujoco_amd/csrc/smj_points.h: index mapping, per-pixel point in the three
frame kinds, NaN rule) compiled for the host by g++ -Wall -Wextra -Werror and checked against long-hand fp64 by a small C++ harness
(tests/points/points_check.cpp); once more under AddressSanitizer / UBSan where their runtime links.  CPU only: stand-alone
programs (tests/host_check.py builds and runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_points.h", "return smj_points_grid(5, 2) != 3;")


def test_point_arithmetic_and_index_mapping(tmp_path):
    print(host_check.check_program(tmp_path, "points"))


def test_point_arithmetic_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "points", sanitizers=True))
