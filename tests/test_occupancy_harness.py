"""The occupancy arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_occ.h: the classification of a range, the ray in the
requested frame, the cells of its ends with their guards, the closed-form line) compiled for the host by g++ -Wall -Wextra -Werror and
checked by a small C++ harness (tests/occ/occ_check.cpp), which also emulates the kernel's scatter serially on a seeded scan and
holds it against long-hand fp64 by the comparison rule of tests/occupancy_ref.py; once more under AddressSanitizer / UBSan where
their runtime links.  CPU only: stand-alone programs (tests/host_check.py builds and runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_occ.h", "float len; return smj_occ_classify(1.f, 0.2f, 5.f, 1, &len) != SMJ_OCC_RETURN;")


def test_classification_line_guards_and_scatter(tmp_path):
    print(host_check.check_program(tmp_path, "occ"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "occ", sanitizers=True))
