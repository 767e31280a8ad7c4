"""The distance-field arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_edt.h: the obstacle predicate, the row rule on the
bit mask, the column rule with its tie order and stop condition, the cut into column strips, the store's groups) compiled for the host
by g++ -Wall -Wextra -Werror and checked by a small C++ harness (tests/edt/edt_check.cpp), which emulates the kernel's three phases
serially for every strip and holds them against its own brute force on seeded grids and grids full of ties; once more under
AddressSanitizer / UBSan where their runtime links.  CPU only: stand-alone programs (tests/host_check.py builds and runs them),
nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_edt.h", "unsigned long long m[1] = {1ull << 5}; return smj_edt_row_offset(m, 9, 0, 7, 0) != -2;")


def test_three_phases_against_brute_force(tmp_path):
    print(host_check.check_program(tmp_path, "edt"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "edt", sanitizers=True))
