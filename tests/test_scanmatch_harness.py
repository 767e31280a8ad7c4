"""The scan-matching arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_match.h: the placed test and the cell of a point,
the packed word, the shifted cell, the clamp of a bias, the score, the index and its inverse, the (J, i) order, the status and the
output pose) compiled for the host by g++ -Wall -Wextra -Werror and checked by a small C++ harness (tests/match/match_check.cpp),
which emulates the kernel's candidate pass and reductions with the kernel's own functions for 64, 128, 256 and 512 threads and holds them
against its own loops on seeded fields full of score ties; once more under AddressSanitizer / UBSan where their runtime links.  CPU
only: stand-alone programs (tests/host_check.py builds and runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_match.h", "int ix, iy; return !(smj_match_cell(0.0f, 0.0f, 1.0f, 0.0f, 0.126f, 0.076f, 0.0f, 0.0f, 0.05f, 4, 4, &ix, &iy) && ix == 2 && iy == 1 "
                            "&& smj_match_bias(-3) == 0 && smj_match_score(1000, 7, 3, -2, 1) == 978 && smj_match_before(5, 3, 5, 4) && smj_match_before(6, 4, 5, 3) "
                            "&& smj_match_index(1, -2, -3, 3, 2) == 35 && smj_match_status(true, 29, 30) == SMJ_MATCH_FEW);")
    # and the header of what the scan entries share: the split of the field's copy into LDS
    host_check.header_alone(tmp_path, "smj_scan.h", "const smj_scan_split_t s = smj_scan_stage_split(0x1003, 40); "
                            "return !(s.sh == 3 && s.lead == 13 && s.groups == 1 && s.tail == 29);")


def test_kernel_phases_against_the_programs_own_loops(tmp_path):
    print(host_check.check_program(tmp_path, "match"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "match", sanitizers=True))
