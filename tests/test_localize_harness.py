"""The particle-filter arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_mcl.h: the weight of a point, cut and w, the offset
of a draw, the threshold of a slot, the ancestor search, the effective sample size, the status) compiled for the host by
g++ -Wall -Wextra -Werror and checked by a small C++ harness (tests/mcl/mcl_check.cpp), which emulates the kernel's integer stage --
per-thread firsts, butterfly, the wave's scan by its six lane moves, the carry across rounds, the search per slot -- with the kernel's
own functions against its own loops for P from 1 to 4096; once more under AddressSanitizer / UBSan where their runtime links.  CPU
only: stand-alone programs (tests/host_check.py builds and runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_mcl.h", "const uint8_t field[4] = {1, 2, 3, 4}; const int C[4] = {0, 3, 3, 10}; "
                            "return !(smj_mcl_point_weight(0.0f, 0.0f, 1.0f, 0.0f, 0.75f, 0.75f, 0.0f, 0.0f, 0.5f, 2, 2, field) == 4 && smj_mcl_cut(9, 4) == 5 "
                            "&& smj_mcl_w(7, 5) == 2 && smj_mcl_offset(0x80000000u, 10) == 5u && smj_mcl_threshold(3, 10, 5u, 4) == 8 && smj_mcl_ancestor(C, 4, 3) == 3 "
                            "&& smj_mcl_ess(10, 50) == 2 && smj_mcl_status(30, 30, 0) == SMJ_MCL_LOST);")


def test_kernel_phases_against_the_programs_own_loops(tmp_path):
    print(host_check.check_program(tmp_path, "mcl"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "mcl", sanitizers=True))
