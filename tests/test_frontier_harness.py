"""The frontier arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_front.h: the state of a cell, the frontier predicate, find
and union, the jump, the schedule, the codes of a root's slot, the order key and the representative's key) compiled for the host by
g++ -Wall -Wextra -Werror and checked by a small C++ harness (tests/front/front_check.cpp), which emulates the kernel's phases with
the kernel's own functions, in both storage modes' indexing and three orders of the union phase, and holds them against its own flood
fill on seeded maps, the serpentine, a spiral and maps full of ties; once more under AddressSanitizer / UBSan where their runtime
links.  CPU only: stand-alone programs (tests/host_check.py builds and runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_front.h", "return !(smj_front_state(1, 0, 2) == SMJ_FRONT_UNKNOWN && smj_front_code(0, 1, 253, 1, 253) == SMJ_FRONT_BLOCKED "
                            "&& smj_front_key_label(smj_front_order_key(9, 12)) == 12 && smj_front_rep_key(9, 21, 15, 2, 2) == 18 && smj_front_max_jumps() == 17);")


def test_phases_against_a_flood_fill(tmp_path):
    print(host_check.check_program(tmp_path, "front"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "front", sanitizers=True))
