"""The height-map arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_hmap.h: the order-preserving key, the cell rule, the
cut into bands, the split of a band store) compiled for the host by g++ -Wall -Wextra -Werror and checked by a small C++ harness
(tests/hmap/hmap_check.cpp), which also emulates the kernel's scatter serially on a seeded image and holds it against long-hand fp64
by the comparison rule of tests/height_map_ref.py; once more under AddressSanitizer / UBSan where their runtime links.  CPU only:
stand-alone programs (tests/host_check.py builds and runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_hmap.h", "return smj_hmap_key(1.f) == 0u;")


def test_key_cell_rule_bands_and_scatter(tmp_path):
    print(host_check.check_program(tmp_path, "hmap"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "hmap", sanitizers=True))
