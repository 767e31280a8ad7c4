"""The mapping arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_map.h: the status of an env, the line of a ray laid into
the map from a pose, the info word of a ray, the steps of a line inside a band) compiled for the host by g++ -Wall -Wextra -Werror
and checked by a small C++ harness (tests/map/map_check.cpp), which holds the band-clipped range against the brute-force set for
every band of five grids and emulates the kernel's records, walk and counters with the kernel's own functions against its own loops;
once more under AddressSanitizer / UBSan where their runtime links.  CPU only: stand-alone programs (tests/host_check.py builds and
runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_map.h", "const float o[2] = {0.5f, 0.0f}, d[2] = {1.0f, 0.0f}; int lo, hi; "
                            "const smj_occ_line_t L = smj_map_line(SMJ_OCC_RETURN, o, d, 2.0f, 1.0f, 1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.5f); "
                            "smj_map_range(L, smj_occ_steps(L), smj_hmap_band(8, 8, 16, 2), &lo, &hi); "
                            "return !(L.ax == 2 && L.ay == 3 && L.bx == 2 && L.by == 7 && lo == 1 && hi == 2 && smj_map_status(0.0f, 0.0f, 0.0f, 4) == SMJ_MAP_GATED "
                            "&& smj_map_info_word(SMJ_OCC_CLEAR, SMJ_OCC_DROP) == 3);")


def test_kernel_phases_against_the_programs_own_loops(tmp_path):
    print(host_check.check_program(tmp_path, "map"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "map", sanitizers=True))
