"""The ray-primitive arithmetic the lidar and depth kernels run (stretch_mujoco_amd/csrc/smj_ray.h: ray_quad, ray_prim_any, ray_prim)
compiled for the host by g++ -Wall -Wextra -Werror and evaluated in fp32 by a small C++ harness (tests/ray/ray_check.cpp) against fp64
closed forms written there as intervals: general poses, the origin inside, exact alignments, thin shapes at range -- the fp32 error
within 16 x the input-rounding floor of each group, hit or miss the same on every ray; once more under AddressSanitizer / UBSan where
their runtime links.  CPU only: stand-alone programs (tests/host_check.py builds and runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_ray.h", "const float p[3] = {-3.f, 0.f, 0.f}, v[3] = {1.f, 0.f, 0.f}, s[3] = {0.5f, 0.f, 0.f}; "
                            "return !(ray_prim_any(RT_SPHERE, s, p, v) == 2.5f && ray_prim(RT_SPHERE, s, p, v, 0.f) == 2.5f && ray_quad(p, v, 0.25f) == 2.5f);")


def test_primitives_in_fp32_against_fp64_intervals(tmp_path):
    print(host_check.check_program(tmp_path, "ray"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "ray", sanitizers=True))
