"""The base-command arithmetic the HIP kernel runs (stretch_mujoco_amd/csrc/smj_drive.h: the cell of a point, the swept
contribution, the window, the blocked predicate, the score, the (score, k) order and the status) compiled for the host by
g++ -Wall -Wextra -Werror and checked by a small C++ harness (tests/drive/drive_check.cpp), which emulates the kernel's reductions
with the kernel's own functions, in three evaluation orders and with lane and round partitions that straddle K = 63, 64, 65, and
holds them against a plain double loop on seeded maps full of score ties; once more under AddressSanitizer / UBSan where their
runtime links.  CPU only: stand-alone programs (tests/host_check.py builds and runs them), nothing is loaded into python."""
import host_check


def test_header_compiles_alone_under_a_host_compiler(tmp_path):
    host_check.header_alone(tmp_path, "smj_drive.h", "return !(smj_drive_cell(0.126f, 0.076f, 0.0f, 0.0f, 0.05f, 4, 4) == 6 && smj_drive_swept(-1, 0, 253, 0) == SMJ_DRIVE_SWEPT_BLOCKS "
                            "&& smj_drive_score(252, 1000, true, 1, 20, -3) == 6037 && smj_drive_before(5, 3, 5, 4) && smj_drive_status(true, 3, 100, 100, 5) == SMJ_DRIVE_ARRIVED);")


def test_reductions_against_a_double_loop(tmp_path):
    print(host_check.check_program(tmp_path, "drive"))


def test_the_same_under_sanitizers(tmp_path):
    print(host_check.check_program(tmp_path, "drive", sanitizers=True))
