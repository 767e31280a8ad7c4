"""When a step call runs the lean twin of the standard Newton build (stretch_mujoco_amd/csrc/smj_kernels_lean.hip; what it leaves out:
smj_step_impl.h SMJ_LEAN) and when the general build, pinned on the CPU: a small C++ harness (tests/routing/lean_check.cpp) loads a
shipped model blob with the library's own loader, sets options and binds slots through the library's own code, and prints what
smj_variants.h routes.  The lean build folds kept manifolds off, no debug slot, staged state and one tree root; a call launches it only
when every one of these holds, the variant is the standard one, the solver is Newton and no profiling slot is bound.  Each
disqualifier ALONE must send the call to the general build, and the hand-over target, pollers and sweep never change.

The robot's own base is a free joint, so the free-joint branches of the kernel are NOT folded and a free joint does not disqualify a
model; `stretch_scene` (the robot, a table and two free objects) goes to the general build because its free objects are tree roots of
their own (and make it a model of another variant)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stretch_mujoco_amd", "csrc")
MODELS = os.path.join(ROOT, "stretch_mujoco_amd", "models")
TAGS = "step pgs prof tall mid midp big38 big38p big50 big50p big sat sat1 sat2 satp sat32 sat32n".split()
K = "smj_step_kernel"


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("lean_routing")
    srcs = []
    for tag in TAGS + ["lean"]:
        p = d / f"probe_{tag}.cpp"
        lean = "#define SMJ_LEAN 1\n" if tag == "lean" else ""   # as csrc/smj_kernels_lean.hip defines it
        p.write_text(f"#define SMJ_BUILD_TAG {tag}\n{lean}#define PROBE_NAME probe_product_{tag}\n#include \"desc_probe.inc\"\n")
        srcs.append(str(p))
    exe = d / "lean_check"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "routing"),
                           os.path.join(ROOT, "tests", "routing", "lean_check.cpp")] + srcs + ["-o", str(exe)])

    def route(scene, *args):
        out = subprocess.run([str(exe), os.path.join(MODELS, scene + ".smjb")] + list(args), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        w = out.stdout.split()
        return dict(zip(w[0::2], w[1::2]))

    return route


def test_the_lean_translation_unit_is_the_standard_newton_build_plus_the_switch():
    with open(os.path.join(CSRC, "smj_kernels_lean.hip")) as f:
        code = [ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith("//")]
    assert code == ["#define SMJ_BUILD_TAG lean", "#define SMJ_LEAN 1", '#include "smj_step_tu.h"']
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "smj_kernels_lean.hip" in f.read()


def test_the_empty_scene_with_default_options_runs_the_lean_build(harness):
    r = harness("stretch_empty", "solver=2")
    assert r["variant"] == "standard" and r["general"] == "step"
    assert r["primary"] == "lean" and r["kernel"] == K + "_lean"
    # the same hand-over target, pollers and sweep as the standard variant's general build
    assert r["poller"] == r["sweep"] == K + "_tall_worker" and r["same_hand_over"] == "1"
    assert (r["nroot"], r["manifold_cache"]) == ("1", "0")   # the folded values ARE this model's defaults


@pytest.mark.parametrize("args, general", [
    (("solver=2", "bind=debug"), "step"),          # a debug slot bound (later or from the start)
    (("solver=2", "manifold_cache=1"), "step"),    # a folded option changed by smj_set_option
    (("solver=0",), "pgs"),                        # PGS
    (("solver=2", "lean_build=0"), "step"),        # the switch
    (("solver=2", "bind=prof"), "prof"),           # the profiling slot: the lean build has no counters
    (("solver=2", "nroot=2"), "step"),             # a second tree root: the exact residual the lean build leaves out
    (("solver=2", "unstaged"), "step"),            # state not on the staging rows
])
def test_each_disqualifier_alone_selects_the_general_build(harness, args, general):
    r = harness("stretch_empty", *args)
    assert r["variant"] == "standard" and r["general"] == general
    assert r["primary"] == general and r["kernel"] == (K if general == "step" else f"{K}_{general}")
    assert r["poller"] == r["sweep"] == K + "_tall_worker" and r["same_hand_over"] == "1"


def test_a_scene_with_free_objects_runs_the_general_build(harness):
    r = harness("stretch_scene", "solver=2")
    assert r["variant"] != "standard" and r["primary"] == r["general"] != "lean"
    assert int(r["nroot"]) > 1


def test_turning_the_option_back_restores_the_lean_build(harness):
    assert harness("stretch_empty", "solver=2", "manifold_cache=1", "manifold_cache=0")["primary"] == "lean"
    assert harness("stretch_empty", "solver=2", "lean_build=0", "lean_build=1")["primary"] == "lean"
