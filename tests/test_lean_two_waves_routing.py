"""The two lean builds of the standard Newton kernel (csrc/smj_builds.h SMJ_LEAN_BUILDS and SMJ_LEAN_TWIN_BUILDS: one and two wavefronts
per env) and which of them option lean_build selects, pinned on the CPU: a C++ harness (tests/routing/lean2_check.cpp) loads a shipped
blob with the library's own loader, sets options through the library's own lists and prints what csrc/smj_variants.h routes
(smj_lean_pick + smj_route_lean, as smj_step calls them).  lean_build 0 / 1 / 2 select the general build / the build tagged `lean` / its
twin for the empty scene, and each disqualifier of smj_lean_eligible still selects the general build whichever lean build is asked for.

The two-wavefront build puts two waves on every SIMD at four envs per CU, so it must fit 256 registers per lane and 32 LDS granules
(40 960 B) per env: the first is read from the built library's code-object metadata (tools/kernel_resources.py), the second from the
kernel source's own Smem, compiled host-only as that build's translation unit sees it (tests/routing/lds_probe.hip)."""
import os
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stretch_mujoco_amd", "csrc")
MODELS = os.path.join(ROOT, "stretch_mujoco_amd", "models")
TAGS = "step pgs prof tall mid midp big38 big38p big50 big50p big sat sat1 sat2 satp sat32 sat32n".split()
LEAN_TAGS = ["lean", "lean2"]   # csrc/smj_builds.h SMJ_LEAN_BUILDS, SMJ_LEAN_TWIN_BUILDS; both units define SMJ_LEAN
K = "smj_step_kernel"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("lean2_routing")
    srcs = []
    for tag in TAGS + LEAN_TAGS:
        p = d / f"probe_{tag}.cpp"
        lean = "#define SMJ_LEAN 1\n" if tag in LEAN_TAGS else ""
        p.write_text(f"#define SMJ_BUILD_TAG {tag}\n{lean}#define PROBE_NAME probe_product_{tag}\n#include \"desc_probe.inc\"\n")
        srcs.append(str(p))
    exe = d / "lean2_check"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "routing"),
                           os.path.join(ROOT, "tests", "routing", "lean2_check.cpp")] + srcs + ["-o", str(exe)])

    def route(scene, *args):
        out = subprocess.run([str(exe), os.path.join(MODELS, scene + ".smjb")] + list(args), capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        w = out.stdout.split()
        return dict(zip(w[0::2], w[1::2]))

    return route


def _kernel(tag):
    return K if tag == "step" else f"{K}_{tag}"


def test_the_twin_unit_is_the_lean_unit_under_another_tag():
    """Wavefronts per env come from the build's row alone: the two translation units differ in the tag."""
    def code(name):
        with open(os.path.join(CSRC, name)) as f:
            return [ln.strip() for ln in f if ln.strip() and not ln.lstrip().startswith("//")]

    assert code("smj_kernels_lean2.hip") == ["#define SMJ_BUILD_TAG lean2", "#define SMJ_LEAN 1", '#include "smj_step_tu.h"']
    assert code("smj_kernels_lean.hip") == ["#define SMJ_BUILD_TAG lean", "#define SMJ_LEAN 1", '#include "smj_step_tu.h"']
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "smj_kernels_lean2.hip" in f.read()


def test_one_lean_build_has_one_wavefront_per_env_and_the_other_two(harness):
    r = harness("stretch_empty", "solver=2")
    assert sorted((r["lean_waves"], r["twin_waves"])) == ["1", "2"]
    assert {r["lean_kernel"], r["twin_kernel"]} == {K + "_lean", K + "_lean2"}


@pytest.mark.parametrize("lean_build, tag", [(0, "step"), (1, "lean"), (2, "lean2")])
def test_lean_build_selects_the_descriptor_for_the_empty_scene(harness, lean_build, tag):
    r = harness("stretch_empty", "solver=2", f"lean_build={lean_build}")
    assert r["variant"] == "standard" and r["general"] == "step"
    assert r["primary"] == tag and r["kernel"] == _kernel(tag)
    assert r["family"] == "std" and r["solvers"] == "1"   # SMJ_CARRIES_NEWTON
    # hand-over target, pollers and sweep stay the standard variant's
    assert r["poller"] == r["sweep"] == K + "_tall_worker" and r["same_hand_over"] == "1"


def test_the_two_wavefront_descriptor_says_two_waves_and_family_std(harness):
    seen = {}
    for lean_build in (1, 2):
        r = harness("stretch_empty", "solver=2", f"lean_build={lean_build}")
        seen[int(r["waves"])] = r
    assert sorted(seen) == [1, 2]
    assert seen[2]["family"] == "std" and seen[2]["variant"] == "standard" and seen[2]["solvers"] == "1"


def test_the_default_call_still_runs_the_build_tagged_lean(harness):
    r = harness("stretch_empty", "solver=2")
    assert r["primary"] == "lean" and r["kernel"] == K + "_lean"


@pytest.mark.parametrize("lean_build", [1, 2])
@pytest.mark.parametrize("args, general", [
    (("solver=2", "bind=debug"), "step"),          # a debug slot bound
    (("solver=2", "manifold_cache=1"), "step"),    # a folded option changed by smj_set_option
    (("solver=0",), "pgs"),                        # PGS
    (("solver=2", "bind=prof"), "prof"),           # the profiling slot: the lean builds have no counters
    (("solver=2", "nroot=2"), "step"),             # a second tree root
    (("solver=2", "unstaged"), "step"),            # state not on the staging rows
])
def test_each_disqualifier_alone_selects_the_general_build_whichever_lean_build_is_asked_for(harness, lean_build, args, general):
    r = harness("stretch_empty", *args, f"lean_build={lean_build}")
    assert r["variant"] == "standard" and r["general"] == general
    assert r["primary"] == general and r["kernel"] == _kernel(general) and r["waves"] == "1"
    assert r["poller"] == r["sweep"] == K + "_tall_worker" and r["same_hand_over"] == "1"


def test_a_scene_of_another_variant_ignores_the_option(harness):
    r = harness("stretch_scene", "solver=2", "lean_build=2")
    assert r["variant"] != "standard" and r["primary"] == r["general"] and r["primary"] not in LEAN_TAGS


def test_turning_the_option_back_and_forth(harness):
    assert harness("stretch_empty", "solver=2", "lean_build=2", "lean_build=1")["primary"] == "lean"
    assert harness("stretch_empty", "solver=2", "lean_build=0", "lean_build=2")["primary"] == "lean2"


def _two_wave_tag(harness):
    r = harness("stretch_empty", "solver=2")
    return "lean" if r["lean_waves"] == "2" else "lean2"


def test_the_two_wavefront_kernel_fits_two_waves_per_simd(harness):
    """Code-object metadata of the built library: on gfx950 .vgpr_count is the unified allocation, architectural + accumulation registers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import re

    import kernel_resources as kr

    tag = _two_wave_tag(harness)
    with open(os.path.join(ROOT, "stretch_mujoco_amd", "libsmj.so"), "rb") as f:
        blob = f.read()
    found = {}
    with tempfile.TemporaryDirectory() as d:
        for n, image in enumerate(kr.code_objects(blob)):
            if (K + "_" + tag).encode() not in image:
                continue
            for name, blk in kr.kernel_notes(image, d, n).items():
                if re.fullmatch(rf"_Z\d+{K}_{tag}8DevModel8DevStateij", name):
                    found[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in
                                   ("vgpr_count", "agpr_count", "group_segment_fixed_size", "max_flat_workgroup_size")}
    assert len(found) == 1, sorted(found)
    meta = next(iter(found.values()))
    print(f"\n{tag}: {meta}")
    assert meta["vgpr_count"] <= 256 and meta["agpr_count"] <= meta["vgpr_count"]
    assert meta["max_flat_workgroup_size"] == 128
    assert meta["group_segment_fixed_size"] == 0   # all of the env's LDS is dynamic: the launcher asks for sizeof(Smem), below


@pytest.mark.parametrize("which", ["two_waves", "one_wave"])
def test_the_lean_builds_take_32_lds_granules_per_env(harness, tmp_path, which):
    two = _two_wave_tag(harness)
    tag = two if which == "two_waves" else ({"lean", "lean2"} - {two}).pop()
    exe = tmp_path / "lds_probe"
    subprocess.check_call([HIPCC, "-O0", "-std=c++17", "--offload-arch=gfx950", "--offload-host-only", "-Wno-unused-variable", "-I", CSRC,
                           f"-DSMJ_BUILD_TAG={tag}", "-DSMJ_LEAN=1", os.path.join(ROOT, "tests", "routing", "lds_probe.hip"), "-o", str(exe)])
    w = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    r = dict(zip(w[0::2], w[1::2]))
    assert r["tag"] == tag and int(r["waves"]) == (2 if which == "two_waves" else 1) and int(r["w2_collision"]) == (which == "two_waves")
    assert int(r["lds_newton"]) == int(r["smem"]) <= 40960
    assert -(-int(r["smem"]) // 1280) == 32   # allocation granules of 1280 B: four envs per CU (163 840 B)
    assert int(r["j_offset"]) % 16 == 0
