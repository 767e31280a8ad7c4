"""Which builds of the step kernel a step call launches (stretch_mujoco_amd/csrc/smj_variants.h over the build table of smj_builds.h),
pinned on the CPU: a small C++ harness (tests/routing) links the routing function with descriptors made exactly as each translation unit
makes its own -- for the product library and for the tools library whose big38, big50, sat, sat2 and satp objects are profiling copies --
and prints the route of every combination; the expectations below are written out from the routing table of the design, not computed by
the code under test."""
import itertools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stretch_mujoco_amd", "csrc")
TAGS = "step pgs prof tall mid midp big38 big38p big50 big50p big sat sat1 sat2 satp sat32 sat32n".split()
PROFILING_COPIES = {"big38", "big50", "sat", "sat2", "satp"}   # csrc/Makefile PROFTU
FAMILIES = {"std": ["step", "pgs", "prof"], "tall": ["tall"], "mid": ["mid", "midp"], "big38": ["big38", "big38p"], "big50": ["big50", "big50p"],
            "big": ["big"], "sat16": ["sat", "sat1", "sat2", "satp"], "sat32": ["sat32", "sat32n"]}
K = "smj_step_kernel"


def run_harness(tmp_path):
    srcs = []
    for lib in ("product", "bigprof"):
        for tag in TAGS:
            p = tmp_path / f"probe_{lib}_{tag}.cpp"
            prof = "#define SMJ_PROFILING 1\n" if lib == "bigprof" and tag in PROFILING_COPIES else ""
            p.write_text(f"#define SMJ_BUILD_TAG {tag}\n{prof}#define PROBE_NAME probe_{lib}_{tag}\n#include \"desc_probe.inc\"\n")
            srcs.append(str(p))
    exe = tmp_path / "routing_check"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "routing"),
                           os.path.join(ROOT, "tests", "routing", "routing_check.cpp")] + srcs + ["-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    return out.stdout.splitlines()


def expected_route(lib, variant, solver, prof, n2w_opt, p2w):
    """(primary kernel, poller kernel, sweep kernel, chunk length at pipeline = 5, pollers at pollers = 2): the routing table."""
    newton = solver == 2
    n2w = 3 if n2w_opt == 1 else n2w_opt
    has_counters = lambda tag: tag == "prof" or (lib == "bigprof" and tag in PROFILING_COPIES)

    def sat32_choice():
        return "sat32n" if newton and (n2w & 2) and not prof else "sat32"

    if variant == 0:
        primary, esc, chunk, pollers = ("prof" if prof else "step" if newton else "pgs"), "tall", 5, 2
    elif variant in (1, 2, 3):
        base, esc, chunk = {1: ("mid", "tall", 8), 2: ("big38", "big", 10), 3: ("big50", "big", 10)}[variant]
        both_solvers_and_counters = lib == "bigprof" and base in PROFILING_COPIES   # the profiling copies of big38 / big50 keep PGS
        primary = base if newton or (prof and both_solvers_and_counters) else base + "p"
        pollers = 0
    elif variant == 4:
        primary, esc, chunk, pollers = "big", None, None, 0
    elif variant == 5:
        if newton:
            primary = "sat2" if (n2w & 1) and (not prof or has_counters("sat2")) else "sat"
        else:
            primary = "satp" if p2w else "sat1"
        esc, chunk, pollers = sat32_choice(), 10, 12
    else:
        primary, esc, chunk, pollers = sat32_choice(), None, None, 0
    name = lambda tag: K if tag == "step" else f"{K}_{tag}"
    sweep = name(esc) + "_worker" if esc else "-"
    return name(primary), (sweep if pollers else "-"), sweep, chunk, pollers


def test_routing_of_every_variant_solver_and_option(tmp_path):
    lines = run_harness(tmp_path)
    routes = {}
    for ln in lines:
        w = ln.split()
        if w[0] == "route":
            routes[(w[1],) + tuple(int(x) for x in w[2:7])] = (w[8], w[10], w[12], int(w[14]), int(w[16]), int(w[18]), int(w[20]))
    combos = list(itertools.product(("product", "bigprof"), range(7), (0, 2), (0, 1), (0, 1, 2, 5), (0, 1)))
    assert len(combos) == 448 and set(routes) == set(combos)
    for key in combos:
        lib, variant, solver, prof, n2w_opt, p2w = key
        primary, poller, sweep, chunk, pipelines, pollers, no_counters = routes[key]
        e_primary, e_poller, e_sweep, e_chunk, e_pollers = expected_route(*key)
        assert (primary, poller, sweep, pollers) == (e_primary, e_poller, e_sweep, e_pollers), (key, routes[key])
        assert pipelines == {0: 1, 1: 1, 2: 2, 3: 2, 4: 0, 5: 2, 6: 0}[variant], key   # 1: always, 2: if option pipeline_big, 0: never
        if e_chunk is not None:
            assert chunk == e_chunk, (key, chunk)
        # the once-per-context warning: PGS with the profiling slot bound on a variant with a PGS twin, and the kernel launched has no counters
        launched_has_counters = primary == K + "_prof" or (lib == "bigprof" and primary.replace(K + "_", "") in PROFILING_COPIES)
        assert no_counters == int(bool(prof) and solver == 0 and variant in (1, 2, 3, 5) and not launched_has_counters), (key, routes[key])


def test_builds_of_one_family_have_equal_capacities(tmp_path):
    builds = {}
    for ln in run_harness(tmp_path):
        w = ln.split()
        if w[0] == "build":
            builds[(w[1], w[2])] = dict(family=w[4], caps=tuple(int(x) for x in w[6:13]), dbg=int(w[14]), solvers=int(w[16]), waves=int(w[18]),
                                        profiling=int(w[20]), kernel=w[22], worker=w[24])
    assert set(builds) == set(itertools.product(("product", "bigprof"), TAGS))
    for family, tags in FAMILIES.items():
        first = builds[("product", tags[0])]
        for lib in ("product", "bigprof"):
            for tag in tags:
                b = builds[(lib, tag)]
                assert b["family"] == family and b["caps"] == first["caps"] and b["dbg"] == first["dbg"], (lib, tag, b, first)
    assert sorted(t for fam in FAMILIES.values() for t in fam) == sorted(TAGS)
    # (nvp, nbp, nent, nefc, ncon, nvs, nsat): the shipped capacities
    assert builds[("product", "step")]["caps"] == (32, 32, 5, 80, 16, 32, 0) and builds[("product", "tall")]["caps"] == (32, 32, 5, 160, 48, 32, 0)
    assert builds[("product", "mid")]["caps"] == (32, 32, 5, 128, 44, 32, 0) and builds[("product", "big")]["caps"] == (64, 32, 8, 224, 64, 64, 0)
    assert builds[("product", "big38")]["caps"] == (64, 32, 8, 160, 48, 38, 0) and builds[("product", "big50")]["caps"] == (64, 32, 8, 160, 48, 50, 0)
    assert builds[("product", "sat")]["caps"] == (32, 32, 5, 208, 56, 32, 16) and builds[("product", "sat32")]["caps"] == (32, 32, 5, 320, 64, 32, 32)
    for (lib, tag), b in builds.items():
        assert b["profiling"] == int(tag == "prof" or (lib == "bigprof" and tag in PROFILING_COPIES)), (lib, tag)
        assert b["waves"] == (2 if tag in ("sat2", "satp", "sat32n") else 1), (lib, tag)
        newton_only = tag in ("step", "sat", "sat2", "sat32n") or (tag in ("mid", "big38", "big50") and not b["profiling"])
        pgs_only = tag in ("pgs", "midp", "big38p", "big50p", "sat1", "satp")
        assert b["solvers"] == (1 if newton_only else 2 if pgs_only else 3), (lib, tag)
        assert b["kernel"] == (K if tag == "step" else f"{K}_{tag}"), (lib, tag)
        assert b["worker"] == (f"{K}_{tag}_worker" if tag in ("tall", "big", "sat32", "sat32n") else "-"), (lib, tag)
