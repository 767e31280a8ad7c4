"""How a step call is launched (stretch_mujoco_amd/csrc/smj_step_plan.h: the table of host-side scheduling options, the architecture
gate and the pure function smj_plan_step that smj_step and the launchers of smj_step_tu.h carry out), pinned on the CPU: a small C++
harness (tests/routing/plan_check.cpp) sets options by name through the library's own list, routes with descriptors made exactly as each
translation unit makes its own, and prints the plan.  The expectations below are written out by hand from the thresholds of the design
(511 / 1024 envs, calls longer than one chunk, 16 * B list entries, sweeps of 64 / 512 workgroups, pollers times the variant's
multiplier), not computed by the code under test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stretch_mujoco_amd", "csrc")
TAGS = "step pgs prof tall mid midp big38 big38p big50 big50p big sat sat1 sat2 satp sat32 sat32n".split()
DEFAULTS = dict(escalate=1, balance=1, balance_min=1, balance_min_envs=1024, pipeline=5, pipeline_big=1, pipeline_min_envs=511, pollers=2,
                pollers_always=0, newton_two_waves=3, pgs_two_waves=1, lean_build=1)
NAMES = [n for n in DEFAULTS if n != "pollers_always"]   # what smj_set_option takes by name


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("step_plan")
    srcs = []
    for tag in TAGS:
        p = d / f"probe_{tag}.cpp"
        p.write_text(f"#define SMJ_BUILD_TAG {tag}\n#define PROBE_NAME probe_product_{tag}\n#include \"desc_probe.inc\"\n")
        srcs.append(str(p))
    exe = d / "plan_check"
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "routing"),
                           os.path.join(ROOT, "tests", "routing", "plan_check.cpp")] + srcs + ["-o", str(exe)])

    def run(*args, rc=0):
        out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert out.returncode == rc, out.stdout + out.stderr
        lines = []
        for ln in out.stdout.splitlines():
            w = ln.split()
            lines.append(dict(zip(w[0::2], (int(x) if x.lstrip("-").isdigit() else x for x in w[1::2]))))
        return lines

    return run


@pytest.fixture(scope="module")
def plan(harness):
    def one(variant, B, *args):
        """the plans of the calls (`n=...`) among the arguments, in order; a single call: its plan"""
        plans = harness(f"variant={variant}", f"B={B}", *args)
        assert len(plans) == sum(a.startswith("n=") for a in args)
        return plans[0] if len(plans) == 1 else plans

    return one


def has(p, **expected):
    got = {k: p[k] for k in expected}
    assert got == expected, p


# ---- the standard variant (Newton, no debug or profiling slot, default options, gfx950 unless the case says otherwise)

def test_standard_4096_envs_50_steps_is_the_full_machinery(plan):
    has(plan("standard", 4096, "n=50"), has_esc=1, esc=1, pipe=1, pipe_len=5, pipe_total=40960, clear_sched=1, redo_need=40960, redo_cap_before=65536,
        grow=0, mark_unpublished=1, ordered=1, poll=1, poller_arg=2, poller_wgs=2, sweep=1, sweep_wgs=512)


def test_pipelining_starts_above_511_envs(plan):
    has(plan("standard", 512, "n=50"), pipe=1, pipe_len=5, pipe_total=5120, ordered=0, poll=1, poller_arg=2)
    has(plan("standard", 511, "n=50"), esc=1, pipe=0, pipe_len=0, pipe_total=511, clear_sched=1, redo_need=511, grow=0, mark_unpublished=0, poll=0,
        sweep=1, sweep_wgs=511)


def test_pipelining_needs_a_call_longer_than_one_chunk(plan):
    has(plan("standard", 4096, "n=5"), pipe=0, pipe_len=0, pipe_total=4096, poll=0, mark_unpublished=0)
    has(plan("standard", 4096, "n=6"), pipe=1, pipe_len=5, pipe_total=8192, poll=1)


def test_sweep_sizes(plan):
    has(plan("standard", 4096, "n=1"), sweep=1, sweep_wgs=64, ordered=1, pipe=0)
    has(plan("standard", 4096, "n=2"), sweep=1, sweep_wgs=64)
    has(plan("standard", 4096, "n=3"), sweep=1, sweep_wgs=512)
    has(plan("standard", 48, "n=1"), sweep=1, sweep_wgs=48)
    has(plan("standard", 48, "n=50"), sweep=1, sweep_wgs=48)


def test_the_escalation_list_starts_at_16_entries_per_env_and_grows_once(plan):
    long_call, next_call = plan("standard", 4096, "n=200", "n=50")
    has(long_call, pipe_total=163840, redo_need=163840, redo_cap_before=65536, grow=1)
    has(next_call, pipe_total=40960, redo_need=40960, redo_cap_before=163840, grow=0)


@pytest.mark.parametrize("slot", ["debug", "prof"])
def test_a_bound_debug_or_profiling_slot_switches_pipelining_off(plan, slot):
    has(plan("standard", 4096, f"bind={slot}", "n=50"), esc=1, pipe=0, pipe_len=0, pipe_total=4096, clear_sched=1, redo_need=4096, mark_unpublished=0,
        poll=0, sweep=1, sweep_wgs=512, ordered=1)


def test_options_of_the_standard_variant(plan):
    has(plan("standard", 4096, "escalate=0", "n=50"), esc=0, pipe=1, pipe_total=40960, clear_sched=1, redo_need=0, grow=0, mark_unpublished=0, poll=0, sweep=0)
    has(plan("standard", 4096, "pipeline=0", "n=50"), pipe=0, pipe_len=0, pipe_total=4096, poll=0, sweep=1)
    has(plan("standard", 4096, "pipeline=10", "n=50"), pipe=1, pipe_len=10, pipe_total=20480)
    has(plan("standard", 4096, "pollers=0", "n=50"), esc=1, pipe=1, poll=0, mark_unpublished=0, sweep=1)
    has(plan("standard", 4096, "pollers=-2", "n=50"), poll=1, poller_arg=-2, poller_wgs=2)
    has(plan("standard", 4096, "pipeline_min_envs=4096", "n=50"), pipe=0)
    has(plan("standard", 4096, "pipeline_big=0", "n=50"), pipe=1)   # (the standard variant always pipelines)


def test_cost_ordered_dispatch(plan):
    has(plan("standard", 4096, "balance=0", "n=50"), ordered=0)
    has(plan("standard", 4096, "balance_min=4", "n=3"), ordered=0)
    has(plan("standard", 4096, "balance_min=4", "n=4"), ordered=1)
    has(plan("standard", 1024, "n=50"), ordered=0, pipe=1)
    has(plan("standard", 1025, "n=50"), ordered=1)
    has(plan("standard", 1024, "balance_min_envs=1023", "n=50"), ordered=1)


# ---- the other variants

def test_mid_chunks_of_eight_and_no_pollers(plan):
    # mark_unpublished: set as for the standard variant although this variant routes no poller -- nobody reads the marks there
    has(plan("mid", 4096, "n=50"), esc=1, pipe=1, pipe_len=8, pipe_total=28672, poll=0, poller_wgs=0, mark_unpublished=1, sweep=1, sweep_wgs=512)
    has(plan("mid", 4096, "pipeline=10", "n=50"), pipe=1, pipe_len=15, pipe_total=4 * 4096)


@pytest.mark.parametrize("variant", ["big38", "big50"])
def test_two_envs_per_cu_builds_pipeline_in_chunks_of_ten(plan, variant):
    has(plan(variant, 4096, "n=50"), esc=1, pipe=1, pipe_len=10, pipe_total=20480, poll=0, sweep=1)
    has(plan(variant, 4096, "n=10"), pipe=0, pipe_total=4096)
    has(plan(variant, 4096, "n=11"), pipe=1, pipe_len=10, pipe_total=8192)
    has(plan(variant, 4096, "pipeline_big=0", "n=50"), pipe=0, pipe_len=0, pipe_total=4096, esc=1, sweep=1)


@pytest.mark.parametrize("variant", ["big", "sat32"])
@pytest.mark.parametrize("B, n", [(48, 1), (4096, 50), (8192, 200)])
def test_variants_without_a_target_run_one_workgroup_per_env_and_nothing_else(plan, variant, B, n):
    has(plan(variant, B, f"n={n}"), has_esc=0, esc=0, pipe=0, pipe_len=0, pipe_total=B, clear_sched=0, redo_need=0, grow=0, mark_unpublished=0, poll=0, sweep=0)


def test_sat_six_pollers_per_unit(plan):
    has(plan("sat", 1024, "n=50"), esc=1, pipe=1, pipe_len=10, pipe_total=5120, ordered=0, poll=1, poller_arg=12, poller_wgs=12, sweep=1)
    has(plan("sat", 1024, "pollers=-3", "n=50"), poll=1, poller_arg=-18, poller_wgs=18)
    has(plan("sat", 1024, "pollers=300", "n=50"), poll=1, poller_arg=1536, poller_wgs=1536)
    has(plan("sat", 1024, "pollers=-300", "n=50"), poll=1, poller_arg=-1536, poller_wgs=1536)


# ---- the architecture gate of smj_create

@pytest.mark.parametrize("arch", ["gfx950", "gfx942", "gfx940", "gfx950:sramecc+"])
def test_architectures_with_in_order_dispatch_keep_the_defaults(harness, arch):
    assert harness("options", f"arch={arch}") == [DEFAULTS]


@pytest.mark.parametrize("arch", ["gfx90a", "gfx1100", "gfx9", "", "null"])
def test_any_other_architecture_and_a_failed_query_switch_pipelining_and_pollers_off(harness, arch):
    assert harness("options", f"arch={arch}") == [dict(DEFAULTS, pipeline=0, pollers=0)]


def test_an_explicit_option_overrides_the_gate(plan):
    gated, asked = plan("standard", 4096, "arch=gfx90a", "n=50", "pipeline=5", "n=50")
    has(gated, esc=1, pipe=0, pipe_total=4096, poll=0, mark_unpublished=0, sweep=1)
    has(asked, esc=1, pipe=1, pipe_len=5, pipe_total=40960, poll=0, mark_unpublished=0, sweep=1)   # (the pollers stay off until asked for too)
    has(plan("standard", 4096, "arch=gfx90a", "pipeline=5", "pollers=2", "n=50"), pipe=1, poll=1, poller_arg=2, mark_unpublished=1)


# ---- static rows instead of dynamic LDS for a PGS launch that can hand steps over

def test_pgs_static_choice(harness):
    choice = lambda *a: harness("pgs_static", *a)[0]
    full, smem = 98304, 40956
    assert choice(0, 1, 0, full, smem, 96) == dict(lds=smem, pgs_cap=96)
    assert choice(2, 1, 0, full, smem, 96) == dict(lds=full, pgs_cap=0)     # Newton
    assert choice(0, 0, 0, full, smem, 96) == dict(lds=full, pgs_cap=0)     # no list: nobody to hand a step to
    assert choice(0, 1, 1, full, smem, 96) == dict(lds=full, pgs_cap=0)     # the sweep
    assert choice(0, 1, 2, full, smem, 96) == dict(lds=full, pgs_cap=0)     # a poller
    assert choice(0, 1, 0, smem, smem, 96) == dict(lds=smem, pgs_cap=0)     # the full request is no larger than the struct
    assert choice(0, 1, 0, smem - 4, smem, 96) == dict(lds=smem - 4, pgs_cap=0)
    assert choice(0, 1, 0, full, smem, 0) == dict(lds=full, pgs_cap=0)      # a build without static rows


# ---- the option table

def test_defaults(harness):
    assert harness("options") == [DEFAULTS]


@pytest.mark.parametrize("name", NAMES)
def test_every_option_of_the_list_round_trips(harness, name):
    assert harness("options", f"{name}=7") == [dict(DEFAULTS, **{name: 7})]
    assert harness("options", f"{name}=7", f"{name}=0") == [dict(DEFAULTS, **{name: 0})]


def test_the_two_options_that_are_not_plain_assignments(harness):
    assert harness("options", "newton_two_waves=1") == [dict(DEFAULTS, newton_two_waves=3)]
    assert harness("options", "newton_two_waves=5") == [dict(DEFAULTS, newton_two_waves=5)]
    assert harness("options", "pollers=-3") == [dict(DEFAULTS, pollers=3, pollers_always=1)]
    assert harness("options", "pollers=-3", "pollers=4") == [dict(DEFAULTS, pollers=4, pollers_always=0)]
    assert harness("options", "pollers=300") == [dict(DEFAULTS, pollers=256)]
    assert harness("options", "pollers=-1000") == [dict(DEFAULTS, pollers=256, pollers_always=1)]


@pytest.mark.parametrize("name", ["chunk", "pipelin", "Pipeline", "pollers_always", "pipe_min_envs", "primary_rows", "lidar_cull", "iterations"])
def test_names_the_list_does_not_hold_are_refused(harness, name):
    # (primary_rows, lidar_cull and the solver options are smj_set_option's business, not this list's; `chunk` is gone)
    assert harness("options", f"{name}=1", rc=3) == [dict(refused=name)]


def test_the_library_takes_these_options_from_the_list_alone():
    with open(os.path.join(CSRC, "smj_capi.hip")) as f:
        capi = f.read()
    assert "smj_set_step_option(c->opt, name, v)" in capi
    for name in NAMES + ["chunk"]:
        assert f'"{name}"' not in capi, name
