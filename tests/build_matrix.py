"""THE TABLE OF DEVICE CASES PER STEP-KERNEL BUILD.  The step kernel is compiled once per row of csrc/smj_builds.h (SMJ_BUILDS) and once
more as the lean twin (SMJ_LEAN_BUILDS); each build is a translation unit of its own -- its own register allocation, its own
multiply-add contraction, its own SMJ_ONLY_NEWTON / SMJ_ONLY_PGS / SMJ_TWO_WAVES folds -- and the CPU lane emulator takes a build's
capacities only, so whether a compiled object computes the right step is seen on the device alone.  Plain data: one or more rows per
build tag, every tag at least once (tests/test_build_matrix.py holds the table to the library's own list of builds and to smj_route on
the CPU; tests/test_gpu_build_matrix.py runs the rows).  TEST INFRASTRUCTURE.

A row:
  tag      the build (csrc/smj_builds.h)
  role     "primary": smj_last_build reports the tag after EVERY step of the case, which compares each step with the fp64 oracle
           "sweep":   the build finishes steps the primary build `via` hands over (option primary_rows lowered under the scenario's rows)
           "twin":    the build is held by the existing device test(s) `held_by` = [(module, function)]: bit for bit against a
                      sibling that has a primary row, or a Newton hand-over test that predates this table
  scene    a shipped blob (stretch_mujoco_amd/models/<scene>.smjb), or model = "pile9": the generated pile of piles() below
  solver   2 Newton, 0 PGS
  options  smj_set_option names -> values that select the build (everything else at its default)
  slots    optional slots bound: ("DEBUG",) = rollout_common.HipBackend(counters=False), ("DEBUG", "PROF") = counters=True
  windows  windows of 50 steps of the state-synchronised run (B = 4)
  seed     of its random controls (5 unless the row says why not)
  script   sweep rows: (ctrl held from mj_resetData, settling steps before the compared 40, rows under the oracle's settled nefc)

OUT OF SCOPE, on purpose: `sat32` / `sat32n` as the PRIMARY kernel of a model with more than 16 satellites.  No shipped blob has more than
16, and compiling one needs MJCF assets a GPU machine does not have; both builds are covered as sweeps / bit-for-bit twins only."""
import math

NEWTON, PGS = 2, 0
DEBUG_ONLY, DEBUG_AND_PROF = ("DEBUG",), ("DEBUG", "PROF")

# the scripts of the Newton hand-over tests (tests/test_gpu_kitchen.py): arm onto the counter | driving, arm out and down towards the table / counter
COUNTER_SCRIPT = ([0.5, -0.5, 0.9, 0.5, 1.0, -0.5, 0.3, 0.0, 0.2, -0.3], 150, 4)
TABLE_SCRIPT = ([1.5, -1.5, 0.3, 0.4, 0, -1.2, 0, 0, 0.5, -0.5], 150, 6)


def _primary(tag, scene, solver, slots=DEBUG_AND_PROF, options=None, windows=2, seed=5, model=None):
    return dict(tag=tag, role="primary", scene=scene, model=model, solver=solver, options=dict(options or {}), slots=slots, windows=windows, seed=seed)


def _sweep(tag, via, scene, script):
    return dict(tag=tag, role="sweep", via=via, scene=scene, model=None, solver=PGS, options={}, slots=(), script=script)


def _twin(tag, *held_by):
    return dict(tag=tag, role="twin", held_by=list(held_by))


ROWS = [
    # ---- the standard variant: the two product builds need the profiling slot UNBOUND (with it smj_route sends both solvers to `prof`);
    # a bound debug slot keeps the lean twin out of the Newton row (smj_variants.h smj_lean_eligible)
    _primary("step", "stretch_empty", NEWTON, DEBUG_ONLY),
    _primary("pgs", "stretch_empty", PGS, DEBUG_ONLY),
    _primary("prof", "stretch_empty", NEWTON),
    _primary("prof", "stretch_empty", PGS),
    # ---- the dense capacity variants, Newton build and PGS twin each on the scene that makes the variant the model's own
    _primary("mid", "stretch_kitchen_standin", NEWTON),
    _primary("midp", "stretch_kitchen_standin", PGS),
    _primary("big38", "stretch_scene", NEWTON),
    # (seed 5 puts env 3's gripper on an object in window 1: both sides stop at the cap of 100 sweeps 3e-2 .. 5e-2 short of their OWN fixed
    # points -- at 400 sweeps and beyond they agree to 6e-3 -- and seven such steps are events no perturbation explains.  Seeds 6, 8 and 9 have
    # such a stretch too; seed 7 has none.  Chosen on the CPU through the lane emulator, before any device run.)
    _primary("big38p", "stretch_scene", PGS, seed=7),
    _primary("big50", "stretch_kitchen4", NEWTON),
    _primary("big50p", "stretch_kitchen4", PGS),
    # ---- the full 64 columns: nine free primitives, 54 dofs, the smallest count beyond big50's 50 columns
    _primary("big", None, NEWTON, (), model="pile9"),
    _primary("big", None, PGS, (), model="pile9"),
    # ---- the 16-satellite family: one and two wavefronts per env, both solvers
    _primary("sat", "stretch_scene_sat", NEWTON, DEBUG_ONLY, {"newton_two_waves": 0}),
    _primary("sat2", "stretch_scene_sat", NEWTON, DEBUG_ONLY),
    _primary("sat1", "stretch_kitchen4_sat", PGS, options={"pgs_two_waves": 0}),
    _primary("satp", "stretch_kitchen4_sat", PGS, options={"pgs_two_waves": 1}),
    # ---- PGS hand-overs
    _sweep("tall", "midp", "stretch_kitchen_standin", COUNTER_SCRIPT),
    _sweep("big", "big38p", "stretch_scene", (TABLE_SCRIPT[0], 320, 6)),   # (under PGS the oracle's rows of this scene wander between 41 and 81 until step 300 and rest at 72 from step 310 on)
    _sweep("big", "big50p", "stretch_kitchen4", TABLE_SCRIPT),
    _sweep("sat32", "satp", "stretch_kitchen4_sat", TABLE_SCRIPT),
    # ---- the Newton hand-overs keep the tests they have
    _twin("tall", ("test_gpu_kitchen", "test_three_envs_per_cu_build_hands_over_to_the_160_row_build"),
          ("test_gpu_parity", "test_capacity_escalation_matches_the_capacity_free_oracle")),
    _twin("big", ("test_gpu_kitchen", "test_big_builds_hand_over_to_the_224_row_build")),
    _twin("sat32", ("test_satellites", "test_gpu_satellite_build_hands_over_to_the_large_build")),
    # ---- builds held bit for bit against a sibling with a primary row
    _twin("lean", ("test_gpu_lean", "test_gpu_lean_build_equals_general_build_bit_for_bit_over_three_launches")),
    _twin("sat32n", ("test_satellites", "test_gpu_newton_two_wavefronts_per_env_equal_one_bit_for_bit"),
          ("test_satellites", "test_gpu_newton_two_wavefronts_at_scale_with_contact_overflow")),
]


def row_id(row):
    if row["role"] == "sweep":
        return f"{row['tag']}-from-{row['via']}"
    if row["role"] == "twin":
        return f"{row['tag']}-twin"
    return f"{row['tag']}-{'newton' if row['solver'] == NEWTON else 'pgs'}"


def rows(role, pile=None):
    """The rows of a role; pile: True / False keeps only the rows on the generated pile / on a shipped scene."""
    return [r for r in ROWS if r["role"] == role and (pile is None or (r.get("model") == "pile9") == pile)]


PILE_SEED, PILE_BODIES, PILES = 23, 9, 2
PILE_SETTLE = 1000   # oracle steps before the compared 100: all nine bodies rest on each other then (25 / 17 contacts, 75 / 51 rows); from the drop only the lowest body touches (at most 7 contacts)


def piles():
    """The MJCF of the `big` rows' models: PILES robot-less piles of nine free primitives dropped on a box and the plane, generated as
    test_collision_fuzz.test_gpu_piles_of_primitives_state_synchronised generates its five- and eight-body piles (same shapes, same angle
    set, same placement rule)."""
    import numpy as np

    from test_collision_fuzz import OPT, SHAPES

    rng = np.random.default_rng(PILE_SEED)
    ang = [0, math.pi / 2, math.pi / 4, 0.3, -math.pi / 2]
    out = []
    for _ in range(PILES):
        bodies = ""
        for k in range(PILE_BODIES):
            a = rng.choice(list(SHAPES)); ta, sa, _ = SHAPES[a]
            e = [rng.choice(ang), rng.choice(ang), rng.choice(ang)]
            bodies += (f'<body pos="{rng.uniform(-0.25, 0.25):.3f} {rng.uniform(-0.2, 0.2):.3f} {0.35 + 0.28 * k:.3f}" euler="{e[0]} {e[1]} {e[2]}"><freejoint/>'
                       f'<geom type="{ta}" size="{sa}" mass="{rng.uniform(0.2, 1.5):.2f}"/></body>')
        out.append('<mujoco><compiler angle="radian"/>' + OPT + '<option timestep="0.002"/><worldbody><geom type="plane" size="0 0 1"/>'
                   '<geom type="box" size=".35 .3 .1" pos="0 0 0.1"/>' + bodies + '</worldbody></mujoco>')
    return out


def pile_blobs():
    from stretch_mujoco_amd import mjcf_compiler, model_blob, model_fuse

    return [model_blob.dumps(model_fuse.prepare_for_kernels(mjcf_compiler.compile_string(x))) for x in piles()]


def blob_of(row):
    """The model a primary / sweep row runs (for the pile rows: the first pile)."""
    import os

    from conftest import MODELS

    if row.get("model") == "pile9":
        return pile_blobs()[0]
    with open(os.path.join(MODELS, row["scene"] + ".smjb"), "rb") as f:
        return f.read()
