"""The table of device cases per step-kernel build (tests/build_matrix.py) against the library's own tables, on the CPU: every build the
library lists has a row, every primary row's tag is the build smj_route launches for that row's model, solver, slots and options, and
every twin row names a test that exists.  The builds and routes come from the routing harness (tests/routing: descriptors made as each
translation unit makes its own, csrc/smj_variants.h linked in), the variant from the loader's own choice (emul.default_variant)."""
import importlib

import pytest

import build_matrix as bm
from emul import emul
from test_build_routing import run_harness

K = "smj_step_kernel"
LEAN_TAGS = {"lean"}   # csrc/smj_builds.h SMJ_LEAN_BUILDS: not a row smj_route chooses among, so not in the harness's list (tests/test_lean_routing.py pins the swap)
N2W_DEFAULT, P2W_DEFAULT = 1, 1   # options newton_two_waves / pgs_two_waves as smj_create leaves them (csrc/smj_step_plan.h: 3, which option value 1 stores; 1)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    builds, routes = set(), {}
    for ln in run_harness(tmp_path_factory.mktemp("routing")):
        w = ln.split()
        if w[0] == "build" and w[1] == "product":
            builds.add(w[2])
        elif w[0] == "route" and w[1] == "product":
            routes[tuple(int(x) for x in w[2:7])] = w[8]   # (variant, solver, prof, newton_two_waves, pgs_two_waves) -> primary kernel
    return builds, routes


def test_every_build_of_the_library_has_a_device_case(harness):
    builds, _ = harness
    assert len(builds) == 17
    assert {r["tag"] for r in bm.ROWS} == builds | LEAN_TAGS
    assert all(r["role"] in ("primary", "sweep", "twin") for r in bm.ROWS)
    # written out by hand: a row taken out of the table (a second solver of a build, one of two hand-overs into `big`) has to pass through here
    assert sorted(bm.row_id(r) for r in bm.ROWS) == sorted(
        "step-newton pgs-pgs prof-newton prof-pgs mid-newton midp-pgs big38-newton big38p-pgs big50-newton big50p-pgs big-newton big-pgs "
        "sat-newton sat2-newton sat1-pgs satp-pgs tall-from-midp big-from-big38p big-from-big50p sat32-from-satp "
        "tall-twin big-twin sat32-twin lean-twin sat32n-twin".split())


def test_builds_the_suite_did_not_compare_per_step_have_a_primary_row():
    """The builds whose per-step oracle comparison on the device is this table's reason to exist: a primary row each -- `big` under both solvers."""
    primary = {(r["tag"], r["solver"]) for r in bm.rows("primary")}
    for tag, solver in (("midp", bm.PGS), ("big50p", bm.PGS), ("big38p", bm.PGS), ("big", bm.NEWTON), ("big", bm.PGS), ("step", bm.NEWTON), ("pgs", bm.PGS),
                        ("sat1", bm.PGS), ("sat2", bm.NEWTON)):
        assert (tag, solver) in primary, (tag, solver)
    assert {(r["tag"], r["via"]) for r in bm.rows("sweep")} == {("tall", "midp"), ("big", "big38p"), ("big", "big50p"), ("sat32", "satp")}


@pytest.mark.parametrize("row", bm.rows("primary"), ids=bm.row_id)
def test_primary_rows_are_what_smj_route_launches(harness, row):
    _, routes = harness
    names = [name for name, _, _ in emul.variants()]
    variant = names.index(emul.default_variant(bm.blob_of(row)))
    assert set(row["options"]) <= {"newton_two_waves", "pgs_two_waves"}, row["options"]   # the options smj_route reads; anything else does not select a build
    assert set(row["slots"]) <= {"DEBUG", "PROF"}
    key = (variant, row["solver"], int("PROF" in row["slots"]), int(row["options"].get("newton_two_waves", N2W_DEFAULT)),
           int(row["options"].get("pgs_two_waves", P2W_DEFAULT)))
    assert routes[key] == (K if row["tag"] == "step" else f"{K}_{row['tag']}"), (key, routes[key])
    if row["tag"] == "step":
        assert "DEBUG" in row["slots"]   # or the call is lean-eligible and `lean` runs in its place (smj_variants.h smj_lean_eligible)


@pytest.mark.parametrize("row", bm.rows("sweep"), ids=bm.row_id)
def test_sweep_rows_are_the_hand_over_smj_route_plans(harness, row):
    """The row's `via` is the primary build of the scene under PGS with no optional slot bound, and its tag the escalation target's PGS build."""
    _, routes = harness
    table = {name: (tag, esc) for name, tag, esc in emul.variants()}
    name = emul.default_variant(bm.blob_of(row))
    variant = list(table).index(name)
    assert routes[(variant, bm.PGS, 0, N2W_DEFAULT, P2W_DEFAULT)] == f"{K}_{row['via']}"
    esc = table[name][1]
    assert esc is not None
    # the target's build under PGS: the escalation variant's own primary choice (`big`, `sat32` carry both solvers), or the named build (`tall`)
    target = routes[(list(table).index(esc), bm.PGS, 0, N2W_DEFAULT, P2W_DEFAULT)].replace(K + "_", "") if esc in table else esc
    assert target == row["tag"], (esc, target)


@pytest.mark.parametrize("row", bm.rows("twin"), ids=bm.row_id)
def test_twin_rows_name_tests_that_exist(row):
    assert row["held_by"]
    for module, function in row["held_by"]:
        assert callable(getattr(importlib.import_module(module), function)), (module, function)


def test_the_pile_is_the_smallest_model_beyond_the_50_column_build():
    from oracle.oracle import Oracle

    assert bm.PILE_BODIES == 9 and len(bm.pile_blobs()) == bm.PILES
    for blob in bm.pile_blobs():
        o = Oracle(blob)
        assert o.dim("nv") == 54 and o.dim("nu") == 0
        o.close()
        assert emul.default_variant(blob) == "big"
