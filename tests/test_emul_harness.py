"""The lane emulator's harness (tests/emul): it asks the library's own tables (csrc/smj_model_load.h, csrc/smj_variants.h, include/smj.h)
for options, slots, variants and hand-over targets instead of restating them.  The expectations here are written out by hand, not
computed from those tables, so that an edit of a table that the emulator follows silently still has to pass through this file."""
import os

import pytest

from conftest import MODELS
from emul import emul
from emul.emul import Emul

DIMS = dict(nq=27, nv=26, nu=10, nlidar=360)   # stretch_empty


def test_options_the_emulator_takes(blob_fused):
    """Every solver option smj_set_option takes by name, plus the two fields only the emulator sets by name; nothing else."""
    e = Emul(blob_fused, DIMS, num_envs=1)
    try:
        for name in ("iterations", "tolerance", "warmstart", "pgs_fixed_iter", "qcqp_exact", "grad_noise", "pgs_island_stop",
                     "max_contacts_per_pair", "solver", "convex_pairs", "multiccd", "sep_cache", "manifold_cache", "pgs_dual_warmstart",
                     "pgs_cap", "multi_serial"):
            assert e.L.emul_set_option(e.c, name.encode(), 0.0) == 0, name
        for name in ("no_such_option", "", "primary_rows", "ls_iterations", "Solver"):
            assert e.L.emul_set_option(e.c, name.encode(), 0.0) == -1, name
        with pytest.raises(AssertionError):
            e.set_option("no_such_option", 1)
    finally:
        e.close()


def test_slots_are_the_headers(blob_fused):
    assert emul.SLOTS == dict(qpos=0, qvel=1, ctrl=2, warm=3, nstep=4, act_len=5, act_vel=6, base=7, gyro=8, accel=9, lidar=10, info=11,
                              debug=12, bctl=15)
    e = Emul(blob_fused, DIMS, num_envs=1)
    try:
        for slot in (-1, 16, 17, 99):   # SMJ_SLOT_CONTACTS (16) is env-major: bind_contacts, not emul_bind
            assert e.L.emul_bind(e.c, slot, None, 1) == -1, slot
        assert e.L.emul_bind(e.c, 13, None, 1) == 0 and e.L.emul_bind(e.c, 14, None, 1) == 0   # PROF, XPOSE: no buffer of Emul, still slots
    finally:
        e.close()


def test_variant_table_and_hand_over_targets():
    names = [name for name, _, _ in emul.variants()]
    assert names == ["standard", "mid", "big38", "big50", "big", "sat", "sat32"]
    assert {name: tag for name, tag, _ in emul.variants()} == dict(standard="step", mid="mid", big38="big38", big50="big50", big="big",
                                                                     sat="sat", sat32="sat32")
    assert {v: emul.escalation(v) for v in names + ["tall", "poison"]} == dict(
        standard="tall", mid="tall", big38="big", big50="big", sat="sat32", tall=None, big=None, sat32=None, poison=None)


def test_library_file_follows_the_build_tag():
    for variant, so in (("standard", "libsmj_emul_step.so"), ("tall", "libsmj_emul_tall.so"), ("mid", "libsmj_emul_mid.so"),
                        ("big38", "libsmj_emul_big38.so"), ("sat32", "libsmj_emul_sat32.so"), ("poison", "libsmj_emul_poison.so")):
        assert os.path.basename(emul.lib(variant)._name) == so
    # capacities come from the build: dof lanes, contacts, satellites
    caps = {v: (emul.lib(v).emul_nvp(), emul.lib(v).emul_ncon_max(), emul.lib(v).emul_nsat_max()) for v in ("standard", "tall", "mid", "big", "sat", "sat32")}
    assert caps == dict(standard=(32, 16, 0), tall=(32, 48, 0), mid=(32, 44, 0), big=(64, 64, 0), sat=(32, 56, 16), sat32=(32, 64, 32))


@pytest.mark.parametrize("scene,library,emulator", [
    ("stretch_empty", "standard", "standard"),
    ("stretch_kitchen_standin", "mid", "tall"),   # the emulator has no escalation of its own: it runs mid's hand-over target
    ("stretch_scene", "big38", "big38"),
    ("stretch_scene_docking", "big50", "big50"),
    ("stretch_kitchen4", "big50", "big50"),
    ("stretch_kitchen_export", "big50", "big50"),
    ("stretch_scene_sat", "sat", "sat"),
    ("stretch_kitchen4_sat", "sat", "sat"),
    ("stretch_kitchen_export_sat", "sat", "sat"),
    ("stretch_kitchen_robocasa", "sat", "sat"),
])
def test_default_variant_of_the_shipped_blobs(scene, library, emulator):
    from oracle.oracle import Oracle

    blob = open(os.path.join(MODELS, scene + ".smjb"), "rb").read()
    assert emul.default_variant(blob) == library
    o = Oracle(blob)
    e = Emul(blob, dict(nq=o.dim("nq"), nv=o.dim("nv"), nu=o.dim("nu"), nlidar=360), num_envs=1)
    try:
        assert e.variant == emulator
    finally:
        e.close()
        o.close()


def test_a_blob_the_loader_refuses_has_no_default_variant(blob_fused):
    with pytest.raises(ValueError):
        emul.default_variant(blob_fused[:64])
