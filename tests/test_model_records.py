"""What the model loader (stretch_mujoco_amd/csrc/smj_model_load.h) makes of a blob, pinned on the CPU: a stand-alone host program
(tests/modelrec/modelrec_check.cpp) loads a blob with smj_load_model against the capacities of the build table and prints the return
code, the error text, the chosen variant, every scalar of DevModel, the size and SHA-256 of every table the loader derives (the per-lane,
plane-pair, geom, pair, row, static-geometry and satellite records), one SHA-256 over the tables it copies, and the layout enums of
smj_model.h.  tests/golden/model_records.json holds that output for every shipped blob -- against all variants, as smj_create offers them,
and against the single row of build `big`, as the escalation model is loaded (the only path with 8 mass-matrix slots per lane for a
32-dof model) -- and for four damaged copies of stretch_empty.smjb.  It was written once, from the loader as it stood before its
positions got names, and is only compared against: a slip in a record layout shows here, not as a physics mismatch.

A hash that differs is localised with `modelrec_check <blob> [--tag big] --dump <table>` of two commits and diff.
`python tests/test_model_records.py --write` is how the golden file was made, with the csrc headers of the commit before this test; the
four strides that were bare literals there (SMJ_SAT_I_STRIDE 8, SMJ_SAT_F_STRIDE 44, SMJ_SGW_STRIDE 32, SMJ_SGB_STRIDE 8) were passed as -D."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stretch_mujoco_amd", "csrc")
MODELS = os.path.join(ROOT, "stretch_mujoco_amd", "models")
GOLDEN = os.path.join(ROOT, "tests", "golden", "model_records.json")
TAGS = "step pgs prof tall mid midp big38 big38p big50 big50p big sat sat1 sat2 satp sat32 sat32n".split()
SCENES = sorted(f[:-5] for f in os.listdir(MODELS) if f.endswith(".smjb"))
DAMAGED = ["wrong_magic", "truncated_entry_table", "entry_past_the_end", "k_ldl_i_missing"]
ENTRY = 88   # bytes of one entry of the blob's table, which starts at byte 16: name[48], dtype, ndim, shape[4], offset, nbytes


def build_exe(d, flags=(), csrc=CSRC):
    srcs = []
    for tag in TAGS:
        p = d / f"probe_{tag}.cpp"
        p.write_text(f"#define SMJ_BUILD_TAG {tag}\n#define PROBE_NAME probe_product_{tag}\n#include \"desc_probe.inc\"\n")
        srcs.append(str(p))
    exe = d / "modelrec_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I", csrc, "-I", os.path.join(ROOT, "tests", "routing"),
                           os.path.join(ROOT, "tests", "modelrec", "modelrec_check.cpp")] + srcs + ["-o", str(exe)])
    return exe


def run(exe, blob, *args):
    env = {k: v for k, v in os.environ.items() if k not in ("SMJ_NO_SEPCACHE", "SMJ_NO_MCACHE")}   # the two switches of the defaults
    out = subprocess.run([str(exe), str(blob)] + list(args), capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def records(exe, blob, *args):
    return dict((ln.partition(" ")[0], ln.partition(" ")[2]) for ln in run(exe, blob, *args).splitlines())


def damage(kind, d):
    """A damaged copy of stretch_empty.smjb in directory d."""
    with open(os.path.join(MODELS, "stretch_empty.smjb"), "rb") as f:
        b = bytearray(f.read())
    if kind == "wrong_magic":
        b[0:8] = b"SMJB0002"
    elif kind == "truncated_entry_table":
        del b[16 + 3 * ENTRY + 10:]
    elif kind == "entry_past_the_end":   # the first entry's nbytes: one byte more than the blob holds after its offset
        offset, = struct.unpack_from("<Q", b, 16 + 72)
        struct.pack_into("<Q", b, 16 + 80, len(b) - offset + 1)
    elif kind == "k_ldl_i_missing":
        count, = struct.unpack_from("<I", b, 8)
        at = [16 + ENTRY * i for i in range(count) if b[16 + ENTRY * i:].startswith(b"k_ldl_i\0")]
        assert len(at) == 1
        b[at[0]] = ord("x")
    p = d / (kind + ".smjb")
    p.write_bytes(bytes(b))
    return p


def collect(exe, d):
    models = {s: {"all": records(exe, os.path.join(MODELS, s + ".smjb")), "big": records(exe, os.path.join(MODELS, s + ".smjb"), "--tag", "big")}
              for s in SCENES}
    return {"models": models, "damaged": {k: records(exe, damage(k, d)) for k in DAMAGED}}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_exe(tmp_path_factory.mktemp("modelrec"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_covers_every_shipped_blob(golden):
    assert sorted(golden["models"]) == SCENES and sorted(golden["damaged"]) == sorted(DAMAGED)
    loads = [s for s in SCENES if golden["models"][s]["all"]["rc"] == "0"]
    assert len(loads) == len(SCENES) - 1 and golden["models"]["stretch_empty_full"]["all"]["rc"] == "-3"
    assert golden["models"]["stretch_empty_full"]["all"]["err"] == "model blob: missing int k_nlevel"
    assert sorted(int(golden["models"][s]["all"]["nsat"]) for s in loads if golden["models"][s]["all"]["nsat"] != "0") == [2, 4, 5, 16]
    # 8 mass-matrix slots per lane for a 32-dof model: the lane record of the single row `big` is the longer one
    e = golden["models"]["stretch_empty"]
    assert e["big"]["rc"] == "0" and e["big"]["variant"] == "big" and e["all"]["variant"] == "standard"
    assert int(e["big"]["k_lanerec"].split()[0]) == 64 * int(e["big"]["smj_lr_stride(8)"]) > int(e["all"]["k_lanerec"].split()[0])


@pytest.mark.parametrize("scene", SCENES)
def test_every_shipped_blob_loads_to_the_pinned_records(exe, golden, scene):
    blob = os.path.join(MODELS, scene + ".smjb")
    assert records(exe, blob) == golden["models"][scene]["all"]
    assert records(exe, blob, "--tag", "big") == golden["models"][scene]["big"]


@pytest.mark.parametrize("kind", DAMAGED)
def test_a_damaged_blob_is_refused_with_the_pinned_code_and_text(exe, golden, kind, tmp_path):
    got = records(exe, damage(kind, tmp_path))
    assert got["rc"] != "0" and got["err"]
    assert got == golden["damaged"][kind]


def test_the_satellite_record_is_the_model_compilers(exe):
    from stretch_mujoco_amd import model_fuse as F
    e = {k: int(v) for k, v in records(exe, os.path.join(MODELS, "stretch_empty.smjb")).items() if k.startswith("SMJ_S")}
    for key, at in F.SAT_I.items():
        assert e["SMJ_SAT_I_STRIDE" if key == "stride" else "SMJ_SR_" + key.upper()] == at
    for key, at in F.SAT_F.items():
        assert (e["SMJ_SAT_F_STRIDE"] if key == "stride" else e["SMJ_SR_" + key.upper()] - e["SMJ_SR_F"]) == at
    assert (e["SMJ_SAT_I_STRIDE"], e["SMJ_SAT_F_STRIDE"]) == (8, 44) and e["SMJ_SR_F"] == 8 and e["SMJ_SR_STRIDE"] == 8 + 44


def test_the_printed_hash_is_sha256_of_the_dumped_words(exe):
    blob = os.path.join(MODELS, "stretch_kitchen4_sat.smjb")
    got = records(exe, blob)
    for table in ("k_lanerec", "k_sgw", "k_satrec"):
        words = [int(w) for w in run(exe, blob, "--dump", table).split()]
        assert got[table] == f"{len(words)} {hashlib.sha256(struct.pack(f'<{len(words)}i', *words)).hexdigest()}"


def test_the_loader_is_clean_under_the_sanitizers(golden, tmp_path):
    from host_check import sanitizers_or_skip
    san = build_exe(tmp_path, sanitizers_or_skip(tmp_path))
    for scene in ("stretch_empty", "stretch_empty_full", "stretch_scene", "stretch_kitchen4_sat", "stretch_kitchen_robocasa"):
        assert records(san, os.path.join(MODELS, scene + ".smjb")) == golden["models"][scene]["all"]
    assert records(san, os.path.join(MODELS, "stretch_empty.smjb"), "--tag", "big") == golden["models"]["stretch_empty"]["big"]
    for kind in DAMAGED:
        assert records(san, damage(kind, tmp_path)) == golden["damaged"][kind]


if __name__ == "__main__":
    import pathlib
    import tempfile
    assert sys.argv[1:] == ["--write"], __doc__
    with tempfile.TemporaryDirectory() as tmp:
        result = collect(build_exe(pathlib.Path(tmp)), pathlib.Path(tmp))
    with open(GOLDEN, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
