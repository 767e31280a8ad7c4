"""TEST INFRASTRUCTURE ONLY -- ctypes wrapper of tests/emul/libsmj_emul_<tag>.so (CPU lane emulator of the HIP kernel, one library per
build tag of csrc/smj_builds.h).  Slots, variants, their builds and hand-over targets and the choice of a variant are asked of the
library's own tables through the emulator (smj_emul.cpp); none is restated here."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np

from stretch_mujoco_amd.lib import CONTACT_WORDS, SLOT

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = {}

# buffer of Emul -> slot of emul_bind (SMJ_SLOT_*, include/smj.h)
SLOTS = dict(qpos=SLOT["QPOS"], qvel=SLOT["QVEL"], ctrl=SLOT["CTRL"], warm=SLOT["WARMSTART"], nstep=SLOT["NSTEP"], act_len=SLOT["ACT_LENGTH"],
             act_vel=SLOT["ACT_VELOCITY"], base=SLOT["BASE_POSE"], gyro=SLOT["GYRO"], accel=SLOT["ACCEL"], lidar=SLOT["LIDAR"], info=SLOT["INFO"],
             debug=SLOT["DEBUG"], bctl=SLOT["BASECTL"])


def _load(name: str, tag: str):
    """libsmj_emul_<tag>.so, or what SMJ_EMUL_LIB_<NAME> names (an experimental build of that variant, tools only)."""
    if name not in _LIB:
        so = "libsmj_emul_%s.so" % tag
        subprocess.check_call(["make", "-C", _HERE, "-s", so])
        L = ctypes.CDLL(os.environ.get("SMJ_EMUL_LIB_" + name.upper()) or os.path.join(_HERE, so))
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.emul_create.restype = vp
        L.emul_create.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ci]
        L.emul_bind.argtypes = [vp, ci, vp, ctypes.c_long]
        L.emul_bind_contacts.argtypes = [vp, vp, ci]
        L.emul_step.argtypes = [vp, ci, ctypes.c_uint]
        L.emul_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_double]
        L.emul_clear_caches.argtypes = [vp]
        L.emul_destroy.argtypes = [vp]
        L.emul_caps.argtypes = [vp]
        L.emul_pick_variant.argtypes = [ctypes.c_char_p, ctypes.c_size_t, vp, ci]
        for f in ("emul_variant_name", "emul_variant_tag", "emul_variant_escalation"):
            getattr(L, f).restype = ctypes.c_char_p
        # event counters of the kernel source, per library and process: tests read differences
        for f in ("emul_sep_skips", "emul_ext_steps", "emul_mc_hits", "emul_isl_total", "emul_isl_swept"):
            getattr(L, f).restype = ctypes.c_long
        _LIB[name] = L
    return _LIB[name]


@functools.lru_cache(None)
def variants() -> tuple:
    """The rows of csrc/smj_variants.h: (name, tag of the Newton build, tag of the hand-over target or None)."""
    L = _load("standard", "step")   # (the table is the same in every library; this one bootstraps the names)
    dec = lambda b: b.decode() if b is not None else None
    return tuple((dec(L.emul_variant_name(v)), dec(L.emul_variant_tag(v)), dec(L.emul_variant_escalation(v))) for v in range(L.emul_nvariants()))


def lib(variant: str = "standard"):
    """A variant's library is the one of its Newton build ("standard": step); any other name is a build tag itself ("tall", "poison")."""
    return _load(variant, {name: tag for name, tag, _ in variants()}.get(variant, variant))


def escalation(variant: str):
    """The variant the device hands a step to that runs out of rows / contacts in `variant`; None: it has none."""
    return {name: esc for name, _, esc in variants()}.get(variant)


def default_variant(blob: bytes) -> str:
    """The variant smj_create starts the model on: the loader's own choice among the capacities of the table's rows."""
    rows = variants()
    caps = (ctypes.c_int * 7 * len(rows))()   # SmjCaps per row (csrc/smj_builds.h)
    for v, (name, _, _) in enumerate(rows):
        lib(name).emul_caps(caps[v])
    v = lib().emul_pick_variant(blob, len(blob), caps, len(rows))
    if v < 0:
        raise ValueError("no kernel variant takes this model")
    return rows[v][0]


# what the padding of a store with ld > B holds (Emul(ld=...)): a NaN with a payload in the fp32 stores, -77 in the int32 ones, both as
# int32 bit patterns -- the values of tests/capi_rig.py
CANARY_BITS = {np.dtype(np.float32): 0x7FC0BEEF, np.dtype(np.int32): -77}


def _canary_store(shape, dtype):
    return np.full(shape, CANARY_BITS[np.dtype(dtype)], np.int32).view(dtype)


class Emul:
    def __init__(self, blob: bytes, dims: dict, num_envs: int = 1, debug: bool = True, variant: str | None = None, ld: int | None = None):
        """variant: a row of csrc/smj_variants.h ("standard", "mid", "big38", "big50", "big", "sat", "sat32") or a build tag ("tall",
        "poison"); default: the one smj_create starts the model on, by the model's size and the blob's capacity hint.
        ld: the leading dimension the slots are bound with (default: num_envs, packed buffers).  With ld > num_envs every buffer is the
        [:, :num_envs] view (zeroed) of a [rows, ld] array of self.store whose other columns hold CANARY_BITS."""
        if variant is None:
            variant = default_variant(blob)
            variant = "tall" if variant == "mid" else variant   # the one difference from smj_create: the emulator has no escalation of its own, so it runs `mid`'s hand-over target
        self.variant = variant
        self.L = lib(variant)
        self.nvp, self.ncon_max, self.nsat_max = self.L.emul_nvp(), self.L.emul_ncon_max(), self.L.emul_nsat_max()
        self.B = B = num_envs
        self.c = self.L.emul_create(blob, len(blob), B)
        if not self.c:
            raise ValueError("emul_create failed")
        nq, nv, nu, nl = dims["nq"], dims["nv"], dims["nu"], dims["nlidar"]
        f = np.float32
        self.ld = B if ld is None else int(ld)
        assert self.ld >= B
        rows = dict(qpos=(nq, f), qvel=(nv, f), ctrl=(nu, f), warm=(nv, f), nstep=(None, np.int32), act_len=(nu, f), act_vel=(nu, f), base=(3, f),
                    gyro=(3, f), accel=(3, f), lidar=(max(nl, 1), f), info=(4, np.int32), bctl=(8, f))
        if debug:
            rows["debug"] = (self.L.emul_debug_floats(), f)
        self.store, self.buf = {}, {}
        for k, (n, dtype) in rows.items():
            if self.ld == B:
                self.store[k] = self.buf[k] = np.zeros(B if n is None else (n, B), dtype)
            else:
                self.store[k] = _canary_store(self.ld if n is None else (n, self.ld), dtype)
                self.buf[k] = self.store[k][..., :B]
                self.buf[k][...] = 0
        self.bind(self.ld)
        # PGS: the emulator starts the sweeps the way MuJoCo does unless a test asks for the kernels' default (a second start from the
        # previous step's forces, option pgs_dual_warmstart = 1) -- most PGS tests compare iterate for iterate with the unmodified oracle
        self.set_option("pgs_dual_warmstart", 0)

    def bind(self, ld: int):
        """Bind every buffer with leading dimension `ld` (tests of the stride itself pass another one than the stores have)."""
        for k, a in self.store.items():
            assert self.L.emul_bind(self.c, SLOTS[k], a.ctypes.data_as(ctypes.c_void_p), ld) == 0

    def bind_contacts(self, cap: int):
        """The contact-readout slot (SMJ_SLOT_CONTACTS): self.rec, env-major [B, cap, CONTACT_WORDS], written by a step with
        lib.READ_CONTACTS; never-written words stay NaN (the one of CANARY_BITS).  With ld > B it is the [:B] view of self.rec_store,
        [ld, cap, CONTACT_WORDS]."""
        assert self.L.emul_contact_words() == CONTACT_WORDS
        if self.ld == self.B:
            self.rec_store = self.rec = _canary_store((self.B, cap, CONTACT_WORDS), np.float32)
        else:
            self.rec_store = _canary_store((self.ld, cap, CONTACT_WORDS), np.float32)
            self.rec = self.rec_store[:self.B]
        assert self.L.emul_bind_contacts(self.c, self.rec.ctypes.data_as(ctypes.c_void_p), cap) == 0

    def set_option(self, name, v):
        assert self.L.emul_set_option(self.c, name.encode(), float(v)) == 0

    def clear_caches(self):
        """What smj_reset drops beside the state: kept manifolds, separating directions, the PGS second start."""
        self.L.emul_clear_caches(self.c)

    def set_poison(self, byte):
        """Fill the emulated LDS with `byte` before every launch (-1: leave whatever the previous launch left)."""
        self.L.emul_set_poison(int(byte))

    def step(self, n=1, read_flags=0):
        self.L.emul_step(self.c, n, read_flags)

    def close(self):
        self.L.emul_destroy(self.c)
        self.c = None

    def __getattr__(self, k):
        if k in self.__dict__.get("buf", {}):
            return self.buf[k]
        raise AttributeError(k)
