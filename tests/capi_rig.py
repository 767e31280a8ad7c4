"""TEST INFRASTRUCTURE ONLY -- a rig over the raw C-ABI (include/smj.h) for the leading-dimension contract: every slot of a context is
bound to the inside of a larger store full of a canary, with ld = B + pad, through smj_create / smj_bind directly (no
StretchBatchSimulator).  `ld` changes addresses and no arithmetic, so a padded context must give what the packed one (pad 0) gives bit
for bit and leave every word it does not own as it was: same_bits() and CapiRig.assert_padding_untouched().

A batch-major slot of `rows` rows is a store [rows + 2, B + pad] -- one guard row above, one below, `pad` columns to the right -- bound at
row 1, column 0.  NSTEP is such a store of one row.  CONTACTS, the env-major slot, is [B + pad + 2, cap, 24] bound at block 1.  fp32
stores are filled with a NaN that carries a payload, int32 stores with -77; everything is compared as int32 bit patterns, so a NaN equals
itself and -0.0 differs from 0.0.  The stores live on the device, or in numpy (device=None: the host self-tests of the comparators)."""
import ctypes
import os

import numpy as np

from stretch_mujoco_amd import lib

CANARY_F32_BITS = 0x7FC0BEEF   # a quiet NaN with payload 0xBEEF
CANARY_I32 = -77
INT_SLOTS = ("NSTEP", "INFO")
OPTIONAL = ("GYRO", "ACCEL", "LIDAR", "DEBUG", "PROF", "XPOSE", "BASECTL", "CONTACTS")
REQUIRED = ("QPOS", "QVEL", "CTRL", "WARMSTART", "NSTEP", "ACT_LENGTH", "ACT_VELOCITY", "BASE_POSE", "INFO")
PROF_ROWS = 48   # what the simulator binds (the header asks for 32)


class Store:
    """One canary-filled allocation and the part of it a slot is bound to.  .bits: the whole store as int32; .view: the part the library
    owns ([:, :B] of the bound rows), in the slot's own type; .ld: the stride to bind with; ptr(): the address to bind."""

    def __init__(self, shape, inner, first, ld, integer, device):
        self.canary = CANARY_I32 if integer else CANARY_F32_BITS
        self.inner, self.first, self.ld, self.integer = inner, first, ld, integer
        if device is None:
            self.bits = np.full(shape, self.canary, np.int32)
            typed = self.bits if integer else self.bits.view(np.float32)
        else:
            import torch

            self.bits = torch.full(shape, self.canary, dtype=torch.int32, device=device)
            typed = self.bits if integer else self.bits.view(torch.float32)
        self.view = typed[inner]

    @classmethod
    def batch_major(cls, rows, B, pad, integer=False, device=None):
        return cls((rows + 2, B + pad), (slice(1, rows + 1), slice(0, B)), B + pad, B + pad, integer, device)

    @classmethod
    def vector(cls, B, pad, device=None):
        """NSTEP: int32 [B] with guard elements on both sides (a batch-major store of one row, .view one-dimensional)."""
        s = cls.batch_major(1, B, pad, True, device)
        s.view = s.bits[1, :B]
        return s

    @classmethod
    def env_major(cls, B, pad, cap, words, device=None):
        return cls((B + pad + 2, cap, words), (slice(1, B + 1),), cap * words, B + pad, False, device)

    def ptr(self):
        base = self.bits.ctypes.data if isinstance(self.bits, np.ndarray) else self.bits.data_ptr()
        return base + 4 * self.first

    def host_bits(self):
        return self.bits.copy() if isinstance(self.bits, np.ndarray) else self.bits.cpu().numpy()

    def snapshot(self):
        """The library's part as int32 bit patterns on the host."""
        h = self.host_bits()[self.inner]
        return h[0] if h.shape[0] == 1 and self.view.ndim == 1 else h

    def assert_padding_untouched(self, name=""):
        h = self.host_bits()
        outside = np.ones(h.shape, bool)
        outside[self.inner] = False
        bad = outside & (h != self.canary)
        assert not bad.any(), (name, "padding / guard words written", int(bad.sum()), np.argwhere(bad)[:5].tolist(), self.inner)


def same_bits(packed, padded):
    """Two snapshots ({slot: int32 bit patterns}) hold the same slots with the same shapes and the same bits."""
    assert sorted(packed) == sorted(padded), (sorted(packed), sorted(padded))
    for name in packed:
        a, b = np.asarray(packed[name]), np.asarray(padded[name])
        assert a.dtype == np.int32 and b.dtype == np.int32 and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        diff = a != b
        assert not diff.any(), (name, "words differ", int(diff.sum()), np.argwhere(diff)[:5].tolist())


def envs_all_differ(snap, names):
    """Non-vacuity of a comparison: in each of `names` no two envs hold the same column (a column mix-up would show)."""
    for name in names:
        a = np.asarray(snap[name])
        cols = a.reshape(-1, a.shape[-1]).T if name != "CONTACTS" else a.reshape(a.shape[0], -1)
        assert len({c.tobytes() for c in cols}) == len(cols), (name, "two envs hold the same values")


class CapiRig:
    """One context on models/<model>.smjb with B envs, every slot bound to a Store with `pad` padding columns.  optional: which of
    OPTIONAL are bound.  Every call runs on torch's current stream; the wrappers return the library's return code."""

    def __init__(self, model, B, pad=0, optional=("GYRO", "ACCEL", "LIDAR", "XPOSE", "BASECTL"), device="cuda:0"):
        from conftest import MODELS

        self.B, self.pad, self.device, self.optional = B, pad, device, tuple(optional)
        assert set(self.optional) <= set(OPTIONAL)
        self.L = lib.load()
        self.ctx = ctypes.c_void_p()
        with open(os.path.join(MODELS, model + ".smjb"), "rb") as f:
            blob = f.read()
        assert self.L.smj_create(blob, len(blob), B, 0, ctypes.byref(self.ctx)) == 0, self.error()
        d = (ctypes.c_int * 16)()
        assert self.L.smj_dims(self.ctx, d) == 0
        self.dims = {k: d[i] for k, i in lib.DIM.items()}
        D = self.dims
        self.rows = dict(QPOS=D["NQ"], QVEL=D["NV"], CTRL=max(D["NU"], 1), WARMSTART=D["NV"], NSTEP=1, ACT_LENGTH=max(D["NU"], 1),
                         ACT_VELOCITY=max(D["NU"], 1), BASE_POSE=3, GYRO=3, ACCEL=3, LIDAR=max(D["NLIDAR"], 1), INFO=4, DEBUG=D["DEBUG_FLOATS"],
                         PROF=PROF_ROWS, XPOSE=12 * D["NBODY"], BASECTL=8)
        self.stores = self.make_stores(pad)
        self.bind_stores(self.stores)

    # ---- stores and binding
    def make_stores(self, pad):
        """A fresh set of stores for every slot of this context, with `pad` padding columns (not bound yet)."""
        st = {}
        for name in REQUIRED + self.optional:
            if name == "NSTEP":
                st[name] = Store.vector(self.B, pad, self.device)
            elif name == "CONTACTS":
                st[name] = Store.env_major(self.B, pad, self.dims["CONTACT_CAP"], lib.CONTACT_WORDS, self.device)
            else:
                st[name] = Store.batch_major(self.rows[name], self.B, pad, name in INT_SLOTS, self.device)
        return st

    def bind(self, name, store, ld=None):
        """smj_bind of one slot (store None: unbind); ld: another stride than the store's own."""
        return self.L.smj_bind(self.ctx, lib.SLOT[name], ctypes.c_void_p(store.ptr()) if store is not None else None,
                               (store.ld if ld is None else ld) if store is not None else 0)

    def bind_stores(self, stores):
        for name, s in stores.items():
            assert self.bind(name, s) == 0, (name, self.error())
        self.stores = stores

    def __getitem__(self, name):
        """The [:, :B] view of a slot (a device tensor in the slot's type)."""
        return self.stores[name].view

    # ---- the library's calls
    def stream(self):
        import torch

        return ctypes.c_void_p(torch.cuda.current_stream(torch.device(self.device)).cuda_stream)

    def sync(self):
        import torch

        torch.cuda.synchronize()

    def error(self):
        return self.L.smj_last_error(self.ctx).decode()

    def last_build(self):
        return self.L.smj_last_build(self.ctx).decode()

    def set_option(self, name, value):
        return self.L.smj_set_option(self.ctx, name.encode(), float(value))

    def step(self, n, flags=0):
        return self.L.smj_step(self.ctx, n, flags, self.stream())

    def reset(self, mask=None):
        """mask: None (all envs) or a uint8 device tensor [B]."""
        return self.L.smj_reset(self.ctx, ctypes.c_void_p(mask.data_ptr()) if mask is not None else None, self.stream())

    def tick(self):
        return self.L.smj_base_controller_tick(self.ctx, self.stream())

    def render_depth(self, cam, width, height, fovy, max_depth):
        import torch

        img = torch.full((self.B, height, width), -3.0, dtype=torch.float32, device=self.device)
        rc = self.L.smj_render_depth(self.ctx, cam, width, height, float(fovy), float(max_depth), ctypes.c_void_p(img.data_ptr()), self.stream())
        return rc, img

    def render_rgb(self, cam, width, height, fovy):
        import torch

        rgb = torch.full((self.B, height, width, 3), 7, dtype=torch.uint8, device=self.device)
        gid = torch.full((self.B, height, width), -9, dtype=torch.int32, device=self.device)
        rc = self.L.smj_render_rgb(self.ctx, cam, width, height, float(fovy), ctypes.c_void_p(rgb.data_ptr()), ctypes.c_void_p(gid.data_ptr()), self.stream())
        return rc, rgb, gid

    # ---- what the comparisons read
    def snapshot(self, stores=None):
        """{slot: the [:, :B] part of every bound slot as int32 bit patterns on the host}."""
        self.sync()
        return {name: s.snapshot() for name, s in (self.stores if stores is None else stores).items()}

    def assert_padding_untouched(self, stores=None):
        self.sync()
        for name, s in (self.stores if stores is None else stores).items():
            s.assert_padding_untouched(name)

    def close(self):
        if self.ctx:
            self.sync()
            self.L.smj_destroy(self.ctx)
            self.ctx = None
