"""The comparators of tests/capi_rig.py can fail: a fake packed result laid into a padded store the way a kernel with the wrong stride
would lay it is caught by same_bits() or by the padding check.  No device and no library: the stores are numpy arrays."""
import numpy as np
import pytest

from capi_rig import CANARY_F32_BITS, CANARY_I32, Store, envs_all_differ, same_bits

B, PAD, ROWS = 3, 5, 4


def _packed(integer):
    v = np.arange(1, ROWS * B + 1).reshape(ROWS, B)
    return v.astype(np.int32) if integer else (v * 0.25).astype(np.float32)


def _lay(store, packed, stride):
    """What a kernel does that indexes the bound pointer with `stride`: word k * stride + env from row 1, column 0 of the store."""
    flat = store.bits.reshape(-1)[store.first:]
    for k in range(packed.shape[0]):
        for e in range(packed.shape[1]):
            flat[k * stride + e] = packed[k, e:e + 1].view(np.int32)[0]


def _outcome(store, packed):
    """Which of the two checks object."""
    caught = []
    try:
        same_bits({"X": packed.view(np.int32)}, {"X": store.snapshot()})
    except AssertionError:
        caught.append("same_bits")
    try:
        store.assert_padding_untouched("X")
    except AssertionError:
        caught.append("padding")
    return caught


@pytest.mark.parametrize("integer", [False, True], ids=["fp32", "int32"])
def test_the_right_stride_passes_and_the_canary_is_what_the_stores_hold(integer):
    s = Store.batch_major(ROWS, B, PAD, integer)
    assert s.bits.shape == (ROWS + 2, B + PAD) and s.view.shape == (ROWS, B) and s.ld == B + PAD
    assert (s.bits == (CANARY_I32 if integer else CANARY_F32_BITS)).all()
    if not integer:
        assert np.isnan(s.view).all()    # a NaN, and one that compares equal to itself as a bit pattern
        same_bits({"X": s.snapshot()}, {"X": s.snapshot()})
    assert s.ptr() == s.bits.ctypes.data + 4 * (B + PAD)    # row 1, column 0
    p = _packed(integer)
    _lay(s, p, s.ld)
    assert _outcome(s, p) == []
    assert np.array_equal(s.view, p)


@pytest.mark.parametrize("integer", [False, True], ids=["fp32", "int32"])
@pytest.mark.parametrize("stride", [B, B + PAD + 1, B + PAD - 1], ids=["stride-B", "stride-ld+1", "stride-ld-1"])
def test_a_wrong_stride_is_caught(stride, integer):
    s = Store.batch_major(ROWS, B, PAD, integer)
    p = _packed(integer)
    _lay(s, p, stride)
    assert _outcome(s, p) == ["same_bits", "padding"]


def test_one_word_in_a_guard_row_or_a_pad_column_is_caught():
    for where in ((0, 1), (ROWS + 1, 0), (2, B), (ROWS, B + PAD - 1)):
        s = Store.batch_major(ROWS, B, PAD)
        s.bits[where] = 0
        assert _outcome(s, s.view.copy()) == ["padding"], where
    s = Store.vector(B, PAD)
    assert s.view.shape == (B,) and s.snapshot().shape == (B,)
    s.bits[1, B] = 0
    with pytest.raises(AssertionError):
        s.assert_padding_untouched("NSTEP")


def test_env_major_store_and_a_swapped_env_are_caught():
    s = Store.env_major(B, PAD, 2, 24)
    assert s.view.shape == (B, 2, 24) and s.ptr() == s.bits.ctypes.data + 4 * 2 * 24
    s.assert_padding_untouched("CONTACTS")
    s.view[:] = np.arange(B, dtype=np.float32)[:, None, None]
    s.assert_padding_untouched("CONTACTS")
    a = s.snapshot()
    envs_all_differ({"CONTACTS": a}, ["CONTACTS"])
    with pytest.raises(AssertionError):
        same_bits({"CONTACTS": a}, {"CONTACTS": a[::-1].copy()})
    s.bits[B + 1, 0, 0] = 0    # the first pad env
    with pytest.raises(AssertionError):
        s.assert_padding_untouched("CONTACTS")


def test_same_bits_tells_signed_zeros_apart_and_wants_the_same_slots():
    z = np.zeros((2, B), np.float32)
    with pytest.raises(AssertionError):
        same_bits({"X": z.view(np.int32)}, {"X": (-z).view(np.int32)})
    with pytest.raises(AssertionError):
        same_bits({"X": z.view(np.int32)}, {"Y": z.view(np.int32)})
    with pytest.raises(AssertionError):
        envs_all_differ({"X": z.view(np.int32)}, ["X"])
