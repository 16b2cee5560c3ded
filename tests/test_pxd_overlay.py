"""Background overlay, host side: the two forms of the checker (tests/pxd_overlay_reference.py) agree on the planted pairs and have the
properties of a pixel-by-pixel saturating sum; the C ABI of the two entry points, the launcher's refusals and the host-side refusals of
``utils.pxd_overlay`` (no GPU needed).  The device side is tests/test_pxd_overlay_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pxd_events_reference as ER
import pxd_overlay_reference as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 13, 37), (2, 40, 259)]
_PLANTED = {}


def _planted(S, H, W):
    """``(columns of a, columns of b, pairs, dense events of a, dense events of b)`` of a shape, built once."""
    if (S, H, W) not in _PLANTED:
        a, b, pairs = OR.planted(S, H, W, seed=S)
        _PLANTED[S, H, W] = (ER.columns(a, S), ER.columns(b, S), pairs, a, b)
    return _PLANTED[S, H, W]


@pytest.mark.parametrize("S,H,W", SHAPES)
def test_the_two_restatements_agree_on_the_planted_pairs(S, H, W):
    import utils
    A, B, pairs, ea, eb = _planted(S, H, W)
    ids_a, ids_b = [p[0] for p in pairs], [p[1] for p in pairs]
    d, s = OR.dense(A, ids_a, B, ids_b, (H, W), S), OR.sparse(A, ids_a, B, ids_b, (H, W), S)
    assert OR.same(d, s)
    off, pos, charge = utils.event_columns(*s, shape=(H, W), n_sensors=S)           # strictly ascending, charges 1 .. 255
    assert off.size == len(pairs) + 1 and pos.size == off[-1] == charge.size
    n = np.diff(off)
    na, nb = np.diff(A[0])[ids_a], np.diff(B[0])[ids_b]
    shared = OR.shared(A, ids_a, B, ids_b, (H, W))
    assert np.array_equal(na + nb - n, shared)
    # the planted patterns are there
    assert n[0] == 0 and n[1] == nb[1] and n[2] == na[2] and shared[1] == shared[2] == 0
    assert shared[3] == na[3] == nb[3] == n[3] and shared[4] > 0 and shared[4] < min(na[4], nb[4])
    full = OR.dense_sum(A, [pairs[5][0]], B, [pairs[5][1]], (H, W), S)[0].reshape(-1)
    assert set(np.unique(full)) == {2, 255} and (ea[2][0].astype(int) + eb[3][0]).reshape(-1)[:4].tolist() == [2, 256, 255, 510]
    assert shared[8] == 0 and n[8] == 4 and shared[9] == 0 and n[9] == H * W and shared[10] == 1 and n[10] == H * W
    one = slice(int(off[10]), int(off[11]))
    assert pos[one][63] == 63 and charge[one][63] == min(int(ea[7].reshape(S, -1)[0, 63]) + 250, 255)
    # ids may repeat, be permuted, or lie outside the columns (an empty event) on either side
    ids_a2, ids_b2 = [1, 99, 1, -1, 3], [2, 1, 99, 7, 4]
    assert OR.same(OR.dense(A, ids_a2, B, ids_b2, (H, W), S), OR.sparse(A, ids_a2, B, ids_b2, (H, W), S))


@pytest.mark.parametrize("S,H,W", SHAPES)
def test_identity_commutativity_and_self_overlay(S, H, W):
    A, B, pairs, ea, eb = _planted(S, H, W)
    every = list(range(len(ea)))
    # an empty event laid over an event leaves it as it is
    assert OR.same(OR.sparse(A, every, B, [0] * len(every), (H, W), S), A)
    assert OR.same(OR.sparse(B, [0] * len(every), A, every, (H, W), S), A)
    # a + b == b + a
    ids_a, ids_b = [p[0] for p in pairs], [p[1] for p in pairs]
    assert OR.same(OR.sparse(A, ids_a, B, ids_b, (H, W), S), OR.sparse(B, ids_b, A, ids_a, (H, W), S))
    # an event over itself: the same positions, min(2 q, 255)
    twice = OR.sparse(A, every, A, every, (H, W), S)
    assert all(np.array_equal(t, a) for t, a in zip(twice[:4], A[:4]))
    assert np.array_equal(twice[4], np.minimum(2 * A[4].astype(np.int64), 255)) and (twice[4] == 255).any() and (twice[4] < 255).any()


def _lib():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.ieagan_last_error.restype = ctypes.c_char_p
    return _hip, lib


def test_overlay_entry_points_are_declared_exported_and_bound():
    _hip, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    for sym in ("ieagan_pxd_event_overlay", "ieagan_pxd_event_overlay_scratch"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    sig = _hip._SIGS["ieagan_pxd_event_overlay"]
    assert len(sig) == 22 and len(_hip._SIGS["ieagan_pxd_event_overlay_scratch"]) == 2
    assert [k for k, t in enumerate(sig) if t is ctypes.c_long] == [3, 9, 16] and _hip._SIGS["ieagan_pxd_event_overlay_scratch"][1] is ctypes.c_long
    assert [k for k, t in enumerate(sig) if t is ctypes.c_int] == [4, 10, 12, 13, 14, 15]
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION == 12       # new entry points only: no struct and no existing signature changed


def test_the_launcher_rejects_bad_arguments_before_any_launch():
    _hip, lib = _lib()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.addressof(buf)
    overlay = lib.ieagan_pxd_event_overlay
    overlay.argtypes = _hip._SIGS["ieagan_pxd_event_overlay"]
    store = dict(pos=p, charge=p, offsets=p, digits=8, events=2, ids=p)
    good = dict({"a_" + k: v for k, v in store.items()}, **{"b_" + k: v for k, v in store.items()}, E=1, S=4, H=8, W=8, capacity=16, out_pos=p,
                out_charge=p, out_offsets=p, scratch=p)
    cases = [(dict(E=0), "E = 0 pairs outside 1 .. 65535"), (dict(E=65536), "outside 1 .. 65535"), (dict(H=0), "bad image size"),
             (dict(S=0), "outside 1 .. 65535"), (dict(S=64, H=8192, W=8192), "does not fit the int32 flat index"),
             (dict(capacity=-1), "capacity = -1 is negative"), (dict(out_pos=None), "out_pos / out_charge is NULL"),
             (dict(out_charge=None), "out_pos / out_charge is NULL"), (dict(out_pos=p + 2), "out_pos is not 4-byte aligned"),
             (dict(out_offsets=None), "out_offsets is NULL"), (dict(out_offsets=p + 4), "out_offsets is NULL or not 8-byte aligned"),
             (dict(scratch=None), "scratch"), (dict(scratch=p + 2), "scratch")]
    for side in "ab":
        cases += [({side + "_pos": None}, f"{side}_pos / {side}_charge is NULL"), ({side + "_charge": None}, f"{side}_pos / {side}_charge is NULL"),
                  ({side + "_pos": p + 2}, f"{side}_pos is not 4-byte aligned"), ({side + "_offsets": None}, f"{side}_offsets is NULL"),
                  ({side + "_offsets": p + 4}, f"{side}_offsets is not 8-byte aligned"), ({side + "_ids": None}, f"{side}_ids is NULL"),
                  ({side + "_ids": p + 1}, f"{side}_ids is NULL or misaligned"), ({side + "_digits": -1}, "is negative"),
                  ({side + "_events": -1}, "is negative")]
    for change, text in cases:
        rc = overlay(*dict(good, **change).values(), None)
        msg = lib.ieagan_last_error().decode()
        assert rc != 0 and msg.startswith("pxd_event_overlay: ") and text in msg, (change, msg)


def test_the_scratch_size_is_non_negative_and_monotone():
    _hip, lib = _lib()
    scratch = lib.ieagan_pxd_event_overlay_scratch
    scratch.argtypes, scratch.restype = _hip._SIGS["ieagan_pxd_event_overlay_scratch"], ctypes.c_long
    Es, caps = [1, 2, 7, 64, 1000, 65535], [0, 1, 255, 256, 257, 4096, 10 ** 5, 10 ** 6, 2 ** 20 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 40]
    table = np.array([[scratch(E, c) for c in caps] for E in Es])
    assert (table >= 0).all() and (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    assert (table[:, 0] >= np.array(Es) + 1).all()              # capacity 0 still needs the running sums of the pairs
    assert scratch(0, 100) == 0 and scratch(-1, 100) == 0 and scratch(5, -1) == 0 and table.max() < 2 ** 20


def _fake_store(shape=(4, 5), n_sensors=3, device="cuda:0", counts=(3, 0, 2)):
    import utils
    s = utils.PXDEventStore.__new__(utils.PXDEventStore)
    s.shape, s.n_sensors, s.device, s.counts = shape, n_sensors, torch.device(device), np.asarray(counts, np.int64)
    return s


def test_host_side_refusals_come_before_any_device_call(monkeypatch):
    import _hip
    import utils

    def no_device(*a, **k):
        raise AssertionError("a device call before the host checks were done")
    monkeypatch.setattr(_hip, "require_gpu", no_device)
    monkeypatch.setattr(_hip, "call", no_device)
    a = _fake_store()
    for other, match in ((_fake_store(shape=(4, 6)), "differ in shape"), (_fake_store(n_sensors=4), "differ in n_sensors"),
                         (_fake_store(device="cuda:1"), "differ in device")):
        with pytest.raises(ValueError, match=match):
            utils.pxd_overlay(a, [0], other)
        with pytest.raises(ValueError, match=match):
            a.overlay([0], other)
    with pytest.raises(ValueError, match="2 ids into a, 3 into b"):
        utils.pxd_overlay(a, [0, 1], _fake_store(), [0, 1, 2])
    with pytest.raises(ValueError, match="capacity is negative"):
        utils.pxd_overlay(a, [0], _fake_store(), capacity=-1)
    with pytest.raises(TypeError, match="must be PXDEventStores"):
        utils.pxd_overlay(a, [0], np.zeros(3))
    digits = utils.PXDDigits.__new__(utils.PXDDigits)
    digits.threshold = -1.0
    with pytest.raises(ValueError, match="threshold = -1.0"):
        utils.PXDEventStore.from_digits(digits)
    with pytest.raises(TypeError, match="PXDDigits"):
        utils.PXDEventStore.from_digits(np.zeros(3))
    for name in ("pxd_overlay", "PXDOverlay"):
        assert hasattr(utils, name)


def test_pairs_of_the_command_line_tool():
    sys.path.insert(0, os.path.join(ROOT, "iea-gan_amd"))
    import overlay_events
    s, b = overlay_events.pairs(3, 5, 7)
    assert s.tolist() == [0, 1, 2, 0, 1, 2, 0] and b.tolist() == [0, 1, 2, 3, 4, 0, 1]
    s, b = overlay_events.pairs(3, 5, 7, seed=4)
    perm = np.random.default_rng(4).permutation(5)
    assert b.tolist() == perm[[0, 1, 2, 3, 4, 0, 1]].tolist() and sorted(perm.tolist()) == [0, 1, 2, 3, 4]


def test_overlay_events_help_runs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "iea-gan_amd", "overlay_events.py"), "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "--background" in p.stdout and "--seed" in p.stdout
