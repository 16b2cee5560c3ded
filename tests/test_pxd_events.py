"""Sparse event store, host side: the checker (tests/pxd_events_reference.py) as a round trip with the digit restatement, every check of the
store's contract (NumPy, before any device call), the event file round trip up to the upload, and the C ABI of the two entry points (no
GPU needed).  The device side is tests/test_pxd_events_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pxd_digits_reference as DR
import pxd_events_reference as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["empty", "random", "empty", "one_sensor", "edges", "full", "empty"]


@pytest.mark.parametrize("S,H,W", [(7, 13, 37), (2, 40, 259)])
def test_checker_round_trip_with_the_digit_restatement(S, H, W):
    events = ER.pattern_events(KINDS, S, H, W, seed=3)
    cols = ER.columns(events, S)
    off = cols[0]
    assert off.shape == (len(KINDS) + 1,) and off[0] == 0 and off[1] == 0 and off[-1] == off[-2] and off[3] == off[2]
    ids = [4, 0, 4, 1, 6, 5, 3, 2]
    back = ER.dense(cols, ids, (H, W), S)
    assert back.dtype == np.uint8 and back.shape == (len(ids) * S, H, W)
    assert np.array_equal(back, np.concatenate([events[i] for i in ids]))
    # ... and forth: the digits of the rebuilt images are the columns again
    index, charge, _, total = DR.digits(ER.dense(cols, range(len(KINDS)), (H, W), S))
    assert total == off[-1] and np.array_equal(charge.numpy(), cols[4])
    pos = (cols[1].astype(np.int64) * H + cols[2]) * W + cols[3]
    event = np.repeat(np.arange(len(KINDS)), np.diff(off))
    assert np.array_equal(index.numpy().astype(np.int64), event * (S * H * W) + pos)
    # an id outside the store is an empty event
    assert not ER.dense(cols, [len(KINDS), -1], (H, W), S).any()
    # the planted patterns are there
    one = events[3].reshape(S, -1).any(1)
    assert one.sum() == 1 and one[S - 2]
    assert (events[5][0] > 0).all() and set(np.unique(events[5][0])) == {1, 255}
    assert (events[4].reshape(S, -1)[:, [0, -1]] > 0).all()
    if H * W > 4096:
        assert (events[4].reshape(S, -1)[:, [4095, 4096]] > 0).all()


def _cols():
    """Three events on 3 sensors of 4 x 5 pixels: 3 digits, none, 2 digits."""
    return dict(event_offsets=np.array([0, 3, 3, 5]), sensor=np.array([0, 0, 2, 1, 1], np.uint8), ucell=np.array([0, 3, 1, 2, 2], np.uint8),
                vcell=np.array([4, 0, 2, 1, 3], np.uint16), charge=np.array([9, 255, 1, 7, 8], np.uint8))


def test_columns_of_a_valid_store():
    import utils
    off, pos, charge = utils.event_columns(**_cols(), shape=(4, 5), n_sensors=3)
    assert off.dtype == np.int64 and pos.dtype == np.int32 and charge.dtype == np.uint8
    assert off.tolist() == [0, 3, 3, 5] and pos.tolist() == [4, 15, 47, 31, 33] and charge.tolist() == [9, 255, 1, 7, 8]
    # a position may fall from one event to the next: only the order INSIDE an event is checked
    assert pos[3] < pos[2]
    empty = utils.event_columns([0], [], [], [], [], shape=(4, 5), n_sensors=3)
    assert empty[0].tolist() == [0] and empty[1].size == 0
    s, u, v = utils.split_positions(pos, (4, 5))
    c = _cols()
    assert np.array_equal(s, c["sensor"]) and np.array_equal(u, c["ucell"]) and np.array_equal(v, c["vcell"])


@pytest.mark.parametrize("change,match", [
    (dict(sensor=[0, 0, 3, 1, 1]), r"event 0: sensor = 3 of digit 2"),
    (dict(ucell=[0, 3, 1, 2, 4]), r"event 2: ucell = 4 of digit 4"),
    (dict(vcell=[4, 0, 2, 5, 3]), r"event 2: vcell = 5 of digit 3"),
    (dict(vcell=np.array([4, 0, 2, -1, 3])), r"event 2: vcell = -1 of digit 3"),
    (dict(charge=[9, 0, 1, 7, 8]), r"event 0: charge = 0 of digit 1"),
    (dict(event_offsets=[1, 3, 3, 5]), r"starts at 1"),
    (dict(event_offsets=[0, 3, 2, 5]), r"decreases at event 1"),
    (dict(event_offsets=[0, 3, 3, 6]), r"sensor has 5 entries, event_offsets ends at 6"),
    (dict(charge=[9, 255, 1, 7]), r"charge has 4 entries, event_offsets ends at 5"),
    (dict(ucell=[3, 0, 1, 2, 2], vcell=[0, 4, 2, 1, 3]), r"event 0: digit 1 .* does not lie behind digit 0"),          # unsorted
    (dict(vcell=[4, 0, 2, 3, 3]), r"event 2: digit 4 .* does not lie behind digit 3"),                                # duplicate
    (dict(event_offsets=[0, 1, 3, 5], sensor=[0, 2, 0, 1, 1]), r"event 1: digit 2 .* does not lie behind digit 1"),    # unsorted across sensors
])
def test_every_breach_of_the_contract_is_a_value_error_before_any_device_call(change, match, monkeypatch):
    import _hip
    import utils

    def no_device(*a, **k):
        raise AssertionError("a device call before the host checks were done")
    monkeypatch.setattr(_hip, "require_gpu", no_device)
    monkeypatch.setattr(_hip, "call", no_device)
    cols = dict(_cols(), **{k: np.asarray(v) for k, v in change.items()})
    with pytest.raises(ValueError, match=match):
        utils.PXDEventStore.from_arrays(**cols, shape=(4, 5), n_sensors=3)
    with pytest.raises(ValueError, match=match):
        utils.event_columns(**cols, shape=(4, 5), n_sensors=3)


def test_a_geometry_beyond_int32_positions_is_refused():
    import utils
    with pytest.raises(ValueError, match="fit int32"):
        utils.event_columns([0], [], [], [], [], shape=(65536, 32768), n_sensors=1)


def test_event_file_round_trip_up_to_the_upload(tmp_path):
    """``write_digits`` -> the host half of ``from_file`` keeps every column; ``events=`` takes a subset in the order asked for."""
    import utils
    S, H, W = 7, 13, 37
    events = ER.pattern_events(KINDS, S, H, W, seed=5)
    cols = ER.columns(events, S)
    path = os.path.join(str(tmp_path), "events.npz")
    utils.write_digits(path, *cols)
    assert utils.event_file_length(path) == len(KINDS)
    off, pos, charge = utils.read_event_columns(path, (H, W), S)
    assert np.array_equal(off, cols[0]) and np.array_equal(charge, cols[4]) and pos.dtype == np.int32
    for got, want in zip(utils.split_positions(pos, (H, W)), cols[1:4]):
        assert np.array_equal(got, want)
    pick = [5, 0, 1, 5, 3]
    soff, spos, scharge = utils.read_event_columns(path, (H, W), S, events=pick)
    assert np.array_equal(np.diff(soff), np.diff(cols[0])[pick])
    s, u, v = utils.split_positions(spos, (H, W))
    assert np.array_equal(ER.dense((soff, s, u, v, scharge), range(len(pick)), (H, W), S), np.concatenate([events[i] for i in pick]))
    with pytest.raises(ValueError, match="events= holds"):
        utils.read_event_columns(path, (H, W), S, events=[len(KINDS)])
    with pytest.raises(ValueError, match=r"event 1: ucell = \d+ of digit \d+ is outside 0 .. 11"):      # the file against a smaller geometry
        utils.read_event_columns(path, (12, W), S)
    np.savez(os.path.join(str(tmp_path), "other.npz"), a=np.zeros(3))
    with pytest.raises(ValueError, match="no event file"):
        utils.read_event_columns(os.path.join(str(tmp_path), "other.npz"))


def test_the_store_has_no_cpu_path():
    import utils
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            utils.PXDEventStore.from_arrays(**_cols(), shape=(4, 5), n_sensors=3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        utils.PXDEventStore(*utils.event_columns(**_cols(), shape=(4, 5), n_sensors=3), shape=(4, 5), n_sensors=3, device="cpu")


def test_event_entry_points_are_declared_exported_and_bound():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for sym in ("ieagan_pxd_event_ingest", "ieagan_pxd_event_dense"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    assert len(_hip._SIGS["ieagan_pxd_event_ingest"]) == 15 and len(_hip._SIGS["ieagan_pxd_event_dense"]) == 12
    assert _hip._SIGS["ieagan_pxd_event_ingest"][3] is ctypes.c_long and _hip._SIGS["ieagan_pxd_event_ingest"][12] is ctypes.c_float
    lib.ieagan_abi_version.restype = ctypes.c_int
    assert lib.ieagan_abi_version() == _hip.ABI_VERSION         # new entry points only: no struct and no existing signature changed


def test_launchers_reject_bad_arguments_before_any_launch():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.ieagan_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_longlong * 64)()
    a = ctypes.addressof(buf)
    ingest, dense = lib.ieagan_pxd_event_ingest, lib.ieagan_pxd_event_dense
    ingest.argtypes, dense.argtypes = _hip._SIGS["ieagan_pxd_event_ingest"], _hip._SIGS["ieagan_pxd_event_dense"]
    good = dict(pos=a, charge=a, offsets=a, n_digits=8, n_events=2, ids=a, E=1, S=4, H=8, W=8)
    for change, text in ((dict(pos=None), "pos / charge is NULL"), (dict(pos=a + 2), "pos is not 4-byte aligned"),
                         (dict(offsets=None), "offsets is NULL"), (dict(offsets=a + 4), "offsets is not 8-byte aligned"),
                         (dict(ids=None), "event_ids is NULL"), (dict(n_digits=-1), "is negative"), (dict(E=0), "E = 0 events"),
                         (dict(E=20000), "outside 1 .. 65535"), (dict(H=0), "bad image size"),
                         (dict(S=64, H=8192, W=8192), "does not fit the int32 flat index")):
        k = dict(good, **change)
        args = (k["pos"], k["charge"], k["offsets"], k["n_digits"], k["n_events"], k["ids"], k["E"], k["S"], k["H"], k["W"])
        for call, who in ((lambda: ingest(*args, 3, None, 0.004, a, None), "pxd_event_ingest: "), (lambda: dense(*args, a, None), "pxd_event_dense: ")):
            rc = call()
            msg = lib.ieagan_last_error().decode()
            assert rc != 0 and msg.startswith(who) and text in msg, (change, msg)
    args = tuple(good.values())
    assert ingest(*args, -1, None, 0.004, a, None) != 0 and "pad = -1" in lib.ieagan_last_error().decode()
    assert ingest(*args, 3, None, 0.004, None, None) != 0 and "out is NULL" in lib.ieagan_last_error().decode()
    assert ingest(*args, 3, a + 2, 0.004, a, None) != 0 and "noise is not 4-byte aligned" in lib.ieagan_last_error().decode()
    assert dense(*args, None, None) != 0 and "out is NULL" in lib.ieagan_last_error().decode()
