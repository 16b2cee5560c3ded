"""The Python half of the PXD surface, host side (no GPU; CPU tensors): the packed read-back every ``result()`` / ``cpu()`` goes through and
the one loader of the event file.  The device side is tests/test_pxd_surface_gpu.py."""
import numpy as np
import pytest
import torch

I32 = [0, -1, 2 ** 31 - 1, -2 ** 31, 7]
U8 = [0, 255, 1, 128, 7]
F32_BITS = [-0x80000000, 0x7FC12345, 0x00000001, 0x3F800000, -0x00800000]     # -0.0, a NaN with a payload, a denormal, 1.0, -inf
I64 = [2 ** 32 + 5, -1, -2 ** 40 - 3, 2 ** 63 - 1, 0]


def _columns(n, lead):
    """Columns of all four dtypes, ``n`` entries each, behind ``lead`` 32-bit words (odd: a 64-bit column packed in the given order
    would start at an odd word)."""
    f32 = torch.tensor(F32_BITS[:n], dtype=torch.int32).view(torch.float32)
    return dict(header=torch.arange(lead, dtype=torch.int32), i32=torch.tensor(I32[:n], dtype=torch.int32),
                u8=torch.tensor(U8[:n], dtype=torch.uint8), f32=f32, mu=torch.tensor(I64[:n], dtype=torch.int64),
                mv=torch.tensor(I64[:n][::-1], dtype=torch.int64))


@pytest.mark.parametrize("lead", [3, 1, 4])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_read_back_round_trip_is_bit_identical_aligned_and_owned(n, lead):
    import utils
    cols = _columns(n, lead)
    if n == 5:
        f = cols["f32"].numpy()
        assert np.signbit(f[0]) and f[0] == 0 and np.isnan(f[1]) and 0 < f[2] < np.finfo(np.float32).tiny
        assert cols["mu"][0] > 2 ** 32 and cols["mu"][2] < -2 ** 32
    host = utils.pxd_read_back(**cols)
    assert set(host) == set(cols)
    for k, t in cols.items():
        a, want = host[k], t.numpy()
        assert a.dtype == want.dtype and a.shape == want.shape, k
        bits = (lambda v: v.view(np.int32)) if a.dtype == np.float32 else (lambda v: v)
        assert np.array_equal(bits(a), bits(want)), k
        assert a.flags.aligned and a.flags.owndata and a.flags.writeable, k
        assert not np.shares_memory(a, want), k


def test_read_back_keeps_a_shape_and_takes_a_strided_column():
    import utils
    table = torch.arange(24, dtype=torch.int64).reshape(4, 6) - 2 ** 35
    host = utils.pxd_read_back(odd=torch.ones(1, dtype=torch.uint8), table=table, every_other=table[:, ::2])
    assert host["table"].shape == (4, 6) and np.array_equal(host["table"], table.numpy())
    assert np.array_equal(host["every_other"], table.numpy()[:, ::2]) and host["every_other"].flags.aligned and host["every_other"].flags.owndata
    assert host["odd"].tolist() == [1]


def _cols():
    """Three events, the second empty (the file of tests/test_pxd_events.py)."""
    return dict(event_offsets=np.array([0, 3, 3, 5]), sensor=np.array([0, 0, 2, 1, 1], np.uint8), ucell=np.array([0, 3, 1, 2, 2], np.uint8),
                vcell=np.array([4, 0, 2, 1, 3], np.uint16), charge=np.array([9, 255, 1, 7, 8], np.uint8))


def test_the_readers_of_an_event_file_agree(tmp_path):
    import utils
    cols = _cols()
    assert list(utils.EVENT_COLUMNS) == list(cols)
    path = str(tmp_path / "events.npz")
    utils.write_digits(path, **cols)
    with np.load(path) as t:
        assert t.files == list(cols) and all(t[k].dtype == utils.EVENT_COLUMNS[k] for k in cols)
    events = list(utils.read_digits(path))
    off, pos, charge = utils.read_event_columns(path, shape=(4, 5), n_sensors=3)
    assert utils.event_file_length(path) == len(events) == off.size - 1 == 3
    assert [len(q) for _, q in events] == np.diff(off).tolist() == [3, 0, 2]
    assert events[1] == (([], [], []), [])
    flat = [(s * 4 + u) * 5 + v for (ss, uu, vv), _ in events for s, u, v in zip(ss, uu, vv)]
    assert flat == pos.tolist() and [q for _, qs in events for q in qs] == charge.tolist() == cols["charge"].tolist()


@pytest.mark.parametrize("lacks", [["charge"], ["event_offsets", "vcell"]])
def test_every_reader_refuses_a_file_that_lacks_a_column(lacks, tmp_path):
    import utils
    path = str(tmp_path / "broken.npz")
    np.savez(path, **{k: v for k, v in _cols().items() if k not in lacks})
    text = f"PXDEventStore: {path} is no event file of write_digits, it lacks {lacks}"
    for read in (lambda: utils.read_event_columns(path, shape=(4, 5), n_sensors=3), lambda: list(utils.read_digits(path)),
                 lambda: utils.event_file_length(path)):
        with pytest.raises(ValueError) as err:
            read()
        assert str(err.value) == text
