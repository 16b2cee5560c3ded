"""Event production, host side: the C ABI of the digit kernel, the event file, the restatement of the reference's digit extraction on the
reference's own output, and the absence of a CPU path (no GPU needed).  The device side is tests/test_pxd_digits_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pxd_digits_reference as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pxd_digits_is_declared_exported_and_bound():
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    header = open(os.path.join(ROOT, "include", "ieagan_hip.h")).read()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for sym in ("ieagan_pxd_digits", "ieagan_pxd_digits_scratch"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert hasattr(lib, sym), sym
        assert sym in _hip.EXPORTS and sym in _hip._SIGS, sym
    assert len(_hip._SIGS["ieagan_pxd_digits"]) == 13 and _hip._SIGS["ieagan_pxd_digits"][6] is ctypes.c_long
    # the scratch query is plain host code: one int32 word per wave of the count launch, four waves a workgroup, a capped grid
    lib.ieagan_pxd_digits_scratch.restype = ctypes.c_long
    lib.ieagan_pxd_digits_scratch.argtypes = [ctypes.c_int] * 3
    for n, h, w in ((40, 250, 768), (80, 250, 768), (7, 13, 37), (40, 58, 64), (1, 1, 1)):
        s = lib.ieagan_pxd_digits_scratch(n, h, w)
        assert s > 0 and s % (4 * n) == 0 and s // 4 <= 2048 + n, (n, h, w, s)
    assert lib.ieagan_pxd_digits_scratch(0, 250, 768) == 0


def test_launcher_rejects_bad_arguments_before_any_launch():
    """Argument checks are host code in front of the first launch: they answer without a device."""
    import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    fn = lib.ieagan_pxd_digits
    vp, i = ctypes.c_void_p, ctypes.c_int
    fn.argtypes = [vp, i, i, i, i, ctypes.c_float, ctypes.c_long, vp, vp, vp, vp, vp, vp]
    fn.restype = i
    lib.ieagan_last_error.restype = ctypes.c_char_p
    buf = (ctypes.c_int * 64)()
    a = ctypes.addressof(buf)
    good = dict(images=a, is_u8=0, N=1, H=2, W=2, threshold=0.0, capacity=4, index=a, charge=a, counts=a, total=a, scratch=a, stream=None)
    bad = [(dict(images=None), "images is NULL"), (dict(is_u8=2), "is_u8"), (dict(N=0), "N = 0"), (dict(H=0), "bad image size"),
           (dict(N=40000, H=250, W=768), "int32 flat index"), (dict(threshold=float("nan")), "NaN"), (dict(capacity=-1), "negative"),
           (dict(index=None), "index / charge is NULL"), (dict(index=a + 2), "4-byte aligned"), (dict(counts=None), "counts / total"),
           (dict(scratch=None), "scratch"), (dict(scratch=a + 1), "scratch"), (dict(images=a + 2), "fp32 images")]
    for over, msg in bad:
        args = dict(good, **over)
        assert fn(*args.values()) != 0, over
        assert msg in lib.ieagan_last_error().decode(), (over, lib.ieagan_last_error().decode())


def test_event_file_reads_back_event_by_event(tmp_path):
    import utils
    rng = np.random.Generator(np.random.PCG64(3))
    events = []
    for e in range(5):                      # event 3 is empty
        ev = np.where(rng.random((40, 250, 768)) < (0.0 if e == 3 else 0.002), rng.integers(1, 256, (40, 250, 768)), 0).astype(np.uint8)
        events.append(DR.queue_format(ev))
    offsets = np.concatenate([[0], np.cumsum([len(c) for _, c in events])])
    cat = lambda k: np.concatenate([np.asarray(nz[k], np.int64) for nz, _ in events])
    path = os.path.join(str(tmp_path), "events.npz")
    utils.write_digits(path, offsets, cat(0), cat(1), cat(2), np.concatenate([np.asarray(c, np.int64) for _, c in events]))
    t = np.load(path)
    assert t["event_offsets"].dtype == np.int64 and t["event_offsets"].shape == (6,)
    assert (t["sensor"].dtype, t["ucell"].dtype, t["vcell"].dtype, t["charge"].dtype) == (np.uint8, np.uint8, np.uint16, np.uint8)
    back = list(utils.read_digits(path))
    assert len(back) == 5 and back[3] == (([], [], []), [])
    for got, want in zip(back, events):
        assert got == want
        assert all(type(v) is int for v in got[1][:3] + got[0][2][:3])
    assert max(max(nz[2]) for nz, c in back if c) > 255            # a v cell that needs the uint16 column
    with pytest.raises(ValueError):
        utils.write_digits(path, offsets, cat(0)[:-1], cat(1), cat(2), cat(2))
    with pytest.raises(ValueError):
        utils.write_digits(path, offsets, cat(0), cat(1) + 300, cat(2), cat(2))


def test_restatement_on_the_reference_export(golden_dir):
    """``adu`` is the reference's own cropped detector-unit output [40, 10, 24]: the restatement equals ``nonzero`` of its uint8 form."""
    adu = np.load(os.path.join(golden_dir, "op_export.npz"))["adu"]
    assert adu.shape == (40, 10, 24) and adu.dtype == np.float32
    u8 = torch.from_numpy(adu).to(torch.uint8)
    nz = u8.nonzero()
    index, charge, counts, total = DR.digits(adu)
    assert total == nz.shape[0] == 5938
    assert torch.equal(index.to(torch.int64), nz[:, 0] * 240 + nz[:, 1] * 24 + nz[:, 2])
    assert torch.equal(charge, u8[u8 > 0]) and torch.equal(counts.to(torch.int64), (u8 > 0).flatten(1).sum(1))
    assert torch.equal(index, torch.sort(index)[0])
    (s, u, v), c = DR.queue_format(adu)
    assert (s, u, v) == tuple(t.tolist() for t in u8.nonzero(as_tuple=True)) and c == u8[u8.nonzero(as_tuple=True)].tolist()
    # the cut removes what lies below it and nothing else
    i7, c7, _, t7 = DR.digits(adu, 7.0)
    keep = torch.from_numpy(adu).flatten()[index.to(torch.int64)] >= 7.0
    assert torch.equal(i7, index[keep]) and torch.equal(c7, charge[keep]) and t7 == int(keep.sum())


def test_unpack_digits_splits_the_flat_index():
    import utils
    shape = (80, 250, 768)
    idx = np.array([0, 767, 768, 250 * 768 - 1, 250 * 768, 39 * 250 * 768 + 5 * 768 + 300, 40 * 250 * 768, 80 * 250 * 768 - 1])
    ev, s, u, v, c = utils.unpack_digits(idx, np.arange(8), shape, 40)
    assert ev.tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and s.tolist() == [0, 0, 0, 0, 1, 39, 0, 39]
    assert u.tolist() == [0, 0, 1, 249, 0, 5, 0, 249] and v.tolist() == [0, 767, 0, 767, 0, 300, 0, 767]
    assert (s.dtype, u.dtype, v.dtype, c.dtype) == (np.uint8, np.uint8, np.uint16, np.uint8)


def test_production_has_no_cpu_fallback(tmp_path, ref_cfg):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import contextlib
    import io
    import model
    import produce
    import utils
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        utils.pxd_digits(torch.zeros(40, 4, 4))
    out = os.path.join(str(tmp_path), "events.npz")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        produce.run(["--synthetic-weights", "--events", "1", "--out", out, "--resolution", "64", "--H_base", "1"])
    assert not os.path.exists(out)
    cfg = dict(ref_cfg, device="cpu", resolution=64, H_base=1)
    with contextlib.redirect_stdout(io.StringIO()):
        G = model.Generator(**cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.generate(G, sparse=True)
