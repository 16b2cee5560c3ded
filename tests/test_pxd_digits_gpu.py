"""Event production on the device (MI355X): the digit kernel against the restatement of the reference's digit extraction
(tests/pxd_digits_reference.py), the capacity protocol, ``model.generate(sparse=True)`` and ``produce.py``.

Every comparison is exact (``torch.equal`` / ``array_equal``): charges are integers, positions are integers, and the order -- ascending
flat index, the order of ``torch.nonzero`` -- is part of the contract.  There are no tolerances."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pxd_digits_reference as DR
import pxd_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _check(d, ev, threshold, tag):
    """A ``PXDDigits`` against the restatement of the host array ``ev``; prints the figures before it asserts."""
    index, charge, counts, total = DR.digits(ev, threshold)
    got_total = int(d.total.cpu())
    print(f"{tag}: threshold {threshold} total {got_total} (restatement {total}) capacity {d.capacity} images {ev.shape[0]}")
    assert d.index.dtype == torch.int32 and d.charge.dtype == torch.uint8 and d.counts.dtype == torch.int32 and d.total.dtype == torch.int32
    assert d.counts.shape == (ev.shape[0],) and d.total.shape == (1,)
    assert got_total == total, tag
    assert torch.equal(d.counts.cpu(), counts), tag
    assert total <= d.capacity, (tag, "the test's capacity is too small")
    assert torch.equal(d.index[:total].cpu(), index), tag
    assert torch.equal(d.charge[:total].cpu(), charge), tag


def _all_hit(kind):
    rng = np.random.Generator(np.random.PCG64(2))
    return rng.integers(8, 256, (1, 250, 768)).astype(np.uint8 if kind == "u8" else np.float32)      # a digit at either cut


CASES = {
    "40x250x768": lambda kind: (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(40, 250, 768, seed=31),
    "7x13x37": lambda kind: (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(7, 13, 37, seed=32, p_hit=0.3),
    "all_zero": lambda kind: np.zeros((40, 58, 64), np.uint8 if kind == "u8" else np.float32),
    "one_all_hit": _all_hit,
}


@pytest.mark.parametrize("threshold", [0.0, 7.0])
@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_against_restatement(case, kind, threshold):
    import utils
    ev = CASES[case](kind)
    n = ev.shape[0]
    if case == "40x250x768" and kind == "f32":       # the planted edge values are there and the two cuts differ on them
        flat = ev.reshape(-1)
        assert ((flat >= 6.78) & (flat < 7)).sum() >= 40 * 4 and (flat == 255.0).any() and ((flat > 0) & (flat < 1)).any()
        assert DR.digits(ev, 0.0)[3] > DR.digits(ev, 7.0)[3]
    d = utils.pxd_digits(torch.from_numpy(ev).to(DEV), threshold=threshold, capacity=ev.size if ev.size < 10 ** 6 else None, n_sensors=n)
    assert d.index.is_cuda and d.capacity == (ev.size if ev.size < 10 ** 6 else max(1024, ev.size // 16))
    _check(d, ev, threshold, f"{case} {kind}")
    if case == "one_all_hit":
        assert int(d.total.cpu()) == 250 * 768 == d.capacity
    idx, chg, counts = d.cpu()
    want = DR.digits(ev, threshold)
    assert np.array_equal(idx, want[0].numpy()) and np.array_equal(chg, want[1].numpy()) and np.array_equal(counts, want[2].numpy())


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_view_one_element_past_a_16_byte_boundary(kind):
    import utils
    ev = (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(6, 21, 53, seed=3, p_hit=0.2)
    t = torch.from_numpy(ev).to(DEV)
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:].copy_(t.reshape(-1))
    view = buf[1:].view(6, 21, 53)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    for thr in (0.0, 7.0, 100.5):
        d = utils.pxd_digits(view, threshold=thr, capacity=ev.size, n_sensors=3)
        assert d.images.data_ptr() == view.data_ptr()
        _check(d, ev, thr, f"{kind} offset view")


def test_values_outside_the_uint8_range():
    """Negative, huge, infinite and NaN pixels (the export epilogue produces none of them; the rule still covers them)."""
    import utils
    ev = R.synthetic_f32(4, 30, 50, seed=8, p_hit=0.1)
    flat = ev.reshape(-1)
    odd = [-1.0, -0.0, np.nan, np.inf, -np.inf, 300.0, 255.5, 1e30, -1e30, 0.5, 256.0, 1.5, 255.0, 254.999, np.nan, 2.0]
    flat[::97] = np.resize(np.array(odd, np.float32), flat[::97].size)
    for thr in (0.0, 7.0):
        _check(utils.pxd_digits(torch.from_numpy(ev).to(DEV), threshold=thr, capacity=ev.size, n_sensors=4), ev, thr, "odd values")


def test_reference_export_fixture(golden_dir):
    import utils
    adu = np.load(os.path.join(golden_dir, "op_export.npz"))["adu"]
    u8 = torch.from_numpy(adu).to(torch.uint8)
    nz = u8.nonzero()
    d = utils.pxd_digits(torch.from_numpy(adu).to(DEV), capacity=adu.size)
    total = int(d.total.cpu())
    assert total == nz.shape[0]
    assert torch.equal(d.index[:total].cpu().to(torch.int64), nz[:, 0] * 240 + nz[:, 1] * 24 + nz[:, 2])
    assert torch.equal(d.charge[:total].cpu(), u8[u8 > 0])
    ev, sensor, ucell, vcell, charge = d.unpack()
    assert np.array_equal(sensor, nz[:, 0].numpy()) and np.array_equal(ucell, nz[:, 1].numpy()) and np.array_equal(vcell, nz[:, 2].numpy())
    assert not ev.any() and np.array_equal(charge, u8[u8 > 0].numpy())
    _check(utils.pxd_digits(u8.to(DEV), capacity=adu.size), u8.numpy(), 0.0, "op_export uint8")


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_capacity_below_total_keeps_counts_and_touches_nothing_beyond(kind):
    import _hip as H
    import utils
    ev = (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(40, 250, 768, seed=41)
    index, charge, counts, total = DR.digits(ev, 0.0)
    x = torch.from_numpy(ev).to(DEV)
    n, h, w = ev.shape
    for cap in (total // 3, 1, 0, total - 1):
        # straight through the C ABI on buffers 64 elements longer than the capacity, pre-filled with a sentinel
        idx_buf = torch.full((cap + 64,), -77, dtype=torch.int32, device=DEV)
        chg_buf = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        hdr = torch.full((n + 1,), -1, dtype=torch.int32, device=DEV)
        scratch = torch.empty(H.lib().ieagan_pxd_digits_scratch(n, h, w), dtype=torch.int32, device=DEV)
        H.call("ieagan_pxd_digits", x.data_ptr(), int(kind == "u8"), n, h, w, 0.0, cap, idx_buf.data_ptr(), chg_buf.data_ptr(), hdr.data_ptr(),
               hdr.data_ptr() + 4 * n, scratch.data_ptr(), H.stream())
        torch.cuda.synchronize()
        print(f"{kind}: capacity {cap} total {int(hdr[n])} (true {total})")
        assert int(hdr[n]) == total and torch.equal(hdr[:n].cpu(), counts)
        assert torch.equal(idx_buf[:cap].cpu(), index[:cap]) and torch.equal(chg_buf[:cap].cpu(), charge[:cap])
        assert bool((idx_buf[cap:] == -77).all()) and bool((chg_buf[cap:] == 0xAB).all())
    # the Python surface never hands back a truncated event
    d = utils.pxd_digits(x, capacity=total // 3)
    assert d.capacity == total // 3 and int(d.total.cpu()) == total
    ev_id, sensor, ucell, vcell, chg = d.unpack()
    assert d.capacity == total and chg.size == total
    i64 = index.to(torch.int64).numpy()
    assert np.array_equal(sensor, i64 // (h * w)) and np.array_equal(ucell, i64 % (h * w) // w) and np.array_equal(vcell, i64 % w)
    assert np.array_equal(chg, charge.numpy()) and not ev_id.any()
    # a copy shorter than the event (what produce.py does after a small batch) is completed, not truncated
    d = utils.pxd_digits(x).start_copy(expect=100)
    idx, chg, cnt = d.cpu()
    assert np.array_equal(idx, index.numpy()) and np.array_equal(chg, charge.numpy()) and np.array_equal(cnt, counts.numpy())


def test_two_runs_are_bit_identical():
    import utils
    x = torch.from_numpy(R.synthetic_f32(40, 250, 768, seed=5)).to(DEV)
    a = utils.pxd_digits(x)
    b = utils.pxd_digits(x)
    total = int(a.total.cpu())
    assert total > 40 * 1500
    assert torch.equal(a.header, b.header)
    assert torch.equal(a.index[:total], b.index[:total]) and torch.equal(a.charge[:total], b.charge[:total])
    assert bool((a.index[1:total] > a.index[:total - 1]).all())          # strictly ascending flat index


def test_call_neither_synchronises_nor_copies_and_replays_from_a_graph():
    """``pxd_digits`` is captured into a HIP graph: a synchronising call or a device-to-host copy inside a capture raises.  The replay
    then runs on new input in the captured buffer."""
    import utils
    ev1 = R.synthetic_u8(40, 58, 64, seed=9)
    ev2 = R.synthetic_u8(40, 58, 64, seed=10)
    x = torch.from_numpy(ev1).to(DEV)
    utils.pxd_digits(x, capacity=8192)             # eager: loads the library
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d = utils.pxd_digits(x, capacity=8192)
    for ev in (ev1, ev2, ev1):
        x.copy_(torch.from_numpy(ev))
        g.replay()
        _check(d, ev, 0.0, "graph replay")
    assert DR.digits(ev1)[3] != DR.digits(ev2)[3]
    del g


def _generator(**over):
    import model
    from defaults import default_config
    cfg = default_config()
    cfg.update(device="cuda", resolution=64, H_base=1, outputroot=None, **over)
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        G = model.Generator(**dict(cfg, no_optim=True)).to(DEV)
    return cfg, G


def test_generate_sparse_equals_restatement_of_generate_dense():
    import model
    cfg, G = _generator()
    G.eval()
    torch.manual_seed(77)
    torch.cuda.manual_seed(77)
    dense = model.generate(G)
    assert dense.shape == (40, 58, 64) and not dense.is_cuda
    torch.manual_seed(77)
    torch.cuda.manual_seed(77)
    sparse = model.generate(G, sparse=True)
    want = DR.queue_format(dense.numpy())
    print("generate: digits", len(want[1]), "of", dense.numel(), "pixels; charge 6 occurs:", 6 in want[1])
    assert len(want[1]) > 0
    assert isinstance(sparse, tuple) and len(sparse) == 2 and len(sparse[0]) == 3
    assert all(isinstance(v, list) for v in sparse[0]) and isinstance(sparse[1], list)
    assert sparse[0][0] == want[0][0] and sparse[0][1] == want[0][1] and sparse[0][2] == want[0][2]
    assert sparse[1] == want[1]
    assert all(type(v) is int for v in sparse[1][:5] + sparse[0][0][:5] + sparse[0][1][:5] + sparse[0][2][:5])


def test_produce_tool_as_a_child_process(tmp_path):
    import produce
    import utils
    tool = os.path.join(ROOT, "iea-gan_amd", "produce.py")
    out = os.path.join(str(tmp_path), "events.npz")
    geom = ["--resolution", "64", "--H_base", "1"]
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, tool, "--synthetic-weights", "--events", "5", "--events_per_batch", "2",
                        "--seed", "11", "--out", out] + geom, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec["events"] == 5 and rec["host_waits"] == 3                   # batches of 2, 2 and 1 events: one planned wait each
    side = json.load(open(out + ".json"))
    assert side["sha256(checkpoint)"] is None and side["events"] == 5 and side["seed"] == 11 and side["synthetic_weights"] is True
    # the same events, dense, in this process: the same weights (seed), the same latents (seed), the same batches
    import train
    cfg = train.parse(geom)
    with contextlib.redirect_stdout(io.StringIO()):
        G, digest = produce.load_generator(cfg, None, synthetic=True, seed=11)
    assert digest is None
    dense = torch.cat([x.cpu() for x in produce.event_batches(G, cfg, 5, 2, 11)]).numpy()
    assert dense.shape == (200, 58, 64)
    events = list(utils.read_digits(out))
    assert len(events) == 5
    t = np.load(out)
    assert t["event_offsets"].shape == (6,) and t["event_offsets"][-1] == rec["digits"] == t["charge"].size > 0
    for e, got in enumerate(events):
        want = DR.queue_format(dense[40 * e:40 * (e + 1)])
        assert got[1] == want[1] and got[0][0] == want[0][0] and got[0][1] == want[0][1] and got[0][2] == want[0][2], e
    # per-sensor hit counts at the 7 ADU cut, both sides: the file's digits with value >= 7 against utils.PXDStatistics on the dense events
    acc = utils.PXDStatistics(n_sensors=40, threshold=7.0, device=DEV)
    acc.update(torch.from_numpy(dense).to(DEV))
    hits = acc.result()["hits"]
    assert hits.shape == (5, 40)
    d7 = utils.pxd_digits(torch.from_numpy(dense).to(DEV), threshold=7.0)
    assert np.array_equal(d7.cpu()[2].reshape(5, 40), hits)
    off = t["event_offsets"]
    for e in range(5):
        s = slice(int(off[e]), int(off[e + 1]))
        assert np.array_equal(np.bincount(t["sensor"][s][t["charge"][s] >= 7], minlength=40), hits[e]), e


def test_produce_from_a_checkpoint_with_the_evaluation_cut(tmp_path):
    """``--weights`` + ``--use_ema`` + ``--threshold 7`` in process: the checkpoint's digest is recorded and no charge below 7 is written."""
    import hashlib
    import produce
    import utils
    cfg, G = _generator()
    cfg.update(outputroot=str(tmp_path))
    wdir = os.path.join(str(tmp_path), cfg["run_name"], "weights")
    os.makedirs(wdir)
    torch.save({k: v.detach().cpu().clone() for k, v in G.state_dict().items()}, os.path.join(wdir, "G_ema.pth"))
    torch.save({}, os.path.join(wdir, "state_dict.pth"))
    out = os.path.join(str(tmp_path), "cut.npz")
    with contextlib.redirect_stdout(io.StringIO()):
        rec = produce.run(["--weights", wdir, "--use_ema", "--events", "3", "--threshold", "7", "--out", out, "--resolution", "64", "--H_base", "1"])
    side = json.load(open(out + ".json"))
    assert side["sha256(checkpoint)"] == hashlib.sha256(open(os.path.join(wdir, "G_ema.pth"), "rb").read()).hexdigest()
    t = np.load(out)
    assert rec["host_waits"] == 3 and t["charge"].size == rec["digits"] > 0 and t["charge"].min() >= 7
    G.eval()
    dense = torch.cat([x.cpu() for x in produce.event_batches(G, cfg, 3, 1, 0)]).numpy()
    for e, got in enumerate(utils.read_digits(out)):
        assert got == DR.queue_format(dense[40 * e:40 * (e + 1)], 7.0), e
