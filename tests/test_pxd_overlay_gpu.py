"""Background overlay on the device (MI355X): ``utils.pxd_overlay`` against the NumPy restatement (tests/pxd_overlay_reference.py) on the
planted pairs, at the three shapes of ``test_pxd_events_gpu.SHAPES``: 7 x 13 x 37 (every offset unaligned), 2 x 40 x 259 (one full image
gives a pair 20 720 input digits, far more than a wave's step of 64 and than a workgroup's 256) and 64 x 24 x 512 (many sensors).

Every comparison is ``np.array_equal`` / ``torch.equal``: positions and charges are integers, no tolerance appears anywhere.  The comparands
(the restatement, ``PXDEventStore.dense``, ``pxd_digits``, ``PXDEventStore.from_dense``) predate the kernel; it is never compared with itself
except where two runs must give the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pxd_events_reference as ER
import pxd_overlay_reference as OR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = {"7x13x37": (7, 13, 37), "2x40x259": (2, 40, 259), "64x24x512": (64, 24, 512)}
_CASES = {}


class Case:
    """The planted events of a shape as two stores, and the restatement of the planted pairs; built once, never changed."""

    def __init__(self, name):
        import utils
        self.S, self.H, self.W = S, H, W = SHAPES[name]
        ea, eb, self.pairs = OR.planted(S, H, W, seed=len(name))
        self.A, self.B = ER.columns(ea, S), ER.columns(eb, S)
        self.a = utils.PXDEventStore.from_arrays(*self.A, shape=(H, W), n_sensors=S, device=DEV)
        self.b = utils.PXDEventStore.from_arrays(*self.B, shape=(H, W), n_sensors=S, device=DEV)
        self.ids_a, self.ids_b = [p[0] for p in self.pairs], [p[1] for p in self.pairs]
        self.want = self.ref(self.ids_a, self.ids_b)

    def ref(self, ids_a, ids_b):
        return OR.sparse(self.A, ids_a, self.B, ids_b, (self.H, self.W), self.S)

    def flat(self, cols):
        """Columns -> ``(offsets int64, pos int32, charge uint8)`` tensors on the host."""
        off, s, u, v, q = cols
        pos = (s.astype(np.int64) * self.H + u) * self.W + v
        return torch.from_numpy(off.astype(np.int64)), torch.from_numpy(pos.astype(np.int32)), torch.from_numpy(q.astype(np.uint8))


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def _dev(ids):
    return torch.tensor(ids, dtype=torch.int32, device=DEV)


def _raw(c, ia, ib, capacity, pos_ptr, charge_ptr, offsets):
    """The entry point itself, on device id tensors."""
    import _hip as H
    E = ia.numel()
    scratch = torch.empty(H.lib().ieagan_pxd_event_overlay_scratch(E, capacity), dtype=torch.int32, device=DEV)
    H.call("ieagan_pxd_event_overlay", *c.a._store_args(ia, E)[:6], *c.b._store_args(ib, E)[:6], E, c.S, c.H, c.W, capacity, pos_ptr, charge_ptr,
           offsets.data_ptr(), scratch.data_ptr(), H.stream())


@pytest.mark.parametrize("name", list(SHAPES))
def test_planted_pairs_against_the_restatement(name):
    import utils
    c = _case(name)
    total = int(c.want[0][-1])
    # host ids: the capacity is the bound the host knows
    ov = utils.pxd_overlay(c.a, c.ids_a, c.b, c.ids_b)
    assert ov.capacity == int(c.a.counts[c.ids_a].sum() + c.b.counts[c.ids_b].sum()) and ov.shape == (c.H, c.W) and ov.n_sensors == c.S
    assert ov.pos.dtype == torch.int32 and ov.charge.dtype == torch.uint8 and ov.offsets.dtype == torch.int64
    assert ov.pos.shape == ov.charge.shape == (ov.capacity,) and ov.offsets.shape == (len(c.pairs) + 1,)
    merged = ov.store()
    got = merged.columns()
    print(f"{name}: {len(c.pairs)} pairs, {ov.capacity} input digits, {total} merged, shared {ov.shared().tolist()}")
    assert OR.same(got, c.want), name
    assert len(merged) == len(c.pairs) and np.array_equal(merged.counts, np.diff(c.want[0])) and merged.pos.numel() == total
    assert np.array_equal(ov.shared(), OR.shared(c.A, c.ids_a, c.B, c.ids_b, (c.H, c.W)))
    # the same ids as device tensors, with the exact capacity
    ov2 = utils.pxd_overlay(c.a, _dev(c.ids_a), c.b, _dev(c.ids_b), capacity=total)
    assert ov2.capacity == total and OR.same(ov2.store().columns(), c.want), name
    assert np.array_equal(ov2.shared(), ov.shared())
    # the method, with b_ids left out: the ids of a
    k = min(len(c.a), len(c.b))
    assert OR.same(c.a.overlay(list(range(k)), c.b).columns(), c.ref(range(k), range(k)))
    # every pair alone: E = 1, the pair starts at merged index 0 (the coincidence of pair 10 lies at the indices 63 and 64)
    for e, (ia, ib) in enumerate(c.pairs):
        want = c.ref([ia], [ib])
        assert OR.same(utils.pxd_overlay(c.a, _dev([ia]), c.b, _dev([ib]), capacity=int(want[0][-1])).store().columns(), want), (name, e)
    with pytest.raises(ValueError, match="capacity= is required"):
        utils.pxd_overlay(c.a, _dev(c.ids_a), c.b, c.ids_b)
    with pytest.raises(IndexError):
        utils.pxd_overlay(c.a, [len(c.a)], c.b, [0])


@pytest.mark.parametrize("name", list(SHAPES))
def test_ids_repeated_permuted_and_outside_the_stores(name):
    import utils
    c = _case(name)
    na, nb = len(c.a), len(c.b)
    ids_a = [1, na, 1, -1, 3, 2 ** 31 - 1, 2, 0, 6, 6]
    ids_b = [2, 1, nb, 7, 4, 5, -7, 0, 8, 7]
    want = c.ref(ids_a, ids_b)
    ov = utils.pxd_overlay(c.a, _dev(ids_a), c.b, _dev(ids_b), capacity=int(want[0][-1]))
    assert OR.same(ov.store().columns(), want), name
    assert np.array_equal(ov.shared(), OR.shared(c.A, ids_a, c.B, ids_b, (c.H, c.W)))
    # an empty event on one side: the other side as it is; a store over itself: min(2 q, 255)
    every = list(range(na))
    assert OR.same(utils.pxd_overlay(c.a, _dev(every), c.b, _dev([nb] * na), capacity=int(c.A[0][-1])).store().columns(), c.A)
    twice = c.a.overlay(every, c.a).columns()
    assert all(np.array_equal(t, a) for t, a in zip(twice[:4], c.A[:4])) and np.array_equal(twice[4], np.minimum(2 * c.A[4].astype(np.int64), 255))


@pytest.mark.parametrize("name", list(SHAPES))
def test_a_capacity_below_the_total_truncates_the_device_result_only(name):
    """Capacity one below the total, and 0 with NULL outputs: the offsets hold the true numbers, nothing is written at or beyond the
    capacity (64 sentinels behind each output), ``store()`` runs again and returns the whole."""
    import utils
    c = _case(name)
    off, pos, charge = c.flat(c.want)
    total = int(off[-1])
    ia, ib = _dev(c.ids_a), _dev(c.ids_b)
    for cap in (total - 1, total // 2, total, total + 5):
        out_pos = torch.full((cap + 64,), -77, dtype=torch.int32, device=DEV)
        out_charge = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        offsets = torch.full((len(c.pairs) + 1,), -1, dtype=torch.int64, device=DEV)
        _raw(c, ia, ib, cap, out_pos.data_ptr(), out_charge.data_ptr(), offsets)
        m = min(total, cap)
        assert torch.equal(offsets.cpu(), off), (name, cap)
        assert torch.equal(out_pos[:m].cpu(), pos[:m]) and torch.equal(out_charge[:m].cpu(), charge[:m]), (name, cap)
        assert bool((out_pos[m:] == -77).all()) and bool((out_charge[m:] == 0xAB).all()), (name, cap)
    offsets = torch.full((len(c.pairs) + 1,), -1, dtype=torch.int64, device=DEV)
    _raw(c, ia, ib, 0, None, None, offsets)
    assert torch.equal(offsets.cpu(), off), name
    ov = utils.pxd_overlay(c.a, ia, c.b, ib, capacity=total - 1)
    assert ov.capacity == total - 1 and int(ov.offsets[-1]) == total
    assert OR.same(ov.store().columns(), c.want) and ov.capacity == total


def test_output_views_one_element_past_a_16_byte_boundary_and_two_calls():
    c = _case("2x40x259")
    off, pos, charge = c.flat(c.want)
    total = int(off[-1])
    ia, ib = _dev(c.ids_a), _dev(c.ids_b)
    seen = []
    for k in (1, 3, 0, 1):                                      # elements past the boundary; the last repeats the first
        out_pos = torch.full((total + 64 + k,), -77, dtype=torch.int32, device=DEV)
        out_charge = torch.full((total + 64 + k,), 0xAB, dtype=torch.uint8, device=DEV)
        assert out_pos.data_ptr() % 16 == 0 and out_charge.data_ptr() % 16 == 0
        offsets = torch.empty(len(c.pairs) + 1, dtype=torch.int64, device=DEV)
        _raw(c, ia, ib, total, out_pos.data_ptr() + 4 * k, out_charge.data_ptr() + k, offsets)
        assert torch.equal(out_pos[k:k + total].cpu(), pos) and torch.equal(out_charge[k:k + total].cpu(), charge) and torch.equal(offsets.cpu(), off), k
        for buf, fill in ((out_pos, -77), (out_charge, 0xAB)):
            assert bool((buf[:k] == fill).all()) and bool((buf[k + total:] == fill).all()), k
        seen.append((out_pos[k:k + total].clone(), out_charge[k:k + total].clone(), offsets))
    assert all(torch.equal(x, y) for x, y in zip(seen[0], seen[3]))         # two calls give the same bytes


def test_the_call_is_captured_into_a_graph_and_replays_with_new_ids():
    """A synchronising call or a copy across PCIe inside a capture raises.  The replay reads the ids that stand in the id tensors then."""
    import utils
    c = _case("7x13x37")
    na, nb = len(c.a), len(c.b)
    sets = [([1, 2, 3], [2, 3, 4]), ([7, 1, 0], [8, 1, 1]), ([na, 4, 1], [0, nb, 2]), ([6, 6, 6], [7, 7, 7])]
    capacity = max(int(c.ref(a, b)[0][-1]) for a, b in sets) + 3
    ia, ib = _dev(sets[0][0]), _dev(sets[0][1])
    utils.pxd_overlay(c.a, ia, c.b, ib, capacity=capacity)      # eager: loads the library
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ov = utils.pxd_overlay(c.a, ia, c.b, ib, capacity=capacity)
    for a, b in sets:
        ia.copy_(torch.tensor(a, dtype=torch.int32))
        ib.copy_(torch.tensor(b, dtype=torch.int32))
        g.replay()
        off, pos, charge = c.flat(c.ref(a, b))
        total = int(off[-1])
        assert torch.equal(ov.offsets.cpu(), off), (a, b)
        assert torch.equal(ov.pos[:total].cpu(), pos) and torch.equal(ov.charge[:total].cpu(), charge), (a, b)
    del g


def test_from_digits_has_the_columns_of_from_dense():
    import utils
    S, H, W = SHAPES["7x13x37"]
    events = ER.pattern_events(["random", "empty", "edges", "one_sensor"], S, H, W, seed=9)
    x = torch.from_numpy(np.concatenate(events)).to(DEV)
    want = utils.PXDEventStore.from_dense(x, n_sensors=S, device=DEV)
    for capacity in (None, 10):                                 # 10: the digits do not fit, from_digits runs pxd_digits again
        got = utils.PXDEventStore.from_digits(utils.pxd_digits(x, 0.0, capacity, n_sensors=S))
        assert got.shape == (H, W) and got.n_sensors == S and got.device == want.device and len(got) == 4
        assert np.array_equal(got.counts, want.counts) and got.counts.dtype == np.int64
        for a, b in ((got.offsets, want.offsets), (got.pos, want.pos), (got.charge, want.charge)):
            assert a.dtype == b.dtype and torch.equal(a, b)
        assert OR.same(got.columns(), ER.columns(events, S))
        assert torch.equal(got.dense([3, 0]), torch.cat([x[3 * S:], x[:S]]))
    # a generated batch as an overlay operand
    sig = utils.PXDEventStore.from_arrays(*ER.columns(events[::-1], S), shape=(H, W), n_sensors=S, device=DEV)
    cols = ER.columns(events, S)
    assert OR.same(sig.overlay([0, 1, 2, 3], got).columns(), OR.sparse(ER.columns(events[::-1], S), range(4), cols, range(4), (H, W), S))
    with pytest.raises(ValueError, match="threshold"):
        utils.PXDEventStore.from_digits(utils.pxd_digits(x, -1.0, n_sensors=S))


@pytest.mark.parametrize("name", ["7x13x37", "2x40x259"])
def test_dense_images_and_validation_downstream_of_the_merged_store(name):
    """``merged.dense`` is the clamped sum of the operands' ``dense``, and every table of a ``PXDValidation`` over it equals the one over that
    sum: the chain downstream does not see where the images came from."""
    import utils
    c = _case(name)
    merged = c.a.overlay(c.ids_a, c.b, c.ids_b)
    ids = list(range(len(c.pairs)))
    summed = torch.clamp(c.a.dense(c.ids_a).to(torch.int16) + c.b.dense(c.ids_b), max=255).to(torch.uint8)
    assert torch.equal(merged.dense(ids), summed)
    assert torch.equal(summed.cpu(), torch.from_numpy(OR.dense_sum(c.A, c.ids_a, c.B, c.ids_b, (c.H, c.W), c.S)))
    results = []
    for images in (merged.dense(ids), summed):
        # a capacity of one digit a pixel: the planted events are far denser than the default capacity expects
        v = utils.PXDValidation(clusters=True, maps=True, capacity=images.numel(), n_sensors=c.S, threshold=7.0, device=DEV)
        v.update(images)
        results.append(v.result())
    assert set(results[0]) == set(results[1]) == {"stats", "clusters", "maps"}
    for part in results[0]:
        assert set(results[0][part]) == set(results[1][part])
        for k, v in results[0][part].items():
            assert np.array_equal(np.asarray(v), np.asarray(results[1][part][k]), equal_nan=np.asarray(v).dtype.kind == "f"), (part, k)
    assert results[0]["stats"]["hits"].sum() > 0 and results[0]["clusters"]["clusters"].sum() > 0


def test_overlay_events_as_a_child_process(tmp_path):
    import utils
    sys.path.insert(0, os.path.join(ROOT, "iea-gan_amd"))
    import overlay_events
    c = _case("7x13x37")
    sig, bg, out = (os.path.join(str(tmp_path), f) for f in ("signal.npz", "background.npz", "mixed.npz"))
    utils.write_digits(sig, *c.A)
    utils.write_digits(bg, *c.B)
    n = 11
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "iea-gan_amd", "overlay_events.py"), "--signal", sig,
                        "--background", bg, "--out", out, "--events", str(n), "--seed", "5", "--shape", str(c.H), str(c.W), "--n_sensors", str(c.S)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    ids_s, ids_b = overlay_events.pairs(len(c.a), len(c.b), n, 5)
    assert sorted(set(ids_b.tolist())) == list(range(len(c.b))) and ids_b.tolist() != list(range(len(c.b))) + [0, 1]
    want = c.ref(ids_s, ids_b)
    with np.load(out) as t:
        assert OR.same([t[k] for k in ("event_offsets", "sensor", "ucell", "vcell", "charge")], want)
    rec = json.load(open(out + ".json"))
    print(rec)
    assert rec == json.loads(p.stdout.strip().splitlines()[-1])
    shared = int(OR.shared(c.A, ids_s, c.B, ids_b, (c.H, c.W)).sum())
    assert rec == dict(events=n, signal_digits=int(np.diff(c.A[0])[ids_s].sum()), background_digits=int(np.diff(c.B[0])[ids_b].sum()),
                       digits=int(want[0][-1]), shared=shared) and shared > 0
