"""The kernels over the sparse digit list and the cluster table at the edges of their shared walk (MI355X): digit totals around the ends of
a wave's step of 64 (63, 64, 65), the smallest that give a wave a second step (257) and the launch a second workgroup (1100: ``cl_blocks``
is 2 from a capacity of 1025 on), none and one, each with the capacity equal to the total and 7 above it.  Images are 4 x 8 x 40 with two
sensors; exactly M pixels are planted, a few of them as touching pairs.

For every case the whole chain runs -- digits, clusters, positions (no cut and a cut that rejects some), hits, region counts (1 x 1 and
2 x 4), the overlay with a second planted batch and the match of the batch against that overlay -- and every array is compared with the
NumPy restatements (tests/pxd_*_reference.py) by ``np.array_equal``; positions are compared as bit patterns.  A capacity of M - 1 is added
for the two products whose tests state what a truncated result is: digits and overlay.  The restatements are first checked against each
other on the host, on these very inputs."""
import functools

import numpy as np
import pytest
import torch

import pxd_corr_reference as XR
import pxd_events_reference as ER
import pxd_match_reference as MR
import pxd_overlay_reference as OR

DEV = "cuda:0"
N, H, W, S = 4, 8, 40, 2
TOTALS = (0, 1, 63, 64, 65, 256, 257, 1100)
SECOND = 97                         # digits of the second planted batch
CUTS = ((0, 0), (100, 150))
REGIONS = ((1, 1), (2, 4))
PITCH = (100, 111)
PER_CLUSTER = ("pu", "pv", "v_start", "qh_u", "qt_u", "qh_v", "qt_v")
INT_COLUMNS = ("cluster", "sensor", "event", "mixed_hit", "flags", "found", "size", "charge", "match", "hi", "mixed_charge", "signal_charge",
               "signal_size", "n_signal", "counts")


@functools.lru_cache(maxsize=None)
def planted(M, seed):
    """uint8 ``[N, H, W]`` with exactly ``M`` pixels above 0: up to eight horizontal pairs of neighbours first, the rest anywhere."""
    rng = np.random.Generator(np.random.PCG64([seed, M]))
    pixels = N * H * W
    taken = []
    for p in rng.permutation(pixels).tolist():
        if len(taken) + 2 > min(M, 16):
            break
        if p % W < W - 1 and p not in taken and p + 1 not in taken:
            taken += [p, p + 1]
    rest = np.setdiff1d(np.arange(pixels), taken)
    taken = np.concatenate([np.asarray(taken, np.int64), rng.permutation(rest)[:M - len(taken)]])
    x = np.zeros(pixels, np.uint8)
    x[taken] = rng.integers(1, 256, taken.size)
    assert np.count_nonzero(x) == M
    return x.reshape(N, H, W)


@functools.lru_cache(maxsize=None)
def reference(M, cuts):
    """The restatement of everything for ``M`` digits: computed once, shared by the tests, never written."""
    signal, second = planted(M, 11), planted(SECOND, 12)
    tables = (np.full((1, H), PITCH[0]), np.full((1, W), PITCH[1]), np.zeros(S, np.int64))
    ref = MR.match(signal, MR.overlay(signal, second), tables, 3, 0.0, *cuts)
    A, B = (ER.columns(list(x.reshape(-1, S, H, W)), S) for x in (signal, second))
    return dict(ref, signal=signal, second=second, A=A, B=B, ids=list(range(N // S)))


@pytest.mark.parametrize("M", TOTALS)
def test_the_restatements_agree_with_each_other_on_the_planted_batches(M):
    for cuts in CUTS:
        ref = reference(M, cuts)
        assert ref["cs"]["index"].size == M and ref["cm"]["index"].size == np.count_nonzero(ref["signal"] | ref["second"])
        assert MR.same_tables(MR.dense(ref["cs"], ref["cm"], ref["shape"]), MR.sparse(ref["cs"], ref["cm"], ref["shape"])), M
    args = (ref["A"], ref["ids"], ref["B"], ref["ids"], (H, W), S)
    assert OR.same(OR.dense(*args), OR.sparse(*args)), M
    assert np.array_equal(OR.dense_sum(*args), MR.overlay(ref["signal"], ref["second"])), M
    if 16 <= M < 1000:
        assert (ref["cs"]["size"] > 1).any() and (ref["cs"]["size"] == 1).any()
        assert 0 < reference(M, CUTS[1])["ps"]["total"] < ref["cs"]["total"]           # the cut rejects some, not all


def _np(t, n):
    return t[:n].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flat(cols):
    off, s, u, v, q = cols
    return off.astype(np.int64), ((s.astype(np.int64) * H + u) * W + v).astype(np.int32), q.astype(np.uint8)


def _capacities(M):
    return sorted({M, M + 7})


@pytest.mark.gpu
@pytest.mark.parametrize("M,cap", [(M, cap) for M in TOTALS for cap in _capacities(M)])
def test_the_chain_against_the_restatements(M, cap):
    import utils
    geometry = utils.PXDGeometry.uniform((H, W), *PITCH, S)
    ref = reference(M, CUTS[0])
    cs, tag = ref["cs"], (M, cap)
    T = cs["total"]
    x = torch.from_numpy(ref["signal"]).to(DEV)
    d = utils.pxd_digits(x, 0.0, cap, S)
    assert int(d.total.cpu()) == M and np.array_equal(d.counts.cpu().numpy(), np.count_nonzero(ref["signal"].reshape(N, -1), axis=1)), tag
    assert np.array_equal(_np(d.index, M), cs["index"]) and np.array_equal(_np(d.charge, M), cs["digit_charge"]), tag
    c = utils.pxd_clusters(d)
    assert int(c.total.cpu()) == T and np.array_equal(c.counts.cpu().numpy(), cs["counts"]) and np.array_equal(_np(c.label, M), cs["label"]), tag
    for k in c.TABLE:
        assert np.array_equal(_np(getattr(c, k), T), cs[k]), (tag, k)
    for regions in REGIONS:
        assert np.array_equal(utils.pxd_region_counts(d, regions).cpu().numpy(), XR.region_counts(ref["signal"], regions, S)), (tag, regions)
    mixed = torch.from_numpy(MR.overlay(ref["signal"], ref["second"])).to(DEV)
    for cuts in CUTS:
        ref = reference(M, cuts)
        ps, hs, Mm = ref["ps"], ref["hs"], ref["cm"]["index"].size
        A = ps["total"]
        p = utils.pxd_cluster_positions(c, seed_cut=cuts[0], charge_cut=cuts[1])
        assert int(p.total.cpu()) == A and np.array_equal(p.counts.cpu().numpy(), ps["counts"]), (tag, cuts)
        assert np.array_equal(_np(p.mu, T), ps["mu"]) and np.array_equal(_np(p.mv, T), ps["mv"]) and np.array_equal(_np(p.cluster, A), ps["cluster"]), (tag, cuts)
        assert np.array_equal(_bits(_np(p.u, A)), _bits(ps["u"])) and np.array_equal(_bits(_np(p.v, A)), _bits(ps["v"])), (tag, cuts)
        h = utils.pxd_hits(p, geometry, 3)
        for k in PER_CLUSTER:
            assert np.array_equal(_np(getattr(h, k), T), hs[k]), (tag, cuts, k)
        assert np.array_equal(_bits(_np(h.u, A)), _bits(hs["u"])) and np.array_equal(_bits(_np(h.v, A)), _bits(hs["v"])), (tag, cuts)
        assert np.array_equal(_np(h.flags, A), hs["flags"]), (tag, cuts)
        # the match of the batch against its overlay with the second batch; the mixed side with its own total and the same slack
        hm = utils.pxd_hits(mixed, geometry, 3, 0.0, *cuts, Mm + cap - M, S)
        mt = utils.pxd_match(h, hm)
        host, want = mt.cpu(), ref["hits"]
        for k in INT_COLUMNS:
            assert host[k].dtype == want[k].dtype and np.array_equal(host[k], want[k]), (tag, cuts, k)
        for k in ("du", "dv"):
            assert np.array_equal(_bits(host[k]), _bits(want[k])), (tag, cuts, k)
        for k in MR.PER_CLUSTER:
            rows = T if k in ("found", "lo", "hi") else ref["cm"]["total"]
            assert np.array_equal(_np(getattr(mt, k), rows), ref["clusters"][k]), (tag, cuts, k)


def _overlay(ref, cap, pos_ptr, charge_ptr, offsets):
    """The entry point itself, on device id tensors."""
    import _hip
    import utils
    a, b = (utils.PXDEventStore.from_arrays(*cols, shape=(H, W), n_sensors=S, device=DEV) for cols in (ref["A"], ref["B"]))
    ids = torch.tensor(ref["ids"], dtype=torch.int32, device=DEV)
    E = ids.numel()
    scratch = torch.empty(_hip.lib().ieagan_pxd_event_overlay_scratch(E, cap), dtype=torch.int32, device=DEV)
    _hip.call("ieagan_pxd_event_overlay", *a._store_args(ids, E)[:6], *b._store_args(ids, E)[:6], E, S, H, W, cap, pos_ptr, charge_ptr,
              offsets.data_ptr(), scratch.data_ptr(), _hip.stream())


@pytest.mark.gpu
@pytest.mark.parametrize("M", TOTALS)
def test_the_overlay_at_the_total_above_it_and_truncated(M):
    """The merged total takes the place of M: capacity total, total + 7 and total - 1.  The offsets hold the true numbers whatever the
    capacity, and nothing is written at or beyond it (64 sentinels behind each output)."""
    ref = reference(M, CUTS[0])
    off, pos, charge = _flat(OR.sparse(ref["A"], ref["ids"], ref["B"], ref["ids"], (H, W), S))
    total = int(off[-1])
    for cap in (total, total + 7, total - 1):
        out_pos = torch.full((cap + 64,), -77, dtype=torch.int32, device=DEV)
        out_charge = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device=DEV)
        offsets = torch.full((off.size,), -1, dtype=torch.int64, device=DEV)
        _overlay(ref, cap, out_pos.data_ptr(), out_charge.data_ptr(), offsets)
        m = min(total, cap)
        assert np.array_equal(offsets.cpu().numpy(), off), (M, cap)
        assert np.array_equal(_np(out_pos, m), pos[:m]) and np.array_equal(_np(out_charge, m), charge[:m]), (M, cap)
        assert bool((out_pos[m:] == -77).all()) and bool((out_charge[m:] == 0xAB).all()), (M, cap)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [M for M in TOTALS if M > 0])
def test_digits_one_below_the_total_are_truncated_on_the_device_only(M):
    """Capacity M - 1: ``counts`` and ``total`` hold the true numbers, the first M - 1 digits are written and nothing behind them."""
    import _hip
    ref = reference(M, CUTS[0])
    x = torch.from_numpy(ref["signal"]).to(DEV)
    cap = M - 1
    index = torch.full((cap + 64,), -77, dtype=torch.int32, device=DEV)
    charge = torch.full((cap + 64,), 0xAB, dtype=torch.uint8, device=DEV)
    header = torch.full((N + 1,), -1, dtype=torch.int32, device=DEV)
    scratch = torch.empty(_hip.lib().ieagan_pxd_digits_scratch(N, H, W), dtype=torch.int32, device=DEV)
    _hip.call("ieagan_pxd_digits", x.data_ptr(), 1, N, H, W, 0.0, cap, index.data_ptr() if cap else None, charge.data_ptr() if cap else None,
              header.data_ptr(), header.data_ptr() + 4 * N, scratch.data_ptr(), _hip.stream())
    assert np.array_equal(header.cpu().numpy(), np.append(np.count_nonzero(ref["signal"].reshape(N, -1), axis=1), M)), M
    assert np.array_equal(_np(index, cap), ref["cs"]["index"][:cap]) and np.array_equal(_np(charge, cap), ref["cs"]["digit_charge"][:cap]), M
    assert bool((index[cap:] == -77).all()) and bool((charge[cap:] == 0xAB).all()), M
