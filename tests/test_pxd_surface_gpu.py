"""The Python half of the PXD surface on the device (MI355X): ``utils.PXDValidation`` against the three accumulators it bundles, fed
separately, and the accumulators fed the product before them against the same accumulators fed the images.

Every comparison is ``array_equal`` (``equal_nan`` for the float tables): both sides run the same kernels on the same input, and the
kernels are bit-identical run to run (tests/test_pxd_*_gpu.py hold them to the NumPy checkers).  There are no tolerances."""
import numpy as np
import pytest
import torch

import pxd_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S, HH, WW, THRESHOLD, CUTS = 4, 64, 96, 7.0, (20, 30)
PARTS = ("stats", "clusters", "maps")


def _events(kind, n=3, p_hit=0.04):
    make = R.synthetic_u8 if kind == "u8" else R.synthetic_f32
    return [torch.from_numpy(make(S, HH, WW, seed=90 + i, p_hit=p_hit)).to(DEV) for i in range(n)]


def _separate(batches, n_sensors=S, threshold=THRESHOLD, cuts=CUTS, capacity=None):
    """The three accumulators fed ``batches`` one after the other -> their results, keyed like ``PXDValidation.result()``."""
    import utils
    kw = dict(n_sensors=n_sensors, threshold=threshold, device=DEV)
    accs = dict(stats=utils.PXDStatistics(**kw), clusters=utils.PXDClusterStatistics(capacity=capacity, **kw),
                maps=utils.PXDClusterMaps(seed_cut=cuts[0], charge_cut=cuts[1], capacity=capacity, **kw))
    for x in batches:
        for acc in accs.values():
            acc.update(x)
    return {k: acc.result() for k, acc in accs.items()}


def _assert_equal(got, want, tag):
    assert set(got) == set(want), tag
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=b.dtype.kind == "f"), (tag, k)


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_bundle_equals_the_three_accumulators_fed_separately(kind):
    import utils
    evs = _events(kind)
    batches = [torch.cat(evs[:2]), evs[2]]
    want = _separate(batches)
    acc = utils.PXDValidation(clusters=True, maps=CUTS, n_sensors=S, threshold=THRESHOLD, device=DEV)
    for x in batches:
        acc.update(x)
    got = acc.result()
    assert tuple(got) == PARTS and got["stats"]["n_events"] == 3
    for part in PARTS:
        _assert_equal(got[part], want[part], f"{kind} {part}")
    assert got["stats"]["hits"].sum() > got["clusters"]["clusters"].sum() > got["maps"]["clusters"].sum() > 0
    assert got["maps"]["shape"] == (HH, WW) and got["stats"]["charge"].dtype == np.float32
    # the parts that are off stay off
    only = utils.PXDValidation(maps=True, n_sensors=S, threshold=THRESHOLD, device=DEV)
    assert only.clusters is None and (only.maps.seed_cut, only.maps.charge_cut) == (0, 0)
    only.update(batches[1])
    assert tuple(only.result()) == ("stats", "maps")
    bare = utils.PXDValidation(n_sensors=S, threshold=THRESHOLD, device=DEV)
    assert bare.clusters is None and bare.maps is None
    # distances and side tables: composed by hand from the three distance functions, with the names of validate.py
    other = _separate(batches[:1])
    dist = dict(utils.pxd_distance(want["stats"], other["stats"]), **utils.pxd_cluster_distance(want["clusters"], other["clusters"]),
                **utils.pxd_map_distance(want["maps"], other["maps"]))
    got_dist = utils.pxd_validation_distance(got, other)
    assert list(got_dist) == list(dist) and len(dist) == 11
    for k, v in dist.items():
        assert got_dist[k] == v or (np.isnan(v) and np.isnan(got_dist[k])), k
    assert got_dist["occ_rel_err"] > 0
    tables = {}
    for part, skip in (("stats", ()), ("clusters", ("n_events",)), ("maps", ("n_events", "shape"))):
        for side, res in (("real", want), ("fake", other)):
            for k, v in res[part].items():
                if k not in skip:
                    tables[f"{side}_{'accepted_clusters' if part == 'maps' and k == 'clusters' else k}"] = np.asarray(v)
    got_tables = utils.pxd_validation_tables(real=got, fake=other)
    assert list(got_tables) == list(tables)
    _assert_equal(got_tables, tables, f"{kind} tables")
    assert {"real_n_events", "fake_clusters", "real_accepted_clusters", "fake_count_map"} <= set(tables) and "real_shape" not in tables


@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_accumulators_take_the_product_before_them(kind):
    import utils
    x = torch.cat(_events(kind, 2))
    want = _separate([x])
    kw = dict(n_sensors=S, threshold=THRESHOLD, device=DEV)
    c = utils.pxd_clusters(x, THRESHOLD, n_sensors=S)
    cs = utils.PXDClusterStatistics(**kw)
    assert cs.update(c) is c
    _assert_equal(cs.result(), want["clusters"], "PXDClusters into PXDClusterStatistics")
    maps = utils.PXDClusterMaps(seed_cut=CUTS[0], charge_cut=CUTS[1], **kw)
    p = maps.update(c)
    assert isinstance(p, utils.PXDClusterPositions) and p.clusters is c and (p.seed_cut, p.charge_cut) == CUTS
    _assert_equal(maps.result(), want["maps"], "PXDClusters into PXDClusterMaps")
    maps = utils.PXDClusterMaps(seed_cut=CUTS[0], charge_cut=CUTS[1], **kw)
    assert maps.update(p) is p
    _assert_equal(maps.result(), want["maps"], "PXDClusterPositions into PXDClusterMaps")
    # a product made another way is refused before anything is launched: the tables stay what they are
    cs_before, maps_before = cs.tables.clone(), maps.tables.clone()
    wrong = {
        "threshold": utils.pxd_clusters(x, 0.0, n_sensors=S),
        "n_sensors": utils.pxd_clusters(x, THRESHOLD, n_sensors=2),
        "image size": utils.pxd_clusters(x[:, :, :64].contiguous(), THRESHOLD, n_sensors=S),
    }
    for what, bad in wrong.items():
        for acc, given in ((cs, bad), (maps, bad), (maps, utils.pxd_cluster_positions(bad, seed_cut=CUTS[0], charge_cut=CUTS[1]))):
            with pytest.raises(ValueError, match=what):
                acc.update(given)
    with pytest.raises(ValueError, match="seed_cut"):
        maps.update(utils.pxd_cluster_positions(c, seed_cut=CUTS[0] + 1, charge_cut=CUTS[1]))
    with pytest.raises(ValueError, match="charge_cut"):
        maps.update(utils.pxd_cluster_positions(c, seed_cut=CUTS[0], charge_cut=0))
    assert torch.equal(cs.tables, cs_before) and torch.equal(maps.tables, maps_before)
    assert len(cs.clusters) == 1 and len(maps.clusters) == 1 and cs.shape == maps.shape == (HH, WW)
    _assert_equal(cs.result(), want["clusters"], "after the refusals")


def test_bundle_refuses_an_overflowed_update():
    import utils
    x = _events("u8", 1)[0]
    assert int((x >= 7).sum()) > 64
    acc = utils.PXDValidation(clusters=True, maps=True, capacity=64, n_sensors=S, threshold=THRESHOLD, device=DEV)
    acc.update(x)
    assert acc.stats.result()["n_events"] == 1
    for part in (acc.clusters, acc.maps, acc):
        with pytest.raises(RuntimeError, match="capacity="):
            part.result()


def test_bundle_update_neither_synchronises_nor_copies_and_replays_from_a_graph():
    """``PXDValidation.update`` is captured into a HIP graph: a synchronising call or a device-to-host copy inside a capture raises.  The
    replay then runs on new input in the captured buffer."""
    import utils
    shape, cuts = (40, 58, 64), (40, 50)
    evs = [torch.from_numpy(R.synthetic_u8(*shape, seed=s, p_hit=0.05)).to(DEV) for s in (9, 10)]
    tabs = [_separate([ev], n_sensors=40, cuts=cuts, capacity=16384) for ev in evs]
    x = evs[0].clone()
    acc = utils.PXDValidation(clusters=True, maps=cuts, capacity=16384, n_sensors=40, threshold=THRESHOLD, device=DEV)
    acc.update(x)                       # eager: loads the library, allocates the tables
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        acc.update(x)
    for i in (0, 1, 0):
        x.copy_(evs[i])
        g.replay()
    res = acc.result()
    per_image = dict(stats=("hits", "charge"), clusters=("clusters",), maps=("clusters",))
    summed = dict(stats=("spectrum",), clusters=("size_spectrum", "charge_spectrum", "seed_spectrum", "size_u_spectrum", "size_v_spectrum"),
                  maps=("count_map", "charge_map", "u_profile", "v_profile"))
    for part in PARTS:
        assert res[part]["n_events"] == 2
        for k in summed[part]:
            assert np.array_equal(res[part][k], 3 * tabs[0][part][k] + tabs[1][part][k]), (part, k)
            assert not np.array_equal(tabs[0][part][k], tabs[1][part][k]), (part, k)
        for k in per_image[part]:
            assert np.array_equal(res[part][k], np.concatenate([tabs[0][part][k], tabs[0][part][k]])), (part, k)
    del g
