"""NumPy checker of ``utils.pxd_cluster_positions`` and ``utils.PXDClusterMaps`` (tests only), on top of the cluster checker
``pxd_clusters_reference.clusters_of_digits``.

Moments are int64 sums (``np.add.at``): ``mu[j] = sum q * row``, ``mv[j] = sum q * column`` over the digits of cluster j.  A cluster is
accepted iff ``seed >= seed_cut and charge >= charge_cut``.  Positions are one float64 division rounded to float32:
``(mu.astype(float64) / charge.astype(float64)).astype(float32)`` -- numerator and denominator are exact integers below 2^53, so this is the
correctly rounded quotient and the device must give the same bits.  Map bins are decided in integers: ``(mu * 25) // (charge * H)``,
``(mv * 48) // (charge * W)``.
"""
import numpy as np

import pxd_clusters_reference as CR

MAP_U, MAP_V = 25, 48


def moments(cl, shape):
    """int64 ``(mu [clusters], mv [clusters])`` of a ``clusters_of_digits`` dict for an ``[N, H, W]`` batch."""
    N, H, W = shape
    rem = cl["index"].astype(np.int64) % (H * W)
    q = cl["digit_charge"].astype(np.int64)
    mu, mv = np.zeros(cl["total"], np.int64), np.zeros(cl["total"], np.int64)
    np.add.at(mu, cl["label"], q * (rem // W))
    np.add.at(mv, cl["label"], q * (rem % W))
    return mu, mv


def float_recipe(m, q):
    return (np.asarray(m).astype(np.float64) / np.asarray(q).astype(np.float64)).astype(np.float32)


def positions(cl, shape, seed_cut=0, charge_cut=0):
    """Everything of the contract of ``ieagan_pxd_cluster_positions`` for the clusters ``cl`` of an ``[N, H, W]`` batch: ``mu`` / ``mv`` of
    every cluster, and for the accepted ones ``cluster`` (row of the table), ``u``, ``v``; ``counts [N]``, ``total``."""
    N, H, W = shape
    mu, mv = moments(cl, shape)
    ok = (cl["seed"].astype(np.int64) >= seed_cut) & (cl["charge"].astype(np.int64) >= charge_cut)
    cluster = np.nonzero(ok)[0].astype(np.int32)
    q = cl["charge"][cluster]
    image = cl["first"][cluster].astype(np.int64) // (H * W)
    return dict(mu=mu, mv=mv, cluster=cluster, u=float_recipe(mu[cluster], q), v=float_recipe(mv[cluster], q),
                counts=np.bincount(image, minlength=N).astype(np.int32), total=int(cluster.size))


def bins(mu, mv, charge, H, W):
    """The integer bin rule: ``(bu, bv)`` = ``(floor(u / H * 25), floor(v / W * 48))`` without a float."""
    mu, mv, q = (np.asarray(a, np.int64) for a in (mu, mv, charge))
    return (mu * MAP_U) // (q * H), (mv * MAP_V) // (q * W)


def maps(cl, pos, shape, n_sensors):
    """The tables of ``utils.PXDClusterMaps`` for one batch: int64 ``count_map`` / ``charge_map [S, 25, 48]``, ``u_profile [S, 25]``,
    ``v_profile [S, 48]`` and ``clusters [events, S]`` (accepted per image)."""
    N, H, W = shape
    j = pos["cluster"]
    q = cl["charge"][j].astype(np.int64)
    bu, bv = bins(pos["mu"][j], pos["mv"][j], q, H, W)
    assert j.size == 0 or (bu.min() >= 0 and bu.max() < MAP_U and bv.min() >= 0 and bv.max() < MAP_V)
    sensor = cl["first"][j].astype(np.int64) // (H * W) % n_sensors
    count, charge = np.zeros((n_sensors, MAP_U, MAP_V), np.int64), np.zeros((n_sensors, MAP_U, MAP_V), np.int64)
    np.add.at(count, (sensor, bu, bv), 1)
    np.add.at(charge, (sensor, bu, bv), q)
    return dict(count_map=count, charge_map=charge, u_profile=count.sum(2), v_profile=count.sum(1),
                clusters=pos["counts"].reshape(-1, n_sensors).astype(np.int64))


def reco(images, threshold=0.0, seed_cut=0, charge_cut=0):
    """``(clusters, positions)`` of ``images`` ``[N, H, W]`` (fp32 or uint8, host)."""
    cl = CR.clusters(images, threshold)
    return cl, positions(cl, np.asarray(images).shape, seed_cut, charge_cut)


def dense_charge(cl, shape):
    """The uint8 charge image ``[N, H, W]`` that the digits of ``cl`` came from (for ``scipy.ndimage.center_of_mass``)."""
    q = np.zeros(int(np.prod(shape)), np.uint8)
    q[cl["index"].astype(np.int64)] = cl["digit_charge"]
    return q.reshape(shape)
