"""NumPy restatement of the signal-hit matching, the checker of ``utils.pxd_match`` and ``utils.PXDMatchStatistics`` (tests only), on top of
the cluster, reconstruction and hit checkers (``pxd_clusters_reference``, ``pxd_reco_reference``, ``pxd_hits_reference``) and the planted
overlay pairs of ``pxd_overlay_reference``.

The rule, in integers.  Two reconstructions over batches of the same ``[N, H, W]``: *signal* and *mixed*.  A signal digit is *found* when its
flat index occurs in the mixed digit list; ``L`` is then the mixed label of that digit.

  per signal cluster j   ``found`` = its found digits; ``lo`` / ``hi`` = smallest / largest ``L`` over them, -1 / -1 when ``found == 0``;
                         ``lo`` is the match
  per mixed cluster k    ``signal_size`` / ``signal_charge`` = number and summed SIGNAL charge of the signal digits found in it;
                         ``n_signal`` = the signal clusters with ``lo == k``
  per signal hit h       (accepted signal cluster j) ``mixed_hit`` = row of the mixed hit whose cluster is ``lo[j]``, or -1; ``flags``: bit 0
                         MATCHED (``found == size``, ``lo == hi >= 0``, that mixed cluster is itself a hit), bit 1 CHANGED (MATCHED and
                         the mixed size or charge differs), bit 2 SHARED (``n_signal[lo] >= 2``); ``du`` / ``dv`` =
                         ``float32(float64(x_mixed) - float64(x_signal))``, 0 when not MATCHED

The per-cluster part comes in two independent forms that must agree:
``dense``   a mixed label image ``[N * H * W]`` (-1: no digit) looked up at the signal pixels, then one pass per signal cluster and per mixed
            cluster in plain Python;
``sparse``  ``np.searchsorted`` of the signal indices in the mixed index list, then ``np.bincount`` / ``np.minimum.at`` / ``np.maximum.at``.

Statistics per sensor of the signal hit, int64 ``[S, 165]``: ``hits``, ``matched``, ``changed``, ``shared`` (MATCHED and SHARED), ``lost``
(not MATCHED); residual u and v (64 bins each) over the MATCHED and CHANGED hits, ``bin = clip(floor(r / w) + 32, 0, 63)`` with ``r`` the
float64 difference and ``w`` the integer bin width; purity (32 bins) over the MATCHED hits, ``min(32 * signal_charge // mixed_charge, 31)``."""
import functools

import numpy as np

import pxd_clusters_reference as CR
import pxd_hits_reference as HR
import pxd_overlay_reference as OR
import pxd_reference as R

MATCHED, CHANGED, SHARED = 1, 2, 4
COUNTERS = ("hits", "matched", "changed", "shared", "lost")
RES_BINS, PURITY_BINS, COLUMNS = 64, 32, 165
RES_U, RES_V, PURITY = 5, 69, 133
PER_CLUSTER = ("found", "lo", "hi", "signal_size", "signal_charge", "n_signal")


def dense(cs, cm, shape):
    """The per-cluster tables from a mixed label image; ``cs`` / ``cm`` are ``clusters_of_digits`` dicts of the signal and the mixed batch."""
    N, H, W = shape
    image = np.full(N * H * W, -1, np.int64)
    image[cm["index"].astype(np.int64)] = cm["label"]
    L = image[cs["index"].astype(np.int64)]
    Ts, Tm = cs["total"], cm["total"]
    found, lo, hi = np.zeros(Ts, np.int64), np.full(Ts, -1, np.int64), np.full(Ts, -1, np.int64)
    size, charge, n_signal = np.zeros(Tm, np.int64), np.zeros(Tm, np.int64), np.zeros(Tm, np.int64)
    members = [[] for _ in range(Ts)]
    for lab, l, q in zip(cs["label"].tolist(), L.tolist(), cs["digit_charge"].tolist()):
        if l >= 0:
            members[lab].append(l)
            size[l] += 1
            charge[l] += q
    for j, ls in enumerate(members):
        if ls:
            found[j], lo[j], hi[j] = len(ls), min(ls), max(ls)
            n_signal[lo[j]] += 1
    return dict(found=found, lo=lo, hi=hi, signal_size=size, signal_charge=charge, n_signal=n_signal)


def sparse(cs, cm, shape=None):
    """The same tables from the two sorted index lists, without an image."""
    si, mi = cs["index"].astype(np.int64), cm["index"].astype(np.int64)
    Ts, Tm = cs["total"], cm["total"]
    p = np.searchsorted(mi, si)
    ok = p < mi.size
    ok[ok] = mi[p[ok]] == si[ok]
    lab, L, q = cs["label"].astype(np.int64)[ok], cm["label"].astype(np.int64)[p[ok]], cs["digit_charge"].astype(np.int64)[ok]
    found = np.bincount(lab, minlength=Ts).astype(np.int64)
    lo, hi = np.full(Ts, np.iinfo(np.int64).max, np.int64), np.full(Ts, -1, np.int64)
    np.minimum.at(lo, lab, L)
    np.maximum.at(hi, lab, L)
    lo[found == 0] = -1
    return dict(found=found, lo=lo, hi=hi, signal_size=np.bincount(L, minlength=Tm).astype(np.int64),
                signal_charge=np.bincount(L, weights=q, minlength=Tm).astype(np.int64),
                n_signal=np.bincount(lo[lo >= 0], minlength=Tm).astype(np.int64))


def same_tables(a, b):
    return all(np.array_equal(a[k], b[k]) for k in PER_CLUSTER)


def per_hit(pc, cs, ps, hs, cm, pm, hm, shape, n_sensors):
    """The per-hit columns from the per-cluster tables ``pc``; ``c*`` clusters, ``p*`` positions (``pxd_reco_reference.positions``), ``h*``
    hits (``pxd_hits_reference.hits``) of the signal (``s``) and the mixed (``m``) batch."""
    N, H, W = shape
    j = ps["cluster"].astype(np.int64)
    inv = np.full(cm["total"], -1, np.int64)
    inv[pm["cluster"].astype(np.int64)] = np.arange(pm["cluster"].size)
    lo, hi, found = pc["lo"][j], pc["hi"][j], pc["found"][j]
    k = np.maximum(lo, 0)
    of = lambda a: np.where(lo >= 0, np.asarray(a, np.int64)[k], 0) if cm["total"] else np.zeros(j.size, np.int64)
    mh = np.where(lo >= 0, inv[k], -1) if cm["total"] else np.full(j.size, -1, np.int64)
    size, charge = cs["size"].astype(np.int64)[j], cs["charge"].astype(np.int64)[j]
    matched = (found == size) & (lo == hi) & (lo >= 0) & (mh >= 0)
    changed = matched & ((of(cm["size"]) != size) | (of(cm["charge"]) != charge))
    shared = (lo >= 0) & (of(pc["n_signal"]) >= 2)
    m = np.maximum(mh, 0)
    diff = lambda key: (np.asarray(hm[key])[m].astype(np.float64) - np.asarray(hs[key]).astype(np.float64)) if mh.size and hm["total"] \
        else np.zeros(j.size, np.float64)
    ru, rv = diff("u"), diff("v")                                # float64, of every hit; meaningful where matched
    image = cs["first"].astype(np.int64)[j] // (H * W)
    return dict(cluster=j.astype(np.int32), sensor=(image % n_sensors).astype(np.int32), event=(image // n_sensors).astype(np.int32),
                mixed_hit=mh.astype(np.int32), flags=(matched * MATCHED + changed * CHANGED + shared * SHARED).astype(np.uint8),
                du=np.where(matched, ru, 0.0).astype(np.float32), dv=np.where(matched, rv, 0.0).astype(np.float32), ru=ru, rv=rv,
                found=found.astype(np.int32), size=size.astype(np.int32), charge=charge.astype(np.int32), match=lo.astype(np.int32),
                hi=hi.astype(np.int32), mixed_charge=of(cm["charge"]).astype(np.int32), signal_charge=of(pc["signal_charge"]).astype(np.int32),
                signal_size=of(pc["signal_size"]).astype(np.int32), n_signal=of(pc["n_signal"]).astype(np.int32),
                counts=ps["counts"].astype(np.int32), matched=matched, changed=changed, shared=shared)


def residual_bin(r, w):
    """``clip(floor(r / w) + 32, 0, 63)``: one float64 division, a floor, the clamp before the conversion."""
    return np.clip(np.floor(np.asarray(r, np.float64) / np.float64(w)) + 32.0, 0.0, 63.0).astype(np.int64)


def purity_bin(signal_charge, mixed_charge):
    return np.minimum(PURITY_BINS * np.asarray(signal_charge, np.int64) // np.asarray(mixed_charge, np.int64), PURITY_BINS - 1)


def tables(ph, n_sensors, w=10):
    """int64 ``[S, 165]`` of one batch from its ``per_hit`` dict."""
    t = np.zeros((n_sensors, COLUMNS), np.int64)
    s, m, mc = ph["sensor"].astype(np.int64), ph["matched"], ph["matched"] & ph["changed"]
    np.add.at(t, (s, 0), 1)
    np.add.at(t, (s[m], 1), 1)
    np.add.at(t, (s[mc], 2), 1)
    np.add.at(t, (s[m & ph["shared"]], 3), 1)
    np.add.at(t, (s[~m], 4), 1)
    np.add.at(t, (s[mc], RES_U + residual_bin(ph["ru"][mc], w)), 1)
    np.add.at(t, (s[mc], RES_V + residual_bin(ph["rv"][mc], w)), 1)
    np.add.at(t, (s[m], PURITY + purity_bin(ph["signal_charge"][m], ph["mixed_charge"][m])), 1)
    return t


def match(signal, mixed, geometry, head_tail=3, threshold=0.0, seed_cut=0, charge_cut=0, n_sensors=None, form=sparse):
    """Everything for two batches of images ``[N, H, W]`` (host): ``dict(cs, ps, hs, cm, pm, hm, clusters, hits)``."""
    shape = np.asarray(signal).shape
    S = len(geometry[2]) if n_sensors is None else n_sensors
    cs, ps, hs = HR.reco_hits(signal, geometry, head_tail, threshold, seed_cut, charge_cut)
    cm, pm, hm = HR.reco_hits(mixed, geometry, head_tail, threshold, seed_cut, charge_cut)
    pc = form(cs, cm, shape)
    return dict(cs=cs, ps=ps, hs=hs, cm=cm, pm=pm, hm=hm, clusters=pc, hits=per_hit(pc, cs, ps, hs, cm, pm, hm, shape, S), shape=shape)


def overlay(signal, background):
    """The saturating sum of two uint8 batches."""
    return np.minimum(signal.astype(np.int32) + background, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def planted_case(S, H, W):
    """The planted overlay pairs of ``pxd_overlay_reference.planted`` as one batch: ``(signal [11 * S, H, W], background, mixed)`` uint8,
    event e = pair e.  Shared by the tests: read, never written."""
    a, b, pairs = OR.planted(S, H, W, seed=S)
    signal, background = np.concatenate([a[i] for i, _ in pairs]), np.concatenate([b[j] for _, j in pairs])
    return signal, background, overlay(signal, background)


@functools.lru_cache(maxsize=None)
def structured_case(n, h, w, seed):
    """The snake / spiral / U / diagonal events of ``pxd_clusters_reference.cached_structured`` (uint8) under an independent sparse random
    background of about 1 % occupancy: ``(signal, background, mixed)``."""
    signal, _ = CR.cached_structured(n, h, w, seed, "u8")
    background = R.synthetic_u8(n, h, w, seed + 1000)
    return signal, background, overlay(signal, background)


@functools.lru_cache(maxsize=None)
def cached_match(case, S, H, W, threshold=0.0, seed_cut=0, charge_cut=0, head_tail=3, unrelated=False):
    """``match`` of a case (``"planted"`` or ``"structured"``, N = 4 * S images then), with the two-type geometry split at ``W // 3``;
    ``unrelated``: the background itself stands in for the mixed batch (two unrelated events)."""
    signal, background, mixed = planted_case(S, H, W) if case == "planted" else structured_case(4 * S, H, W, 3)
    geometry = HR.two_type_geometry((H, W), W // 3, S)
    return match(signal, background if unrelated else mixed, geometry, head_tail, threshold, seed_cut, charge_cut)
