"""NumPy / Python union-find over the digit list, the checker of ``utils.pxd_clusters`` and ``utils.PXDClusterStatistics`` (tests only).

Input is the digit list of ``pxd_digits_reference.digits``: flat index ``n*H*W + r*W + c`` ascending, uint8 charge.  Two digits are
neighbours iff they lie in the same image and ``|dr| <= 1 and |dc| <= 1``; a cluster is a connected component; clusters are numbered by
the flat index of their first digit -- the raster numbering of ``scipy.ndimage.label(img > 0, structure=ones((3, 3)))`` per image with a
running offset (``tests/test_pxd_clusters.py`` pins that).  Every quantity is an integer.
"""
import functools

import numpy as np

import pxd_digits_reference as DR
import pxd_reference as R

SIZE_BINS, CHARGE_BINS, SEED_BINS, EXTENT_BINS = 64, 256, 256, 32


def size_bin(size):
    return np.minimum(np.asarray(size, np.int64), SIZE_BINS) - 1


def charge_bin(charge):
    return np.minimum(np.asarray(charge, np.int64) >> 3, CHARGE_BINS - 1)


def extent_bin(s):
    return np.minimum(np.asarray(s, np.int64), EXTENT_BINS) - 1


def clusters_of_digits(index, charge, shape):
    """Everything of the contract for the digit list ``(index, charge)`` of an ``[N, H, W]`` batch: dict of ``label [digits]``, ``first``,
    ``size``, ``charge``, ``seed``, ``size_u``, ``size_v`` ``[clusters]``, ``counts [N]``, ``total``."""
    N, H, W = shape
    index = np.asarray(index, np.int64)
    charge = np.asarray(charge, np.int64)
    M = index.size
    rem = index % (H * W)
    r, c = rem // W, rem % W
    parent = list(range(M))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    # the four neighbours that precede a digit in flat order: (dr, dc) = (0, -1), (-1, -1), (-1, 0), (-1, 1)
    for dr, dc in ((0, -1), (-1, -1), (-1, 0), (-1, 1)):
        ok = (r + dr >= 0) & (c + dc >= 0) & (c + dc < W)
        target = index + dr * W + dc
        j = np.searchsorted(index, target)
        ok &= j < M
        ok[ok] = index[j[ok]] == target[ok]
        for a, b in zip(np.nonzero(ok)[0].tolist(), j[ok].tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:                                    # the smaller root wins: the root of a set is its first digit
                parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(k) for k in range(M)], np.int64)
    roots = np.unique(root)                                 # ascending first digit = cluster number
    label = np.searchsorted(roots, root)
    T = roots.size
    size = np.bincount(label, minlength=T)
    csum = np.bincount(label, weights=charge, minlength=T).astype(np.int64)
    seed = np.zeros(T, np.int64)
    np.maximum.at(seed, label, charge)
    lo_r, lo_c = np.full(T, H, np.int64), np.full(T, W, np.int64)
    hi_r, hi_c = np.full(T, -1, np.int64), np.full(T, -1, np.int64)
    np.minimum.at(lo_r, label, r)
    np.maximum.at(hi_r, label, r)
    np.minimum.at(lo_c, label, c)
    np.maximum.at(hi_c, label, c)
    first = index[roots]
    return dict(label=label.astype(np.int32), first=first.astype(np.int32), size=size.astype(np.int32), charge=csum.astype(np.int32),
                seed=seed.astype(np.uint8), size_u=(hi_r - lo_r + 1).astype(np.int32), size_v=(hi_c - lo_c + 1).astype(np.int32),
                counts=np.bincount(first // (H * W), minlength=N).astype(np.int32), total=int(T),
                index=index.astype(np.int32), digit_charge=charge.astype(np.uint8))


def clusters(images, threshold=0.0):
    """``clusters_of_digits`` of the digits of ``images`` ``[N, H, W]`` (fp32 or uint8, host) at ``threshold``."""
    images = np.asarray(images)
    index, charge, _, _ = DR.digits(images, threshold)
    return clusters_of_digits(index.numpy(), charge.numpy(), images.shape)


def spectra(cl, shape, n_sensors):
    """The tables of ``utils.PXDClusterStatistics`` for one batch: int64 ``size_spectrum [S, 64]``, ``charge_spectrum [S, 256]``,
    ``seed_spectrum [S, 256]``, ``size_u_spectrum`` / ``size_v_spectrum [S, 32]`` and ``clusters [events, S]``."""
    N, H, W = shape
    sensor = cl["first"].astype(np.int64) // (H * W) % n_sensors

    def table(bins, n):
        t = np.zeros((n_sensors, n), np.int64)
        np.add.at(t, (sensor, bins), 1)
        return t

    return dict(size_spectrum=table(size_bin(cl["size"]), SIZE_BINS), charge_spectrum=table(charge_bin(cl["charge"]), CHARGE_BINS),
                seed_spectrum=table(cl["seed"].astype(np.int64), SEED_BINS), size_u_spectrum=table(extent_bin(cl["size_u"]), EXTENT_BINS),
                size_v_spectrum=table(extent_bin(cl["size_v"]), EXTENT_BINS), clusters=cl["counts"].reshape(-1, n_sensors).astype(np.int64))


def scipy_labels(images, threshold=0.0):
    """Per-digit cluster numbers from ``scipy.ndimage.label`` with ``ones((3, 3))`` per image and a running offset (needs scipy)."""
    from scipy import ndimage
    images = np.asarray(images)
    N, H, W = images.shape
    index, _, _, _ = DR.digits(images, threshold)
    mask = np.zeros(N * H * W, bool)
    mask[index.numpy().astype(np.int64)] = True
    mask = mask.reshape(N, H, W)
    out, offset = [], 0
    for n in range(N):
        lab, cnt = ndimage.label(mask[n], structure=np.ones((3, 3)))
        out.append(lab[mask[n]].astype(np.int64) - 1 + offset)
        offset += cnt
    return np.concatenate(out) if out else np.zeros(0, np.int64), offset


def _snake(h, w):
    """One-pixel-wide serpentine over the rows 0 .. R: the even rows full, the odd rows one pixel, alternately at the right and left end."""
    R_ = min(h - 1, 40) // 2 * 2
    px = []
    for r in range(R_ + 1):
        if r % 2 == 0:
            px += [(r, c) for c in range(w)]
        else:
            px.append((r, w - 1 if (r // 2) % 2 == 0 else 0))
    return px


def _spiral(h, w):
    """Square spiral from (0, 0) inwards, one pixel wide, one empty pixel between successive turns."""
    L = min(h, w, 41) - 1
    r = c = 0
    px = [(0, 0)]
    step, d = L, 0
    moves = ((0, 1), (1, 0), (0, -1), (-1, 0))
    legs = 0
    while step > 0:
        for _ in range(step):
            r, c = r + moves[d][0], c + moves[d][1]
            px.append((r, c))
        d = (d + 1) % 4
        legs += 1
        if legs == 3 or (legs > 3 and (legs - 3) % 2 == 0):
            step -= 2
    return px


def structured_event(n, h, w, seed, kind="f32"):
    """``(images [n, h, w], plants)``: the sparse random background of ``pxd_reference.synthetic_*`` (about 1 % occupancy, edge values
    planted) with shapes planted on it (needs n >= 4, h >= 24, w >= 48).  Everything within one pixel of a planted shape is cleared
    first, so a shape is one cluster of exactly its own pixels.  ``plants``: name -> ``(flat index of one pixel, pixel count)``; pairs
    that must NOT be joined are named ``*_a`` / ``*_b``.
      image 0   serpentine snake over the top rows;      image 1   a spiral
      image 2   a U of two 3-wide arms that join in the last row only, a pure diagonal chain whose middle pixel holds 6.9 ADU (a digit
                of charge 6 at threshold 0, none at threshold 7: the chain splits), the last pixel, and (h-1, w/2)
      image 3   a 2 x 2 block in every corner (so its first pixel follows the last pixel of image 2), (0, w/2) below image 2's (h-1, w/2),
                and the pair (h/2, w-1), (h/2+1, 0): adjacent in flat index, no neighbours.
      the last image gets the four corner blocks as well."""
    assert n >= 4 and h >= 24 and w >= 48
    ev = (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(n, h, w, seed).copy()
    rng = np.random.Generator(np.random.PCG64([seed, 17]))
    plants = {}
    shapes = {i: [] for i in range(n)}

    def add(img, name, px, value=None):
        shapes[img].append((px, value))
        r0, c0 = px[0]
        plants[name] = (img * h * w + r0 * w + c0, len(set(px)))

    add(0, "snake", _snake(h, w))
    add(1, "spiral", _spiral(h, w))
    u = [(r, c) for r in range(h) for c in (2, 3, 4, 10, 11, 12)] + [(h - 1, c) for c in range(5, 10)]
    add(2, "u", u)
    L = min(h - 2, w - 24)
    add(2, "diagonal", [(i, 20 + i) for i in range(L)])
    add(2, "diagonal_cut", [(L // 2, 20 + L // 2)], 6.9)
    add(2, "image_a", [(h - 1, w - 1)])
    add(2, "column_a", [(h - 1, w // 2)])
    corners = lambda: [[(0, 0), (0, 1), (1, 0), (1, 1)], [(0, w - 2), (0, w - 1), (1, w - 2), (1, w - 1)],
                       [(h - 2, 0), (h - 2, 1), (h - 1, 0), (h - 1, 1)], [(h - 2, w - 2), (h - 2, w - 1), (h - 1, w - 2), (h - 1, w - 1)]]
    for img in sorted({3, n - 1}):
        for k, px in enumerate(corners()):
            add(img, f"corner{k}_{img}", px)
    plants["image_b"] = plants["corner0_3"]
    add(3, "column_b", [(0, w // 2)])
    add(3, "wrap_a", [(h // 2, w - 1)])
    add(3, "wrap_b", [(h // 2 + 1, 0)])
    for img, items in shapes.items():
        for px, _ in items:
            for r, c in px:
                ev[img, max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = 0
        for px, value in items:
            for r, c in px:
                v = rng.uniform(8, 255) if value is None else value
                ev[img, r, c] = np.uint8(v) if kind == "u8" else np.float32(v)
    ev[0, 0, 0] = 255                   # the snake's seed
    return ev, plants


@functools.lru_cache(maxsize=None)
def cached_structured(n, h, w, seed, kind):
    return structured_event(n, h, w, seed, kind)        # shared by the tests: read, never written
