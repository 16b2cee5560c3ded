"""NumPy restatement of the background overlay, the checker of ``utils.pxd_overlay`` (tests only), in two independent forms, and the pairs of
events the tests plant their patterns in.

Columns are those of an event file (``event_offsets``, ``sensor``, ``ucell``, ``vcell``, ``charge``: ``pxd_events_reference``).  Output event
``e`` is event ``ids_a[e]`` of ``A`` with event ``ids_b[e]`` of ``B`` laid over it: every pixel that is a digit in either, a pixel of both with
``min(qa + qb, 255)``.  An event number outside its columns is an empty event.

``dense``   the dense uint8 images of both sides, added in int32 and clipped, and the digit restatement of the sum;
``sparse``  per pair ``np.union1d`` of the positions and ``np.add.at`` of the charges, clipped -- no image."""
import numpy as np

import pxd_events_reference as ER


def dense_sum(A, ids_a, B, ids_b, shape, n_sensors):
    """uint8 ``[E * S, H, W]``: the clamped sum of the dense images of both sides."""
    return np.minimum(ER.dense(A, ids_a, shape, n_sensors).astype(np.int32) + ER.dense(B, ids_b, shape, n_sensors), 255).astype(np.uint8)


def dense(A, ids_a, B, ids_b, shape, n_sensors):
    total = dense_sum(A, ids_a, B, ids_b, shape, n_sensors)
    return ER.columns(list(total.reshape(-1, n_sensors, *shape)), n_sensors)


def _event(cols, i, shape):
    """``(pos, charge)`` int64 of event ``i``; empty when ``i`` is outside the columns."""
    off, sensor, ucell, vcell, charge = (np.asarray(c) for c in cols)
    if not 0 <= i < off.size - 1:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    s = slice(int(off[i]), int(off[i + 1]))
    return (sensor[s].astype(np.int64) * shape[0] + ucell[s]) * shape[1] + vcell[s], charge[s].astype(np.int64)


def sparse(A, ids_a, B, ids_b, shape, n_sensors):
    H, W = shape
    off, pos, charge = [0], [], []
    for ia, ib in zip(np.asarray(ids_a, np.int64).reshape(-1), np.asarray(ids_b, np.int64).reshape(-1)):
        (pa, qa), (pb, qb) = _event(A, ia, shape), _event(B, ib, shape)
        p = np.union1d(pa, pb)
        q = np.zeros(p.size, np.int64)
        np.add.at(q, np.searchsorted(p, pa), qa)
        np.add.at(q, np.searchsorted(p, pb), qb)
        pos.append(p)
        charge.append(np.minimum(q, 255))
        off.append(off[-1] + p.size)
    pos, charge = np.concatenate(pos).astype(np.int64), np.concatenate(charge)
    return np.asarray(off, np.int64), (pos // (H * W)).astype(np.uint8), (pos % (H * W) // W).astype(np.uint8 if H <= 256 else np.uint16), \
        (pos % W).astype(np.uint16), charge.astype(np.uint8)


def shared(A, ids_a, B, ids_b, shape):
    """int64 ``[E]``: the pixels of every pair that are a digit on both sides."""
    return np.asarray([np.intersect1d(_event(A, ia, shape)[0], _event(B, ib, shape)[0]).size
                       for ia, ib in zip(np.asarray(ids_a).reshape(-1), np.asarray(ids_b).reshape(-1))], np.int64)


def same(got, want):
    """Two sets of columns hold the same events."""
    return len(got) == len(want) == 5 and all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))


def planted(S, H, W, seed=0):
    """``(events_a, events_b, pairs)``: two lists of dense uint8 events ``[S, H, W]`` and the pairs ``(event of a, event of b)`` that hold
    the planted patterns (needs ``S >= 2`` and ``H * W > 64``):
     0  empty + empty                      1  empty + random                     2  random + empty
     3  random + the same event: every digit a duplicate, saturation from q >= 128
     4  random + an independent random: 30 % each, about 9 % coincidences, interleaved
     5  full + full: every pixel of image 0 a duplicate with the sums 1 + 1, 255 + 1 = 256, 1 + 254 = 255 and 255 + 255
     6  sparse + edges (digits on the first and last pixel of every image)
     7  one_sensor + sparse
     8  the last pixel of sensor 0 + the first pixel of sensor 1: neighbours in the merged order, no coincidence
     9  the even pixels of sensor 0 + the odd ones: every item of the merged order comes from the other list than the one before
    10  the odd pixels + the even ones and pixel 63: one coincidence, at the merged indices 63 and 64 (either side of a step of 64)"""
    HW = H * W
    assert S >= 2 and HW > 64
    zeros = lambda: np.zeros((S, H, W), np.uint8)
    rng = np.random.Generator(np.random.PCG64([seed, 23]))
    full_b = ER.pattern_event("full", S, H, W, seed + 7)
    full_b[0] = np.array([1, 1, 254, 255], np.uint8)[np.arange(HW) % 4].reshape(H, W)
    last, first, even, odd, even63 = zeros(), zeros(), zeros(), zeros(), zeros()
    last.reshape(S, -1)[0, -1], last.reshape(S, -1)[1, 5] = 200, 9
    first.reshape(S, -1)[1, 0], first.reshape(S, -1)[0, 3] = 100, 8
    even.reshape(S, -1)[0, 0::2] = rng.integers(1, 256, (HW + 1) // 2)
    odd.reshape(S, -1)[0, 1::2] = rng.integers(1, 256, HW // 2)
    even63[:] = even
    even63.reshape(S, -1)[0, 63] = 250
    random = ER.pattern_event("random", S, H, W, seed + 1)
    a = [zeros(), random, ER.pattern_event("full", S, H, W, seed + 2), ER.pattern_event("sparse", S, H, W, seed + 3),
         ER.pattern_event("one_sensor", S, H, W, seed + 4), last, even, odd]
    b = [zeros(), ER.pattern_event("random", S, H, W, seed + 5), random, full_b, ER.pattern_event("edges", S, H, W, seed + 6),
         ER.pattern_event("sparse", S, H, W, seed + 8), first, odd, even63]
    pairs = [(0, 0), (0, 1), (1, 0), (1, 2), (1, 1), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8)]
    return a, b, pairs
