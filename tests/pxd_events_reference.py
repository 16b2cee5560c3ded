"""NumPy restatement of the sparse event store, the checker of ``utils.PXDEventStore`` (tests only): the columns of an event file
(``event_offsets``, ``sensor``, ``ucell``, ``vcell``, ``charge``) and a list of event numbers -> the dense uint8 images ``[E * S, H, W]`` of
those events; its inverse through ``pxd_digits_reference.digits``; and the events the tests plant their digit patterns in.

An event number outside ``[0, events)`` is an empty event (what the kernel does with a device id it cannot check on the host)."""
import numpy as np

import pxd_digits_reference as DR


def dense(columns, event_ids, shape, n_sensors):
    """uint8 ``[E * S, H, W]``: image ``e * S + s`` is sensor ``s`` of event ``event_ids[e]``."""
    off, sensor, ucell, vcell, charge = (np.asarray(c) for c in columns)
    H, W = shape
    ids = np.asarray(event_ids, np.int64).reshape(-1)
    out = np.zeros((ids.size * n_sensors, H, W), np.uint8)
    for e, i in enumerate(ids):
        if 0 <= i < off.size - 1:
            s = slice(int(off[i]), int(off[i + 1]))
            out[e * n_sensors + sensor[s].astype(np.int64), ucell[s].astype(np.int64), vcell[s].astype(np.int64)] = charge[s]
    return out


def columns(events, n_sensors):
    """Dense uint8 events (a list of ``[S, H, W]`` arrays) -> the columns of their event file, through the restatement of the reference's
    digit extraction: digits in ascending (sensor, ucell, vcell), every nonzero charge."""
    S = n_sensors
    off, sensor, ucell, vcell, charge = [0], [], [], [], []
    for ev in events:
        assert ev.dtype == np.uint8 and ev.shape[0] == S
        index, chg, _, total = DR.digits(ev, 0.0)
        index = index.numpy().astype(np.int64)
        _, H, W = ev.shape
        sensor.append(index // (H * W))
        ucell.append(index % (H * W) // W)
        vcell.append(index % W)
        charge.append(chg.numpy())
        off.append(off[-1] + total)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.asarray(off, np.int64), cat(sensor, np.uint8), cat(ucell, np.uint8 if events[0].shape[1] <= 256 else np.uint16), \
        cat(vcell, np.uint16), cat(charge, np.uint8)


def pattern_event(kind, S, H, W, seed):
    """One dense uint8 event ``[S, H, W]`` with a planted pattern:
    ``empty``       no digit;
    ``random``      30 % of the pixels are digits, charges 1 .. 255;
    ``sparse``      1 % occupancy;
    ``one_sensor``  every digit sits in one sensor (the last but one), the other images are empty;
    ``edges``       sparse, plus a digit on the first and on the last pixel of every image and, where an image has them, on pixels 4095 and
                    4096 (either side of a 4096-pixel tile boundary);
    ``full``        image 0: every pixel is a digit, charges 1 and 255 alternating; the other images sparse."""
    rng = np.random.Generator(np.random.PCG64([seed, 17]))
    ev = np.zeros((S, H, W), np.uint8)
    rand = lambda p: np.where(rng.random((S, H, W)) < p, rng.integers(1, 256, (S, H, W)), 0).astype(np.uint8)
    if kind == "empty":
        return ev
    if kind == "random":
        return rand(0.3)
    if kind == "sparse":
        return rand(0.01)
    if kind == "one_sensor":
        ev[max(S - 2, 0)] = rand(0.3)[0]
        return ev
    if kind == "edges":
        ev = rand(0.01)
        flat = ev.reshape(S, -1)
        flat[:, 0], flat[:, -1] = 200, 3
        if H * W > 4096:
            flat[:, 4095], flat[:, 4096] = 77, 78
        return ev
    if kind == "full":
        ev = rand(0.01)
        ev[0] = np.where(np.arange(H * W).reshape(H, W) % 2 == 0, 1, 255).astype(np.uint8)
        return ev
    raise ValueError(kind)


def pattern_events(kinds, S, H, W, seed=0):
    return [pattern_event(k, S, H, W, seed + 101 * i) for i, k in enumerate(kinds)]
