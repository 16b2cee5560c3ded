"""The PXD detector surface, this project's own (no counterpart in the reference's ``utils``): detector-level validation statistics
(csrc/pxd_stats.hip), event production as sparse digits (csrc/pxd_digits.hip), clusters of the digits and their spectra
(csrc/pxd_clusters.hip), cluster reconstruction -- cuts, charge-weighted positions, per-sensor position maps (csrc/pxd_reco.hip) --, hits in the local
frame of a sensor with a geometry given as data (csrc/pxd_hits.hip), the event and hit files of ``produce.py`` and the store that keeps such a file's events on the device and expands them into the network input
(csrc/pxd_events.hip), the overlay of the events of two stores, pixel by pixel in the sparse format (csrc/pxd_overlay.hip), the match of
the signal hits to the hits of the mixed events, hit by hit (csrc/pxd_match.hip), and the correlations between the region occupancies of one
event -- exact Pearson and Spearman tables from integer moments and ranks (csrc/pxd_corr.hip) --, and the hits in a global frame with the
inner / outer-layer hit doublets of an event (csrc/pxd_doublets.hip).  ``utils`` re-exports every name defined here."""
from __future__ import annotations

import numpy as np
import torch

import _hip as H


def _sensor_images(images, n_sensors, who, device=None):
    """What every entry point does with its input: ``[N, H, W]`` (or ``[N, 1, H, W]``) fp32 or uint8 sensor images, whole events of
    ``n_sensors``, as a contiguous tensor on ``device`` (default: the images' own GPU, the current one for host images)."""
    H.require_gpu()
    if images.dim() == 4 and images.shape[1] == 1:
        images = images[:, 0]
    if images.dim() != 3 or images.dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"{who} expects fp32 or uint8 sensor images [N, H, W] in detector units")
    if images.shape[0] == 0 or images.shape[0] % n_sensors:
        raise ValueError(f"{who}: {images.shape[0]} images are not whole events of {n_sensors} sensors")
    if device is None:
        device = images.device if images.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return images.to(device, non_blocking=True).contiguous()


def _ptrs(capacity, *tensors):
    """Device pointers of ``tensors`` for a launcher; None each when the capacity is 0 (nothing is written then, NULL is accepted)."""
    return [t.data_ptr() if capacity else None for t in tensors]


def _header(N, device):
    """The int32 header ``[N + 1]`` every launch of the chain fills -- ``counts [N]``, then ``total [1]`` -- and its two device pointers."""
    header = torch.empty(N + 1, dtype=torch.int32, device=device)
    return header, header.data_ptr(), header.data_ptr() + 4 * N


def pxd_read_back(**tensors):
    """One packed read-back: the named tensors (any dtypes, shapes and lengths, empty ones included) as bytes in one tensor on their
    device, one copy to the host, one wait -> dict of NumPy arrays by name, each in its tensor's dtype and shape, bit for bit.  The widest
    elements are packed first, so every column starts at a multiple of its element size; each array is a copy that owns its memory."""
    order = sorted(tensors.items(), key=lambda kt: -kt[1].element_size())
    host = torch.cat([t.contiguous().reshape(-1).view(torch.uint8) for _, t in order]).cpu()      # the one device-to-host copy
    parts = host.split([t.numel() * t.element_size() for _, t in order])
    return {k: p.view(t.dtype).numpy().reshape(tuple(t.shape)).copy() for (k, t), p in zip(order, parts)}


class _PXDProduct:
    """What the device-side results of the chain (digits -> clusters -> positions) share: the ``counts`` / ``total`` views of their header
    and the rule that the host never sees a truncated event.  A subclass says how the chain is run again (``_again(capacity)``)."""

    def _set_header(self, header, source=None):
        if source is not None:          # the product before this one: its images, geometry, capacity and threshold hold
            vars(self).update((k, getattr(source, k)) for k in ("images", "capacity", "n_sensors", "shape", "threshold"))
        self.header, self.counts, self.total = header, header[:self.shape[0]], header[self.shape[0]:]

    def _grow(self, total):
        """The digit total exceeds the capacity: the chain is run again with ``capacity = total`` and its result adopted."""
        vars(self).update((k, v) for k, v in vars(self._again(total)).items() if not k.startswith("_"))

    def _host_columns(self, columns):
        """``pxd_read_back`` of the tensors ``columns()``, ``digit_header`` among them; after ``_grow`` if need be (a second read-back then)."""
        host = pxd_read_back(**columns())
        if host["digit_header"][-1] > self.capacity:
            self._grow(int(host["digit_header"][-1]))
            host = pxd_read_back(**columns())
        return host


class _PXDAccumulator:
    """What the three accumulators share: the fields, the ``update`` preamble (input, device, image size), the ``result`` preamble (one
    packed read-back, the overflow refusal) and the per-image tables ``[events, S]``.  A subclass names its device table (``_table``; with
    ``_overflow`` its last word counts the updates that held more digits than the capacity) and its per-image lists (``_per_image``)."""
    _table, _per_image, _overflow = "tables", ("clusters",), True

    def __init__(self, n_sensors=40, threshold=7.0, capacity=None, device=None):
        self.n_sensors, self.threshold, self.capacity = int(n_sensors), float(threshold), capacity if capacity is None else int(capacity)
        self.device = torch.device(device) if device is not None else None
        self.reset()

    def reset(self):
        vars(self).update({self._table: None, "shape": None}, **{k: [] for k in self._per_image})

    def _input(self, given, who, *products):
        """The ``update`` preamble.  Images: ``_sensor_images`` on the accumulator's device.  One of ``products`` (the results of the chain
        this accumulator would run itself): taken as it is, after a ``ValueError`` when it was not made the way the accumulator makes it."""
        me, product = type(self).__name__, isinstance(given, products)
        x = given if product else _sensor_images(given, self.n_sensors, who, self.device)
        device = x.header.device if product else x.device
        for k in ("n_sensors", "threshold", "seed_cut", "charge_cut", "regions", "device") if product else ():
            made, mine = (device.index, self.device and self.device.index) if k == "device" else (getattr(x, k, None), getattr(self, k, None))
            if made != mine and None not in (made, mine):
                raise ValueError(f"{me}.update: the {type(x).__name__} was made with {k} = {made}, not {mine}")
        self.device = self.device or device
        if self.shape not in (None, tuple(x.shape[1:])):
            raise ValueError(f"{me}.update: image size {tuple(x.shape[1:])} differs from the accumulated {self.shape}")
        self.shape = tuple(x.shape[1:])
        return x

    def _host_tables(self):
        """The ``result`` preamble -> ``(table, {name: per-image table [events, S]})`` on the host, the overflow word taken off."""
        who = type(self).__name__
        if not getattr(self, self._per_image[0]):
            raise RuntimeError(f"{who}.result() before any update()")
        host = pxd_read_back(table=getattr(self, self._table), **{k: torch.cat(getattr(self, k)) for k in self._per_image})
        table = host.pop("table")
        if self._overflow and table[-1] != 0:
            raise RuntimeError(f"{who}: {int(table[-1])} update(s) held more digits than the capacity"
                               f"{'' if self.capacity is None else ' of %d' % self.capacity}, their clusters are truncated: "
                               f"pass a larger capacity= to {who}")
        per_image = {k: v.reshape(-1, self.n_sensors) for k, v in host.items()}
        return table[:-1] if self._overflow else table, dict(per_image, n_events=host[self._per_image[0]].size // self.n_sensors)


def _rel_err(real, fake, ok):
    """Mean over the sensors ``ok`` of |fake - real| / real (a NaN of ``fake`` counts as 0); NaN when there is no such sensor."""
    r, f = np.asarray(real, np.float64), np.nan_to_num(np.asarray(fake, np.float64), nan=0.0)
    return float(np.mean(np.abs(f[ok] - r[ok]) / r[ok])) if ok.any() else float("nan")


def _w1(real_hist, fake_hist, width=1.0):
    """1-D Wasserstein distance between two spectra ``[S, bins]``, bins ``width`` wide, pooled over the sensors, normalised; NaN if one is empty."""
    hr = np.asarray(real_hist, np.float64).sum(0)
    hf = np.asarray(fake_hist, np.float64).sum(0)
    if hr.sum() > 0 and hf.sum() > 0:
        return float(np.abs(np.cumsum(hf / hf.sum()) - np.cumsum(hr / hr.sum())).sum() * width)
    return float("nan")

# ---------------------------------------------------------------------------------------------------------
# detector-level validation (reference Evaluation/eval_all.py:75-120): per-sensor occupancy, mean hit charge, ADC spectrum
# ---------------------------------------------------------------------------------------------------------
PXD_OCC_BINS = 200          # eval_all.py:78: bh.axis.Regular(200, 0, 0.02) over the per-image occupancy


def pxd_bin_edges():
    """The 252 edges of the 251 ADC-spectrum bins (eval_all.py:77): [-1, 1, 7, 8, 9, ..., 256]."""
    return np.concatenate([np.array([-1.0, 1.0, 7.0]), np.linspace(8, 256, 249)])


def pxd_bin_index(v):
    """The bin rule of ``ieagan_pxd_stats`` restated on the host: ``v < 1 -> 0; v < 7 -> 1; else 2 + min(floor(v) - 7, 248)``.
    Equals ``np.histogram(v, pxd_bin_edges())`` for every v in [-1, 256]."""
    v = np.asarray(v, dtype=np.float64)
    return np.where(v < 1, 0, np.where(v < 7, 1, 2 + np.minimum(np.floor(np.minimum(v, 255.0)) - 7, 248))).astype(np.int64)


class PXDStatistics(_PXDAccumulator):
    """Accumulator of the reference's per-event detector statistics (eval_all.py:75-101 ``get_stats``) over batches of sensor images in
    detector units, ``[N, H, W]`` fp32 (``Generator(..., export=True)``) or uint8 (event files); image ``n`` is sensor
    ``n % n_sensors``.  ``update`` is one HIP launch pair (csrc/pxd_stats.hip) on the current stream: it neither synchronises nor
    copies to the host; ``result()`` does the single read-back."""
    _table, _per_image, _overflow = "spectrum", ("hits", "charge"), False       # spectrum: int64 [S, 251], the kernel's 64-bit counters

    def __init__(self, n_sensors=40, threshold=7.0, device=None):
        super().__init__(n_sensors, threshold, None, device)

    def update(self, images):
        x = self._input(images, "PXDStatistics.update")
        N, Hh, Ww = x.shape
        if self.spectrum is None:
            self.spectrum = torch.zeros(self.n_sensors, H.PXD_BINS, dtype=torch.int64, device=self.device)
        hits = torch.empty(N, dtype=torch.int32, device=self.device)
        charge = torch.empty(N, dtype=torch.float32, device=self.device)
        scratch = torch.empty(H.lib().ieagan_pxd_stats_scratch(N, Hh, Ww), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            H.call("ieagan_pxd_stats", x.data_ptr(), int(x.dtype == torch.uint8), N, Hh, Ww, self.n_sensors, self.threshold,
                   self.spectrum.data_ptr(), hits.data_ptr(), charge.data_ptr(), scratch.data_ptr(), H.stream())
        self.hits.append(hits)
        self.charge.append(charge)
        return hits, charge

    def result(self):
        """NumPy tables: ``spectrum [S, 251]``, ``occupancy [S]`` (mean over events of hits / (H*W)), ``mean_charge [S]`` (mean over
        the events in which the sensor had a hit of charge / hits; NaN for a sensor that never had one), ``occ_hist [200]`` over
        [0, 0.02) of every per-image occupancy plus ``occ_overflow``, ``n_events``; and the per-image ``hits`` / ``charge`` ``[E, S]``.
        The occupancy bin is ``(hits * 10000) // (H*W)`` in integers: a bin edge of ``linspace(0, 0.02, 201)`` is then decided
        exactly, not by float rounding."""
        spectrum, per_image = self._host_tables()
        hits, charge = per_image["hits"].astype(np.int64), per_image["charge"]
        px = self.shape[0] * self.shape[1]
        occupancy = (hits.astype(np.float64) / px).mean(0)
        has = hits > 0
        per = np.where(has, charge.astype(np.float64) / np.maximum(hits, 1), 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_charge = per.sum(0) / has.sum(0)
        b = (hits.reshape(-1) * 10000) // px
        occ_hist = np.bincount(b[b < PXD_OCC_BINS], minlength=PXD_OCC_BINS).astype(np.int64)
        return dict(spectrum=spectrum, occupancy=occupancy, mean_charge=mean_charge, occ_hist=occ_hist,
                    occ_overflow=int((b >= PXD_OCC_BINS).sum()), n_events=int(hits.shape[0]), hits=hits, charge=charge)


def pxd_distance(real, fake):
    """Three distances between two ``PXDStatistics.result()`` tables (float64, host): ``occ_rel_err`` / ``charge_rel_err`` = mean over
    the sensors with real occupancy > 0 of |fake - real| / real (a fake sensor that never had a hit counts with mean charge 0, i.e.
    a relative error of 1); ``spectrum_w1`` = the 1-D Wasserstein distance in ADU between the hit spectra (bins 2 .. 250, one ADU
    wide, pooled over the sensors, each normalised to 1), NaN when one side has no hit at all."""
    occ_r = np.asarray(real["occupancy"], np.float64)
    return dict(occ_rel_err=_rel_err(occ_r, fake["occupancy"], occ_r > 0),
                charge_rel_err=_rel_err(real["mean_charge"], fake["mean_charge"], occ_r > 0),
                spectrum_w1=_w1(np.asarray(real["spectrum"])[:, 2:], np.asarray(fake["spectrum"])[:, 2:]))


# ---------------------------------------------------------------------------------------------------------
# event production (reference Physics_Analysis/create_g1.py:62-79): sparse digits (sensor, u cell, v cell, charge)
# ---------------------------------------------------------------------------------------------------------
PXD_DIGITS_FRACTION = 16    # default capacity of pxd_digits: one digit per 16 pixels (6.25 %; PXD background sits near 1 %)


class PXDDigits(_PXDProduct):
    """Device-side result of ``pxd_digits``: ``index`` int32 ``[capacity]`` (flat position ``n*H*W + r*W + c``, ascending), ``charge``
    uint8 ``[capacity]``, ``counts`` int32 ``[N]``, ``total`` int32 ``[1]`` -- only the first ``min(total, capacity)`` digits are
    written.  ``start_copy`` enqueues the device-to-host copies, ``cpu()`` / ``unpack()`` wait for them (one wait)."""
    _again = lambda self, capacity: pxd_digits(self.images, self.threshold, capacity, self.n_sensors)

    def __init__(self, images, threshold, capacity, n_sensors, header, index, charge):
        self.images, self.threshold, self.capacity, self.n_sensors = images, threshold, capacity, n_sensors
        self.shape, self.index, self.charge, self._host = tuple(images.shape), index, charge, None
        self._set_header(header)

    copied = property(lambda self: self._host[3] if self._host else 0, doc="Digits covered by the last ``start_copy`` (0 before the first).")

    def start_copy(self, expect=None, buffers=None):
        """Enqueue the copy of the header (``counts``, ``total``) and of the first ``expect`` digits (default: ``capacity``) into
        pinned host memory on the current stream, and record an event; does not wait.  ``buffers``: pinned tensors
        ``(header int32 [>= N+1], index int32, charge uint8)`` to reuse instead of allocating."""
        m = self.capacity if expect is None else max(0, min(int(expect), self.capacity))
        N = self.shape[0]
        if buffers is None:
            buffers = (torch.empty(N + 1, dtype=torch.int32, pin_memory=True), torch.empty(m, dtype=torch.int32, pin_memory=True),
                       torch.empty(m, dtype=torch.uint8, pin_memory=True))
        hdr, idx, chg = buffers
        if hdr.numel() < N + 1 or idx.numel() < m or chg.numel() < m:
            raise ValueError("PXDDigits.start_copy: a host buffer is too short")
        with torch.cuda.device(self.header.device):
            hdr[:N + 1].copy_(self.header, non_blocking=True)
            idx[:m].copy_(self.index[:m], non_blocking=True)
            chg[:m].copy_(self.charge[:m], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self._host = (hdr, idx, chg, m, ev)
        return self

    def cpu(self):
        """NumPy ``(index [total], charge [total], counts [N])``: waits once for the copies of ``start_copy`` (started here when the
        caller did not).  Never truncated: when ``total`` exceeds the capacity the kernel is run again with ``capacity = total``, and
        when it exceeds what was copied the rest is copied -- a second wait, on those paths only."""
        if self._host is None:
            self.start_copy()
        hdr, idx, chg, m, ev = self._host
        ev.synchronize()
        N = self.shape[0]
        counts, total = hdr[:N].numpy().copy(), int(hdr[N])
        if total > self.capacity:
            self._grow(total)
            m = 0                       # of the new arrays nothing is copied yet
        index, charge = idx[:min(m, total)].numpy().copy(), chg[:min(m, total)].numpy().copy()
        if total > m:
            index = np.concatenate([index, self.index[m:total].cpu().numpy()])
            charge = np.concatenate([charge, self.charge[m:total].cpu().numpy()])
        return index, charge, counts

    def unpack(self):
        """NumPy ``(event, sensor, ucell, vcell, charge)`` of every digit, in ascending flat index: image ``n`` is sensor
        ``n % n_sensors`` of event ``n // n_sensors``, ``ucell`` the row and ``vcell`` the column (create_g1.py:77, :106)."""
        index, charge, _ = self.cpu()
        return unpack_digits(index, charge, self.shape, self.n_sensors)


def unpack_digits(index, charge, shape, n_sensors=40):
    """Flat digit positions of an ``[N, H, W]`` batch -> ``(event, sensor, ucell, vcell, charge)`` arrays."""
    N, Hh, Ww = shape
    index = np.asarray(index)
    if index.dtype != np.int32:                 # the kernel's own int32 positions are split in int32 (N*H*W < 2^31)
        index = index.astype(np.int64)
    n, rest = np.divmod(index, index.dtype.type(Hh * Ww))
    r, c = np.divmod(rest, index.dtype.type(Ww))
    return ((n // n_sensors).astype(np.int32), (n % n_sensors).astype(np.uint8 if n_sensors <= 256 else np.int32),
            r.astype(np.uint8 if Hh <= 256 else np.uint16), c.astype(np.uint16), np.asarray(charge, np.uint8))


def pxd_digits(images, threshold=0.0, capacity=None, n_sensors=40):
    """Sparse digits of a batch of sensor images in detector units, ``[N, H, W]`` fp32 (``Generator(..., export=True)``) or uint8 (event
    files), compacted on the device (csrc/pxd_digits.hip): the reference's ``.to(uint8)`` / ``nonzero()`` / gather
    (Physics_Analysis/create_g1.py:73-79) without the dense tensor crossing PCIe.  A pixel is a digit iff its truncated charge
    ``q = uint8(min(max(v, 0), 255))`` is positive and ``v >= threshold`` (0: the reference's production behaviour, 7: the evaluation
    cut); digits come in ascending flat index, the order of ``torch.nonzero``, bit-identical run to run.

    Launches on the current stream, neither synchronises nor copies; with ``capacity`` given it can be captured into a HIP graph.
    ``capacity`` (digits) defaults to one per 16 pixels (``N*H*W // 16``, at least 1024).  ``counts`` and ``total`` of the returned
    ``PXDDigits`` always hold the true numbers; its ``cpu()`` / ``unpack()`` rerun with a larger capacity instead of truncating."""
    x = _sensor_images(images, n_sensors, "pxd_digits")
    dev = x.device
    N, Hh, Ww = x.shape
    if N * Hh * Ww >= 2 ** 31:
        raise ValueError(f"pxd_digits: {N} x {Hh} x {Ww} pixels do not fit the int32 flat index; split the batch")
    capacity = max(1024, N * Hh * Ww // PXD_DIGITS_FRACTION) if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError("pxd_digits: capacity is negative")
    header, counts, total = _header(N, dev)
    index = torch.empty(capacity, dtype=torch.int32, device=dev)
    charge = torch.empty(capacity, dtype=torch.uint8, device=dev)
    scratch = torch.empty(H.lib().ieagan_pxd_digits_scratch(N, Hh, Ww), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_digits", x.data_ptr(), int(x.dtype == torch.uint8), N, Hh, Ww, float(threshold), capacity,
               *_ptrs(capacity, index, charge), counts, total, scratch.data_ptr(), H.stream())
    return PXDDigits(x, float(threshold), capacity, int(n_sensors), header, index, charge)


# ---------------------------------------------------------------------------------------------------------
# detector-level validation, cluster level: connected components of the digits and their spectra (csrc/pxd_clusters.hip)
# ---------------------------------------------------------------------------------------------------------
class PXDClusters(_PXDProduct):
    """Device-side result of ``pxd_clusters``: the ``PXDDigits`` it was built from (``digits``), ``label`` int32 ``[capacity]`` (cluster
    number of digit k) and the cluster table ``first`` / ``size`` / ``charge`` / ``size_u`` / ``size_v`` int32 and ``seed`` uint8, all
    ``[capacity]`` (a batch has at most as many clusters as digits), ``counts`` int32 ``[N]`` (clusters per image), ``total`` int32
    ``[1]``.  Only the first ``min(digits.total, capacity)`` labels and the first ``total`` table rows are written."""
    TABLE = ("first", "size", "charge", "seed", "size_u", "size_v")
    _again = lambda self, capacity: pxd_clusters(self.images, self.threshold, capacity, self.n_sensors)

    def __init__(self, digits, label, first, size, charge, seed, size_u, size_v, header):
        self.digits, self.label = digits, label
        self.first, self.size, self.charge, self.seed, self.size_u, self.size_v = first, size, charge, seed, size_u, size_v
        self._set_header(header, digits)

    def cpu(self):
        """One read-back (``pxd_read_back``: one copy, one wait) -> dict of NumPy arrays trimmed to the true totals: per digit ``index``,
        ``digit_charge``, ``label``; per cluster ``first``, ``size``, ``charge``, ``seed``, ``size_u``, ``size_v``, ``sensor``
        (``first // (H*W) % n_sensors``), ``event``; ``counts [N]``, ``digit_counts [N]``.  Never truncated (``_host_columns``)."""
        N, Hh, Ww = self.shape
        host = self._host_columns(lambda: dict(digit_header=self.digits.header, header=self.header, index=self.digits.index,
                                               digit_charge=self.digits.charge, label=self.label, **{k: getattr(self, k) for k in self.TABLE}))
        dtotal, total = int(host["digit_header"][N]), int(host["header"][N])
        out = {k: host[k][:dtotal].copy() for k in ("index", "label", "digit_charge")}
        out.update((k, host[k][:total].copy()) for k in self.TABLE)
        image = out["first"] // np.int32(Hh * Ww)
        return dict(out, sensor=(image % self.n_sensors).astype(np.int32), event=(image // self.n_sensors).astype(np.int32),
                    counts=host["header"][:N].copy(), digit_counts=host["digit_header"][:N].copy())


def pxd_clusters(images_or_digits, threshold=0.0, capacity=None, n_sensors=40):
    """Clusters of a batch of sensor images ``[N, H, W]`` (fp32 or uint8 device tensor: ``pxd_digits(images, threshold, capacity,
    n_sensors)`` runs first) or of an existing ``PXDDigits`` (its threshold, capacity and sensors hold): connected components of the
    digits under 8-connectivity inside an image, numbered by the flat index of their first digit -- the raster numbering of
    ``scipy.ndimage.label(img > 0, ones((3, 3)))`` per image with a running offset -- with size, summed charge, seed charge and row /
    column extent per cluster, all integers, bit-identical run to run (csrc/pxd_clusters.hip).

    Launches on the current stream, neither synchronises nor copies; with ``capacity`` given it can be captured into a HIP graph.  When
    the digit total exceeds the capacity the device result covers the first ``capacity`` digits; ``PXDClusters.cpu()`` reruns instead
    of handing back a truncated event."""
    H.require_gpu()
    d = images_or_digits if isinstance(images_or_digits, PXDDigits) else pxd_digits(images_or_digits, threshold, capacity, n_sensors)
    N, Hh, Ww = d.shape
    if Hh * Ww * 255 >= 2 ** 31:
        raise ValueError(f"pxd_clusters: {Hh} x {Ww} pixels x 255 do not fit the int32 cluster charge")
    dev, C = d.index.device, d.capacity
    i32 = lambda: torch.empty(C, dtype=torch.int32, device=dev)
    label, first, size, charge, size_u, size_v = i32(), i32(), i32(), i32(), i32(), i32()
    seed = torch.empty(C, dtype=torch.uint8, device=dev)
    header, counts, total = _header(N, dev)
    scratch = torch.empty(H.lib().ieagan_pxd_clusters_scratch(N, Hh, Ww, C), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_clusters", *_ptrs(C, d.index, d.charge), d.total.data_ptr(), N, Hh, Ww, C,
               *_ptrs(C, label, first, size, charge, seed, size_u, size_v), counts, total, scratch.data_ptr(), H.stream())
    return PXDClusters(d, label, first, size, charge, seed, size_u, size_v, header)


class PXDClusterStatistics(_PXDAccumulator):
    """Accumulator of per-sensor cluster spectra over batches of sensor images in detector units (``[N, H, W]`` fp32 or uint8, image ``n``
    is sensor ``n % n_sensors``), beside ``PXDStatistics``: ``update`` runs digits -> clusters -> ``ieagan_pxd_cluster_stats`` on the
    current stream and neither synchronises nor copies; ``result()`` does the single read-back.  Counters are exact int64.
    ``capacity`` (digits per update) defaults to that of ``pxd_digits``; an update whose digit total exceeds it is counted on the device
    and makes ``result()`` raise: a truncated event is never reported.  ``update`` also takes the ``PXDClusters`` of the batch and then
    launches the statistics kernel alone.  ``tables``: int64 ``[S * 640 + 1]`` on the device, the spectra, then the overflow counter."""

    def update(self, images_or_clusters):
        c = self._input(images_or_clusters, "pxd_digits", PXDClusters)      # a wrong dtype or rank is reported as by pxd_digits
        if not isinstance(c, PXDClusters):
            c = pxd_clusters(c, self.threshold, self.capacity, self.n_sensors)
        (N, Hh, Ww), S = c.shape, self.n_sensors
        if self.tables is None:
            self.tables = torch.zeros(S * H.PXD_CLUSTER_BINS + 1, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            H.call("ieagan_pxd_cluster_stats", *_ptrs(c.capacity, c.first, c.size, c.charge, c.seed, c.size_u, c.size_v), c.total.data_ptr(),
                   c.digits.total.data_ptr(), N, Hh, Ww, S, c.capacity, self.tables.data_ptr(),
                   self.tables.data_ptr() + 8 * S * H.PXD_CLUSTER_BINS, H.stream())
        self.clusters.append(c.counts)
        return c

    def result(self):
        """NumPy tables: int64 ``size_spectrum [S, 64]`` (bin ``min(size, 64) - 1``), ``charge_spectrum [S, 256]`` (bin
        ``min(charge >> 3, 255)``, 8 ADU a bin), ``seed_spectrum [S, 256]``, ``size_u_spectrum`` / ``size_v_spectrum [S, 32]`` (bin
        ``min(s, 32) - 1``), ``clusters`` int32 ``[events, S]`` (clusters per image) and ``n_events``.  Raises when an update overflowed."""
        table, per_image = self._host_tables()
        rows = table.reshape(self.n_sensors, H.PXD_CLUSTER_BINS)
        return dict({k: rows[:, a:a + n].copy() for k, (a, n) in H.PXD_CLUSTER_COLUMNS.items()}, **per_image)


def pxd_cluster_distance(real, fake):
    """Four distances between two ``PXDClusterStatistics.result()`` tables (float64, host): ``cluster_rate_rel_err`` = mean over the
    sensors with real clusters of |fake - real| / real of the mean clusters per image; ``size_w1`` (pixels), ``cluster_charge_w1`` (ADU,
    bins of 8) and ``seed_w1`` (ADU) = 1-D Wasserstein distances between the spectra pooled over the sensors and normalised to 1 (the
    construction of ``pxd_distance`` for the ADC spectrum), NaN when one side has no cluster at all."""
    r = np.asarray(real["clusters"], np.float64).mean(0)
    out = dict(cluster_rate_rel_err=_rel_err(r, np.asarray(fake["clusters"], np.float64).mean(0), r > 0))
    for name, key, width in (("size_w1", "size_spectrum", 1.0), ("cluster_charge_w1", "charge_spectrum", 8.0), ("seed_w1", "seed_spectrum", 1.0)):
        out[name] = _w1(real[key], fake[key], width)
    return out


# ---------------------------------------------------------------------------------------------------------
# cluster reconstruction: seed / cluster-charge cuts, charge-weighted positions and per-sensor position maps (csrc/pxd_reco.hip)
# ---------------------------------------------------------------------------------------------------------
def _check_cuts(who, seed_cut, charge_cut):
    seed_cut, charge_cut = int(seed_cut), int(charge_cut)
    if seed_cut < 0 or charge_cut < 0:
        raise ValueError(f"{who}: seed_cut = {seed_cut} / charge_cut = {charge_cut} is negative")
    return seed_cut, charge_cut


class PXDClusterPositions(_PXDProduct):
    """Device-side result of ``pxd_cluster_positions``: the ``PXDClusters`` it came from (``clusters``), the moments ``mu`` / ``mv`` int64
    ``[capacity]`` of every cluster (row j of the table: sum of charge x row, charge x column), and for the clusters that pass the cuts, in
    cluster order: ``cluster`` int32 (row of the table), ``u`` / ``v`` fp32 (charge-weighted row / column in cell units, the centre of cell
    ``r`` is ``r``), all ``[capacity]``; ``counts`` int32 ``[N]`` (accepted clusters per image), ``total`` int32 ``[1]``.  Only the first
    ``clusters.total`` moments and the first ``total`` rows of ``cluster`` / ``u`` / ``v`` are written."""
    _again = lambda self, capacity: pxd_cluster_positions(self.images, self.threshold, self.seed_cut, self.charge_cut, capacity, self.n_sensors)

    def __init__(self, clusters, seed_cut, charge_cut, mu, mv, cluster, u, v, header):
        self.clusters, self.seed_cut, self.charge_cut = clusters, seed_cut, charge_cut
        self.mu, self.mv, self.cluster, self.u, self.v = mu, mv, cluster, u, v
        self._set_header(header, clusters)

    def cpu(self):
        """One read-back (``pxd_read_back``: one copy, one wait) -> dict of NumPy arrays trimmed to the true total, one entry per accepted
        cluster: ``cluster``, ``u``, ``v``, ``mu``, ``mv`` and, gathered through ``cluster``, ``sensor``, ``event``, ``size``, ``charge``,
        ``seed``, ``size_u``, ``size_v``; plus ``counts [N]``.  Never truncated (``_host_columns``)."""
        N, Hh, Ww = self.shape
        host = self._host_columns(lambda: dict(digit_header=self.clusters.digits.header, header=self.header, cluster=self.cluster, u=self.u, v=self.v,
                                               mu=self.mu, mv=self.mv, **{k: getattr(self.clusters, k) for k in PXDClusters.TABLE}))
        total = int(host["header"][N])
        cluster = host["cluster"][:total].copy()
        image = host["first"][cluster] // np.int32(Hh * Ww)
        return dict({k: host[k][:total].copy() for k in ("u", "v")}, cluster=cluster, sensor=(image % self.n_sensors).astype(np.int32),
                    event=(image // self.n_sensors).astype(np.int32), counts=host["header"][:N].copy(),
                    **{k: host[k][cluster] for k in ("mu", "mv", "size", "charge", "seed", "size_u", "size_v")})


def pxd_cluster_positions(images_or_clusters, threshold=0.0, seed_cut=0, charge_cut=0, capacity=None, n_sensors=40):
    """Reconstructed clusters of a batch of sensor images ``[N, H, W]`` (fp32 or uint8 device tensor: ``pxd_clusters(images, threshold,
    capacity, n_sensors)`` runs first) or of an existing ``PXDClusters`` (its threshold, capacity and sensors hold): the clusters with
    ``seed >= seed_cut and charge >= charge_cut`` (integers in ADU; 0 accepts everything), in cluster order, with their charge-weighted
    position ``u = sum(q * row) / sum(q)``, ``v = sum(q * column) / sum(q)`` (csrc/pxd_reco.hip).  The sums are exact 64-bit integers and
    the division is one IEEE float64 division rounded to fp32, so ``(mu.astype(float64) / charge.astype(float64)).astype(float32)`` on the
    host gives the same bits; bit-identical run to run.

    Launches on the current stream, neither synchronises nor copies; with ``capacity`` given it can be captured into a HIP graph.  When
    the digit total exceeds the capacity the device result covers the first ``capacity`` digits; ``PXDClusterPositions.cpu()`` reruns
    instead of handing back a truncated event."""
    H.require_gpu()
    seed_cut, charge_cut = _check_cuts("pxd_cluster_positions", seed_cut, charge_cut)
    c = images_or_clusters if isinstance(images_or_clusters, PXDClusters) else pxd_clusters(images_or_clusters, threshold, capacity, n_sensors)
    d = c.digits
    N, Hh, Ww = c.shape
    dev, C = c.label.device, c.capacity
    mu, mv = (torch.empty(C, dtype=torch.int64, device=dev) for _ in range(2))
    cluster = torch.empty(C, dtype=torch.int32, device=dev)
    u, v = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(2))
    header, counts, total = _header(N, dev)
    scratch = torch.empty(H.lib().ieagan_pxd_cluster_positions_scratch(N, Hh, Ww, C), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_cluster_positions", *_ptrs(C, d.index, d.charge, c.label), d.total.data_ptr(), *_ptrs(C, c.first, c.charge, c.seed),
               c.total.data_ptr(), N, Hh, Ww, C, seed_cut, charge_cut, *_ptrs(C, mu, mv, cluster, u, v), counts, total, scratch.data_ptr(),
               H.stream())
    return PXDClusterPositions(c, seed_cut, charge_cut, mu, mv, cluster, u, v, header)


class PXDClusterMaps(_PXDAccumulator):
    """Accumulator of per-sensor position maps of the reconstructed clusters over batches of sensor images in detector units (``[N, H, W]``
    fp32 or uint8, image ``n`` is sensor ``n % n_sensors``), beside ``PXDClusterStatistics``: where on a sensor the clusters that pass the
    cuts lie, on a fixed grid of 25 x 48 bins over the image.  ``update`` runs digits -> clusters -> positions ->
    ``ieagan_pxd_cluster_maps`` on the current stream and neither synchronises nor copies; ``result()`` does the single read-back.
    Counters are exact int64; the bin of a cluster is decided in integers.  ``capacity`` (digits per update) defaults to that of
    ``pxd_digits``; an update whose digit total exceeds it is counted on the device and makes ``result()`` raise.  ``update`` also takes
    the ``PXDClusters`` of the batch (positions -> maps are launched) or its ``PXDClusterPositions`` (the maps kernel alone).  ``tables``:
    int64 ``[2 * S * 25 * 48 + 1]`` on the device, count map, charge map, then the overflow counter."""

    def __init__(self, n_sensors=40, threshold=7.0, seed_cut=0, charge_cut=0, capacity=None, device=None):
        self.seed_cut, self.charge_cut = _check_cuts("PXDClusterMaps", seed_cut, charge_cut)
        super().__init__(n_sensors, threshold, capacity, device)

    def update(self, images_or_product):
        p = self._input(images_or_product, "pxd_digits", PXDClusters, PXDClusterPositions)      # a wrong dtype or rank is reported as by pxd_digits
        if not isinstance(p, PXDClusterPositions):
            p = pxd_cluster_positions(p, self.threshold, self.seed_cut, self.charge_cut, self.capacity, self.n_sensors)
        c, (N, Hh, Ww) = p.clusters, p.shape
        S, B = self.n_sensors, H.PXD_MAP_U * H.PXD_MAP_V
        if self.tables is None:
            self.tables = torch.zeros(2 * S * B + 1, dtype=torch.int64, device=self.device)
        t = self.tables.data_ptr()
        with torch.cuda.device(self.device):
            H.call("ieagan_pxd_cluster_maps", *_ptrs(p.capacity, p.cluster), p.total.data_ptr(), *_ptrs(p.capacity, c.first, c.charge, p.mu, p.mv),
                   c.total.data_ptr(), c.digits.total.data_ptr(), N, Hh, Ww, S, p.capacity, t, t + 8 * S * B, t + 16 * S * B, H.stream())
        self.clusters.append(p.counts)
        return p

    def result(self):
        """NumPy tables: int64 ``count_map`` / ``charge_map [S, 25, 48]`` (accepted clusters and their summed charge per bin
        ``(floor(u / H * 25), floor(v / W * 48))``), ``u_profile [S, 25]`` and ``v_profile [S, 48]`` (sums of ``count_map`` over the other
        axis), ``clusters`` int32 ``[events, S]`` (accepted clusters per image), ``n_events`` and ``shape`` (the image size ``(H, W)``,
        which gives the bins their width in pixels).  Raises when an update overflowed."""
        table, per_image = self._host_tables()
        count_map, charge_map = table.reshape(2, self.n_sensors, H.PXD_MAP_U, H.PXD_MAP_V)
        return dict(count_map=count_map, charge_map=charge_map, u_profile=count_map.sum(2), v_profile=count_map.sum(1), **per_image,
                    shape=self.shape)


def pxd_map_distance(real, fake):
    """Four distances between two ``PXDClusterMaps.result()`` tables (float64, host): ``accepted_rate_rel_err`` = mean over the sensors
    with real accepted clusters of |fake - real| / real of the mean accepted clusters per image; ``u_profile_w1`` / ``v_profile_w1`` = 1-D
    Wasserstein distances in pixels (bins ``H / 25`` and ``W / 48`` wide) between the row / column profiles pooled over the sensors and
    normalised to 1, NaN when one side has no cluster at all; ``map_tv`` = mean over the sensors with real clusters of the total-variation
    distance ``0.5 * sum |p_fake - p_real|`` between the normalised 25 x 48 maps (a fake sensor without a cluster counts as 1), NaN when no
    sensor has a real cluster."""
    Hh, Ww = real["shape"]
    r = np.asarray(real["clusters"], np.float64).mean(0)
    out = dict(accepted_rate_rel_err=_rel_err(r, np.asarray(fake["clusters"], np.float64).mean(0), r > 0),
               u_profile_w1=_w1(real["u_profile"], fake["u_profile"], Hh / H.PXD_MAP_U),
               v_profile_w1=_w1(real["v_profile"], fake["v_profile"], Ww / H.PXD_MAP_V))
    mr = np.asarray(real["count_map"], np.float64).reshape(len(r), -1)
    mf = np.asarray(fake["count_map"], np.float64).reshape(len(r), -1)
    nr, nf = mr.sum(1), mf.sum(1)
    tv = [0.5 * np.abs(mf[s] / nf[s] - mr[s] / nr[s]).sum() if nf[s] > 0 else 1.0 for s in np.nonzero(nr > 0)[0]]
    out["map_tv"] = float(np.mean(tv)) if tv else float("nan")
    return out


# ---------------------------------------------------------------------------------------------------------
# intra-event correlations: per-event region counts, their exact second moments and ranks (csrc/pxd_corr.hip)
# ---------------------------------------------------------------------------------------------------------
def _check_regions(who, regions, n_sensors, shape=None):
    """``regions = (RU, RV)`` as two ints, after the bounds of the kernels: ``RU, RV >= 1``, ``n_sensors * RU * RV <= 1024`` and, once the
    image size is known, ``RU <= H``, ``RV <= W``."""
    try:
        ru, rv = (int(v) for v in regions)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: regions must be a pair (RU, RV), got {regions!r}") from None
    if ru < 1 or rv < 1:
        raise ValueError(f"{who}: regions = {ru} x {rv} must be at least 1 x 1")
    if int(n_sensors) * ru * rv > H.PXD_CORR_MAX_COLUMNS:
        raise ValueError(f"{who}: {n_sensors} sensors x {ru} x {rv} regions are more than {H.PXD_CORR_MAX_COLUMNS} columns")
    if shape is not None and (ru > shape[0] or rv > shape[1]):
        raise ValueError(f"{who}: regions = {ru} x {rv} are finer than the {shape[0]} x {shape[1]} pixels of a sensor")
    return ru, rv


def _region_counts(d, regions, overflow):
    """``ieagan_pxd_region_counts`` of a ``PXDDigits``: the int32 ``[E, R]`` table; ``overflow``: the device address of the int64 word."""
    (N, Hh, Ww), S, (ru, rv), dev = d.shape, d.n_sensors, regions, d.index.device
    x = torch.empty(N // S, S * ru * rv, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_region_counts", *_ptrs(d.capacity, d.index), d.total.data_ptr(), N, Hh, Ww, S, ru, rv, d.capacity, x.data_ptr(),
               overflow, H.stream())
    return x


def _gram(x, tables):
    """``ieagan_pxd_gram``: the moments of the int32 table ``x [E, R]`` added into ``tables`` (int64, gram ``[R * R]`` then sum ``[R]``)."""
    E, R = x.shape
    with torch.cuda.device(x.device):
        H.call("ieagan_pxd_gram", x.data_ptr(), E, R, tables.data_ptr(), tables.data_ptr() + 8 * R * R, H.stream())


def pxd_region_counts(images_or_digits, regions=(1, 1), threshold=0.0, capacity=None, n_sensors=40):
    """The per-event occupancy table of a batch, int32 ``[E, R]`` on the device (csrc/pxd_corr.hip): a grid of ``regions = (RU, RV)`` lies
    over every sensor, a digit at row ``r``, column ``c`` of image ``n`` belongs to event ``n // S``, sensor ``s = n % S`` and region
    ``ru = r * RU // H``, ``rv = c * RV // W`` (integers), and counts for column ``(s * RU + ru) * RV + rv`` of ``R = S * RU * RV <= 1024``.
    Input: sensor images ``[N, H, W]`` (``pxd_digits(images, threshold, capacity, n_sensors)`` runs first) or an existing ``PXDDigits``
    (its threshold, capacity and sensors hold).  ``(1, 1)`` counts whole sensors.  int32 atomics only: bit-identical run to run.

    Launches on the current stream, neither synchronises nor copies.  When the digit total exceeds the capacity the table covers the
    first ``capacity`` digits (``PXDDigits.total`` holds the true number); ``PXDCorrelations`` refuses such an update in ``result()``."""
    H.require_gpu()
    d = images_or_digits if isinstance(images_or_digits, PXDDigits) else pxd_digits(images_or_digits, threshold, capacity, n_sensors)
    regions = _check_regions("pxd_region_counts", regions, d.n_sensors, d.shape[1:])
    return _region_counts(d, regions, torch.zeros(1, dtype=torch.int64, device=d.index.device).data_ptr())


def _correlation(n, gram, total):
    """The coefficient table ``[R, R]`` float64 of the integer moments of ``n`` events: ``cov_ij = n * gram_ij - total_i * total_j`` and
    ``var_i = cov_ii`` in exact integers (Python ``int``: ``n * gram`` can pass 2**63), ``rho_ij = float(cov_ij) / sqrt(float(var_i) *
    float(var_j))``; NaN where a variance is 0 or ``n < 2``."""
    g, s = np.asarray(gram).astype(object), np.asarray(total).astype(object)
    cov = int(n) * g - np.outer(s, s)
    var = np.array([float(v) for v in np.diagonal(cov)], np.float64)
    ok = (var[:, None] != 0) & (var[None, :] != 0) & (int(n) >= 2)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = cov.astype(np.float64) / np.sqrt(var[:, None] * var[None, :])
    return np.where(ok, rho, np.nan)


class PXDCorrelations(_PXDAccumulator):
    """Accumulator of the correlations between the region occupancies of one event, over the events: what ties the 40 sensor images of
    an event together (a busy event is busy on every sensor), which no per-sensor statistic sees.  ``regions = (RU, RV)``: the grid over a
    sensor, ``R = n_sensors * RU * RV <= 1024`` columns (``pxd_region_counts``); ``(1, 1)`` is the sensor-level matrix.  ``update`` takes
    images, the ``PXDDigits`` of the batch or its ``PXDClusters`` (their digits) and launches ``ieagan_pxd_region_counts`` and
    ``ieagan_pxd_gram`` on the current stream; it keeps the batch's table ``[E, R]`` on the device and neither synchronises nor copies.
    ``result()`` ranks the columns of the whole table (``ieagan_pxd_ranks``, at most 65535 events), takes the moments of the ranks and
    does the single read-back.  Every device number is an exact integer; the host does the float64 arithmetic on the tables.  ``capacity``
    (digits per update) defaults to that of ``pxd_digits``; an update whose digit total exceeds it is counted on the device and makes
    ``result()`` raise.  ``tables``: int64 ``[R * R + R + 1]`` on the device, gram, sum, then the overflow counter."""
    _per_image = ("counts", "rank_tables")          # rank_tables: the one int64 table of the ranks' moments, made by result()

    def __init__(self, n_sensors=40, threshold=7.0, regions=(1, 1), capacity=None, device=None):
        self.regions = _check_regions("PXDCorrelations", regions, n_sensors)
        super().__init__(n_sensors, threshold, capacity, device)

    def update(self, images_or_product):
        d = self._input(images_or_product, "pxd_digits", PXDDigits, PXDClusters)        # a wrong dtype or rank is reported as by pxd_digits
        if isinstance(d, PXDClusters):
            d = d.digits
        elif not isinstance(d, PXDDigits):
            d = pxd_digits(d, self.threshold, self.capacity, self.n_sensors)
        _check_regions("PXDCorrelations.update", self.regions, self.n_sensors, self.shape)
        R = self.n_sensors * self.regions[0] * self.regions[1]
        if self.tables is None:
            self.tables = torch.zeros(R * R + R + 1, dtype=torch.int64, device=self.device)
        x = _region_counts(d, self.regions, self.tables.data_ptr() + 8 * (R * R + R))
        _gram(x, self.tables)
        self.counts.append(x)
        return x

    def result(self):
        """NumPy tables.  Integers: ``gram`` int64 ``[R, R]`` (sum over the events of ``x_i * x_j``, symmetric) and ``sum`` int64 ``[R]`` of
        the counts, ``rank_gram`` / ``rank_sum`` the same of ``rank2 = 2 * #{smaller} + #{equal} + 1`` (twice the mid-rank of a count among
        the events, ``2 * scipy.stats.rankdata``), ``counts`` int32 ``[events, R]``, ``n_events``, ``regions`` and ``shape`` (the image size).
        Float64 ``[R, R]``: ``pearson`` from ``(sum, gram)`` and ``spearman`` from ``(rank_sum, rank_gram)`` by ``cov_ij = n * G_ij - s_i *
        s_j`` in exact integers and ``float(cov_ij) / sqrt(float(var_i) * float(var_j))``; NaN where a column never varies or with fewer
        than 2 events.  Raises when an update overflowed, before any update and beyond 65535 events."""
        who = type(self).__name__
        if not self.counts:
            raise RuntimeError(f"{who}.result() before any update()")
        x = self.counts[0] if len(self.counts) == 1 else torch.cat(self.counts)
        E, R = x.shape
        if E > H.PXD_CORR_MAX_EVENTS:
            raise ValueError(f"{who}.result: {E} events are more than the {H.PXD_CORR_MAX_EVENTS} the rank transform takes")
        rank2, moments = torch.empty_like(x), torch.zeros(R * R + R, dtype=torch.int64, device=x.device)
        with torch.cuda.device(x.device):
            H.call("ieagan_pxd_ranks", x.data_ptr(), E, R, rank2.data_ptr(), H.stream())
        _gram(rank2, moments)
        self.counts, self.rank_tables = [x], [moments]
        table, host = self._host_tables()           # the one read-back; refuses an overflow
        ranks, counts = host["rank_tables"].reshape(-1), host["counts"].reshape(E, R)
        gram, total = table[:R * R].reshape(R, R), table[R * R:]
        rank_gram, rank_sum = ranks[:R * R].reshape(R, R), ranks[R * R:]
        return dict(gram=gram, sum=total, rank_gram=rank_gram, rank_sum=rank_sum, counts=counts, n_events=E, regions=self.regions,
                    shape=self.shape, pearson=_correlation(E, gram, total), spearman=_correlation(E, rank_gram, rank_sum))


def pxd_correlation_distance(real, fake):
    """Four distances between two ``PXDCorrelations.result()`` tables (float64, host), over the pairs ``i < j`` whose real coefficient is
    defined (a fake NaN counts as 0): ``pearson_rms`` / ``spearman_rms`` = root mean square of ``rho_fake - rho_real``;
    ``spearman_max_abs`` = the largest such difference; ``spearman_strength_err`` = mean ``|rho_fake|`` minus mean ``|rho_real|`` (negative:
    the generator under-correlates).  NaN when no pair is defined.  ``ValueError`` when ``regions``, the columns or ``shape`` differ."""
    for k in ("regions", "shape"):
        if tuple(real[k]) != tuple(fake[k]):
            raise ValueError(f"pxd_correlation_distance: the two sides differ in {k}: {real[k]} and {fake[k]}")
    if np.shape(real["spearman"]) != np.shape(fake["spearman"]):
        raise ValueError(f"pxd_correlation_distance: the two sides differ in columns: {np.shape(real['spearman'])[0]} and {np.shape(fake['spearman'])[0]}")
    upper = np.triu(np.ones(np.shape(real["spearman"]), bool), 1)

    def pairs(name):            # the real and the fake coefficient of every pair that counts
        r = np.asarray(real[name], np.float64)
        ok = upper & ~np.isnan(r)
        return r[ok], np.nan_to_num(np.asarray(fake[name], np.float64), nan=0.0)[ok]
    (pr, pf), (sr, sf) = pairs("pearson"), pairs("spearman")
    rms = lambda r, f: float(np.sqrt(np.mean((f - r) ** 2))) if r.size else float("nan")
    return dict(pearson_rms=rms(pr, pf), spearman_rms=rms(sr, sf),
                spearman_max_abs=float(np.abs(sf - sr).max()) if sr.size else float("nan"),
                spearman_strength_err=float(np.abs(sf).mean() - np.abs(sr).mean()) if sr.size else float("nan"))


class PXDValidation:
    """The accumulators of one side of a validation, fed together: ``stats`` (a ``PXDStatistics``), ``clusters`` (a ``PXDClusterStatistics``
    with ``clusters=True``, else None), ``maps`` (a ``PXDClusterMaps`` without cuts with ``maps=True``, with the cuts of ``maps=(seed_cut,
    charge_cut)``, else None) and ``correlations`` (a ``PXDCorrelations`` of whole sensors with ``correlations=True``, on the grid of
    ``correlations=(RU, RV)``, else None); ``n_sensors``, ``threshold``, ``device`` and, where there is one, ``capacity`` go to each.
    ``update`` runs the chain once -- digits, clusters, positions -- and hands each accumulator the product before it (the correlations
    run ``pxd_digits`` alone when the chain is off); like the parts it neither synchronises nor copies."""

    def __init__(self, clusters=False, maps=False, capacity=None, correlations=False, **kw):
        self.capacity, self.stats = capacity, PXDStatistics(**kw)
        self.clusters = PXDClusterStatistics(capacity=capacity, **kw) if clusters else None
        seed_cut, charge_cut = maps if isinstance(maps, (tuple, list)) else (0, 0)
        self.maps = PXDClusterMaps(seed_cut=seed_cut, charge_cut=charge_cut, capacity=capacity, **kw) if maps not in (False, None) else None
        regions = correlations if isinstance(correlations, (tuple, list)) else (1, 1)
        self.correlations = PXDCorrelations(regions=regions, capacity=capacity, **kw) if correlations not in (False, None) else None

    def update(self, images):
        x = _sensor_images(images, self.stats.n_sensors, "PXDValidation.update", self.stats.device)
        self.stats.update(x)
        if self.clusters is not None or self.maps is not None:
            c = pxd_clusters(x, self.stats.threshold, self.capacity, self.stats.n_sensors)
            for acc in filter(None, (self.clusters, self.maps, self.correlations)):
                acc.update(c)
        elif self.correlations is not None:
            self.correlations.update(x)

    def result(self):
        """``{"stats": ..., "clusters": ..., "maps": ..., "correlations": ...}``: the ``result()`` of every accumulator that is on."""
        return {part: getattr(self, part).result() for part, _, _ in _PARTS if getattr(self, part) is not None}


# the parts of a PXDValidation.result(): name, distance function, and the keys that are no table of their own beside the statistics'
_PARTS = (("stats", pxd_distance, ()), ("clusters", pxd_cluster_distance, ("n_events",)), ("maps", pxd_map_distance, ("n_events", "shape")),
          ("correlations", pxd_correlation_distance, ("n_events", "shape", "regions")))
# the tables of a part that would share a name with another part's: their name in pxd_validation_tables
_TABLE_NAMES = {("maps", "clusters"): "accepted_clusters", ("correlations", "counts"): "region_counts"}


def pxd_validation_distance(real, fake):
    """``pxd_distance``, ``pxd_cluster_distance``, ``pxd_map_distance`` and ``pxd_correlation_distance`` of the parts both
    ``PXDValidation.result()`` have, in one dict."""
    return {k: v for part, distance, _ in _PARTS if part in real and part in fake for k, v in distance(real[part], fake[part]).items()}


def pxd_validation_tables(**sides):
    """``pxd_validation_tables(real=r, fake=f)``: every table of each side's ``PXDValidation.result()`` as ``<side>_<name>``, part by part;
    the per-image ``clusters`` of the maps are ``<side>_accepted_clusters``, beside the cluster statistics' ``<side>_clusters``, and the
    per-event ``counts`` of the correlations are ``<side>_region_counts``."""
    return {f"{side}_{_TABLE_NAMES.get((part, k), k)}": np.asarray(v) for part, _, skip in _PARTS
            for side, res in sides.items() for k, v in res.get(part, {}).items() if k not in skip}


# the columns of the event file of ``produce.py`` / ``pack_events.py`` and their types: the events, then four columns of the digits
EVENT_COLUMNS = dict(event_offsets=np.int64, sensor=np.uint8, ucell=np.uint8, vcell=np.uint16, charge=np.uint8)
_digit_columns = lambda *columns: dict(zip(list(EVENT_COLUMNS)[1:], map(np.asarray, columns)))


def _load_event_file(path, columns=tuple(EVENT_COLUMNS)):
    """The arrays ``columns`` of an event file, after the check that it is one."""
    with np.load(path) as t:
        missing = [k for k in EVENT_COLUMNS if k not in t.files]
        if missing:
            raise ValueError(f"PXDEventStore: {path} is no event file of write_digits, it lacks {missing}")
        return [t[k] for k in columns]


def write_digits(path, event_offsets, sensor, ucell, vcell, charge):
    """The event file of ``produce.py`` (``.npz``): ``event_offsets`` int64 ``[events + 1]`` (the digits of event ``e`` are
    ``[event_offsets[e], event_offsets[e + 1])``), ``sensor`` uint8, ``ucell`` uint8, ``vcell`` uint16, ``charge`` uint8."""
    event_offsets = np.asarray(event_offsets, np.int64)
    cols = _digit_columns(sensor, ucell, vcell, charge)
    if event_offsets.ndim != 1 or event_offsets.size < 1 or event_offsets[0] != 0 or (np.diff(event_offsets) < 0).any():
        raise ValueError("write_digits: event_offsets must start at 0 and not decrease")
    for k, v in cols.items():
        if v.ndim != 1 or v.size != event_offsets[-1]:
            raise ValueError(f"write_digits: {k} has {v.size} entries, event_offsets ends at {event_offsets[-1]}")
    if cols["sensor"].size and (cols["sensor"].max() > 255 or cols["ucell"].max() > 255 or cols["vcell"].max() > 65535):
        raise ValueError("write_digits: a sensor / ucell / vcell value does not fit the file's uint8 / uint8 / uint16 columns")
    with open(path, "wb") as fh:
        np.savez(fh, event_offsets=event_offsets, **{k: v.astype(EVENT_COLUMNS[k]) for k, v in cols.items()})


def read_digits(path):
    """Yields the events of a ``produce.py`` file in the format ``create_g1.generate`` puts on its queue (create_g1.py:79, read by
    ``DigitCreator.event`` :105-106): ``((sensor, ucell, vcell) lists, charges list)``."""
    off, sensor, ucell, vcell, charge = _load_event_file(path)
    for e in range(off.size - 1):
        s = slice(int(off[e]), int(off[e + 1]))
        yield (sensor[s].tolist(), ucell[s].tolist(), vcell[s].tolist()), charge[s].tolist()


# ---------------------------------------------------------------------------------------------------------
# hits: positions of the accepted clusters in the local frame of their sensor, head-tail for wide clusters (csrc/pxd_hits.hip)
# ---------------------------------------------------------------------------------------------------------
class PXDGeometry:
    """The cell pitches of ``K`` sensor types as data: ``u_pitch`` int ``[K, H]`` (rows), ``v_pitch`` int ``[K, W]`` (columns) in integer
    geometry units of ``unit_mm`` mm (default 0.5 um, in which every nominal PXD pitch and half-pitch is an integer), and ``kind`` int ``[S]``,
    the type of every sensor (default: 40 sensors of type 0, valid only when ``K == 1``).

    Derived per type and axis: the doubled, centred cell centres ``x2[k] = 2 * sum(pitch[:k]) + pitch[k] - sum(pitch)`` -- twice the distance
    of the centre of cell ``k`` from the sensor centre, an integer even for odd pitches.  ``u_x2``, ``u_pitch``, ``v_x2``, ``v_pitch`` and
    ``kind`` are int32 NumPy arrays; ``tables(device)`` gives their device copies, uploaded once per device on first use.

    ``ValueError`` for a pitch outside ``1 .. 4095``, a total length ``sum(pitch) >= 2**20`` units, a ``kind`` outside ``0 .. K-1`` and shapes
    that disagree.  These bounds are what makes ``pxd_hits`` exact: ``|x2| < 2**20``, a cluster charge is below ``2**31`` (``H * W * 255 <
    2**31``, checked by the launchers), so a moment ``sum q * x2`` stays below ``2**51``, the head-tail numerator ``(x2[lo] + x2[hi]) * D + 2 *
    (q_tail * p[hi] - q_head * p[lo]) * (s - 2)`` below ``2**52 + 2**45`` and every product of the clamp comparison inside int64: numerator
    and denominator of a position convert to float64 without rounding."""

    def __init__(self, u_pitch, v_pitch, kind=None, unit_mm=5e-4):
        u, v = np.asarray(u_pitch), np.asarray(v_pitch)
        if u.ndim != 2 or v.ndim != 2 or u.shape[0] != v.shape[0] or 0 in u.shape + v.shape or u.dtype.kind not in "iu" or v.dtype.kind not in "iu":
            raise ValueError(f"PXDGeometry: u_pitch {u.shape} {u.dtype} / v_pitch {v.shape} {v.dtype} are not integer arrays [K, H] and [K, W]")
        u, v = u.astype(np.int64), v.astype(np.int64)
        if kind is None and u.shape[0] != 1:
            raise ValueError(f"PXDGeometry: {u.shape[0]} sensor types need a kind [S]")
        kind = np.zeros(40, np.int64) if kind is None else np.asarray(kind)
        if kind.ndim != 1 or kind.size == 0 or kind.dtype.kind not in "iu":
            raise ValueError(f"PXDGeometry: kind {kind.shape} {kind.dtype} is not an integer array [S]")
        for name, p in (("u_pitch", u), ("v_pitch", v)):
            if p.min() < 1 or p.max() > 4095:
                raise ValueError(f"PXDGeometry: {name} holds {int(p.min())} .. {int(p.max())}, outside 1 .. 4095")
            if p.sum(1).max() >= 2 ** 20:
                raise ValueError(f"PXDGeometry: a sensor is {int(p.sum(1).max())} units long along {name[0]}, not below 2**20")
        if kind.min() < 0 or kind.max() >= u.shape[0]:
            raise ValueError(f"PXDGeometry: kind holds {int(kind.min())} .. {int(kind.max())}, outside the {u.shape[0]} type(s)")
        x2 = lambda p: (2 * (np.cumsum(p, 1) - p) + p - p.sum(1, keepdims=True)).astype(np.int32)
        self.u_pitch, self.v_pitch, self.u_x2, self.v_x2 = u.astype(np.int32), v.astype(np.int32), x2(u), x2(v)
        self.kind, self.unit_mm, self._device = kind.astype(np.int32), float(unit_mm), {}
        self.K, self.H, self.W, self.S = u.shape[0], u.shape[1], v.shape[1], kind.size
        self.u_length, self.v_length = u.sum(1), v.sum(1)           # units, per type

    TABLES = ("u_x2", "u_pitch", "v_x2", "v_pitch", "kind")

    def tables(self, device):
        """The five int32 tables on ``device`` (dict by name); the upload happens once per device."""
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device) for k in self.TABLES}
        return self._device[device]

    @classmethod
    def uniform(cls, shape, u_pitch, v_pitch, n_sensors=40, unit_mm=5e-4):
        """One type, every cell ``u_pitch`` x ``v_pitch`` units, ``n_sensors`` sensors of ``shape = (H, W)`` cells."""
        Hh, Ww = shape
        return cls(np.full((1, Hh), int(u_pitch)), np.full((1, Ww), int(v_pitch)), np.zeros(int(n_sensors), np.int64), unit_mm)

    @classmethod
    def belle2(cls, shape=(250, 768), n_sensors=40):
        """The nominal Belle II PXD in units of 0.5 um: u pitch 50 um everywhere; v pitch fine on the cells 0 .. 255 and coarse on 256 .. 767
        -- 55 / 60 um on the sensors 0 .. 15 (layer 1, 12.5 x 44.8 mm sensitive), 70 / 85 um on the sensors 16 .. 39 (layer 2, 12.5 x 61.44 mm),
        the sensor order of the reference's ``create_g1.py:95``.  These are design values written down from memory: the reference holds no
        geometry, and neither they nor the end that carries the fine pitch have been checked against basf2.  Pass the true tables of the
        conditions database to ``PXDGeometry`` where it matters.  Only 250 x 768 cells and 40 sensors have this geometry."""
        if tuple(shape) != (250, 768) or int(n_sensors) != 40:
            raise ValueError(f"PXDGeometry.belle2: the PXD has 40 sensors of 250 x 768 cells, not {n_sensors} of {tuple(shape)}")
        v = np.array([[110] * 256 + [120] * 512, [140] * 256 + [170] * 512])
        return cls(np.full((2, 250), 100), v, np.array([0] * 16 + [1] * 24))


class PXDHits(_PXDProduct):
    """Device-side result of ``pxd_hits``: the ``PXDClusterPositions`` it came from (``positions``), the ``geometry`` and ``head_tail``; per
    cluster (row j of the table, the first ``clusters.total`` rows written) the physical moments ``pu`` / ``pv`` int64, the first column
    ``v_start`` int32 and the edge charges ``qh_u`` / ``qt_u`` / ``qh_v`` / ``qt_v`` int32; per accepted cluster, in the order of
    ``positions.cluster`` (the first ``total`` rows written), ``u`` / ``v`` fp32 in geometry units from the sensor centre and ``flags`` uint8
    (bit 0 / 1: u / v used head-tail, bit 2 / 3: u / v was clamped to the cluster's extent).  All ``[capacity]``; ``counts`` / ``total`` are
    those of the positions: the accepted clusters are the hits."""
    _again = lambda self, capacity: pxd_hits(self.images, self.geometry, self.head_tail, self.threshold, self.seed_cut, self.charge_cut, capacity,
                                             self.n_sensors)
    PER_CLUSTER, PER_HIT = ("pu", "pv", "v_start", "qh_u", "qt_u", "qh_v", "qt_v"), ("u", "v", "flags")

    def __init__(self, positions, geometry, head_tail, **arrays):
        self.positions, self.geometry, self.head_tail = positions, geometry, head_tail
        self.seed_cut, self.charge_cut = positions.seed_cut, positions.charge_cut
        vars(self).update(arrays)
        self._set_header(positions.header, positions)

    def cpu(self):
        """One read-back (``pxd_read_back``: one copy, one wait) -> dict of NumPy arrays trimmed to the true total, one entry per hit:
        ``cluster``, ``sensor``, ``event``, ``u``, ``v`` (fp32, geometry units), ``u_mm``, ``v_mm`` (float64: ``u.astype(float64) *
        unit_mm``), ``charge``, ``seed``, ``size``, ``size_u``, ``size_v``, ``u_start``, ``v_start`` (first row / column of the cluster),
        ``flags``; plus ``counts [N]``.  Never truncated (``_host_columns``)."""
        N, Hh, Ww = self.shape
        host = self._host_columns(lambda: dict(digit_header=self.positions.clusters.digits.header, header=self.header,
                                               cluster=self.positions.cluster, u=self.u, v=self.v, flags=self.flags, v_start=self.v_start,
                                               **{k: getattr(self.positions.clusters, k) for k in PXDClusters.TABLE}))
        total = int(host["header"][N])
        cluster = host["cluster"][:total].copy()
        image, rest = np.divmod(host["first"][cluster], np.int32(Hh * Ww))
        out = {k: host[k][:total].copy() for k in ("u", "v", "flags")}
        return dict(out, cluster=cluster, sensor=(image % self.n_sensors).astype(np.int32), event=(image // self.n_sensors).astype(np.int32),
                    u_mm=out["u"].astype(np.float64) * self.geometry.unit_mm, v_mm=out["v"].astype(np.float64) * self.geometry.unit_mm,
                    u_start=(rest // np.int32(Ww)).astype(np.int32), counts=host["header"][:N].copy(),
                    **{k: host[k][cluster] for k in ("charge", "seed", "size", "size_u", "size_v", "v_start")})


def pxd_hits(images_or_product, geometry, head_tail=3, threshold=0.0, seed_cut=0, charge_cut=0, capacity=None, n_sensors=40):
    """Hits of a batch of sensor images ``[N, H, W]`` (fp32 or uint8 device tensor: ``pxd_cluster_positions(images, threshold, seed_cut,
    charge_cut, capacity, n_sensors)`` runs first), of an existing ``PXDClusters`` (positions with the cuts run first) or of an existing
    ``PXDClusterPositions`` (its cuts, threshold, capacity and sensors hold): the position of every accepted cluster in the local frame of
    its sensor, origin at the sensor centre, in the integer units of ``geometry`` (a ``PXDGeometry``; ``PXDHits.cpu()`` scales to mm in
    float64).  This is the project's own statement of the head-tail form; agreement with basf2 is not claimed.  Along one axis a cluster of
    charge ``Q`` covers the cells ``lo .. hi`` (``s`` of them); ``x2`` / ``p`` are the doubled centres and pitches of its sensor's type:

    * ``s < head_tail`` (or ``head_tail == 0``: never head-tail; otherwise ``head_tail >= 3``): centre of gravity, ``num = sum q * x2[cell]``,
      ``den = 2 * Q``;
    * else head-tail with the charges ``q_head`` / ``q_tail`` in the cells ``lo`` / ``hi`` and ``D = Q - q_head - q_tail``:
      ``num = (x2[lo] + x2[hi]) * D + 2 * (q_tail * p[hi] - q_head * p[lo]) * (s - 2)``, ``den = 4 * D`` -- that is ``(x_lo + x_hi) / 2 +
      (q_tail * p_hi - q_head * p_lo) / (2 * q_centre)`` with ``q_centre = D / (s - 2)``;
    * the result is clamped, in integers, to ``[x2[lo] - p[lo], x2[hi] + p[hi]] / 2``: a hit lies inside its cluster's bounding box;
    * ``position = float32(float64(num) / float64(den))``: ``num`` and ``den`` are exact integers below 2^53 (``PXDGeometry``), so the same
      recipe on the host gives the same bits; bit-identical run to run.

    Position errors and signal-to-noise cuts (both need a per-pixel noise map) and a basf2 writer are out of scope; global coordinates are
    ``pxd_space_points``.
    Launches on the current stream, neither synchronises nor copies; with ``capacity`` given it can be captured into a HIP graph.  When the
    digit total exceeds the capacity the device result covers the first ``capacity`` digits; ``PXDHits.cpu()`` reruns instead of handing
    back a truncated event.  ``ValueError`` when the geometry's ``H``, ``W`` or ``S`` are not the batch's."""
    H.require_gpu()
    head_tail = int(head_tail)
    if head_tail != 0 and head_tail < 3:
        raise ValueError(f"pxd_hits: head_tail = {head_tail} is neither 0 (never) nor >= 3")
    if not isinstance(geometry, PXDGeometry):
        raise TypeError("pxd_hits: geometry must be a PXDGeometry")
    p = images_or_product
    if not isinstance(p, PXDClusterPositions):
        p = pxd_cluster_positions(p, threshold, seed_cut, charge_cut, capacity, n_sensors)
    c, d = p.clusters, p.clusters.digits
    N, Hh, Ww = p.shape
    if (geometry.H, geometry.W, geometry.S) != (Hh, Ww, p.n_sensors):
        raise ValueError(f"pxd_hits: the geometry has {geometry.S} sensors of {geometry.H} x {geometry.W} cells, the batch {p.n_sensors} of {Hh} x {Ww}")
    dev, C = p.cluster.device, p.capacity
    new = lambda dtype: torch.empty(C, dtype=dtype, device=dev)
    out = dict(pu=new(torch.int64), pv=new(torch.int64), **{k: new(torch.int32) for k in PXDHits.PER_CLUSTER[2:]}, u=new(torch.float32),
               v=new(torch.float32), flags=new(torch.uint8))
    t = geometry.tables(dev)
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_hits", *_ptrs(C, d.index, d.charge, c.label), d.total.data_ptr(), *_ptrs(C, c.first, c.charge, c.size_u, c.size_v),
               c.total.data_ptr(), *_ptrs(C, p.cluster), p.total.data_ptr(), *(t[k].data_ptr() for k in PXDGeometry.TABLES), N, Hh, Ww, p.n_sensors,
               geometry.K, C, head_tail, *_ptrs(C, *(out[k] for k in PXDHits.PER_CLUSTER + PXDHits.PER_HIT)), None, H.stream())
    return PXDHits(p, geometry, head_tail, **out)


# the columns of the hit file of ``produce.py --hits`` and their types: the events, then nine columns of the hits
HIT_COLUMNS = dict(event_offsets=np.int64, sensor=np.uint8, u_mm=np.float32, v_mm=np.float32, charge=np.int32, seed=np.uint8, size=np.uint16,
                   size_u=np.uint16, size_v=np.uint16, flags=np.uint8)


def write_hits(path, event_offsets, sensor, u_mm, v_mm, charge, seed, size, size_u, size_v, flags, unit_mm=5e-4):
    """The hit file of ``produce.py --hits`` (``.npz``): ``event_offsets`` int64 ``[events + 1]`` (the hits of event ``e`` are
    ``[event_offsets[e], event_offsets[e + 1])``), per hit ``sensor`` uint8, ``u_mm`` / ``v_mm`` float32 (local position from the sensor
    centre), ``charge`` int32, ``seed`` uint8, ``size`` / ``size_u`` / ``size_v`` uint16, ``flags`` uint8 (``PXDHits``), and the scalar
    ``unit_mm`` of the geometry the positions were computed in."""
    event_offsets = np.asarray(event_offsets, np.int64)
    cols = dict(zip(list(HIT_COLUMNS)[1:], map(np.asarray, (sensor, u_mm, v_mm, charge, seed, size, size_u, size_v, flags))))
    if event_offsets.ndim != 1 or event_offsets.size < 1 or event_offsets[0] != 0 or (np.diff(event_offsets) < 0).any():
        raise ValueError("write_hits: event_offsets must start at 0 and not decrease")
    for k, v in cols.items():
        if v.ndim != 1 or v.size != event_offsets[-1]:
            raise ValueError(f"write_hits: {k} has {v.size} entries, event_offsets ends at {event_offsets[-1]}")
    for k in ("sensor", "seed", "size", "size_u", "size_v", "flags") if event_offsets[-1] else ():
        if cols[k].min() < 0 or cols[k].max() > np.iinfo(HIT_COLUMNS[k]).max:
            raise ValueError(f"write_hits: a {k} value does not fit the file's {np.dtype(HIT_COLUMNS[k]).name} column")
    with open(path, "wb") as fh:
        np.savez(fh, event_offsets=event_offsets, unit_mm=np.float64(unit_mm), **{k: v.astype(HIT_COLUMNS[k]) for k, v in cols.items()})


def read_hits(path):
    """The arrays of a ``write_hits`` file as a dict: the ``HIT_COLUMNS`` and ``unit_mm`` (float)."""
    with np.load(path) as t:
        missing = [k for k in list(HIT_COLUMNS) + ["unit_mm"] if k not in t.files]
        if missing:
            raise ValueError(f"read_hits: {path} is no hit file of write_hits, it lacks {missing}")
        return dict({k: t[k] for k in HIT_COLUMNS}, unit_mm=float(t["unit_mm"]))


# ---------------------------------------------------------------------------------------------------------
# sparse event store: the events of a digit file resident on the device, expanded into the network input (csrc/pxd_events.hip)
# ---------------------------------------------------------------------------------------------------------
def _event_of(event_offsets, k):
    """The event that holds digit ``k``."""
    return int(np.searchsorted(event_offsets, k, side="right") - 1)


def event_columns(event_offsets, sensor, ucell, vcell, charge, shape=(250, 768), n_sensors=40, who="PXDEventStore"):
    """The host half of ``PXDEventStore``: the columns of an event file -> ``(offsets int64 [events + 1], pos int32 [D], charge uint8 [D])``
    with ``pos = (sensor * H + ucell) * W + vcell``, after every check of the store's contract, in NumPy and without a device call.
    ``ValueError`` -- naming the first offending event -- for offsets that do not start at 0 or decrease, column lengths that disagree, a
    sensor / ucell / vcell outside the geometry, a charge of 0, and positions that are not strictly ascending inside an event (unsorted or
    duplicate digits)."""
    Hh, Ww = (int(v) for v in shape)
    S = int(n_sensors)
    if S <= 0 or Hh <= 0 or Ww <= 0 or S * Hh * Ww >= 2 ** 31:
        raise ValueError(f"{who}: {S} sensors of {Hh} x {Ww} pixels are no geometry whose positions fit int32")
    off = np.asarray(event_offsets)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"{who}: event_offsets must be a 1-D integer array of events + 1 entries")
    off = off.astype(np.int64)
    if off[0] != 0:
        raise ValueError(f"{who}: event_offsets starts at {off[0]}, not at 0")
    down = np.nonzero(np.diff(off) < 0)[0]
    if down.size:
        raise ValueError(f"{who}: event_offsets decreases at event {int(down[0])} ({off[down[0]]} -> {off[down[0] + 1]})")
    cols = _digit_columns(sensor, ucell, vcell, charge)
    for k, v in cols.items():
        if v.ndim != 1 or v.size != off[-1]:
            raise ValueError(f"{who}: {k} has {v.size} entries, event_offsets ends at {off[-1]}")
        if v.size and not np.issubdtype(v.dtype, np.integer):
            raise ValueError(f"{who}: {k} is {v.dtype}, not an integer column")
    for k, limit in (("sensor", S), ("ucell", Hh), ("vcell", Ww)):
        bad = np.nonzero((cols[k] < 0) | (cols[k] >= limit))[0]
        if bad.size:
            raise ValueError(f"{who}: event {_event_of(off, bad[0])}: {k} = {int(cols[k][bad[0]])} of digit {int(bad[0])} is outside 0 .. {limit - 1}")
    bad = np.nonzero((cols["charge"] <= 0) | (cols["charge"] > 255))[0]
    if bad.size:
        raise ValueError(f"{who}: event {_event_of(off, bad[0])}: charge = {int(cols['charge'][bad[0]])} of digit {int(bad[0])} is outside 1 .. 255")
    pos = ((cols["sensor"].astype(np.int64) * Hh + cols["ucell"]) * Ww + cols["vcell"]).astype(np.int32)
    if pos.size > 1:
        step = np.diff(pos) <= 0
        starts = off[1:-1]
        step[starts[(starts > 0) & (starts < pos.size)] - 1] = False          # the first digit of an event follows nothing
        bad = np.nonzero(step)[0]
        if bad.size:
            k = int(bad[0]) + 1
            raise ValueError(f"{who}: event {_event_of(off, k)}: digit {k} (position {int(pos[k])}) does not lie behind digit {k - 1} (position "
                             f"{int(pos[k - 1])}): the digits of an event must be sorted by (sensor, ucell, vcell) without duplicates")
    return off, pos, cols["charge"].astype(np.uint8)


def select_events(event_offsets, events, *columns):
    """``(offsets, *columns)`` of the events ``events`` (numbers into ``event_offsets``, any order, repeats allowed) of a digit list."""
    off = np.asarray(event_offsets, np.int64)
    ev = np.asarray(events, np.int64).reshape(-1)
    if ev.size and (ev.min() < 0 or ev.max() >= off.size - 1):
        raise ValueError(f"PXDEventStore: events= holds {int(ev.min())} .. {int(ev.max())}, the file has {off.size - 1} events")
    counts = (off[1:] - off[:-1])[ev]
    new = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    take = np.repeat(off[:-1][ev] - new[:-1], counts) + np.arange(new[-1], dtype=np.int64)
    return (new,) + tuple(np.asarray(c)[take] for c in columns)


def read_event_columns(path, shape=(250, 768), n_sensors=40, events=None):
    """The host half of ``PXDEventStore.from_file``: the file of ``write_digits`` -> checked ``(offsets, pos, charge)`` of ``event_columns``,
    of all events or of the subset ``events``."""
    off, pos, charge = event_columns(*_load_event_file(path), shape, n_sensors, who=f"PXDEventStore ({path})")
    return (off, pos, charge) if events is None else select_events(off, events, pos, charge)


def split_positions(pos, shape=(250, 768)):
    """Positions of a store -> the ``(sensor, ucell, vcell)`` columns of the event file."""
    Hh, Ww = shape
    s, rest = np.divmod(np.asarray(pos, np.int64), Hh * Ww)
    u, v = np.divmod(rest, Ww)
    return s, u, v


def event_file_length(path):
    """Number of events in a file of ``write_digits`` (reads the offsets only)."""
    return int(_load_event_file(path, ("event_offsets",))[0].size - 1)


class PXDEventStore:
    """Events of sparse PXD digits resident on the device: ``pos`` int32 ``[D]`` (``(sensor * H + ucell) * W + vcell``, strictly ascending
    inside an event), ``charge`` uint8 ``[D]``, ``offsets`` int64 ``[events + 1]`` -- about 5 bytes a digit, 0.4 MB for a 40 x 250 x 768 event at
    1 % occupancy against 7.7 MB dense.  ``ingest`` / ``dense`` expand E events in one HIP launch (csrc/pxd_events.hip) on the current
    stream: no file read, no host-to-device copy and, with a device id tensor, no synchronisation.  Build one with ``from_file`` (the
    ``produce.py`` / ``write_digits`` format), ``from_arrays`` or ``from_dense``; every check of the contract runs on the host before the
    upload (``event_columns``)."""

    def __init__(self, offsets, pos, charge, shape=(250, 768), n_sensors=40, device=None):
        """Checked host columns (``event_columns``) -> the device.  Use the ``from_*`` constructors."""
        if device is not None and torch.device(device).type != "cuda":
            raise RuntimeError(f"PXDEventStore lives on a HIP device, not on {device}: there is no CPU path")
        H.require_gpu()
        self.shape, self.n_sensors = (int(shape[0]), int(shape[1])), int(n_sensors)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        offsets = np.ascontiguousarray(offsets, np.int64)
        self.counts = np.diff(offsets)
        self.offsets = torch.from_numpy(offsets).to(self.device)
        self.pos = torch.from_numpy(np.ascontiguousarray(pos, np.int32)).to(self.device)
        self.charge = torch.from_numpy(np.ascontiguousarray(charge, np.uint8)).to(self.device)

    @classmethod
    def from_arrays(cls, event_offsets, sensor, ucell, vcell, charge, shape=(250, 768), n_sensors=40, device=None):
        return cls(*event_columns(event_offsets, sensor, ucell, vcell, charge, shape, n_sensors), shape, n_sensors, device)

    @classmethod
    def from_file(cls, path, shape=(250, 768), n_sensors=40, events=None, device=None):
        """The event file of ``produce.py`` / ``write_digits``; ``events``: the event numbers to keep (a rank's shard), chosen before the upload."""
        return cls(*read_event_columns(path, shape, n_sensors, events), shape, n_sensors, device)

    @classmethod
    def from_dense(cls, events, n_sensors=40, device=None):
        """Dense uint8 events (arrays or tensors ``[k * n_sensors, H, W]``, or ``*.npy`` paths) -> a store.  Every item goes through
        ``pxd_digits`` (threshold 0: every nonzero charge), so it is compacted on the device and only its digits are kept."""
        if isinstance(events, (str, np.ndarray, torch.Tensor)):
            events = [events]
        pos, charge, counts, shape = [], [], [], None
        for ev in events:
            name = ev if isinstance(ev, str) else "<array>"
            ev = np.load(ev) if isinstance(ev, str) else ev
            x = ev if isinstance(ev, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ev))
            if x.dtype != torch.uint8 or x.dim() != 3:
                raise TypeError(f"PXDEventStore.from_dense: {name} is {tuple(x.shape)} {x.dtype}, not uint8 [k * n_sensors, H, W]")
            if shape not in (None, tuple(x.shape[1:])):
                raise ValueError(f"PXDEventStore.from_dense: {name} has images of {tuple(x.shape[1:])}, the events before it of {shape}")
            shape = tuple(x.shape[1:])
            if device is not None and not x.is_cuda:
                x = x.to(device)
            index, chg, cnt = pxd_digits(x, threshold=0.0, n_sensors=n_sensors).cpu()
            per = int(n_sensors) * shape[0] * shape[1]
            pos.append((index.astype(np.int64) % per).astype(np.int32))
            charge.append(chg)
            counts.append(cnt.reshape(-1, int(n_sensors)).sum(1))
        if shape is None:
            raise ValueError("PXDEventStore.from_dense: no events")
        offsets = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
        return cls(offsets, np.concatenate(pos), np.concatenate(charge), shape, n_sensors, device)

    @classmethod
    def _from_device(cls, counts, offsets, pos, charge, shape, n_sensors):
        """A store over tensors that are on the device already (``offsets`` int64 ``[events + 1]``, ``pos`` int32, ``charge`` uint8) and the
        host copy of the digits per event, ``counts``; the caller vouches for the store's contract.  Nothing is copied."""
        self = cls.__new__(cls)
        self.shape, self.n_sensors, self.device = (int(shape[0]), int(shape[1])), int(n_sensors), offsets.device
        self.counts, self.offsets, self.pos, self.charge = np.asarray(counts, np.int64), offsets, pos, charge
        return self

    @classmethod
    def from_digits(cls, digits):
        """The ``PXDDigits`` of a batch of whole events (``pxd_digits`` of generated or recorded images) -> a store of those events, made on
        the device: ``pos = index % (S * H * W)``, the charges as they stand (a view of the digits' tensor), the offsets from the counts
        summed per event.  The one read-back is the digit header (``counts``, ``total``: 4 bytes an image), which also triggers the usual
        rerun with ``capacity = total`` when the digits did not fit; no digit crosses PCIe.  ``ValueError`` for digits made with a negative
        threshold (with ``threshold >= 0`` every charge of ``pxd_digits`` is in 1 .. 255 and the positions ascend strictly: the store's
        contract holds by construction)."""
        if not isinstance(digits, PXDDigits):
            raise TypeError("PXDEventStore.from_digits takes the PXDDigits of pxd_digits")
        if not digits.threshold >= 0:
            raise ValueError(f"PXDEventStore.from_digits: the digits were made with threshold = {digits.threshold}, not >= 0")
        (N, Hh, Ww), S = digits.shape, digits.n_sensors
        header = pxd_read_back(header=digits.header)["header"]
        total = int(header[N])
        if total > digits.capacity:
            digits._grow(total)
        with torch.cuda.device(digits.header.device):
            pos = torch.remainder(digits.index[:total], S * Hh * Ww)
            per_event = digits.counts.view(-1, S).sum(1, dtype=torch.int64)
            offsets = torch.cat([per_event.new_zeros(1), torch.cumsum(per_event, 0)])
        return cls._from_device(header[:N].reshape(-1, S).sum(1), offsets, pos, digits.charge[:total], (Hh, Ww), S)

    def overlay(self, event_ids, other, other_ids=None, capacity=None):
        """The events ``event_ids`` of this store with the events ``other_ids`` (default: the same numbers) of ``other`` laid over them, as a
        new store: ``pxd_overlay(self, event_ids, other, other_ids, capacity).store()``."""
        return pxd_overlay(self, event_ids, other, other_ids, capacity).store()

    def __len__(self):
        return int(self.counts.size)

    @property
    def nbytes(self):
        """Bytes the store holds on the device."""
        return int(self.pos.numel() * 4 + self.charge.numel() + self.offsets.numel() * 8)

    def columns(self):
        """NumPy ``(event_offsets, sensor, ucell, vcell, charge)``: the columns of the event file (one read-back)."""
        s, u, v = split_positions(self.pos.cpu().numpy(), self.shape)
        return self.offsets.cpu().numpy(), s, u, v, self.charge.cpu().numpy()

    def save(self, path):
        """Writes the store as an event file (``write_digits``)."""
        write_digits(path, *self.columns())

    def _ids(self, event_ids, who):
        """``event_ids`` -> int32 device tensor ``[E]``.  An int or a sequence is range-checked here and uploaded; an int32 tensor on the store's
        device is taken as it is -- nothing crosses PCIe, nothing synchronises, and an id outside the store then gives an empty event."""
        if isinstance(event_ids, torch.Tensor) and event_ids.is_cuda:
            if event_ids.dtype != torch.int32 or event_ids.dim() != 1 or event_ids.device != self.device:
                raise TypeError(f"{who}: a device id tensor must be int32 [E] on {self.device}, got {event_ids.dtype} "
                                f"{tuple(event_ids.shape)} on {event_ids.device}")
            ids = event_ids.contiguous()
        else:
            host = np.asarray(event_ids.numpy() if isinstance(event_ids, torch.Tensor) else event_ids)
            if host.dtype.kind not in "iu" or host.ndim > 1:
                raise TypeError(f"{who}: event_ids must be an int, a sequence of ints or an int32 device tensor")
            host = host.reshape(-1).astype(np.int64)
            if host.size and (host.min() < 0 or host.max() >= len(self)):
                raise IndexError(f"{who}: event ids {int(host.min())} .. {int(host.max())} outside the store's 0 .. {len(self) - 1}")
            ids = torch.from_numpy(host.astype(np.int32)).to(self.device)
        E = int(ids.numel())
        if E == 0 or E * self.n_sensors > 65535:
            raise ValueError(f"{who}: {E} event(s) of {self.n_sensors} sensors: one call takes 1 .. {65535 // self.n_sensors} events")
        return ids, E

    def _store_args(self, ids, E):
        return (H.ptr(self.pos) or None, H.ptr(self.charge) or None, self.offsets.data_ptr(), int(self.pos.numel()), len(self), ids.data_ptr(), E,
                self.n_sensors, self.shape[0], self.shape[1])

    def ingest(self, event_ids, noise=None, scale=4e-3, pad=3):
        """The network input of the events ``event_ids``: fp32 ``[E * n_sensors, 1, H + 2*pad, W]``, bit for bit what ``utils.ingest_event``
        gives on their dense uint8 images.  ``noise`` as there: explicit U[0,1) draws ``[E * n_sensors, H + 2*pad, W]``; None = drawn on the
        device; False = no dequantisation noise."""
        ids, E = self._ids(event_ids, "PXDEventStore.ingest")
        pad = int(pad)
        if pad < 0:
            raise ValueError("PXDEventStore.ingest: pad is negative")
        N, (Hh, Ww) = E * self.n_sensors, self.shape
        with torch.cuda.device(self.device):
            out = torch.empty(N, 1, Hh + 2 * pad, Ww, dtype=torch.float32, device=self.device)
            if noise is None:
                noise = torch.rand(N, Hh + 2 * pad, Ww, device=self.device)
            elif noise is False:
                noise = None
            else:
                noise = noise.to(self.device, torch.float32).contiguous()
                if noise.numel() != out.numel():
                    raise ValueError("noise must have the padded shape [E * n_sensors, H + 2*pad, W]")
            H.call("ieagan_pxd_event_ingest", *self._store_args(ids, E), pad, H.ptr(noise), float(scale), out.data_ptr(), H.stream())
        return out

    def dense(self, event_ids):
        """The dense uint8 images ``[E * n_sensors, H, W]`` of the events ``event_ids``: the input of every ``PXD*`` accumulator."""
        ids, E = self._ids(event_ids, "PXDEventStore.dense")
        with torch.cuda.device(self.device):
            out = torch.empty(E * self.n_sensors, *self.shape, dtype=torch.uint8, device=self.device)
            H.call("ieagan_pxd_event_dense", *self._store_args(ids, E), out.data_ptr(), H.stream())
        return out


# ---------------------------------------------------------------------------------------------------------
# background overlay: the events of two stores added pixel by pixel, in the sparse format (csrc/pxd_overlay.hip)
# ---------------------------------------------------------------------------------------------------------
def _n_ids(ids):
    """The number of event ids in what ``PXDEventStore._ids`` takes, found on the host."""
    return int(ids.numel()) if isinstance(ids, torch.Tensor) else int(np.asarray(ids).size)


class PXDOverlay:
    """Device-side result of ``pxd_overlay``: ``pos`` int32 ``[capacity]``, ``charge`` uint8 ``[capacity]`` -- the merged events back to back,
    only the first ``min(total, capacity)`` digits written -- and ``offsets`` int64 ``[E + 1]``, the start of every merged event and the
    total, the true numbers whatever the capacity; plus ``capacity``, ``shape`` and ``n_sensors``."""

    def __init__(self, a, a_ids, b, b_ids, capacity, pos, charge, offsets):
        self._pairs = (a, a_ids, b, b_ids)          # the stores and the ids as the caller gave them
        self.capacity, self.shape, self.n_sensors = capacity, a.shape, a.n_sensors
        self.pos, self.charge, self.offsets, self._host = pos, charge, offsets, None

    def _host_offsets(self):
        """``offsets`` on the host: one ``pxd_read_back`` (8 * (E + 1) bytes, one wait), kept.  When the total exceeds the capacity the overlay
        is run again with ``capacity = total`` and adopted (a second read-back, on that path only): the host never sees a truncated event."""
        if self._host is None:
            host = pxd_read_back(offsets=self.offsets)["offsets"]
            if host[-1] > self.capacity:
                a, a_ids, b, b_ids = self._pairs
                again = pxd_overlay(a, a_ids, b, b_ids, int(host[-1]))
                self.capacity, self.pos, self.charge, self.offsets = again.capacity, again.pos, again.charge, again.offsets
                host = pxd_read_back(offsets=self.offsets)["offsets"]
            self._host = host
        return self._host

    def store(self):
        """The merged events as a ``PXDEventStore`` over the first ``total`` digits: the offsets are read back (``_host_offsets``) and give
        the new store's ``counts``; the digits stay where they are, none goes through the host."""
        host = self._host_offsets()
        total = int(host[-1])
        return PXDEventStore._from_device(np.diff(host), self.offsets, self.pos[:total], self.charge[:total], self.shape, self.n_sensors)

    def shared(self):
        """int64 ``[E]``: the pixels of every pair that held a digit in both events, ``na + nb - n_out``, on the host from the three count
        arrays (device ids are read back for it; an id outside its store counts no digit)."""
        out = np.diff(self._host_offsets())
        a, a_ids, b, b_ids = self._pairs
        n = 0
        for store, ids in ((a, a_ids), (b, b_ids)):
            ids = (ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)).reshape(-1).astype(np.int64)
            inside = (ids >= 0) & (ids < len(store))
            n = n + np.where(inside, store.counts[np.where(inside, ids, 0)] if len(store) else 0, 0)
        return (n - out).astype(np.int64)


def pxd_overlay(a, a_ids, b, b_ids=None, capacity=None):
    """Overlay of sparse events on the device (csrc/pxd_overlay.hip): merged event ``e`` holds every pixel that is a digit in event
    ``a_ids[e]`` of the store ``a`` or in event ``b_ids[e]`` (default: ``a_ids[e]``) of the store ``b``, in ascending position; a pixel of
    one event keeps its charge, a pixel of both gets ``min(qa + qb, 255)``, the ADC's saturation -- what the clamped sum of the dense images
    gives, without a dense image.  Ids as everywhere in ``PXDEventStore``: host ids are range-checked, an int32 device tensor is taken as it
    is and an id outside its store is an empty event.

    ``capacity`` (digits of the result) defaults, with host ids, to the digits of all the events named, a bound the host knows; with a
    device id tensor on either side it must be given.  Launches on the current stream, neither synchronises nor copies; with device ids it
    can be captured into a HIP graph.  ``offsets`` of the returned ``PXDOverlay`` always holds the true numbers; its ``store()`` reruns with a
    larger capacity instead of truncating.  ``ValueError`` when the stores differ in ``shape``, ``n_sensors`` or ``device``, when the id lists
    differ in length and for a missing or negative capacity."""
    if not isinstance(a, PXDEventStore) or not isinstance(b, PXDEventStore):
        raise TypeError("pxd_overlay: a and b must be PXDEventStores")
    for k in ("shape", "n_sensors", "device"):
        if getattr(a, k) != getattr(b, k):
            raise ValueError(f"pxd_overlay: the stores differ in {k}: {getattr(a, k)} and {getattr(b, k)}")
    if b_ids is None:
        b_ids = a_ids
    if _n_ids(a_ids) != _n_ids(b_ids):
        raise ValueError(f"pxd_overlay: {_n_ids(a_ids)} ids into a, {_n_ids(b_ids)} into b")
    on_device = any(isinstance(i, torch.Tensor) and i.is_cuda for i in (a_ids, b_ids))
    if capacity is None and on_device:
        raise ValueError("pxd_overlay: with a device id tensor the host does not know the events, capacity= is required")
    if capacity is not None and int(capacity) < 0:
        raise ValueError("pxd_overlay: capacity is negative")
    H.require_gpu()
    ia, E = a._ids(a_ids, "pxd_overlay (a_ids)")
    ib, _ = b._ids(b_ids, "pxd_overlay (b_ids)")
    if capacity is None:
        capacity = sum(int(s.counts[np.asarray(i, np.int64).reshape(-1)].sum()) for s, i in ((a, a_ids), (b, b_ids)) if len(s))
    capacity = int(capacity)
    dev = a.device
    with torch.cuda.device(dev):
        pos = torch.empty(capacity, dtype=torch.int32, device=dev)
        charge = torch.empty(capacity, dtype=torch.uint8, device=dev)
        offsets = torch.empty(E + 1, dtype=torch.int64, device=dev)
        scratch = torch.empty(H.lib().ieagan_pxd_event_overlay_scratch(E, capacity), dtype=torch.int32, device=dev)
        H.call("ieagan_pxd_event_overlay", *a._store_args(ia, E)[:6], *b._store_args(ib, E)[:6], E, a.n_sensors, a.shape[0], a.shape[1], capacity,
               *_ptrs(capacity, pos, charge), offsets.data_ptr(), scratch.data_ptr(), H.stream())
    return PXDOverlay(a, a_ids, b, b_ids, capacity, pos, charge, offsets)


# ---------------------------------------------------------------------------------------------------------
# signal-hit matching under background: what became of every signal hit once background lay over it (csrc/pxd_match.hip)
# ---------------------------------------------------------------------------------------------------------
PXD_MATCHED, PXD_CHANGED, PXD_SHARED = 1, 2, 4          # the bits of ``PXDMatch.flags``
PXD_RESIDUAL_BINS, PXD_PURITY_BINS = 64, 32


def _same_geometry(a, b):
    return a is b or (isinstance(a, PXDGeometry) and isinstance(b, PXDGeometry) and a.unit_mm == b.unit_mm and
                      all(np.array_equal(getattr(a, k), getattr(b, k)) for k in PXDGeometry.TABLES))


def _check_match_sides(signal, mixed, who="pxd_match"):
    """Both sides are ``PXDHits`` made the same way over batches of the same shape on one device, or ``TypeError`` / ``ValueError``."""
    if not isinstance(signal, PXDHits) or not isinstance(mixed, PXDHits):
        raise TypeError(f"{who}: signal and mixed must be the PXDHits of pxd_hits")
    for k in ("shape", "n_sensors", "threshold", "seed_cut", "charge_cut", "head_tail"):
        if getattr(signal, k) != getattr(mixed, k):
            raise ValueError(f"{who}: the two PXDHits differ in {k}: {getattr(signal, k)} and {getattr(mixed, k)}")
    if not _same_geometry(signal.geometry, mixed.geometry):
        raise ValueError(f"{who}: the two PXDHits differ in geometry")
    if signal.header.device != mixed.header.device:
        raise ValueError(f"{who}: the two PXDHits differ in device: {signal.header.device} and {mixed.header.device}")


class PXDMatch:
    """Device-side result of ``pxd_match``: the two ``PXDHits`` (``signal``, ``mixed``); per signal cluster (row j of the signal table, the
    first ``signal.positions.clusters.total`` rows written) ``found`` / ``lo`` / ``hi`` int32 ``[signal.capacity]``; per mixed cluster
    ``signal_size`` / ``signal_charge`` / ``n_signal`` int32 ``[mixed.capacity]``; per signal hit, in the order of
    ``signal.positions.cluster`` (the first ``signal.total`` rows written), ``mixed_hit`` int32, ``flags`` uint8 (``PXD_MATCHED``,
    ``PXD_CHANGED``, ``PXD_SHARED``), ``du`` / ``dv`` fp32 in geometry units.  ``header`` / ``counts`` / ``total`` are those of the signal
    hits: the product has one row per signal hit."""
    PER_SIGNAL_CLUSTER, PER_MIXED_CLUSTER, PER_HIT = ("found", "lo", "hi"), ("signal_size", "signal_charge", "n_signal"), ("mixed_hit", "flags", "du", "dv")

    def __init__(self, signal, mixed, **arrays):
        self.signal, self.mixed = signal, mixed
        self.shape, self.n_sensors, self.geometry = signal.shape, signal.n_sensors, signal.geometry
        self.header, self.counts, self.total = signal.header, signal.counts, signal.total
        vars(self).update(arrays)

    def _columns(self):
        s, m = self.signal, self.mixed
        sc, mc = s.positions.clusters, m.positions.clusters
        return dict(digit_header=sc.digits.header, mixed_digit_header=mc.digits.header, header=s.header, cluster_header=sc.header,
                    mixed_cluster_header=mc.header, cluster=s.positions.cluster, first=sc.first, size=sc.size, charge=sc.charge,
                    mixed_charge=mc.charge, **{k: getattr(self, k) for k in self.PER_SIGNAL_CLUSTER + self.PER_MIXED_CLUSTER + self.PER_HIT})

    def cpu(self):
        """One read-back (``pxd_read_back``: one copy, one wait) -> dict of NumPy arrays trimmed to the true totals, one entry per signal
        hit: ``cluster`` (row of the signal table), ``sensor``, ``event``, ``mixed_hit``, ``flags``, ``du``, ``dv`` (fp32, geometry units),
        ``du_mm``, ``dv_mm`` (float64: ``du.astype(float64) * unit_mm``), ``found``, ``size``, ``charge`` (of the signal cluster),
        ``match`` and ``hi`` (its smallest and largest mixed cluster, -1: none) and, of the mixed cluster ``match`` (0 where there is
        none), ``mixed_charge``, ``signal_charge``, ``signal_size``, ``n_signal``; plus ``counts [N]``.  Never truncated: when a side's
        digit total exceeds its capacity that side is grown and the match run again (a second read-back, on that path only)."""
        N, Hh, Ww = self.shape
        host = pxd_read_back(**self._columns())
        grown = False
        for side, key in ((self.signal, "digit_header"), (self.mixed, "mixed_digit_header")):
            if host[key][N] > side.capacity:
                side._grow(int(host[key][N]))
                grown = True
        if grown:
            vars(self).update(vars(pxd_match(self.signal, self.mixed)))
            host = pxd_read_back(**self._columns())
        total = int(host["header"][N])
        cluster = host["cluster"][:total].copy()
        image = host["first"][cluster] // np.int32(Hh * Ww)
        out = {k: host[k][:total].copy() for k in self.PER_HIT}
        match = host["lo"][cluster]
        ok, k = match >= 0, np.maximum(match, 0)
        of_match = lambda a: np.where(ok, a[k], 0).astype(a.dtype) if a.size else np.zeros(total, a.dtype)
        return dict(out, cluster=cluster, sensor=(image % self.n_sensors).astype(np.int32), event=(image // self.n_sensors).astype(np.int32),
                    du_mm=out["du"].astype(np.float64) * self.geometry.unit_mm, dv_mm=out["dv"].astype(np.float64) * self.geometry.unit_mm,
                    match=match, counts=host["header"][:N].copy(), **{k: host[k][cluster] for k in ("found", "hi", "size", "charge")},
                    **{k: of_match(host[k]) for k in ("mixed_charge", "signal_charge", "signal_size", "n_signal")})


def pxd_match(signal, mixed):
    """What became of every signal hit once background was laid over it (csrc/pxd_match.hip).  ``signal`` and ``mixed`` are the ``PXDHits``
    of two batches of the same ``[N, H, W]``, made with the same sensors, threshold, cuts, ``head_tail`` and geometry on one device; in the
    intended use ``mixed`` comes from the signal events with background laid over them (``PXDEventStore.overlay``), but the rule holds
    for any two batches.  The join is pixel identity, in integers: a signal digit is *found* when its flat index is a mixed digit, ``L`` is
    then that digit's mixed cluster.

    * per signal cluster ``found`` (its found digits) and ``lo`` / ``hi`` (smallest / largest ``L``, -1 when nothing was found); ``lo`` is
      the match.  For a true overlay ``found == size`` and ``lo == hi``: a connected set stays connected in a superset;
    * per mixed cluster ``signal_size`` / ``signal_charge`` (number and summed signal charge of the signal digits found in it, at most the
      mixed charge) and ``n_signal`` (signal clusters matched to it);
    * per signal hit ``mixed_hit`` (row of the mixed hit of the matched cluster, or -1), ``flags`` -- ``PXD_MATCHED``: every digit found in
      one mixed cluster that is itself a hit; ``PXD_CHANGED``: matched, and the mixed cluster's size or charge differs; ``PXD_SHARED``:
      ``n_signal >= 2`` -- and ``du`` / ``dv`` = ``float32(float64(x_mixed) - float64(x_signal))`` in geometry units, 0 when not matched
      and exactly 0 when matched and unchanged.

    Integer atomics only: bit-identical run to run.  Launches on the current stream, neither synchronises nor copies, and can be captured
    into a HIP graph.  When a side's digit total exceeds its capacity the device result covers the digits that fit; ``PXDMatch.cpu()``
    reruns instead of handing back a truncated event.  Track-level quantities, time windows and a match by anything other than pixel
    identity are out of scope.  ``ValueError`` when the two sides differ in shape, sensors, threshold, cuts, ``head_tail``, geometry or device."""
    _check_match_sides(signal, mixed)
    H.require_gpu()
    s, m = signal, mixed
    sp, sc, sd = s.positions, s.positions.clusters, s.positions.clusters.digits
    mp, mc, md = m.positions, m.positions.clusters, m.positions.clusters.digits
    (N, Hh, Ww), dev, Cs, Cm = s.shape, s.header.device, s.capacity, m.capacity
    new = lambda n, dtype=torch.int32: torch.empty(n, dtype=dtype, device=dev)
    out = dict({k: new(Cs) for k in PXDMatch.PER_SIGNAL_CLUSTER}, **{k: new(Cm) for k in PXDMatch.PER_MIXED_CLUSTER}, mixed_hit=new(Cs),
               flags=new(Cs, torch.uint8), du=new(Cs, torch.float32), dv=new(Cs, torch.float32))
    scratch = new(H.lib().ieagan_pxd_match_scratch(N, Hh, Ww, Cm))
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_match", *_ptrs(Cs, sd.index, sd.charge, sc.label), sd.total.data_ptr(), *_ptrs(Cs, sc.size, sc.charge),
               sc.total.data_ptr(), *_ptrs(Cs, sp.cluster), sp.total.data_ptr(), *_ptrs(Cs, s.u, s.v), *_ptrs(Cm, md.index, mc.label),
               md.total.data_ptr(), *_ptrs(Cm, mc.size, mc.charge), mc.total.data_ptr(), *_ptrs(Cm, mp.cluster), mp.total.data_ptr(),
               *_ptrs(Cm, m.u, m.v), N, Hh, Ww, Cs, Cm, *_ptrs(Cs, *(out[k] for k in PXDMatch.PER_SIGNAL_CLUSTER)),
               *_ptrs(Cm, *(out[k] for k in PXDMatch.PER_MIXED_CLUSTER)), *_ptrs(Cs, *(out[k] for k in PXDMatch.PER_HIT)),
               *_ptrs(Cm, scratch), H.stream())
    return PXDMatch(s, m, **out)


class PXDMatchStatistics(_PXDAccumulator):
    """Accumulator of the per-sensor fate of the signal hits over batches, beside the other ``PXD*`` accumulators: ``update(signal_hits,
    mixed_hits)`` runs ``pxd_match`` and ``ieagan_pxd_match_stats`` on the current stream, ``update(match)`` with an existing ``PXDMatch``
    launches the statistics kernel alone; neither synchronises nor copies, ``result()`` does the single read-back.  Counters are exact
    int64.  An update in which a side's digit total exceeds the capacity of its ``PXDHits`` is counted on the device and makes ``result()``
    raise: a truncated event is never reported.  ``residual_bin``: the width of a residual bin in geometry units (default 10 = 5 um with the
    default unit).  ``tables``: int64 ``[S * 165 + 1]`` on the device, the rows of the sensors, then the overflow counter."""
    _table, _per_image, _overflow = "tables", ("hits",), False       # the overflow word is refused in result(), with this class's own text

    def __init__(self, n_sensors=40, residual_bin=10, device=None):
        self.residual_bin = int(residual_bin)
        if self.residual_bin < 1:
            raise ValueError(f"PXDMatchStatistics: residual_bin = {residual_bin} is not >= 1")
        super().__init__(n_sensors, 0.0, None, device)
        self.threshold, self.unit_mm = None, None          # the threshold is that of the hits, whatever it is

    def update(self, signal_or_match, mixed=None):
        if isinstance(signal_or_match, PXDMatch):
            if mixed is not None:
                raise TypeError("PXDMatchStatistics.update: a PXDMatch holds both sides, mixed= must be left out")
            mt = signal_or_match
        else:
            _check_match_sides(signal_or_match, mixed, "PXDMatchStatistics.update")
            mt = None
        x = self._input(mt or signal_or_match, "PXDMatchStatistics.update", PXDMatch, PXDHits)
        if self.unit_mm not in (None, x.geometry.unit_mm):
            raise ValueError(f"PXDMatchStatistics.update: the geometry unit {x.geometry.unit_mm} mm differs from the accumulated {self.unit_mm}")
        self.unit_mm = x.geometry.unit_mm
        if mt is None:
            mt = pxd_match(signal_or_match, mixed)
        s, m, S = mt.signal, mt.mixed, self.n_sensors
        sc, mc = s.positions.clusters, m.positions.clusters
        (N, Hh, Ww), Cs, Cm = mt.shape, s.capacity, m.capacity
        if self.tables is None:
            self.tables = torch.zeros(S * H.PXD_MATCH_BINS + 1, dtype=torch.int64, device=self.device)
        t = self.tables.data_ptr()
        with torch.cuda.device(self.device):
            H.call("ieagan_pxd_match_stats", *_ptrs(Cs, s.positions.cluster), s.total.data_ptr(), *_ptrs(Cs, sc.first), sc.total.data_ptr(),
                   sc.digits.total.data_ptr(), *_ptrs(Cs, s.u, s.v), *_ptrs(Cm, mc.charge), mc.total.data_ptr(), m.total.data_ptr(),
                   mc.digits.total.data_ptr(), *_ptrs(Cm, m.u, m.v), *_ptrs(Cs, mt.lo), *_ptrs(Cm, mt.signal_charge),
                   *_ptrs(Cs, mt.mixed_hit, mt.flags), N, Hh, Ww, S, Cs, Cm, self.residual_bin, t, t + 8 * S * H.PXD_MATCH_BINS, H.stream())
        self.hits.append(mt.counts)
        return mt

    def result(self):
        """NumPy tables: int64 ``hits`` / ``matched`` / ``changed`` / ``shared`` / ``lost`` ``[S]`` by the sensor of the signal hit
        (``shared``: matched hits whose mixed cluster holds two or more signal clusters; ``lost = hits - matched``); float64
        ``efficiency = matched / hits``, ``changed_fraction`` and ``shared_fraction`` (of matched), NaN where the denominator is 0;
        ``residual_u`` / ``residual_v [S, 64]`` over the matched and changed hits (bin ``clamp(floor(r / residual_bin) + 32, 0, 63)`` of
        the float64 difference ``r`` in geometry units) and ``purity [S, 32]`` over the matched hits (bin ``min(32 * signal_charge //
        mixed_charge, 31)``); ``residual_bin``, ``unit_mm``; ``hits_per_image`` int32 ``[events, S]`` and ``n_events``.  Raises when an
        update overflowed."""
        table, per_image = self._host_tables()
        if table[-1] != 0:
            raise RuntimeError(f"PXDMatchStatistics: {int(table[-1])} update(s) held more digits than the capacity of their PXDHits, their "
                               "clusters are truncated: make the hits with a larger capacity=")
        rows = table[:-1].reshape(self.n_sensors, H.PXD_MATCH_BINS)
        out = {k: rows[:, i].copy() for i, k in enumerate(H.PXD_MATCH_COUNTERS)}
        with np.errstate(invalid="ignore", divide="ignore"):
            out.update(efficiency=out["matched"] / out["hits"], changed_fraction=out["changed"] / out["matched"],
                       shared_fraction=out["shared"] / out["matched"])
        out.update((k, rows[:, a:a + n].copy()) for k, (a, n) in H.PXD_MATCH_COLUMNS.items())
        return dict(out, residual_bin=self.residual_bin, unit_mm=self.unit_mm, hits_per_image=per_image["hits"], n_events=per_image["n_events"])


def _pooled(result, num, den):
    d = float(np.asarray(result[den]).sum())
    return float(np.asarray(result[num]).sum()) / d if d > 0 else float("nan")


def pxd_match_distance(real, fake):
    """Six distances between two ``PXDMatchStatistics.result()`` tables -- the same signal under recorded and under generated background
    -- (float64, host): ``efficiency_abs_err``, ``changed_abs_err``, ``shared_abs_err`` = absolute differences of the fractions pooled over
    the sensors (matched / hits, changed / matched, shared / matched; NaN when a denominator is 0); ``residual_u_w1`` / ``residual_v_w1`` =
    1-D Wasserstein distances in mm between the residual spectra and ``purity_w1`` (in units of purity, bins of 1 / 32), pooled over the
    sensors and normalised to 1, NaN when one side is empty.  ``ValueError`` when the two sides differ in ``residual_bin`` or ``unit_mm``."""
    for k in ("residual_bin", "unit_mm"):
        if real[k] != fake[k]:
            raise ValueError(f"pxd_match_distance: the two sides differ in {k}: {real[k]} and {fake[k]}")
    out = {name: abs(_pooled(fake, num, den) - _pooled(real, num, den))
           for name, num, den in (("efficiency_abs_err", "matched", "hits"), ("changed_abs_err", "changed", "matched"),
                                  ("shared_abs_err", "shared", "matched"))}
    width = float(real["residual_bin"]) * float(real["unit_mm"])
    return dict(out, residual_u_w1=_w1(real["residual_u"], fake["residual_u"], width), residual_v_w1=_w1(real["residual_v"], fake["residual_v"], width),
                purity_w1=_w1(real["purity"], fake["purity"], 1.0 / PXD_PURITY_BINS))


# ---------------------------------------------------------------------------------------------------------
# space points and inner / outer-layer hit doublets: the hits in a global frame, paired across the two layers (csrc/pxd_doublets.hip)
# ---------------------------------------------------------------------------------------------------------
PXD_SUB = 16                    # sub-units per geometry unit: u * 16.0f is exact in fp32
PXD_COORD_LIMIT = 2 ** 23       # every corner of every sensor lies below this many sub-units from the origin, along every axis


class PXDPlacement:
    """Where the sensors sit in space, as data, in sub-units of 1 / 16 geometry unit (31.25 nm at the default ``unit_mm = 5e-4``):
    ``origin`` int ``[S, 3]`` (the sensor centre), ``u_axis`` / ``v_axis`` int ``[S, 3]`` (the global directions of local u, the rows, and
    local v, the columns, as Q30 integers, ``|a| <= 2**30``), ``layer`` int ``[S]`` (0 inner, 1 outer, -1 ignored) and ``pairs`` uint8
    ``[S, S]``: a doublet of inner sensor ``i`` and outer sensor ``o`` counts only when ``pairs[i, o] != 0`` (default: 1 wherever ``layer[i]
    == 0 and layer[o] == 1``; entries outside that pattern are always zeroed).  The integer tables are the geometry: ``origin``, ``u_axis``,
    ``v_axis``, ``layer`` are int32 NumPy arrays, ``tables(device)`` gives their device copies, uploaded once per device on first use.

    ``ValueError`` for shapes that disagree, more than 255 sensors, a ``layer`` outside ``-1 .. 1``, ``|axis| > 2**30`` and -- with
    ``geometry`` (a ``PXDGeometry``) given here, else in ``pxd_space_points`` -- any sensor corner whose global coordinate reaches ``2**23``
    sub-units.  That bound is what keeps ``pxd_doublets`` exact: ``|x|, |y|, |z| < 2**23`` and ``r < 2**23.5``, so ``x_a x_b + y_a y_b``
    and the cross product stay below ``2**47``, ``tan_q12 * dot`` below ``2**62`` and ``z_a r_b - z_b r_a`` below ``2**48``."""
    TABLES = ("origin", "u_axis", "v_axis", "layer", "pairs")

    def __init__(self, origin, u_axis, v_axis, layer, pairs=None, unit_mm=5e-4, geometry=None):
        o, ua, va, la = (np.asarray(a) for a in (origin, u_axis, v_axis, layer))
        if la.ndim != 1 or la.size == 0 or any(a.shape != (la.size, 3) for a in (o, ua, va)) or any(a.dtype.kind not in "iu" for a in (o, ua, va, la)):
            raise ValueError(f"PXDPlacement: origin {o.shape} / u_axis {ua.shape} / v_axis {va.shape} / layer {la.shape} are not integer arrays "
                             "[S, 3], [S, 3], [S, 3] and [S]")
        S = la.size
        if S > 255:
            raise ValueError(f"PXDPlacement: {S} sensors are more than 255")
        o, ua, va, la = (a.astype(np.int64) for a in (o, ua, va, la))
        if la.min() < -1 or la.max() > 1:
            raise ValueError(f"PXDPlacement: layer holds {int(la.min())} .. {int(la.max())}, outside -1 .. 1")
        if max(np.abs(ua).max(), np.abs(va).max()) > 2 ** 30:
            raise ValueError("PXDPlacement: an axis component is beyond 2**30 in Q30")
        if np.abs(o).max() >= PXD_COORD_LIMIT:
            raise ValueError(f"PXDPlacement: a sensor centre reaches 2**23 sub-units ({int(np.abs(o).max())})")
        pattern = ((la[:, None] == 0) & (la[None, :] == 1)).astype(np.uint8)
        if pairs is None:
            pairs = pattern
        else:
            pairs = np.asarray(pairs)
            if pairs.shape != (S, S):
                raise ValueError(f"PXDPlacement: pairs {pairs.shape} is not [S, S] = [{S}, {S}]")
            pairs = (pairs != 0).astype(np.uint8) * pattern
        self.origin, self.u_axis, self.v_axis, self.layer = (a.astype(np.int32) for a in (o, ua, va, la))
        self.pairs, self.unit_mm, self.S, self._device, self._checked = np.ascontiguousarray(pairs), float(unit_mm), S, {}, []
        if geometry is not None:
            self.check_corners(geometry)

    def check_corners(self, geometry):
        """``ValueError`` when a corner of a sensor of ``geometry`` reaches ``2**23`` sub-units along a global axis, when the geometry has
        other sensors or another unit; remembered per geometry."""
        if any(g is geometry for g in self._checked):
            return
        if not isinstance(geometry, PXDGeometry):
            raise TypeError("PXDPlacement: geometry must be a PXDGeometry")
        if geometry.S != self.S or geometry.unit_mm != self.unit_mm:
            raise ValueError(f"PXDPlacement: {self.S} sensors in units of {self.unit_mm} mm, the geometry has {geometry.S} in units of {geometry.unit_mm} mm")
        half_u = (geometry.u_length[geometry.kind].astype(np.int64) * PXD_SUB + 1) // 2        # sub-units, rounded up
        half_v = (geometry.v_length[geometry.kind].astype(np.int64) * PXD_SUB + 1) // 2
        ua, va, o = (a.astype(np.int64) for a in (self.u_axis, self.v_axis, self.origin))
        for su in (-1, 1):
            for sv in (-1, 1):
                corner = o + ((ua * (su * half_u)[:, None] + va * (sv * half_v)[:, None] + 2 ** 29) >> 30)
                if np.abs(corner).max() >= PXD_COORD_LIMIT:
                    s = int(np.argmax(np.abs(corner).max(1)))
                    raise ValueError(f"PXDPlacement: a corner of sensor {s} reaches 2**23 sub-units ({int(np.abs(corner[s]).max())}): "
                                     f"{PXD_COORD_LIMIT * self.unit_mm / PXD_SUB:.1f} mm is the limit at this unit")
        self._checked.append(geometry)

    def tables(self, device):
        """The five tables on ``device`` (dict by name; int32, ``pairs`` uint8); the upload happens once per device."""
        device = torch.device(device)
        if device not in self._device:
            self._device[device] = {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device) for k in self.TABLES}
        return self._device[device]

    def same_as(self, other):
        return self is other or (isinstance(other, PXDPlacement) and self.unit_mm == other.unit_mm and
                                 all(np.array_equal(getattr(self, k), getattr(other, k)) for k in self.TABLES))

    @classmethod
    def from_float(cls, origin_mm, u_axis, v_axis, layer, pairs=None, unit_mm=5e-4, geometry=None):
        """Float tables rounded once, on the host: ``round(x / unit_mm * 16)`` for the origin in mm, ``round(a * 2**30)`` for the axes."""
        o = np.rint(np.asarray(origin_mm, np.float64) / unit_mm * PXD_SUB).astype(np.int64)
        ua, va = (np.rint(np.asarray(a, np.float64) * 2.0 ** 30).astype(np.int64) for a in (u_axis, v_axis))
        return cls(o, ua, va, np.asarray(layer), pairs, unit_mm, geometry)

    @classmethod
    def barrel(cls, geometry, radii, ladders, per_ladder=2, pairs=None):
        """Two concentric barrels for the sensors of ``geometry``, inner layer first: layer ``L`` has ``ladders[L]`` ladders at radius
        ``radii[L]`` mm, ladder ``j`` at azimuth ``2 pi j / ladders[L]`` with a radial normal, u tangential towards increasing phi and v
        along +z; the ``per_ladder`` sensors of a ladder lie end to end along z about z = 0 (sensor ``k`` centred at ``(k - (per_ladder -
        1) / 2) * v_length``).  Sensor ``s = per_ladder * j + k`` in the inner layer, the outer layer follows.  No tilt."""
        n = [int(v) for v in ladders]
        per = int(per_ladder)
        if len(n) != 2 or len(radii) != 2 or min(n) < 1 or per < 1 or per * sum(n) != geometry.S:
            raise ValueError(f"PXDPlacement.barrel: ladders {tuple(ladders)} x {per_ladder} sensors are not the {geometry.S} sensors of the geometry")
        origin, ua, va, layer = [], [], [], []
        for L in (0, 1):
            for j in range(n[L]):
                phi = 2.0 * np.pi * j / n[L]
                for k in range(per):
                    s = len(layer)
                    length = float(geometry.v_length[geometry.kind[s]]) * geometry.unit_mm
                    origin.append([radii[L] * np.cos(phi), radii[L] * np.sin(phi), (k - (per - 1) / 2.0) * length])
                    ua.append([-np.sin(phi), np.cos(phi), 0.0])
                    va.append([0.0, 0.0, 1.0])
                    layer.append(L)
        return cls.from_float(origin, ua, va, layer, pairs, geometry.unit_mm, geometry)

    @classmethod
    def belle2(cls, geometry, radii=(14.0, 22.0), ladders=(8, 12)):
        """The nominal Belle II PXD barrel for ``PXDGeometry.belle2``: eight inner ladders at radius 14.0 mm and twelve outer ladders at
        22.0 mm, ladder ``j`` at azimuth ``2 pi j / n``, normals radial, u tangential towards increasing phi, v along +z, the two sensors
        of a ladder end to end with centres at ``z = -+ v_length / 2``, no windmill tilt; sensor order of the reference's
        ``create_g1.py:95`` (``s = 2 j + k`` in layer 1, ``16 + 2 j + k`` in layer 2).  These are design values written down from memory:
        the reference holds no geometry, and neither the radii, the azimuth of ladder 0, the missing tilt nor which sensor of a ladder
        lies forward have been checked against basf2.  Pass the true ``radii`` / ``ladders``, or the tables of the conditions database to
        ``PXDPlacement`` itself, where it matters."""
        return cls.barrel(geometry, radii, ladders, 2)


class PXDSpacePoints(_PXDProduct):
    """Device-side result of ``pxd_space_points``: the ``PXDHits`` it came from (``hits``), the ``placement``, and per hit row (the first
    ``total`` written) ``x`` / ``y`` / ``z`` / ``r`` int32 in sub-units, ``sensor`` int32 and ``role`` int8 (the layer of the hit's sensor),
    all ``[capacity]``; ``offsets`` int32 ``[N + 1]``, the exclusive prefix of ``counts``.  ``counts`` / ``total`` are those of the hits."""
    _again = lambda self, capacity: pxd_space_points(self.hits._again(capacity), self.placement)
    PER_HIT = ("x", "y", "z", "r", "sensor", "role")

    def __init__(self, hits, placement, offsets, **arrays):
        self.hits, self.placement, self.geometry, self.offsets = hits, placement, hits.geometry, offsets
        self.seed_cut, self.charge_cut, self.head_tail = hits.seed_cut, hits.charge_cut, hits.head_tail
        vars(self).update(arrays)
        self._set_header(hits.header, hits)

    def _columns(self):
        return dict(digit_header=self.hits.positions.clusters.digits.header, header=self.header, offsets=self.offsets,
                    **{k: getattr(self, k) for k in self.PER_HIT})

    def cpu(self):
        """One read-back (``pxd_read_back``: one copy, one wait) -> dict of NumPy arrays trimmed to the true total, one entry per hit:
        ``x``, ``y``, ``z``, ``r`` (int32, sub-units), ``x_mm``, ``y_mm``, ``z_mm``, ``r_mm`` (float64: ``x * unit_mm / 16``), ``sensor``,
        ``role``, ``event``; plus ``counts [N]`` and ``offsets [N + 1]``.  Never truncated (``_host_columns``)."""
        N = self.shape[0]
        host = self._host_columns(self._columns)
        total = int(host["header"][N])
        out = {k: host[k][:total].copy() for k in self.PER_HIT}
        image = np.searchsorted(host["offsets"], np.arange(total), side="right") - 1
        out.update((k + "_mm", out[k].astype(np.float64) * self.placement.unit_mm / PXD_SUB) for k in ("x", "y", "z", "r"))
        return dict(out, event=(image // self.n_sensors).astype(np.int32), counts=host["header"][:N].copy(), offsets=host["offsets"].copy())


def pxd_space_points(hits, placement):
    """The hits of a ``PXDHits`` in the global frame of a ``PXDPlacement``, in sub-units of 1 / 16 geometry unit (csrc/pxd_doublets.hip).
    With ``lu = int(rintf(u * 16.0f))`` (one exact fp32 multiply, one round to nearest even) and ``lv`` likewise, for ``c = x, y, z``:
    ``X_c = origin[s, c] + ((u_axis[s, c] * lu + v_axis[s, c] * lv + 2**29) >> 30)`` with an int64 arithmetic shift, and ``r =
    isqrt(x**2 + y**2)`` exactly; ``s`` is the sensor of the hit's cluster.  ``rintf`` is the last float of the chain: the same recipe in
    Python integers gives the same numbers, and two calls write the same bytes.

    Launches on the current stream, neither synchronises nor copies, and can be captured into a HIP graph.  ``ValueError`` when the
    placement does not fit the hits' geometry (sensors, unit, a corner at or beyond ``2**23`` sub-units)."""
    H.require_gpu()
    if not isinstance(hits, PXDHits) or not isinstance(placement, PXDPlacement):
        raise TypeError("pxd_space_points: expects the PXDHits of pxd_hits and a PXDPlacement")
    placement.check_corners(hits.geometry)
    p, c = hits.positions, hits.positions.clusters
    N, Hh, Ww = hits.shape
    dev, C = hits.u.device, hits.capacity
    out = {k: torch.empty(C, dtype=torch.int8 if k == "role" else torch.int32, device=dev) for k in PXDSpacePoints.PER_HIT}
    offsets = torch.empty(N + 1, dtype=torch.int32, device=dev)
    t = placement.tables(dev)
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_space_points", *_ptrs(C, p.cluster), hits.total.data_ptr(), *_ptrs(C, c.first), c.total.data_ptr(),
               hits.counts.data_ptr(), *_ptrs(C, hits.u, hits.v), *(t[k].data_ptr() for k in PXDPlacement.TABLES[:4]), N, Hh, Ww, hits.n_sensors,
               C, *_ptrs(C, *(out[k] for k in PXDSpacePoints.PER_HIT)), offsets.data_ptr(), H.stream())
    return PXDSpacePoints(hits, placement, offsets, **out)


def pxd_doublet_windows(dphi=0.3, z0_mm=10.0, unit_mm=5e-4):
    """The two windows of ``pxd_doublets`` as the integers that are the rule: ``tan_q12 = round(tan(dphi) * 4096)`` in ``1 .. 32768`` and
    ``z0_sub = round(z0_mm / unit_mm * 16)`` in ``0 .. 2**23 - 1``; ``ValueError`` outside."""
    dphi, z0_mm = float(dphi), float(z0_mm)
    tan_q12 = int(round(np.tan(dphi) * 4096)) if 0.0 < dphi < np.pi / 2 else 0
    z0_sub = int(round(z0_mm / unit_mm * PXD_SUB)) if z0_mm >= 0 else -1
    if not 1 <= tan_q12 <= 32768:
        raise ValueError(f"pxd_doublets: dphi = {dphi} rad gives tan_q12 = {tan_q12}, outside 1 .. 32768")
    if not 0 <= z0_sub < PXD_COORD_LIMIT:
        raise ValueError(f"pxd_doublets: z0_mm = {z0_mm} gives z0_sub = {z0_sub}, outside 0 .. 2**23 - 1")
    return tan_q12, z0_sub


class PXDDoublets:
    """Device-side result of ``pxd_doublets``: the ``PXDSpacePoints`` (``points``), the windows ``tan_q12`` / ``z0_sub``, ``partners`` int32
    ``[points.capacity]`` (the doublets of an inner hit row, 0 for every other row of an event), ``event_doublets`` int32 ``[E]``,
    ``pair_doublets`` int32 ``[S, S]`` (per inner and outer sensor), ``total`` int32 ``[1]`` and the list ``inner`` / ``outer`` int32 ``[doublet_capacity]``: the hit rows of the first ``min(total,
    doublet_capacity)`` doublets in ascending ``(inner, outer)`` order.  ``partners``, ``event_doublets``, ``pair_doublets`` and ``total`` are always whole.
    ``header`` / ``counts`` are those of the hits."""

    def __init__(self, points, tan_q12, z0_sub, doublet_capacity, **arrays):
        self.points, self.placement, self.tan_q12, self.z0_sub, self.doublet_capacity = points, points.placement, tan_q12, z0_sub, doublet_capacity
        vars(self).update((k, getattr(points, k)) for k in ("shape", "n_sensors", "threshold", "seed_cut", "charge_cut", "header", "counts", "capacity"))
        vars(self).update(arrays)

    def _columns(self):
        return dict(digit_header=self.points.hits.positions.clusters.digits.header, header=self.header, offsets=self.points.offsets,
                    total=self.total, partners=self.partners, event_doublets=self.event_doublets, inner=self.inner, outer=self.outer)

    def cpu(self):
        """One read-back (``pxd_read_back``: one copy, one wait) -> dict of NumPy arrays: ``inner`` / ``outer`` ``[total]`` (hit rows),
        ``event`` ``[total]``, ``partners`` ``[hits]``, ``event_doublets`` ``[E]``, ``total``, ``tan_q12``, ``z0_sub``.  Never truncated:
        when the digit total exceeds the hits' capacity the chain is run again, when ``total`` exceeds ``doublet_capacity`` the doublets
        are (a second read-back, on those paths only)."""
        N = self.shape[0]
        host = pxd_read_back(**self._columns())
        grow = int(host["digit_header"][N]) > self.capacity
        if grow:
            self.points._grow(int(host["digit_header"][N]))
        if grow or int(host["total"][0]) > self.doublet_capacity:
            again = _doublets(self.points, self.tan_q12, self.z0_sub, None if grow else int(host["total"][0]))
            vars(self).update(vars(again))
            host = pxd_read_back(**self._columns())
            if int(host["total"][0]) > self.doublet_capacity:           # after a grown chain: the default capacity may not do either
                vars(self).update(vars(_doublets(self.points, self.tan_q12, self.z0_sub, int(host["total"][0]))))
                host = pxd_read_back(**self._columns())
        total, hits = int(host["total"][0]), int(host["header"][N])
        inner = host["inner"][:total].copy()
        image = np.searchsorted(host["offsets"], inner, side="right") - 1
        return dict(inner=inner, outer=host["outer"][:total].copy(), event=(image // self.n_sensors).astype(np.int32),
                    partners=host["partners"][:hits].copy(), event_doublets=host["event_doublets"].copy(), total=total,
                    tan_q12=self.tan_q12, z0_sub=self.z0_sub)


def _doublets(points, tan_q12, z0_sub, capacity=None):
    """``ieagan_pxd_doublets`` of a ``PXDSpacePoints`` with the integer windows; ``capacity`` (doublets) defaults to the hits' capacity."""
    (N, _, _), S, dev, C = points.shape, points.n_sensors, points.x.device, points.capacity
    D = C if capacity is None else int(capacity)
    if D < 0:
        raise ValueError("pxd_doublets: capacity is negative")
    new = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    out = dict(partners=new(C), event_doublets=new(N // S), pair_doublets=new(S * S).view(S, S), total=new(1), inner=new(D), outer=new(D))
    scratch = new(H.lib().ieagan_pxd_doublets_scratch(N, S, C))
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_doublets", *_ptrs(C, *(getattr(points, k) for k in PXDSpacePoints.PER_HIT)), points.offsets.data_ptr(),
               points.total.data_ptr(), points.placement.tables(dev)["pairs"].data_ptr(), N, S, C, tan_q12, z0_sub, D, *_ptrs(C, out["partners"]),
               out["event_doublets"].data_ptr(), out["pair_doublets"].data_ptr(), out["total"].data_ptr(), *_ptrs(D, out["inner"], out["outer"]),
               scratch.data_ptr(), H.stream())
    return PXDDoublets(points, tan_q12, z0_sub, D, **out)


def pxd_doublets(hits_or_points, placement=None, dphi=0.3, z0_mm=10.0, capacity=None):
    """Inner / outer-layer hit doublets of a batch (csrc/pxd_doublets.hip): the first question tracking asks the PXD.  Input: a ``PXDHits``
    with a ``PXDPlacement`` (``pxd_space_points`` runs first) or an existing ``PXDSpacePoints``.  The host turns the windows into integers
    once (``pxd_doublet_windows``): ``tan_q12 = round(tan(dphi) * 4096)``, ``z0_sub = round(z0_mm / unit_mm * 16)``; the integers are the
    rule.  Hit ``a`` with ``role == 0`` and hit ``b`` with ``role == 1`` of the same event form a doublet iff, in int64,

    * ``pairs[sensor_a, sensor_b] != 0``;
    * ``dot = x_a x_b + y_a y_b > 0`` and ``abs(x_a y_b - y_a x_b) << 12 <= tan_q12 * dot``: the azimuth window ``|dphi|``;
    * ``r_b > r_a`` and ``abs(z_a r_b - z_b r_a) <= z0_sub * (r_b - r_a)``: the straight line through both hits in (r, z) meets the beam
      line within ``+- z0``.

    The list ``inner`` / ``outer`` holds the hit rows of every doublet in ascending ``(inner, outer)`` order, ``capacity`` of them
    (default: the hits' capacity); on overflow it holds the first ``capacity`` of that order, ``partners`` / ``event_doublets`` /
    ``pair_doublets`` / ``total`` stay whole and ``PXDDoublets.cpu()`` reruns with a larger capacity instead of returning a truncated list.  No float exists on the
    device after ``rintf``: two calls write the same bytes.  Launches on the current stream, neither synchronises nor copies; with
    ``capacity`` given it can be captured into a HIP graph.  Triplets with the SVD, curvature or pT windows, alignment, the windmill
    geometry, doublets labelled by ``pxd_match`` truth and position errors are out of scope."""
    H.require_gpu()
    points = hits_or_points
    if isinstance(points, PXDSpacePoints):
        if placement is not None and not points.placement.same_as(placement):
            raise ValueError("pxd_doublets: the PXDSpacePoints were made with another placement")
    elif isinstance(points, PXDHits):
        if placement is None:
            raise TypeError("pxd_doublets: PXDHits need a placement")
        points = pxd_space_points(points, placement)
    else:
        raise TypeError("pxd_doublets: expects the PXDHits of pxd_hits or the PXDSpacePoints of pxd_space_points")
    return _doublets(points, *pxd_doublet_windows(dphi, z0_mm, points.placement.unit_mm), capacity)


class PXDDoubletStatistics(_PXDAccumulator):
    """Accumulator of the doublet statistics over batches, beside the other ``PXD*`` accumulators: how many hit pairs across the two layers
    are compatible with one track from the interaction region -- the number that decides how many fake track seeds a background makes, and
    that sees whether the hits of an event are spatially coherent.  ``update`` takes images, any chain product up to ``PXDHits``, a
    ``PXDSpacePoints`` or a ``PXDDoublets``, runs what is missing and ``ieagan_pxd_doublet_stats`` on the current stream; it neither
    synchronises nor copies, ``result()`` does the single read-back.  Counters are exact int64.  An update whose digit total exceeds the
    ``capacity`` (digits) is counted on the device and makes ``result()`` raise.  The statistics never read the list of doublets, so the
    ``doublet_capacity`` of the doublets an update makes (default: the digit capacity) bounds only that list.  ``tables``: int64 ``[5 +
    S * S + 64 + 251 + 1]`` on the device, the overflow counter last."""
    _per_image = ("hits",)

    def __init__(self, placement, geometry, n_sensors=40, threshold=7.0, dphi=0.3, z0_mm=10.0, seed_cut=0, charge_cut=0, head_tail=3,
                 capacity=None, doublet_capacity=None, device=None):
        if not isinstance(placement, PXDPlacement) or not isinstance(geometry, PXDGeometry):
            raise TypeError("PXDDoubletStatistics: expects a PXDPlacement and a PXDGeometry")
        if placement.S != int(n_sensors):
            raise ValueError(f"PXDDoubletStatistics: the placement has {placement.S} sensors, not {n_sensors}")
        placement.check_corners(geometry)
        self.placement, self.geometry, self.head_tail = placement, geometry, int(head_tail)
        self.seed_cut, self.charge_cut = _check_cuts("PXDDoubletStatistics", seed_cut, charge_cut)
        self.tan_q12, self.z0_sub = pxd_doublet_windows(dphi, z0_mm, placement.unit_mm)
        self.doublet_capacity = doublet_capacity if doublet_capacity is None else int(doublet_capacity)
        super().__init__(n_sensors, threshold, capacity, device)

    def update(self, images_or_product):
        d = self._input(images_or_product, "pxd_digits", PXDClusters, PXDClusterPositions, PXDHits, PXDSpacePoints, PXDDoublets)
        if not isinstance(d, (PXDHits, PXDSpacePoints, PXDDoublets)):
            d = pxd_hits(d, self.geometry, self.head_tail, self.threshold, self.seed_cut, self.charge_cut, self.capacity, self.n_sensors)
        if isinstance(d, PXDHits):
            d = pxd_space_points(d, self.placement)
        if not self.placement.same_as(d.placement):
            raise ValueError(f"PXDDoubletStatistics.update: the {type(d).__name__} was made with another placement")
        if isinstance(d, PXDSpacePoints):
            d = _doublets(d, self.tan_q12, self.z0_sub, self.doublet_capacity)
        if (d.tan_q12, d.z0_sub) != (self.tan_q12, self.z0_sub):
            raise ValueError(f"PXDDoubletStatistics.update: the PXDDoublets were made with the windows {(d.tan_q12, d.z0_sub)}, not {(self.tan_q12, self.z0_sub)}")
        p, S, (N, _, _), C = d.points, self.n_sensors, d.shape, d.capacity
        words = len(H.PXD_DOUBLET_COUNTERS) + S * S + H.PXD_PARTNER_BINS + H.PXD_BINS
        if self.tables is None:
            self.tables = torch.zeros(words + 1, dtype=torch.int64, device=self.device)
        t = self.tables.data_ptr()
        with torch.cuda.device(self.device):
            H.call("ieagan_pxd_doublet_stats", *_ptrs(C, p.role), p.offsets.data_ptr(), p.total.data_ptr(),
                   p.hits.positions.clusters.digits.total.data_ptr(), self.placement.tables(self.device)["layer"].data_ptr(), *_ptrs(C, d.partners),
                   d.event_doublets.data_ptr(), d.pair_doublets.data_ptr(), N, S, C, t, t + 8 * words, H.stream())
        self.hits.append(d.counts)
        return d

    def result(self):
        """NumPy tables: int64 ``events``, ``inner_hits``, ``outer_hits``, ``doublets``, ``candidates`` (the sum over the events of ``n_in *
        n_out``), ``sensor_pairs [S, S]`` (doublets per inner and outer sensor), ``partners_spectrum [64]`` (over the inner hits, last bin
        open), ``event_doublets_spectrum [251]`` (over the events, the bins of ``pxd_bin_index``); float64 ``doublets_per_event`` and
        ``acceptance = doublets / candidates`` (NaN without events / candidates); the windows ``tan_q12`` / ``z0_sub``, the placement's
        ``origin`` / ``u_axis`` / ``v_axis`` / ``layer`` / ``pairs``, ``shape``; ``hits`` int32 ``[events, S]`` and ``n_events``.  Raises
        when an update overflowed."""
        table, per_image = self._host_tables()
        S, n = self.n_sensors, len(H.PXD_DOUBLET_COUNTERS)
        out = {k: int(table[i]) for i, k in enumerate(H.PXD_DOUBLET_COUNTERS)}
        ratio = lambda a, b: float(a) / float(b) if b > 0 else float("nan")
        return dict(out, sensor_pairs=table[n:n + S * S].reshape(S, S).copy(), partners_spectrum=table[n + S * S:n + S * S + H.PXD_PARTNER_BINS].copy(),
                    event_doublets_spectrum=table[n + S * S + H.PXD_PARTNER_BINS:].copy(), doublets_per_event=ratio(out["doublets"], out["events"]),
                    acceptance=ratio(out["doublets"], out["candidates"]), tan_q12=self.tan_q12, z0_sub=self.z0_sub, shape=self.shape,
                    **{k: getattr(self.placement, k).copy() for k in PXDPlacement.TABLES}, hits=per_image["hits"], n_events=per_image["n_events"])


def pxd_doublet_distance(real, fake):
    """Four distances between two ``PXDDoubletStatistics.result()`` tables (float64, host): ``doublet_rate_rel_err`` = |fake - real| / real
    of the doublets per event; ``acceptance_rel_err`` = the same of ``doublets / candidates``, the fraction of the inner x outer hit pairs
    of an event that pass the windows -- the number that sees spatial coherence, whatever the occupancies are; ``partners_w1`` = the 1-D
    Wasserstein distance between the normalised spectra of partners per inner hit; ``sensor_pair_l1`` = the L1 distance of the two
    normalised ``[S, S]`` tables.  NaN where a real denominator is 0 or a side is empty.  ``ValueError`` when the windows, the placement
    tables or the shapes differ."""
    for k in ("tan_q12", "z0_sub", "shape"):
        if tuple(np.atleast_1d(real[k])) != tuple(np.atleast_1d(fake[k])):
            raise ValueError(f"pxd_doublet_distance: the two sides differ in {k}: {real[k]} and {fake[k]}")
    for k in PXDPlacement.TABLES:
        if not np.array_equal(real[k], fake[k]):
            raise ValueError(f"pxd_doublet_distance: the two sides differ in the placement table {k}")
    rel = lambda r, f: abs(f - r) / r if r == r and r > 0 and f == f else float("nan")
    pr, pf = np.asarray(real["sensor_pairs"], np.float64), np.asarray(fake["sensor_pairs"], np.float64)
    l1 = float(np.abs(pf / pf.sum() - pr / pr.sum()).sum()) if pr.sum() > 0 and pf.sum() > 0 else float("nan")
    return dict(doublet_rate_rel_err=rel(real["doublets_per_event"], fake["doublets_per_event"]),
                acceptance_rel_err=rel(real["acceptance"], fake["acceptance"]),
                partners_w1=_w1(np.asarray(real["partners_spectrum"])[None], np.asarray(fake["partners_spectrum"])[None]), sensor_pair_l1=l1)
