"""Train-step utilities behind the reference's ``utils`` surface (reference ``utils/__init__.py``:
Distribution 41-120, prepare_z_y 124-158, seed_rng 218-226, toggle_grad 261-263, make_mask 266-275,
apply_ema 809-837, ortho 843-859).  Host-side bookkeeping of the reference (sample sheets, plots,
Inception statistics) is out of scope of the MI355X hot path.  Checkpoint I/O, metadata and singular-value
logging keep the reference's signatures and on-disk layout (load_weights 592, write_metadata 671, save_weights 689,
save_and_sample 299, get_singular_values 572).
"""
from __future__ import annotations

import os as _os
import sys as _sys

import numpy as np
import torch

import _hip as H


def _fall_through_to_reference_checkout():
    """The reference's scripts also import the host-side bookkeeping sub-modules ``utils.configuration``,
    ``utils.logging``, ``utils.dataloader``, ``utils.plot``, ``utils.norm`` and ``utils.noise`` (reference
    train.py:16-19, utils/__init__.py:30).  They are outside the accelerated path and are not re-implemented here:
    when a reference checkout is on ``sys.path`` behind this package (``dropin.py``), its
    ``utils/`` directory is appended to this package's search path so those sub-modules resolve to the user's own
    files, while every name defined in this file keeps shadowing the reference's ``utils/__init__.py``."""
    here = _os.path.dirname(_os.path.abspath(__file__))
    for p in list(_sys.path):
        cand = _os.path.join(_os.path.abspath(p or "."), "utils")
        if cand != here and cand not in __path__ and _os.path.isfile(_os.path.join(cand, "configuration.py")):
            __path__.append(cand)


_fall_through_to_reference_checkout()


class Distribution(torch.Tensor):
    """Latent / label holder refilled in place by ``sample_()``."""

    def init_distribution(self, dist_type: str, **kwargs):
        self.dist_type, self.dist_kwargs = dist_type, kwargs
        if dist_type in ("normal", "censored_normal"):
            self.mean, self.var = kwargs["mean"], kwargs["var"]
        elif dist_type in ("categorical", "permuted"):
            self.num_categories = kwargs["num_categories"]
        elif dist_type != "bernoulli":
            raise NotImplementedError(f"Distribution '{dist_type}' is not implemented")

    def sample_(self):
        if self.dist_type == "normal":
            self.normal_(self.mean, self.var)
        elif self.dist_type == "censored_normal":
            self.normal_(self.mean, self.var)
            self.relu_()
        elif self.dist_type == "categorical":
            self.random_(0, self.num_categories)
        elif self.dist_type == "bernoulli":
            self.bernoulli_()
        elif self.dist_type == "permuted":
            self.copy_(torch.randperm(self.num_categories, device=self.device))
        else:
            raise NotImplementedError(f"Distribution '{self.dist_type}' is not implemented")

    def to(self, *args, **kwargs):
        new_obj = Distribution(self)
        new_obj.init_distribution(self.dist_type, **self.dist_kwargs)
        new_obj.data = super().to(*args, **kwargs)
        return new_obj


def prepare_z_y(G_batch_size, dim_z, nclasses, device="cuda", fp16=False, z_var=1.0, z_dist="normal", threshold=1,
                y_dist="permuted", ngd=False, fixed=False):
    if ngd or fp16:
        raise NotImplementedError("prepare_z_y: ngd / fp16 latents are not part of the MI355X path")
    z_ = Distribution(torch.randn(G_batch_size, dim_z, requires_grad=False))
    if z_dist in ("normal", "censored_normal"):
        z_.init_distribution(z_dist, mean=0, var=z_var)
    elif z_dist == "bernoulli":
        z_.init_distribution(z_dist)
    else:
        raise NotImplementedError(f"z_dist {z_dist}")
    z_ = z_.to(device, torch.float32)
    y_ = Distribution(torch.zeros(G_batch_size, requires_grad=False))
    y_.init_distribution("categorical" if y_dist == "categorical" else "permuted", num_categories=nclasses, device=device)
    y_ = y_.to(device, torch.int64)
    return z_, y_


def seed_rng(seed):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
    np.random.seed(seed)


def toggle_grad(model, on_or_off):
    for p in model.parameters():
        p.requires_grad = on_or_off


def make_mask(labels, n_cls, device):
    """[n_cls, n_samples] one-hot of the labels, built on the device (no host round trip)."""
    return (torch.arange(n_cls, device=labels.device)[:, None] == labels[None, :]).to(torch.long).to(device)


class apply_ema(object):
    """EMA of ``source`` into ``target`` over every state-dict entry (parameters AND buffers): one fused
    launch over the two flat arenas."""

    def __init__(self, source, target, decay=0.9999, start_itr=0):
        self.source, self.target, self.decay, self.start_itr = source, target, decay, start_itr
        self._decay_dev, self._decay_host = None, None
        print("Initializing EMA parameters to be source parameters...")
        with torch.no_grad():
            tgt = self.target.state_dict()
            for k, v in self.source.state_dict().items():
                tgt[k].copy_(v)

    def _arenas(self):
        from arena import Arena
        out = []
        for net in (self.source, self.target):
            a = net.__dict__.get("_arena")
            probe = next(net.parameters())
            if a is None or a.root is not net or not a.contains(probe):
                a = Arena(net)
                if hasattr(net, "_plan"):
                    net._plan = None
            out.append(a)
        return out

    def decay_dirty(self, itr=None):
        """True when ``push_decay(itr)`` would write the device scalar."""
        decay = 0.0 if (itr and itr < self.start_itr) else self.decay
        return self._decay_dev is None or decay != self._decay_host

    def push_decay(self, itr=None):
        """Mirror the decay for iteration ``itr`` into the device scalar the kernel reads (no-op when
        unchanged); called by ``update`` and once per replay when the step runs from a HIP graph."""
        decay = 0.0 if (itr and itr < self.start_itr) else self.decay
        if self._decay_dev is None:
            self._decay_dev = torch.tensor([decay], dtype=torch.float32, device=next(self.source.parameters()).device)
        elif decay != self._decay_host:
            self._decay_dev.fill_(decay)
        self._decay_host = decay

    def update(self, itr=None):
        H.require_gpu()
        src, tgt = self._arenas()
        assert src.flat.numel() == tgt.flat.numel(), "EMA source / target layouts differ"
        if not torch.cuda.is_current_stream_capturing():
            self.push_decay(itr)
        H.call("ieagan_ema_update", tgt.flat.data_ptr(), src.flat.data_ptr(), src.flat.numel(), self._decay_dev.data_ptr(),
               H.stream())


def _ortho_plan(arena, params):
    """Work lists of the batched ortho launch for the 2-D+ parameters ``params`` of one arena (cached per set)."""
    key = tuple(id(p) for p in params)
    plans = arena.__dict__.setdefault("_ortho_plans", {})
    if key in plans:
        return plans[key]
    offs = {id(p): o for p, o, _ in arena.param_slices}
    ksplit = H.lib().ieagan_ortho_ksplit()
    tile = 64
    table, gtiles, atiles, goff = [], [], [], 0
    for li, p in enumerate(params):
        R, K = p.shape[0], p.numel() // p.shape[0]
        M, red = (R, K) if R <= K else (K, R)
        table.append([offs[id(p)], R, K, goff])
        goff += (M * M + 7) // 8 * 8
        nt = (M + tile - 1) // tile
        for ti in range(nt):
            for tj in range(nt):
                for sp in range((red + ksplit - 1) // ksplit):
                    gtiles.append([li, ti, tj, sp])
        for ti in range((R + tile - 1) // tile):
            for tj in range((K + tile - 1) // tile):
                atiles.append([li, ti, tj, 0])
    dev = arena.flat.device
    plan = dict(table=torch.tensor(table, dtype=torch.int64, device=dev), ngt=len(gtiles), nat=len(atiles),
                gtiles=torch.tensor(gtiles, dtype=torch.int32, device=dev), atiles=torch.tensor(atiles, dtype=torch.int32, device=dev),
                gram=torch.empty(goff, dtype=torch.float32, device=dev))
    plans[key] = plan
    return plan


def ortho(model, strength=1e-4, blacklist=None):
    """Modified orthogonal regularisation added straight to ``param.grad`` (reference utils/__init__.py:843-859):
    grad += 2*strength * ((W W^T) (.) (1 - I)) W for every parameter with >= 2 dims outside ``blacklist`` -- ONE batched
    HIP call over the network's flat arena (csrc/ortho.hip).  Tall matrices are evaluated as
    W (W^T W) - diag(|w_i|^2) W so the Gram matrix is [in, in] (256x256 for G.linear, not 24576x24576)."""
    H.require_gpu()
    from arena import arena_of
    blacklist = blacklist or []
    arena = arena_of(model)
    if not arena.grads_attached():                      # stand-alone module: move its gradients into one flat buffer
        old = [(p, p.grad) for p, _, _ in arena.param_slices]
        arena.attach_grads()
        with torch.no_grad():
            for p, g in old:
                if g is not None:
                    p.grad.copy_(g)
    params = [p for p in model.parameters() if p.dim() >= 2 and not any(p is b for b in blacklist) and p.grad is not None]
    if not params:
        return
    plan = _ortho_plan(arena, params)
    H.call("ieagan_ortho_grad", arena.flat.data_ptr(), arena.grad.data_ptr(), plan["table"].data_ptr(), plan["gtiles"].data_ptr(),
           plan["ngt"], plan["atiles"].data_ptr(), plan["nat"], plan["gram"].data_ptr(), plan["gram"].numel(), float(strength),
           H.stream())


# ---------------------------------------------------------------------------------------------------------
# the steps either side of the train step
# ---------------------------------------------------------------------------------------------------------
def ingest_event(ev_u8, noise=None, scale=4e-3, pad=3, device=None):
    """uint8 sensor images of one event ``[N, Hin, W]`` (host or device) -> the network input fp32 ``[N, 1, Hin+2*pad, W]``
    on the GPU: the reference's ``Pad -> ToTensor -> fn_lognorm255 -> UniformNoise(4e-3) -> Normalize(0.5, 0.5)`` chain
    (utils/dataloader.py:66-77) as one HIP kernel.  Only the uint8 pixels cross PCIe (7.7 MB per 40x250x768 event
    instead of 31.5 MB of fp32).  ``noise``: explicit U[0,1) draws ``[N, Hin+2*pad, W]`` (parity tests); None = drawn on
    the device; False = no dequantisation noise."""
    H.require_gpu()
    dev = torch.device(device) if device is not None else (ev_u8.device if ev_u8.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    if ev_u8.dtype != torch.uint8 or ev_u8.dim() != 3:
        raise TypeError("ingest_event expects a uint8 tensor [N, H, W]")
    ev = ev_u8.to(dev, non_blocking=True).contiguous()
    N, Hin, W = ev.shape
    out = torch.empty(N, 1, Hin + 2 * pad, W, dtype=torch.float32, device=dev)
    if noise is None:
        noise = torch.rand(N, Hin + 2 * pad, W, device=dev)
    elif noise is False:
        noise = None
    else:
        noise = noise.to(dev, torch.float32).contiguous()
        if noise.numel() != out.numel():
            raise ValueError("noise must have the padded shape [N, Hin + 2*pad, W]")
    H.call("ieagan_event_ingest", ev.data_ptr(), H.ptr(noise), out.data_ptr(), N, Hin, W, pad, float(scale), H.stream())
    return out


def feature_statistics(feats):
    """Mean and unbiased covariance (np.cov(rowvar=False)) of a feature matrix [n, d], float64, on the features' device."""
    f = feats.to(torch.float64)
    mu = f.mean(0)
    fc = f - mu
    return mu, fc.t() @ fc / (f.shape[0] - 1)


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1-mu2|^2 + Tr(S1) + Tr(S2) - 2 Tr((S1 S2)^(1/2)) evaluated on the device (reference: scipy ``sqrtm`` on the host,
    mycleanfid/fid.py:431-468).  For positive semi-definite S1, S2 the trace term equals sum(sqrt(eig(S1^(1/2) S2 S1^(1/2)))),
    two symmetric eigen-decompositions in float64 -- no complex arithmetic and no eps retry for singular products."""
    H.require_gpu()
    mu1, mu2, s1, s2 = (torch.as_tensor(t).to("cuda" if not torch.as_tensor(t).is_cuda else torch.as_tensor(t).device, torch.float64)
                        for t in (mu1, mu2, sigma1, sigma2))
    w1, v1 = torch.linalg.eigh(s1)
    r1 = (v1 * w1.clamp_min(0).sqrt()) @ v1.t()
    w = torch.linalg.eigvalsh(r1 @ s2 @ r1)
    diff = mu1 - mu2
    return float(diff.dot(diff) + torch.trace(s1) + torch.trace(s2) - 2.0 * w.clamp_min(0).sqrt().sum())


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


class PXDStatistics:
    """Accumulator of the reference's per-event detector statistics (eval_all.py:75-101 ``get_stats``) over batches of sensor images in
    detector units, ``[N, H, W]`` fp32 (``Generator(..., export=True)``) or uint8 (event files); image ``n`` is sensor
    ``n % n_sensors``.  ``update`` is one HIP launch pair (csrc/pxd_stats.hip) on the current stream: it neither synchronises nor
    copies to the host; ``result()`` does the single read-back."""

    def __init__(self, n_sensors=40, threshold=7.0, device=None):
        self.n_sensors, self.threshold = int(n_sensors), float(threshold)
        self.device = torch.device(device) if device is not None else None
        self.reset()

    def reset(self):
        self.spectrum = None            # int64 [S, 251] on the device (the kernel's 64-bit unsigned counters)
        self.hits, self.charge, self.shape = [], [], None

    def update(self, images):
        H.require_gpu()
        if images.dim() == 4 and images.shape[1] == 1:
            images = images[:, 0]
        if images.dim() != 3 or images.dtype not in (torch.float32, torch.uint8):
            raise TypeError("PXDStatistics.update expects fp32 or uint8 sensor images [N, H, W] in detector units")
        if images.shape[0] == 0 or images.shape[0] % self.n_sensors:
            raise ValueError(f"PXDStatistics.update: {images.shape[0]} images are not whole events of {self.n_sensors} sensors")
        if self.device is None:
            self.device = images.device if images.is_cuda else torch.device("cuda", torch.cuda.current_device())
        x = images.to(self.device, non_blocking=True).contiguous()
        N, Hh, Ww = x.shape
        if self.shape is None:
            self.shape = (Hh, Ww)
        elif self.shape != (Hh, Ww):
            raise ValueError(f"PXDStatistics.update: image size {(Hh, Ww)} differs from the accumulated {self.shape}")
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
        if not self.hits:
            raise RuntimeError("PXDStatistics.result() before any update()")
        S = self.n_sensors
        px = self.shape[0] * self.shape[1]
        packed = torch.cat([self.spectrum.reshape(-1), torch.cat(self.hits).to(torch.int64),
                            torch.cat(self.charge).view(torch.int32).to(torch.int64)]).cpu().numpy()      # the one device-to-host copy
        spectrum = packed[:S * H.PXD_BINS].reshape(S, H.PXD_BINS).copy()
        n = (packed.size - S * H.PXD_BINS) // 2
        hits = packed[S * H.PXD_BINS:S * H.PXD_BINS + n].reshape(-1, S)
        charge = packed[S * H.PXD_BINS + n:].astype(np.int32).view(np.float32).reshape(-1, S)
        occupancy = (hits.astype(np.float64) / px).mean(0)
        has = hits > 0
        per = np.where(has, charge.astype(np.float64) / np.maximum(hits, 1), 0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean_charge = per.sum(0) / has.sum(0)
        b = (hits.reshape(-1) * 10000) // px
        occ_hist = np.bincount(b[b < PXD_OCC_BINS], minlength=PXD_OCC_BINS).astype(np.int64)
        return dict(spectrum=spectrum, occupancy=occupancy, mean_charge=mean_charge, occ_hist=occ_hist,
                    occ_overflow=int((b >= PXD_OCC_BINS).sum()), n_events=int(hits.shape[0]), hits=hits.copy(), charge=charge.copy())


def pxd_distance(real, fake):
    """Three distances between two ``PXDStatistics.result()`` tables (float64, host): ``occ_rel_err`` / ``charge_rel_err`` = mean over
    the sensors with real occupancy > 0 of |fake - real| / real (a fake sensor that never had a hit counts with mean charge 0, i.e.
    a relative error of 1); ``spectrum_w1`` = the 1-D Wasserstein distance in ADU between the hit spectra (bins 2 .. 250, one ADU
    wide, pooled over the sensors, each normalised to 1), NaN when one side has no hit at all."""
    def rel(r, f, ok):
        r, f = np.asarray(r, np.float64), np.nan_to_num(np.asarray(f, np.float64), nan=0.0)
        return float(np.mean(np.abs(f[ok] - r[ok]) / r[ok])) if ok.any() else float("nan")

    occ_r = np.asarray(real["occupancy"], np.float64)
    out = dict(occ_rel_err=rel(occ_r, fake["occupancy"], occ_r > 0),
               charge_rel_err=rel(real["mean_charge"], fake["mean_charge"], occ_r > 0))
    hr = np.asarray(real["spectrum"], np.float64)[:, 2:].sum(0)
    hf = np.asarray(fake["spectrum"], np.float64)[:, 2:].sum(0)
    if hr.sum() > 0 and hf.sum() > 0:
        out["spectrum_w1"] = float(np.abs(np.cumsum(hf / hf.sum()) - np.cumsum(hr / hr.sum())).sum())
    else:
        out["spectrum_w1"] = float("nan")
    return out


# ---------------------------------------------------------------------------------------------------------
# event production (reference Physics_Analysis/create_g1.py:62-79): sparse digits (sensor, u cell, v cell, charge)
# ---------------------------------------------------------------------------------------------------------
PXD_DIGITS_FRACTION = 16    # default capacity of pxd_digits: one digit per 16 pixels (6.25 %; PXD background sits near 1 %)


class PXDDigits:
    """Device-side result of ``pxd_digits``: ``index`` int32 ``[capacity]`` (flat position ``n*H*W + r*W + c``, ascending), ``charge``
    uint8 ``[capacity]``, ``counts`` int32 ``[N]``, ``total`` int32 ``[1]`` -- only the first ``min(total, capacity)`` digits are
    written.  ``start_copy`` enqueues the device-to-host copies, ``cpu()`` / ``unpack()`` wait for them (one wait)."""

    def __init__(self, images, threshold, capacity, n_sensors, header, index, charge):
        self.images, self.threshold, self.capacity, self.n_sensors = images, threshold, capacity, n_sensors
        self.shape = tuple(images.shape)
        self.header, self.index, self.charge = header, index, charge
        self.counts, self.total = header[:self.shape[0]], header[self.shape[0]:]
        self._host = None

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
            full = pxd_digits(self.images, self.threshold, capacity=total, n_sensors=self.n_sensors)
            self.capacity, self.header, self.index, self.charge = total, full.header, full.index, full.charge
            self.counts, self.total = full.counts, full.total
            return self.index.cpu().numpy(), self.charge.cpu().numpy(), counts
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
    H.require_gpu()
    if images.dim() == 4 and images.shape[1] == 1:
        images = images[:, 0]
    if images.dim() != 3 or images.dtype not in (torch.float32, torch.uint8):
        raise TypeError("pxd_digits expects fp32 or uint8 sensor images [N, H, W] in detector units")
    if images.shape[0] == 0 or images.shape[0] % n_sensors:
        raise ValueError(f"pxd_digits: {images.shape[0]} images are not whole events of {n_sensors} sensors")
    dev = images.device if images.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = images.to(dev, non_blocking=True).contiguous()
    N, Hh, Ww = x.shape
    if N * Hh * Ww >= 2 ** 31:
        raise ValueError(f"pxd_digits: {N} x {Hh} x {Ww} pixels do not fit the int32 flat index; split the batch")
    capacity = max(1024, N * Hh * Ww // PXD_DIGITS_FRACTION) if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError("pxd_digits: capacity is negative")
    header = torch.empty(N + 1, dtype=torch.int32, device=dev)
    index = torch.empty(capacity, dtype=torch.int32, device=dev)
    charge = torch.empty(capacity, dtype=torch.uint8, device=dev)
    scratch = torch.empty(H.lib().ieagan_pxd_digits_scratch(N, Hh, Ww), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_digits", x.data_ptr(), int(x.dtype == torch.uint8), N, Hh, Ww, float(threshold), capacity,
               index.data_ptr() if capacity else None, charge.data_ptr() if capacity else None, header.data_ptr(),
               header.data_ptr() + 4 * N, scratch.data_ptr(), H.stream())
    return PXDDigits(x, float(threshold), capacity, int(n_sensors), header, index, charge)


# ---------------------------------------------------------------------------------------------------------
# detector-level validation, cluster level: connected components of the digits and their spectra (csrc/pxd_clusters.hip)
# ---------------------------------------------------------------------------------------------------------
class PXDClusters:
    """Device-side result of ``pxd_clusters``: the ``PXDDigits`` it was built from (``digits``), ``label`` int32 ``[capacity]`` (cluster
    number of digit k) and the cluster table ``first`` / ``size`` / ``charge`` / ``size_u`` / ``size_v`` int32 and ``seed`` uint8, all
    ``[capacity]`` (a batch has at most as many clusters as digits), ``counts`` int32 ``[N]`` (clusters per image), ``total`` int32
    ``[1]``.  Only the first ``min(digits.total, capacity)`` labels and the first ``total`` table rows are written."""

    def __init__(self, digits, label, first, size, charge, seed, size_u, size_v, header):
        self.digits, self.capacity, self.n_sensors, self.shape = digits, digits.capacity, digits.n_sensors, digits.shape
        self.label, self.first, self.size, self.charge, self.seed, self.size_u, self.size_v = label, first, size, charge, seed, size_u, size_v
        self.header = header
        self.counts, self.total = header[:self.shape[0]], header[self.shape[0]:]

    def cpu(self):
        """One read-back (every array packed into one device tensor, one copy, one wait) -> dict of NumPy arrays trimmed to the true
        totals: per digit ``index``, ``digit_charge``, ``label``; per cluster ``first``, ``size``, ``charge``, ``seed``, ``size_u``,
        ``size_v``, ``sensor`` (``first // (H*W) % n_sensors``), ``event``; ``counts [N]``, ``digit_counts [N]``.  Never truncated: when
        the digit total exceeds the capacity, digits and clusters are run again with ``capacity = total`` (a second read-back, on that
        path only)."""
        N, Hh, Ww = self.shape
        d = self.digits
        i32 = lambda t: t.to(torch.int32)
        packed = torch.cat([d.header, self.header, d.index, self.label, self.first, self.size, self.charge, self.size_u, self.size_v,
                            i32(d.charge), i32(self.seed)]).cpu().numpy()
        dcounts, dtotal = packed[:N].copy(), int(packed[N])
        counts, total = packed[N + 1:2 * N + 1].copy(), int(packed[2 * N + 1])
        if dtotal > self.capacity:
            full = pxd_clusters(d.images, d.threshold, capacity=dtotal, n_sensors=self.n_sensors)
            for k in ("digits", "capacity", "label", "first", "size", "charge", "seed", "size_u", "size_v", "header", "counts", "total"):
                setattr(self, k, getattr(full, k))
            return full.cpu()
        C = self.capacity
        col = lambda k, m: packed[2 * N + 2 + k * C:2 * N + 2 + k * C + m].copy()
        first = col(2, total)
        image = first // np.int32(Hh * Ww)
        return dict(index=col(0, dtotal), label=col(1, dtotal), first=first, size=col(3, total), charge=col(4, total), size_u=col(5, total),
                    size_v=col(6, total), digit_charge=col(7, dtotal).astype(np.uint8), seed=col(8, total).astype(np.uint8),
                    sensor=(image % self.n_sensors).astype(np.int32), event=(image // self.n_sensors).astype(np.int32), counts=counts,
                    digit_counts=dcounts)


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
    header = torch.empty(N + 1, dtype=torch.int32, device=dev)
    scratch = torch.empty(H.lib().ieagan_pxd_clusters_scratch(N, Hh, Ww, C), dtype=torch.int32, device=dev)
    p = (lambda t: t.data_ptr()) if C else (lambda t: None)
    with torch.cuda.device(dev):
        H.call("ieagan_pxd_clusters", p(d.index), p(d.charge), d.total.data_ptr(), N, Hh, Ww, C, p(label), p(first), p(size), p(charge),
               p(seed), p(size_u), p(size_v), header.data_ptr(), header.data_ptr() + 4 * N, scratch.data_ptr(), H.stream())
    return PXDClusters(d, label, first, size, charge, seed, size_u, size_v, header)


class PXDClusterStatistics:
    """Accumulator of per-sensor cluster spectra over batches of sensor images in detector units (``[N, H, W]`` fp32 or uint8, image ``n``
    is sensor ``n % n_sensors``), beside ``PXDStatistics``: ``update`` runs digits -> clusters -> ``ieagan_pxd_cluster_stats`` on the
    current stream and neither synchronises nor copies; ``result()`` does the single read-back.  Counters are exact int64.
    ``capacity`` (digits per update) defaults to that of ``pxd_digits``; an update whose digit total exceeds it is counted on the device
    and makes ``result()`` raise: a truncated event is never reported."""

    def __init__(self, n_sensors=40, threshold=7.0, capacity=None, device=None):
        self.n_sensors, self.threshold = int(n_sensors), float(threshold)
        self.capacity = None if capacity is None else int(capacity)
        self.device = torch.device(device) if device is not None else None
        self.reset()

    def reset(self):
        self.tables = None              # int64 [S * 640 + 1] on the device: the spectra, then the overflow counter
        self.clusters, self.shape = [], None

    def update(self, images):
        H.require_gpu()
        if images.dim() == 4 and images.shape[1] == 1:
            images = images[:, 0]
        if self.device is None:
            self.device = images.device if images.is_cuda else torch.device("cuda", torch.cuda.current_device())
        if images.dim() == 3 and self.shape is not None and self.shape != tuple(images.shape[1:]):
            raise ValueError(f"PXDClusterStatistics.update: image size {tuple(images.shape[1:])} differs from the accumulated {self.shape}")
        c = pxd_clusters(images.to(self.device, non_blocking=True), self.threshold, self.capacity, self.n_sensors)
        N, Hh, Ww = c.shape
        self.shape = (Hh, Ww)
        S = self.n_sensors
        if self.tables is None:
            self.tables = torch.zeros(S * H.PXD_CLUSTER_BINS + 1, dtype=torch.int64, device=self.device)
        p = (lambda t: t.data_ptr()) if c.capacity else (lambda t: None)
        with torch.cuda.device(self.device):
            H.call("ieagan_pxd_cluster_stats", p(c.first), p(c.size), p(c.charge), p(c.seed), p(c.size_u), p(c.size_v), c.total.data_ptr(),
                   c.digits.total.data_ptr(), N, Hh, Ww, S, c.capacity, self.tables.data_ptr(),
                   self.tables.data_ptr() + 8 * S * H.PXD_CLUSTER_BINS, H.stream())
        self.clusters.append(c.counts)
        return c

    def result(self):
        """NumPy tables: int64 ``size_spectrum [S, 64]`` (bin ``min(size, 64) - 1``), ``charge_spectrum [S, 256]`` (bin
        ``min(charge >> 3, 255)``, 8 ADU a bin), ``seed_spectrum [S, 256]``, ``size_u_spectrum`` / ``size_v_spectrum [S, 32]`` (bin
        ``min(s, 32) - 1``), ``clusters`` int32 ``[events, S]`` (clusters per image) and ``n_events``.  Raises when an update overflowed."""
        if not self.clusters:
            raise RuntimeError("PXDClusterStatistics.result() before any update()")
        S, B = self.n_sensors, H.PXD_CLUSTER_BINS
        packed = torch.cat([self.tables, torch.cat(self.clusters).to(torch.int64)]).cpu().numpy()      # the one device-to-host copy
        overflow = int(packed[S * B])
        if overflow != 0:
            raise RuntimeError(f"PXDClusterStatistics: {overflow} update(s) held more digits than the capacity"
                               f"{'' if self.capacity is None else ' of %d' % self.capacity}, their clusters are truncated: "
                               "pass a larger capacity= to PXDClusterStatistics")
        rows = packed[:S * B].reshape(S, B)
        out = {k: rows[:, a:a + n].copy() for k, (a, n) in H.PXD_CLUSTER_COLUMNS.items()}
        out["clusters"] = packed[S * B + 1:].astype(np.int32).reshape(-1, S)
        out["n_events"] = int(out["clusters"].shape[0])
        return out


def pxd_cluster_distance(real, fake):
    """Four distances between two ``PXDClusterStatistics.result()`` tables (float64, host): ``cluster_rate_rel_err`` = mean over the
    sensors with real clusters of |fake - real| / real of the mean clusters per image; ``size_w1`` (pixels), ``cluster_charge_w1`` (ADU,
    bins of 8) and ``seed_w1`` (ADU) = 1-D Wasserstein distances between the spectra pooled over the sensors and normalised to 1 (the
    construction of ``pxd_distance`` for the ADC spectrum), NaN when one side has no cluster at all."""
    r = np.asarray(real["clusters"], np.float64).mean(0)
    f = np.asarray(fake["clusters"], np.float64).mean(0)
    ok = r > 0
    out = dict(cluster_rate_rel_err=float(np.mean(np.abs(f[ok] - r[ok]) / r[ok])) if ok.any() else float("nan"))
    for name, key, width in (("size_w1", "size_spectrum", 1.0), ("cluster_charge_w1", "charge_spectrum", 8.0), ("seed_w1", "seed_spectrum", 1.0)):
        hr = np.asarray(real[key], np.float64).sum(0)
        hf = np.asarray(fake[key], np.float64).sum(0)
        if hr.sum() > 0 and hf.sum() > 0:
            out[name] = float(np.abs(np.cumsum(hf / hf.sum()) - np.cumsum(hr / hr.sum())).sum() * width)
        else:
            out[name] = float("nan")
    return out


def write_digits(path, event_offsets, sensor, ucell, vcell, charge):
    """The event file of ``produce.py`` (``.npz``): ``event_offsets`` int64 ``[events + 1]`` (the digits of event ``e`` are
    ``[event_offsets[e], event_offsets[e + 1])``), ``sensor`` uint8, ``ucell`` uint8, ``vcell`` uint16, ``charge`` uint8."""
    event_offsets = np.asarray(event_offsets, np.int64)
    cols = dict(sensor=np.asarray(sensor), ucell=np.asarray(ucell), vcell=np.asarray(vcell), charge=np.asarray(charge))
    if event_offsets.ndim != 1 or event_offsets.size < 1 or event_offsets[0] != 0 or (np.diff(event_offsets) < 0).any():
        raise ValueError("write_digits: event_offsets must start at 0 and not decrease")
    for k, v in cols.items():
        if v.ndim != 1 or v.size != event_offsets[-1]:
            raise ValueError(f"write_digits: {k} has {v.size} entries, event_offsets ends at {event_offsets[-1]}")
    if cols["sensor"].size and (cols["sensor"].max() > 255 or cols["ucell"].max() > 255 or cols["vcell"].max() > 65535):
        raise ValueError("write_digits: a sensor / ucell / vcell value does not fit the file's uint8 / uint8 / uint16 columns")
    with open(path, "wb") as fh:
        np.savez(fh, event_offsets=event_offsets, sensor=cols["sensor"].astype(np.uint8), ucell=cols["ucell"].astype(np.uint8),
                 vcell=cols["vcell"].astype(np.uint16), charge=cols["charge"].astype(np.uint8))


def read_digits(path):
    """Yields the events of a ``produce.py`` file in the format ``create_g1.generate`` puts on its queue (create_g1.py:79, read by
    ``DigitCreator.event`` :105-106): ``((sensor, ucell, vcell) lists, charges list)``."""
    with np.load(path) as t:
        off, sensor, ucell, vcell, charge = (t[k] for k in ("event_offsets", "sensor", "ucell", "vcell", "charge"))
    for e in range(off.size - 1):
        s = slice(int(off[e]), int(off[e + 1]))
        yield (sensor[s].tolist(), ucell[s].tolist(), vcell[s].tolist()), charge[s].tolist()


def count_parameters(module):
    print("Number of parameters: {}".format(sum(p.data.nelement() for p in module.parameters())))


# ---------------------------------------------------------------------------------------------------------
# checkpoint I/O, metadata and singular-value logging with the reference's signatures, file layout and key format
# (utils/__init__.py: join_strings 229, rename_weight_keys 242, save_and_sample 299, get_singular_values 572,
#  load_weights 592, write_metadata 671, save_weights 689): <outputroot>/<run_name>/{weights,logs,samples}/...
# ---------------------------------------------------------------------------------------------------------
def join_strings(delimiter, strings):
    return delimiter.join([s for s in strings if s])


def rename_weight_keys(state_dict, fragment, replacement):
    from collections import OrderedDict
    return OrderedDict((k.replace(fragment, replacement) if isinstance(k, str) else k, v) for k, v in state_dict.items())


def _run_dir(configuration, sub):
    import pathlib
    return pathlib.Path(configuration["outputroot"]).joinpath(configuration["run_name"]).joinpath(sub)


def _host_copy(sd):
    """State-dict entries are views of the network's flat arena: store detached host copies."""
    return type(sd)((k, v.detach().cpu().clone()) for k, v in sd.items())


def save_weights(G, D, state_dict, configuration, name_suffix=None, G_ema=None):
    """{G, G_optim, D, D_optim, state_dict, G_ema}[_suffix].pth under <outputroot>/<run_name>/weights; the optimizer
    files are in torch.optim.Adam's own state-dict format (``FusedAdam.state_dict``), so either implementation loads
    the other's checkpoint."""
    wdir = _run_dir(configuration, "weights")
    wdir.mkdir(parents=True, exist_ok=True)
    print("Saving weights to %s%s..." % (wdir.absolute(), "/" + name_suffix if name_suffix else ""))
    path = lambda stem: "%s/%s.pth" % (wdir.absolute(), join_strings("_", [stem, name_suffix]))
    torch.save(_host_copy(G.state_dict()), path("G"))
    torch.save(G.optim.state_dict(), path("G_optim"))
    torch.save(_host_copy(D.state_dict()), path("D"))
    torch.save(D.optim.state_dict(), path("D_optim"))
    torch.save({k: v for k, v in state_dict.items() if k != "config"}, path("state_dict"))
    if G_ema is not None:
        torch.save(_host_copy(G_ema.state_dict()), path("G_ema"))


def load_weights(G, D, state_dict, configuration, weight_name=None, G_ema=None, strict=True, load_optim=True):
    wdir = _run_dir(configuration, "weights")
    print(f"Loading {weight_name + ' ' if weight_name else ''}weights from {wdir.absolute()}...")
    path = lambda stem: wdir.joinpath(f"{join_strings('_', [stem, weight_name])}.pth").absolute()
    # always to the host first: the tensors are copied into the (already placed) flat arenas, and a data-parallel
    # rank must not create a context on GPU 0 by unpickling another rank's CUDA tensors
    read = lambda stem: torch.load(path(stem), map_location="cpu")

    def load_net(net, stem, old, new):
        sd = read(stem)
        try:
            net.load_state_dict(sd, strict=strict)
        except RuntimeError:
            print("Mismatch between file weight keys and model keys. Try renaming.")
            net.load_state_dict(rename_weight_keys(sd, old, new), strict=strict)

    if G is not None:
        load_net(G, "G", "transG", "RR_G")
        if load_optim:
            G.optim.load_state_dict(read("G_optim"))
    if D is not None:
        load_net(D, "D", "transcoder", "RR_D")
        if load_optim:
            D.optim.load_state_dict(read("D_optim"))
    saved = read("state_dict")
    for item in state_dict:
        if item in saved:
            state_dict[item] = saved[item]
    if G_ema is not None:
        load_net(G_ema, "G_ema", "transG", "RR_G")


def write_metadata(configuration, state_dict):
    import datetime
    ldir = _run_dir(configuration, "logs")
    ldir.mkdir(parents=True, exist_ok=True)
    with open(ldir.joinpath("metalog.txt").absolute(), "w") as f:
        f.write("datetime: %s\n" % str(datetime.datetime.now()))
        f.write("state: %s\n" % str(state_dict))


def get_singular_values(module, prefix):
    """{'<prefix>_<state-dict key with dots as underscores>': sigma} for every ``sv`` buffer (reference key format, e.g.
    ``G_linear_sv0``), read back with ONE device-to-host copy -- the reference does one ``.item()`` per layer, ~211 host
    synchronisations every sv_log_interval iterations."""
    names, vals = [], []
    for k, v in module.state_dict().items():
        if "sv" in k:
            names.append(k)
            vals.append(v.reshape(-1)[:1])
    if not names:
        return {}
    host = torch.cat(vals).float().cpu().tolist()
    return {f"{prefix}_{n}".replace(".", "_"): float(x) for n, x in zip(names, host)}


def denorm(x, crop=True):
    """[-1, 1] network range -> detector units [0, 255] (+ the 3-row crop): reference utils/norm.py:34-46."""
    x = torch.pow(256.0, x.float() * 0.5 + 0.5) - 1.0
    x = x.clamp(0, 255)
    return x[..., 3:-3, :] if crop else x


def save_and_sample(G, D, G_ema, z_, y_, fixed_z, fixed_y, state_dict, config):
    """Checkpoint copy + fixed-latent sample of the current generator (reference utils/__init__.py:299-365).  The
    sample is written as ``samples/fixed_samples<itr>.npy`` (detector units, [N, 1, H-6, W]); the reference's JPEG
    sheet additionally needs torchvision and is written only when that is importable."""
    save_weights(G, D, state_dict, config, "copy%d" % state_dict["itr"], G_ema if config["ema"] else None)
    if config["num_save_copies"] > 0:
        state_dict["save_num"] = (state_dict["save_num"] + 1) % config["num_save_copies"]
    which_G = G_ema if (config["ema"] and config["use_ema"]) else G
    with torch.no_grad():
        imgs = denorm(which_G(fixed_z, fixed_y).float()).cpu()
    sdir = _run_dir(config, "samples")
    sdir.mkdir(parents=True, exist_ok=True)
    np.save(str(sdir.joinpath(f"fixed_samples{state_dict['itr']}.npy").absolute()), imgs.numpy())
    try:
        from torchvision.utils import save_image
    except Exception:
        return
    save_image(imgs, sdir.joinpath(f"fixed_samples{state_dict['itr']}.jpg").absolute(), nrow=int(imgs.shape[0] ** 0.5),
               normalize=False)
