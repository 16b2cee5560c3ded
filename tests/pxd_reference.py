"""NumPy restatement of the reference's detector-level statistics, the checker of ``utils.PXDStatistics`` (tests only).

Restates, per batch of sensor images in detector units (reference paths relative to its repository root):
* ``Evaluation/eval_all.py:115``  the cut: ``imgs[imgs < THRESHOLD] = 0`` (THRESHOLD = 7);
* ``:89``                         ``mask = imgs > 0``;
* ``:90, :100``                   per-image occupancy = mean of the mask, per-sensor occupancy = its mean over the events;
* ``:91-96, :99``                 per-image mean hit charge = sum(where(mask, imgs, 0)) / sum(mask), per sensor its mean over the events;
* ``:77, :97``                    the ADC spectrum over the edges ``[-1, 1, 7] + linspace(8, 256, 249)`` (``np.histogram``; the reference
                                  fills one pooled histogram, here one per sensor: their sum over the sensors is the reference's);
* ``:78, :98``                    the histogram of the per-image occupancies, 200 bins over [0, 0.02).
Deviation, shared with the product and stated in its docstring: the occupancy bin is decided in integers,
``(hits * 10000) // (H * W)`` -- with 250 x 768 pixels every 96th hit count sits exactly on an edge of ``linspace(0, 0.02, 201)``, where
a float comparison may round either way.  Sums are float64.  Image ``n`` is sensor ``n % n_sensors`` (``y = arange(40).repeat(E)``).
"""
import numpy as np

EDGES = np.array([-1.0, 1.0, 7.0] + list(np.linspace(8, 256, 249)))


def get_stats(images, n_sensors, threshold=7.0):
    imgs = np.asarray(images).astype(np.float64)
    N, H, W = imgs.shape
    assert N % n_sensors == 0
    imgs = np.where(imgs < threshold, 0.0, imgs)                # eval_all.py:115
    mask = imgs > 0                                             # :89
    hits = mask.reshape(N, -1).sum(1)
    charge = np.where(mask, imgs, 0.0).reshape(N, -1).sum(1)    # :93
    spectrum = np.zeros((n_sensors, len(EDGES) - 1), np.int64)
    for n in range(N):
        spectrum[n % n_sensors] += np.histogram(imgs[n].ravel(), EDGES)[0]      # :97
    hits_es = hits.reshape(-1, n_sensors)
    charge_es = charge.reshape(-1, n_sensors)
    occupancy = (hits_es / float(H * W)).mean(0)                # :90, :100
    has = hits_es > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        per = charge_es / hits_es                               # :91-95 (NaN where an image has no hit, as in the reference)
        mean_charge = np.where(has, per, 0.0).sum(0) / has.sum(0)      # == per.mean(0) (:99) whenever that is finite
    b = (hits * 10000) // (H * W)                               # :78, :98 with the integer edge rule
    occ_hist = np.bincount(b[b < 200], minlength=200).astype(np.int64)
    return dict(spectrum=spectrum, hits=hits_es, charge=charge_es, occupancy=occupancy, mean_charge=mean_charge, occ_hist=occ_hist,
                occ_overflow=int((b >= 200).sum()), n_events=N // n_sensors)


def synthetic_u8(n, h, w, seed, p_hit=0.01):
    """``train.synthetic_event``-like uint8 images, plus planted values either side of the cut and at the ends of the spectrum."""
    rng = np.random.Generator(np.random.PCG64([seed, 11]))
    hit = rng.random((n, h, w)) < p_hit
    ev = np.where(hit, rng.uniform(8, 255, (n, h, w)), 0.0).astype(np.uint8)
    flat = ev.reshape(n, -1)
    plant = np.array([1, 5, 6, 7, 8, 9, 254, 255], np.uint8)
    for i in range(n):
        pos = rng.choice(flat.shape[1], size=len(plant), replace=False)
        flat[i, pos] = plant
    return ev


def synthetic_f32(n, h, w, seed, p_hit=0.01):
    """fp32 images with fractional hit values, values planted on both sides of 1, 7, 8 and 255, and values in [6.78, 7) that the
    export epilogue lets through and the 7 ADU cut must remove."""
    rng = np.random.Generator(np.random.PCG64([seed, 13]))
    hit = rng.random((n, h, w)) < p_hit
    ev = np.where(hit, rng.uniform(8, 255, (n, h, w)), 0.0).astype(np.float32)
    flat = ev.reshape(n, -1)
    f = np.float32
    plant = [0.999, 1.0, np.nextafter(f(1), f(0)), np.nextafter(f(1), f(2)), 6.78, 6.9, 6.99, np.nextafter(f(7), f(0)), 7.0,
             np.nextafter(f(7), f(8)), 7.5, np.nextafter(f(8), f(0)), 8.0, np.nextafter(f(8), f(9)), 254.99,
             np.nextafter(f(255), f(0)), 255.0]
    plant = np.array(plant, np.float32)
    for i in range(n):
        pos = rng.choice(flat.shape[1], size=len(plant), replace=False)
        flat[i, pos] = plant
    return ev
