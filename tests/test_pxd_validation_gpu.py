"""Detector-level validation on the device (MI355X): the statistics kernel against the NumPy restatement of the reference's
``get_stats`` (tests/pxd_reference.py), the accumulator, ``train_fns.validate``, ``train.py --val_every`` and ``validate.py``.

Bounds: spectrum, hit counts and the occupancy histogram are integers and must be EQUAL; the occupancy is float64 from integers on
both sides (1e-12 relative); the charge is a float32 sum of ``hits`` positive terms against a float64 sum, relative error at most
``hits * 2^-24`` in any summation order; ``mean_charge`` is a mean of positive per-image ratios, so the largest per-image bound of
the sensor holds for it."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pxd_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _check(res, ref, tag):
    """``PXDStatistics.result()`` against the restatement; prints every figure before it asserts."""
    hits, ref_hits = res["hits"], ref["hits"]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.abs(res["charge"].astype(np.float64) - ref["charge"]) / ref["charge"]
    rel = np.where(ref_hits > 0, rel, 0.0)
    bound = ref_hits * 2.0 ** -24
    ok = np.isfinite(ref["mean_charge"])
    mc_rel = np.abs(res["mean_charge"][ok] - ref["mean_charge"][ok]) / ref["mean_charge"][ok]
    mc_bound = bound.max(0)[ok]
    occ_rel = np.abs(res["occupancy"] - ref["occupancy"]) / np.maximum(ref["occupancy"], 1e-300)
    print(f"{tag}: events {res['n_events']} hits/image {ref_hits.min()}..{ref_hits.max()} occupancy {ref['occupancy'].min():.5f}.."
          f"{ref['occupancy'].max():.5f} overflow {ref['occ_overflow']} charge rel err max {rel.max():.3e} (bound {bound.max():.3e}) "
          f"mean_charge rel err max {mc_rel.max() if mc_rel.size else 0.0:.3e} occupancy rel err max {occ_rel.max():.3e}")
    assert res["n_events"] == ref["n_events"]
    assert np.array_equal(res["spectrum"], ref["spectrum"]), tag
    assert np.array_equal(hits, ref_hits), tag
    assert np.array_equal(res["occ_hist"], ref["occ_hist"]) and res["occ_overflow"] == ref["occ_overflow"], tag
    assert (occ_rel <= 1e-12).all(), tag
    assert (rel <= bound).all(), (tag, float(rel.max()))
    assert np.array_equal(res["charge"][ref_hits == 0], np.zeros((ref_hits == 0).sum(), np.float32))
    assert np.array_equal(np.isnan(res["mean_charge"]), ~ok), tag
    assert (mc_rel <= mc_bound).all(), (tag, float(mc_rel.max()) if mc_rel.size else 0.0)


CASES = [(40, 250, 768, 40, 0.01), (40, 58, 64, 40, 0.01), (7, 13, 37, 7, 0.3), (80, 250, 768, 40, 0.01)]


@pytest.mark.parametrize("kind", ["u8", "f32"])
@pytest.mark.parametrize("n,h,w,s,p", CASES, ids=["40x250x768", "40x58x64", "7x13x37", "80x250x768"])
def test_kernel_against_numpy_restatement(kind, n, h, w, s, p):
    import utils
    ev = (R.synthetic_u8 if kind == "u8" else R.synthetic_f32)(n, h, w, seed=17 + n + h, p_hit=p)
    ref = R.get_stats(ev, s, threshold=7.0)
    if h * w >= 58 * 64 and p == 0.01:
        if (h, w) == (250, 768):          # the data the bounds were written for: no empty sensor, occupancies inside the histogram's range
            assert ref["hits"].min() >= 1500 and 0.008 < ref["occupancy"].min() and ref["occupancy"].max() < 0.012
        assert np.isfinite(ref["mean_charge"]).all() and ref["occ_overflow"] == 0
    acc = utils.PXDStatistics(n_sensors=s, threshold=7.0, device=DEV)
    hits, charge = acc.update(torch.from_numpy(ev).to(DEV))
    assert hits.is_cuda and hits.dtype == torch.int32 and charge.dtype == torch.float32 and hits.shape == (n,)
    res = acc.result()
    assert res["spectrum"].sum() == n * h * w           # every pixel is in exactly one bin
    _check(res, ref, f"{kind} {n}x{h}x{w}")


def test_unaligned_views_and_other_thresholds():
    """An image batch that starts 1 element (4 bytes / 1 byte) past a 16-byte boundary, and cuts other than 7 ADU (bin 1 fills)."""
    import utils
    for kind, gen in (("u8", R.synthetic_u8), ("f32", R.synthetic_f32)):
        ev = gen(6, 21, 53, seed=3, p_hit=0.2)
        t = torch.from_numpy(ev).to(DEV)
        buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
        buf[1:].copy_(t.reshape(-1))
        view = buf[1:].view(6, 21, 53)
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        for thr in (7.0, 3.0, 0.0, 100.5):
            acc = utils.PXDStatistics(n_sensors=3, threshold=thr, device=DEV)
            acc.update(view)
            _check(acc.result(), R.get_stats(ev, 3, threshold=thr), f"{kind} offset view, cut {thr}")


def test_updates_accumulate_and_charge_is_bit_reproducible():
    import utils
    ev = torch.from_numpy(R.synthetic_f32(40, 250, 768, seed=5)).to(DEV)
    acc = utils.PXDStatistics(n_sensors=40, device=DEV)
    h1, c1 = acc.update(ev)
    one = acc.spectrum.clone()
    h2, c2 = acc.update(ev)
    assert torch.equal(c1, c2) and torch.equal(h1, h2)
    assert torch.equal(acc.spectrum, 2 * one)
    res = acc.result()
    assert res["n_events"] == 2 and np.array_equal(res["hits"][0], res["hits"][1])
    assert np.array_equal(res["charge"][0].view(np.int32), res["charge"][1].view(np.int32))
    acc.reset()
    acc.update(ev[:40])
    assert torch.equal(acc.spectrum, one) and acc.result()["n_events"] == 1
    with pytest.raises(ValueError):
        acc.update(ev[:39])
    with pytest.raises(ValueError):
        acc.update(ev[:, :100])


def _networks(ema=True, **over):
    import model
    from defaults import default_config
    cfg = default_config()
    cfg.update(device="cuda", resolution=64, H_base=1, ema=ema, val_events=2, outputroot=None, **over)
    torch.manual_seed(1234)
    with contextlib.redirect_stdout(io.StringIO()):
        G = model.Generator(**cfg).to(DEV)
        G_ema = model.Generator(**dict(cfg, skip_init=True, no_optim=True)).to(DEV)
    G_ema.load_state_dict(G.state_dict())
    return cfg, G, G_ema


def test_generator_export_into_statistics_end_to_end():
    import utils
    cfg, G, _ = _networks()
    G.eval()
    gen = torch.Generator(device=DEV).manual_seed(7)
    acc = utils.PXDStatistics(n_sensors=40, threshold=7.0, device=DEV)
    outs = []
    with torch.no_grad():
        for _ in range(2):
            z = torch.randn(40, G.dim_z, generator=gen, device=DEV)
            rdof = torch.randn(40, G.rdof_dim, generator=gen, device=DEV)
            x = G(z, torch.arange(40, device=DEV), rdof=rdof, export=True)
            assert x.shape == (40, 58, 64) and x.dtype == torch.float32
            acc.update(x)
            outs.append(x.cpu().numpy())
    _check(acc.result(), R.get_stats(np.concatenate(outs), 40, threshold=7.0), "G(export=True) 2 events 40x58x64")


def test_update_neither_synchronises_nor_copies_to_the_host():
    """``update`` is captured into a HIP graph: a synchronising call or a device-to-host copy inside a capture raises."""
    import utils
    ev = torch.from_numpy(R.synthetic_u8(40, 58, 64, seed=9)).to(DEV)
    ref = R.get_stats(ev.cpu().numpy(), 40)
    acc = utils.PXDStatistics(n_sensors=40, device=DEV)
    acc.update(ev)                      # eager: loads the library, allocates the spectrum
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        acc.update(ev)
    g.replay()
    res = acc.result()
    assert res["n_events"] == 2
    assert np.array_equal(res["spectrum"], 2 * ref["spectrum"])
    assert np.array_equal(res["hits"], np.concatenate([ref["hits"], ref["hits"]]))
    del g


def _snapshot(nets):
    snap = dict(cpu=torch.get_rng_state().clone(), cuda=torch.cuda.get_rng_state(DEV).clone(), np=np.random.get_state())
    snap["flags"] = [[m.training for m in net.modules()] for net in nets]
    snap["state"] = [{k: v.detach().clone() for k, v in net.state_dict().items()} for net in nets]
    return snap


def _assert_unchanged(before, after):
    assert torch.equal(before["cpu"], after["cpu"]) and torch.equal(before["cuda"], after["cuda"])
    for a, b in zip(before["np"], after["np"]):
        assert np.array_equal(a, b)
    assert before["flags"] == after["flags"]
    for sa, sb in zip(before["state"], after["state"]):
        assert list(sa) == list(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("ema", [True, False])
def test_validate_observes_only(ema, tmp_path):
    import train, train_fns, utils
    cfg, G, G_ema = _networks(ema=ema)
    cfg.update(outputroot=str(tmp_path))
    assert any(k.endswith("u0") for k in G.state_dict()) and any("stored_mean" in k or "running_mean" in k for k in G.state_dict())
    real = utils.PXDStatistics(n_sensors=40, threshold=cfg["val_threshold"], device=DEV)
    for i in range(2):
        real.update(torch.from_numpy(train.synthetic_event(40, 58, 64, 100 + i)))
    G.train()
    G_ema.train()
    with torch.no_grad():               # one training-mode pass first: the plan / arena exist, u0 and the running statistics have moved
        G(torch.randn(40, G.dim_z, device=DEV), torch.arange(40, device=DEV))
    torch.cuda.synchronize()
    before = _snapshot((G, G_ema))
    rec = train_fns.validate(G, G_ema, real, {"itr": 5}, cfg)
    torch.cuda.synchronize()
    _assert_unchanged(before, _snapshot((G, G_ema)))
    assert rec["which"] == ("G_ema" if ema else "G") and rec["itr"] == 5 and rec["n_events"] == 2
    rec2 = train_fns.validate(G, G_ema, real.result(), {"itr": 6}, cfg)        # its own generator: the same events, the same numbers
    for k in ("occ_rel_err", "charge_rel_err", "spectrum_w1"):
        assert np.isfinite(rec[k]) and rec[k] >= 0 and rec2[k] == rec[k], (k, rec, rec2)
    lines = open(os.path.join(str(tmp_path), cfg["run_name"], "logs", "validation_rank0.jsonl")).read().strip().splitlines()
    assert [json.loads(ln) for ln in lines] == [rec, rec2]
    assert set(rec) == {"itr", "n_events", "which", "occ_rel_err", "charge_rel_err", "spectrum_w1"}
    _assert_unchanged(before, _snapshot((G, G_ema)))


RUN_ARGS = ["--synthetic", "4", "--resolution", "64", "--H_base", "1", "--max_iters", "4", "--val_every", "2", "--val_events", "2"]


def _train(tmp_path, *extra):
    """``clip_norm`` is set because with the shipped ``clip_norm: null`` the generator's optimiser never steps (reference quirk kept by
    train_fns): the saved G_optim.pth could not be at step 4, and validation would see the same G four times."""
    import train
    cfg = train.parse(RUN_ARGS + ["--clip_norm", "1e9", "--outputroot", str(tmp_path)] + list(extra))
    with contextlib.redirect_stdout(io.StringIO()):
        state = train.run(cfg)
    run_dir = os.path.join(str(tmp_path), cfg["run_name"])
    return cfg, state, run_dir


@pytest.mark.parametrize("mode", ["eager", "graph", "graph_no_ema"])
def test_train_run_with_periodic_validation(mode, tmp_path):
    extra = {"eager": [], "graph": ["--hip_graph", "true"], "graph_no_ema": ["--hip_graph", "true", "--ema", "false"]}[mode]
    cfg, state, run_dir = _train(tmp_path, *extra)
    assert state["itr"] == 4
    lines = open(os.path.join(run_dir, "logs", "validation_rank0.jsonl")).read().strip().splitlines()
    recs = [json.loads(ln) for ln in lines]
    print(mode, recs)
    assert [r["itr"] for r in recs] == [2, 4]
    for r in recs:
        assert r["n_events"] == 2 and r["which"] == ("G" if mode == "graph_no_ema" else "G_ema")
        for k in ("occ_rel_err", "charge_rel_err", "spectrum_w1"):
            assert np.isfinite(r[k]) and r[k] >= 0, r
    metrics = [json.loads(ln) for ln in open(os.path.join(run_dir, "logs", "metrics_rank0.jsonl")).read().strip().splitlines()]
    assert len(metrics) == 4
    for m in metrics:
        assert all(np.isfinite(v) for v in m.values()), m
    osd = torch.load(os.path.join(run_dir, "weights", "G_optim.pth"))
    assert float(osd["state"][0]["step"]) == 4.0
    sd = torch.load(os.path.join(run_dir, "weights", "G.pth"))
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())


def test_validation_is_off_by_default(tmp_path):
    cfg, state, run_dir = _train(tmp_path, "--val_every", "0")
    assert state["itr"] == 4
    assert not os.path.exists(os.path.join(run_dir, "logs", "validation_rank0.jsonl"))


def test_validate_tool_as_a_child_process(tmp_path):
    import train
    cfg, state, run_dir = _train(tmp_path)
    tool = os.path.join(ROOT, "iea-gan_amd", "validate.py")
    out = os.path.join(str(tmp_path), "tables.npz")
    geom = ["--resolution", "64", "--H_base", "1"]
    for ema in ([], ["--use_ema"]):
        p = subprocess.run([sys.executable, tool, "--weights", os.path.join(run_dir, "weights"), "--synthetic", "3", "--events", "3",
                            "--out", out] + ema + geom, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        rec = json.loads(p.stdout.strip().splitlines()[-1])
        assert {"occ_rel_err", "charge_rel_err", "spectrum_w1"} <= set(rec) and rec["n_events"] == 3
        assert rec["which"] == ("G_ema" if ema else "G")
        assert all(np.isfinite(rec[k]) and rec[k] >= 0 for k in ("occ_rel_err", "charge_rel_err", "spectrum_w1")), rec
        t = np.load(out)
        for side in ("real", "fake"):
            assert t[f"{side}_spectrum"].shape == (40, 251) and t[f"{side}_occupancy"].shape == (40,)
            assert t[f"{side}_mean_charge"].shape == (40,) and t[f"{side}_occ_hist"].shape == (200,)
            assert int(t[f"{side}_n_events"]) == 3 and t[f"{side}_spectrum"].sum() == 3 * 40 * 58 * 64
        assert t["bin_edges"].shape == (252,)
    d = os.path.join(str(tmp_path), "events")
    os.makedirs(d)
    for i in range(3):
        np.save(os.path.join(d, f"event_{i}.npy"), train.synthetic_event(40, 58, 64, 50 + i))
    p = subprocess.run([sys.executable, tool, "--dataroot", d, "--compare", d, "--events", "3", "--out", out] + geom,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["occ_rel_err"] == 0.0 and rec["charge_rel_err"] == 0.0 and rec["spectrum_w1"] == 0.0 and rec["which"] == "files"
    t = np.load(out)
    assert np.array_equal(t["real_spectrum"], t["fake_spectrum"]) and int(t["fake_n_events"]) == 3
