#!/usr/bin/env python3
"""Benchmark of the IEA-GAN G+D train step on MI355X (BASELINE.json metric: events/s).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Workload at every N: BASELINE configs[1] per GPU -- one event (40 sensors x 256x768, i.e. 250x768 padded)
per step, bf16 activations, hinge loss only, RRM on; synthetic PXD-like events (a rotation of 4 different ones, so the
losses stay in their non-saturated regime), seeded orthogonal weights.
N > 1: events shard data-parallel (one per rank and step), gradients are all-reduced over RCCL
(``parallel.py``); value = events all ranks processed / max-over-ranks wall time ("weak" scaling).

A plain run sets up, warms up, times ``--steps`` steps of configs[1] and prints one JSON line (rank 0) with ``metric``, ``value``
(events/s), ``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step`` and the losses of the last timed step.  ``--dump-outputs DIR``
also writes what that last step computed (the five losses; G / D / G_ema state after it, a fixed seeded sample) as DIR/<name>.npy.
``--full`` adds everything else:
* ``roofline``: the kernel family with the largest share of GPU time.  ``achieved`` = ALGORITHMIC bytes (or FLOPs) of its
  launches -- the layer-granular figures of SURVEY 8d, ``tools/arch_calc.py``: conv bytes = 2 N (Hs Ws Cin + H W Cout) --
  divided by their HIP-event time measured in this run on the launch stream; ``launcher_accounted`` repeats the fraction with
  the bytes the launches really have to move (plus ReLU masks / shortcut operands); ``traffic`` = HBM bytes per launch from
  the committed rocprofv3 PMC passes (NOT measured in this run: see ``traffic_source``).
* ``families``: every family with its HBM and MFMA fractions.
* ``cpu_baseline``: the CPU oracle (plain PyTorch restatement of the reference step, oracle/) timed on this host.
* ``dp_exchange_slack_ms`` (data parallel): a few steps with HIP-event pairs around the gradient exchange.
* ``configs3`` (N = 1, unless --no-configs3): the same measurement for BASELINE configs[3] -- 4 events per GPU and step with
  DiffAugment + CR_DiffAug consistency regularisation + uniformity loss; ``configs4``: configs[1] with the fp8 conv path.
"""
import argparse
import contextlib
import faulthandler
import io
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "iea-gan_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np
import torch
import torch.distributed as dist

PEAK_BF16_TFLOPS = 2500.0     # dense bf16 MFMA peak of MI355X (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0         # HBM3E spec (6.3 TB/s measured achievable)
STEP_GFLOP = 5328.8           # algorithmic work per event-step (SURVEY 8d / BASELINE.md section 3)
BENCH_LR = 1e-7               # see bench_config(): keeps both hinge terms of D unsaturated over the timed steps
CPU_FULL_FILES = ("r04_cpu_full.json", "r03_cpu_full.json", "r02_cpu_full.json")                 # newest first
PMC_FILES = ("r04_pmc_traffic.json", "r04a_pmc_traffic.json", "r03_pmc_traffic.json", "r02_pmc_traffic.json")      # newest first


def synth_event(n, h, w, seed):
    """PXD-like synthetic event: background -1, ~1 % log-normalised hits, 4e-3 dequantisation noise."""
    rng = np.random.Generator(np.random.PCG64([seed, 77]))
    hit = rng.random((n, 1, h, w)) < 0.01
    u = rng.uniform(0.03, 1.0, (n, 1, h, w))
    img = np.where(hit, np.log(255.0 * u + 1.0) / math.log(256.0), 0.0) + 4e-3 * rng.random((n, 1, h, w))
    return torch.from_numpy((2.0 * img - 1.0).astype(np.float32))


def bench_config(which=1):
    from defaults import default_config
    cfg = default_config()
    # clip_norm must be finite or the reference's control flow never steps G's optimiser -- a benchmark without
    # the G update would skip real work.
    cfg.update(device="cuda", clip_norm=1e9)
    # Regime of the timed steps: both discriminator hinge terms must stay ACTIVE (relu(1 - D(x)) > 0 and relu(1 + D(G(z))) > 0), or one
    # of the two full D backward passes propagates exact zeros (round-2 review).  A randomly initialised D puts every logit near -11 and
    # the shipped lr of 5e-5 (Adam, beta1 = 0: every weight moves by ~lr per step) swings them through the margin within two steps, so
    # the bench (i) centres the logits once with D.linear0.bias (measure(): calibrate) and (ii) trains with a learning rate small enough
    # that 40 steps stay inside the margin.  Neither changes the arithmetic of a step: same launches, same bytes, same FLOPs.
    cfg.update(G_lr=BENCH_LR, D_lr=BENCH_LR)
    if which == 1:      # configs[1]: hinge loss only, RRM on
        cfg.update(contra_lambda=0.0, IEA_loss=False, Uniformity_loss=False)
    elif which == 3:    # configs[3]: 4 events/GPU, diff_aug + cr_diff_aug + uniformity loss (full default loss composition)
        cfg.update(events_per_step=4, Con_reg=True, diff_aug=True, Uniformity_loss=True)
    else:               # configs[4]: configs[1] with e4m3 MFMA operands in the forward of the C >= 64 3x3 layers
        cfg.update(contra_lambda=0.0, IEA_loss=False, Uniformity_loss=False, conv_dtype="fp8")
    return cfg


def physical_cores():
    try:
        pairs, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    pairs.add((phys, core))
                phys = core = None
        return len(pairs) or None
    except OSError:
        return None


def cpu_threads():
    """Threads for the CPU leg: the cores this process may really use -- min(affinity mask, physical cores, cgroup CPU quota)."""
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = max(1, int(float(q) / float(per)))
    except (OSError, ValueError):
        pass
    phys = physical_cores()
    n = min(x for x in (avail, phys, quota) if x)
    return n, {"host_logical_cpus_available": avail, "host_physical_cores": phys, "cgroup_cpu_quota": quota}


def cpu_baseline(cfg, mode="sub", threads=None):
    """The oracle's train step at full 256x768 resolution on this host's cores.  ``full``: all 40 sensors, 1 warm-up + 1
    timed step (minutes of CPU time and ~30 GB of host memory).  ``sub`` (default, bounded to tens of
    seconds): the first 8 of the 40 sensors -- BatchNorm / RRM / losses over that sub-event -- one timed step, scaled
    by 40 / 8 (the conv work, > 95 % of the CPU time, is linear in the sensor count)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ieagan_oracle as O
    auto, host = cpu_threads()
    threads = threads or auto
    torch.set_num_threads(threads)
    sensors = 40 if mode == "full" else 8
    c = dict(cfg, device="cpu", events_per_step=1)
    g_state, d_state = O.synth_nets(c, 101, 202)
    h, w = c["resolution"], c["resolution"] * c["H_base"]
    x = O.synth_event(sensors, h, w, 303)
    y = torch.arange(sensors)
    gen = torch.Generator().manual_seed(1)
    noise = {}
    for ph in "dg":
        noise["z_" + ph] = torch.randn(sensors, 128, generator=gen)
        noise["rdof_" + ph] = torch.randn(sensors, 4, generator=gen)
        noise["aug_" + ph] = O.diffaug_draws(sensors, h, w, generator=gen)
    times = []
    for rep in range(2 if mode == "full" else 1):
        gsd, gp = O.as_trainable(g_state)
        dsd, dp = O.as_trainable(d_state)
        ts = O.TrainState(gsd, dsd, gp, dp, c)
        t0 = time.time()
        O.train_step(ts, x, y, noise, itr=1)
        times.append(time.time() - t0)
    dt = times[-1]
    sample = (f"one oracle train step (fp32, PyTorch CPU) at 256x768 on all 40 sensors after one warm-up step: {dt:.1f} s "
              f"(warm-up {times[0]:.1f} s)" if mode == "full" else
              f"one oracle train step (fp32, PyTorch CPU) at 256x768 on {sensors} of 40 sensors: {dt:.1f} s, "
              f"scaled x{40 // sensors} to a full event")
    torch.set_num_threads(1)           # park the intra-op pool: nothing after the CPU leg needs it (and it must be idle at exit)
    res = {"value": 1.0 / (dt * 40.0 / sensors), "unit": "events/s", "cores": threads, "kind": "port", "sample": sample, **host}
    if mode != "full":
        # next to the bounded sample: the full 40-sensor step as last recorded with --cpu-baseline full (committed, not re-timed here)
        for name in CPU_FULL_FILES:
            path = os.path.join(ROOT, "profiles", name)
            if os.path.exists(path):
                try:
                    full = json.load(open(path)).get("cpu_baseline") or {}
                    res["full_event_recorded"] = {"value": full.get("value"), "unit": full.get("unit"), "cores": full.get("cores"),
                                                  "sample": full.get("sample"), "source": f"profiles/{name}"}
                except Exception as e:
                    print(f"bench: cannot read {path}: {e}", file=sys.stderr)
                break
    return res


def pmc_families():
    """HBM bytes per launch from the committed rocprofv3 PMC passes (FETCH_SIZE / WRITE_SIZE, corrected as the guide says)."""
    for name in PMC_FILES:
        path = os.path.join(ROOT, "profiles", name)
        if os.path.exists(path):
            try:
                d = json.load(open(path))
                return d.get("families", {}), f"profiles/{name}" + (f" @ {d['git_head']}" if d.get("git_head") else "")
            except Exception as e:         # a malformed file must not silently turn into 'no traffic figure'
                print(f"bench: cannot read {path}: {e}", file=sys.stderr)
    return {}, None


def git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True, timeout=10).stdout.strip() or None
    except Exception:
        return None


def roofline_of(r, total_ms, pmc, pmc_src):
    """Roofline block of one kernel family record (bytes_min / flops = tools/arch_calc.py's layer-granular figures)."""
    ridge = PEAK_BF16_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)          # ~312 FLOP/B
    sec = r["ms"] * 1e-3
    bmin = r.get("bytes_min") or r["bytes"]
    hbm = bmin / sec / 1e9 if bmin else None
    hbm_l = r["bytes"] / sec / 1e9 if r["bytes"] else None
    tf = r["flops"] / sec / 1e12 if r["flops"] else None
    ai = r["flops"] / bmin if (r["flops"] and bmin) else None
    mfma_bound = ai is not None and ai >= ridge
    out = {"kernel": r["name"], "bound": "mfma" if mfma_bound else "hbm",
           "achieved": tf if mfma_bound else hbm, "peak": PEAK_BF16_TFLOPS if mfma_bound else PEAK_HBM_GBS,
           "unit": "TFLOP/s" if mfma_bound else "GB/s"}
    out["frac"] = (out["achieved"] / out["peak"]) if out["achieved"] is not None else None
    fam = pmc.get(r["name"].split(" ")[0])
    out.update(traffic=fam["hbm_bytes_per_launch"] if fam else None,
               traffic_source=(pmc_src + " (rocprofv3 --pmc passes of that build; not measured in this run)") if fam else None,
               hbm_frac=hbm / PEAK_HBM_GBS if hbm else None, mfma_frac=tf / PEAK_BF16_TFLOPS if tf else None,
               launcher_accounted={"GBs": hbm_l, "hbm_frac": hbm_l / PEAK_HBM_GBS if hbm_l else None,
                                   "bytes_per_launch": r["bytes"] / max(r["launches"], 1)},
               algorithmic_bytes_per_launch=bmin / max(r["launches"], 1),
               algorithmic_flops_per_launch=r["flops"] / max(r["launches"], 1), launches=r["launches"],
               avg_launch_ms=r["ms"] / max(r["launches"], 1), share_of_kernel_time=r["ms"] / total_ms,
               arithmetic_intensity=ai)
    return out


DUMP_STATE_SAMPLE = 4_000_000      # elements per network state kept by --dump-outputs (3 networks x 16 MB + the losses < 64 MB)
DUMP_SEED = 20240917               # fixed: the same element positions are sampled in every run and every build


def timed_outputs(losses, nets):
    """The arrays a caller of the timed train step receives: the five losses it returns (float64) and the post-step state of
    G, D and G_ema -- every floating-point state_dict entry (parameters, BatchNorm / spectral-norm buffers) flattened in
    state_dict order to float32; above DUMP_STATE_SAMPLE elements a fixed seeded sample of positions (sorted) is kept."""
    out = {f"loss_{k}": np.array([v], dtype=np.float64) for k, v in losses.items()}
    for name, net in nets.items():
        flat = torch.cat([t.detach().reshape(-1).float().cpu() for t in net.state_dict().values() if t.is_floating_point()]).numpy()
        if flat.size > DUMP_STATE_SAMPLE:
            flat = flat[np.sort(np.random.default_rng(DUMP_SEED).choice(flat.size, DUMP_STATE_SAMPLE, replace=False))]
        out[f"{name}_state"] = flat.astype(np.float32)
    return out


def write_outputs(d, arrays):
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)


def measure(cfg, args, rank, world, local, tag):
    """Build the networks for ``cfg``, warm up, time ``args.steps`` steps, optionally time every kernel family."""
    import _hip
    import model
    import parallel
    import train_fns
    import utils
    dev = torch.device("cuda", local)
    E = int(cfg.get("events_per_step", 1))
    force_dp = bool(os.environ.get("IEAGAN_FORCE_DP")) and dist.is_initialized()     # 1-rank rehearsal of the DP path
    utils.seed_rng(cfg["seed"])
    # the seeded initialisation runs on the host: on one intra-op thread, so that its roundings (orthogonal init's QR) and with them
    # the weights every run starts from do not depend on the thread count of the machine
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    with contextlib.redirect_stdout(io.StringIO()):
        G = model.Generator(**cfg).to(dev)
        D = model.Discriminator(**cfg).to(dev)
        G_ema = model.Generator(**dict(cfg, skip_init=True, no_optim=True)).to(dev)
        ema = utils.apply_ema(G, G_ema, cfg["ema_decay"], cfg["ema_start"])
    torch.set_num_threads(threads)
    GD = model.G_D(G, D)
    h, w = cfg["resolution"], cfg["resolution"] * cfg["H_base"]
    n_rot = 4
    xs = [torch.cat([synth_event(40, h, w, cfg["seed"] + 1000 * rank + 10 * i + e) for e in range(E)]).to(dev) for i in range(n_rot)]
    y = torch.arange(40, device=dev).repeat(E)
    # calibrate: centre the logits of this random initialisation between the two hinge margins (same on every rank: same seed)
    G.train(); D.train()
    with torch.no_grad():
        zc = torch.randn(40 * E, G.dim_z, device=dev)
        lf = D(G(zc, y), y)[2] if cfg["conditional_strategy"] == "Contra" else D(G(zc, y), y)
        lr_ = D(xs[0], y)[2] if cfg["conditional_strategy"] == "Contra" else D(xs[0], y)
        D.linear0.bias.sub_(0.5 * (lf.float().mean() + lr_.float().mean()))
    if world > 1 or force_dp:
        parallel.set_context(parallel.GradSync(overlap=True, force=force_dp))
        for net in (G, D):
            net._prepare()
            parallel.broadcast_flat(net._arena.flat)
        parallel.broadcast_flat(ema._arenas()[1].flat)
    z_, y_ = utils.prepare_z_y(40 * E, G.dim_z, cfg["n_classes"], device=dev)
    state = {"itr": 0}
    train = train_fns.GAN_training_function(G, D, GD, z_, y_, ema, state, cfg, dev)
    G.train(); D.train(); G_ema.train()

    trace = []

    def step():
        state["itr"] += 1
        out = train(xs[state["itr"] % n_rot], y)
        trace.append(out)
        return out

    for _ in range(max(args.warmup, 3 if cfg["hip_graph"] else 0)):    # graph mode: 2 eager steps + capture
        step()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # per-kernel timing is part of the full record (or asked for by --shape-tags); a plain run times the steps alone
    timing = not args.no_kernel_timing and (args.full or args.shape_tags)
    eager_timing = timing and not cfg["hip_graph"]
    if eager_timing:            # eager mode: HIP events bracket every launch inside the timed region itself
        _hip.call("ieagan_prof_reset")
        _hip.prof_enable(True)
    steps = args.steps if tag == "configs1" else max(2, min(args.steps, 5))
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    fence()
    dt = time.perf_counter() - t0
    if eager_timing:
        _hip.prof_enable(False)
    # what the last timed step handed its caller: read before any later pass (kernel timing, DP slack) moves the weights on
    dumped = timed_outputs(out, {"G": G, "D": D, "G_ema": G_ema}) if (args.dump_outputs and tag == "configs1" and rank == 0) else None
    prof_steps = steps
    recs = None
    if timing and cfg["hip_graph"]:
        # A replayed HIP graph cannot carry per-launch event pairs: time the SAME launches (same shapes,
        # same kernels) in eager steps right after the timed region.
        # The weight-gradient launches of these steps stay on the main stream (in the timed region they run on a side stream under
        # the dgrad chain): a launch's duration is then its own, as in the rocprofv3 kernel trace, which serialises dispatches too.
        import ops
        prof_steps = min(steps, 3)
        side = [ops.opts_of_net(net).wgrad_side_stream for net in (G, D)]
        for net in (G, D):              # per-network execution option (ops.ExecOptions): only the two networks being timed change
            ops.set_options(net, wgrad_side_stream=False)
        _hip.call("ieagan_prof_reset")
        _hip.prof_enable(2 if args.shape_tags else 1)
        for _ in range(prof_steps):
            state["itr"] += 1
            train.step_tensor(xs[state["itr"] % n_rot], y)
        torch.cuda.synchronize()
        _hip.prof_enable(False)
        for net, sv in zip((G, D), side):
            ops.set_options(net, wgrad_side_stream=sv)
    if timing:
        recs = sorted(_hip.prof_collect(), key=lambda r: -r["ms"])
    if world > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    dp_slack = None
    sync = parallel.get_context()
    if sync is not None and args.full:
        # data parallel: does the side stream's work (all-reduce + ortho + Adam + EMA) finish before the main stream asks for it?
        # HIP-event pairs (side stream done, main stream arrives at its wait) over a few steps AFTER the timed region.
        sync.trace = True
        for _ in range(5):
            step()
        dp_slack = {k: [round(v, 3) for v in vs] for k, vs in sync.slack_ms().items()}
        sync.trace = False
    parallel.set_context(None)
    train.close()           # graphs, side streams, queued spectral-norm passes: released here, in order, not at interpreter teardown
    if args.trace_losses and rank == 0:
        for i, o in enumerate(trace):
            print(f"[{tag}] step {i}: " + "  ".join(f"{k} {v:.4f}" for k, v in o.items()), file=sys.stderr)
    return dict(dt=dt, steps=steps, out=out, recs=recs, prof_steps=prof_steps, eager_timing=eager_timing, h=h, w=w, E=E,
                timed_losses=trace[-steps:], dp_slack=dp_slack, dumped=dumped)


def kernel_report(res, m, args):
    recs, prof_steps = m["recs"], m["prof_steps"]
    total = sum(r["ms"] for r in recs) or 1.0
    pmc, pmc_src = pmc_families()
    res["roofline"] = roofline_of(recs[0], total, pmc, pmc_src)
    ridge = PEAK_BF16_TFLOPS * 1e12 / (PEAK_HBM_GBS * 1e9)
    mf = [r for r in recs if r["flops"] > 0 and r["bytes"] and r["flops"] / (r.get("bytes_min") or r["bytes"]) >= ridge / 4]
    if mf:
        res["roofline_conv_mfma"] = dict(roofline_of(mf[0], total, pmc, pmc_src), bound="mfma", unit="TFLOP/s", peak=PEAK_BF16_TFLOPS,
                                         achieved=mf[0]["flops"] / (mf[0]["ms"] * 1e-3) / 1e12,
                                         frac=mf[0]["flops"] / (mf[0]["ms"] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS)
    fams = []
    for r in recs[:(400 if args.shape_tags else 14)]:
        sec = r["ms"] * 1e-3
        bmin = r.get("bytes_min") or r["bytes"]
        fams.append({"name": r["name"], "launches_per_step": r["launches"] / prof_steps, "ms_per_step": r["ms"] / prof_steps,
                     "tflops": (r["flops"] / sec / 1e12) if r["flops"] else None, "GBs": (bmin / sec / 1e9) if bmin else None,
                     "mfma_frac": (r["flops"] / sec / 1e12 / PEAK_BF16_TFLOPS) if r["flops"] else None,
                     "hbm_frac": (bmin / sec / 1e9 / PEAK_HBM_GBS) if bmin else None,
                     "algorithmic_gbytes_per_step": bmin / prof_steps / 1e9 if bmin else None,
                     "launcher_gbytes_per_step": r["bytes"] / prof_steps / 1e9 if r["bytes"] else None})
    res["families"] = fams
    res["kernel_ms_per_step_total"] = total / prof_steps
    res["launches_per_step"] = sum(r["launches"] for r in recs) / prof_steps
    res["kernel_timing"] = ("HIP events around every launch inside the timed region" if m["eager_timing"] else
                            f"HIP events around every launch in {prof_steps} eager steps run right after the timed graph replays, weight-gradient launches "
                            "serialised with the rest (the timed replays overlap them on a side stream)")
    if m["E"] == 1 and m["h"] == 256:
        try:        # cross-check of the launchers' 8(d) byte accounting against the architecture calculator
            import arch_calc
            calc = arch_calc.step_family_gbytes()
            got = {"conv1x1_fwd_dgrad": 0.0, "conv3x3_fwd_dgrad": 0.0, "conv1x1_wgrad": 0.0, "conv3x3_wgrad": 0.0, "conv1x1_bwd_fused": 0.0,
                   "conv3x3_bwd_fused": 0.0}
            for r in recs:
                fam = r["name"].split(" ")[0]
                key = {"conv1x1_gather": "conv1x1_fwd_dgrad", "conv3x3_halo": "conv3x3_fwd_dgrad", "conv3x3_gather": "conv3x3_fwd_dgrad",
                       "conv1x1_wgrad": "conv1x1_wgrad", "conv3x3_wgrad": "conv3x3_wgrad", "conv1x1_bwd": "conv1x1_bwd_fused",
                       "conv3x3_bwd": "conv3x3_bwd_fused"}.get(fam)
                if key:
                    got[key] += (r.get("bytes_min") or r["bytes"]) / prof_steps / 1e9
            # The fused backward launches carry the dgrad AND the wgrad bytes of their layers, so the per-family figures no longer line up
            # one to one: what must agree is, per kernel size, ALL conv launches together against the calculator's forward + dgrad (as
            # launched) + wgrad total -- for the 1x1 layers minus the share that runs inside d_stem (first DBlock's conv1 / conv_sc).
            def both(calc_gb, meas_gb):
                return {"calculator_gbytes": calc_gb, "measured_launches_gbytes": meas_gb, "agree_within_3pct": abs(meas_gb - calc_gb) <= 0.03 * calc_gb}
            res["arch_calc_check"] = {
                "conv1x1_all": both(calc["conv1x1_fwd_dgrad_as_launched"] + calc["conv1x1_wgrad"] - calc["d_stem_1x1"],
                                    got["conv1x1_fwd_dgrad"] + got["conv1x1_wgrad"] + got["conv1x1_bwd_fused"]),
                "conv3x3_all": both(calc["conv3x3_fwd_dgrad_as_launched"] + calc["conv3x3_wgrad"],
                                    got["conv3x3_fwd_dgrad"] + got["conv3x3_wgrad"] + got["conv3x3_bwd_fused"]),
                "per_family_measured_gbytes": got, "d_stem_1x1_calculator_gbytes": calc["d_stem_1x1"]}
            if not all(v["agree_within_3pct"] for k, v in res["arch_calc_check"].items() if isinstance(v, dict) and "agree_within_3pct" in v):
                print("bench: arch_calc_check DISAGREES: " + json.dumps(res["arch_calc_check"]), file=sys.stderr)
        except Exception as e:
            res["arch_calc_check"] = f"unavailable: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="the full record: per-kernel timing / roofline, configs[3] and configs[4], the CPU baseline, data-parallel slack "
                         "(a plain run times configs[1] alone)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (losses, sampled G / D / G_ema state) "
                         "as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline", choices=("sub", "full"), default="sub",
                    help="sub: 8 of 40 sensors x5 (tens of seconds); full: 40 sensors, 1 warm-up + 1 timed step (minutes, ~30 GB)")
    ap.add_argument("--no-kernel-timing", action="store_true", help="skip the per-kernel HIP-event timing")
    ap.add_argument("--no-configs3", action="store_true", help="skip the additional configs[3] (4 events/GPU + Con_reg) measurement")
    ap.add_argument("--only-configs3", action="store_true", help="run configs[3] as the headline workload (tuning aid)")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--no-graph", action="store_true", help="run the step eagerly instead of replaying a HIP graph")
    ap.add_argument("--shape-tags", action="store_true", help="per-kernel timing split by layer shape (tuning aid)")
    ap.add_argument("--trace-losses", action="store_true", help="print the losses of every step to stderr (tuning aid)")
    ap.add_argument("--lr", type=float, default=None, help="override G_lr / D_lr of the benchmark configuration (tuning aid)")
    ap.add_argument("--serial-wgrad", action="store_true", help="weight-gradient launches on the main stream (tuning aid: step time = sum of "
                                                               "all launches + gaps; the difference to the kernel-time total is launch overhead)")
    ap.add_argument("--only", choices=("configs1",), default=None, help="skip configs[3] / configs[4] (tuning aid; same as --no-configs3)")
    ap.add_argument("--conv-dtype", choices=("bf16", "fp8"), default=None, help="run the headline workload with this conv_dtype (tuning aid)")
    args = ap.parse_args()
    faulthandler.enable()
    if args.only:
        args.no_configs3 = True

    import _hip
    import parallel

    rank, world, local = parallel.init_from_env("nccl")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE is {world}: launch with torch.distributed.run --nproc-per-node {args.gpus}")
    _hip.require_gpu()
    torch.cuda.set_device(local)
    if args.serial_wgrad:
        import ops
        ops.DEFAULTS.wgrad_side_stream = False         # seeds the options of every network built below

    def cfg_for(which):
        cfg = bench_config(which)
        if args.lr is not None:
            cfg.update(G_lr=args.lr, D_lr=args.lr)
        if args.conv_dtype is not None and which == 1:
            cfg.update(conv_dtype=args.conv_dtype)
        cfg["resolution"] = args.resolution
        cfg["hip_graph"] = not args.no_graph
        if args.resolution != 256:
            cfg["H_base"] = 1
        return cfg

    cfg = cfg_for(3 if args.only_configs3 else 1)
    m = measure(cfg, args, rank, world, local, "configs1")
    if rank != 0:
        if world > 1:
            parallel.shutdown()
        return
    E, h, w, dt, steps = m["E"], m["h"], m["w"], m["dt"], m["steps"]
    desc1 = (f"BASELINE configs[1]: 1 event (40x1x{h}x{w}) per GPU per step, hinge loss only, RRM on, DiffAugment on, ortho reg + "
             "Adam + EMA in the timed region, fp32 master weights, 4 synthetic events in rotation")
    desc3 = (f"BASELINE configs[3]: 4 events (160x1x{h}x{w}) per GPU per step, DiffAugment + CR_DiffAug consistency regularisation "
             "(third D pass) + contrastive + IEA + uniformity losses, RRM on")
    res = {"metric": "events/sec (40x250x768) per G+D train step", "value": world * E * steps / dt, "unit": "events/s",
           "n_gpus": world, "steps": steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / steps,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
           "config": {"workload": desc3 if args.only_configs3 else desc1, "events_per_gpu_per_step": E,
                      "parallelism": f"dp{world}", "clip_norm": cfg["clip_norm"], "hip_graph": bool(cfg["hip_graph"]),
                      "lr": cfg["G_lr"], "regime": "D logits centred once (linear0.bias), lr small enough that both hinge terms stay active "
                                                   "in every timed step (see hinge_unsaturated_in_every_timed_step)"},
           "losses_last_step": m["out"], "roofline": None, "cpu_baseline": None,
           "step_tflops_algorithmic": STEP_GFLOP * 1e-3 * world * steps / dt if (args.resolution == 256 and E == 1) else None,
           "git_head": git_head()}
    sat = [o for o in m["timed_losses"] if not (o["D_loss_real"] > 0.0 and o["D_loss_fake"] > 0.0)]
    res["hinge_unsaturated_in_every_timed_step"] = not sat          # both D hinge terms > 0: every backward pass carries non-zero gradients
    res["config"]["hinge_unsaturated_in_every_timed_step"] = not sat
    res["config"]["losses_last_step"] = m["out"]
    if m["dp_slack"] is not None:
        res["dp_exchange_slack_ms"] = dict(m["dp_slack"], note="per step: ms between the side stream finishing a network's all-reduce + update and "
                                           "the main stream reaching its wait for it (positive: fully hidden; negative: the main stream stalled)")
    if m["recs"]:
        kernel_report(res, m, args)
        if res.get("roofline") and res.get("roofline_conv_mfma"):
            res["roofline"]["conv_mfma_frac"] = res["roofline_conv_mfma"]["frac"]
            res["roofline"]["conv_mfma_kernel"] = res["roofline_conv_mfma"]["kernel"]
    if m["dumped"] is not None:
        write_outputs(args.dump_outputs, m["dumped"])
    if world == 1 and args.full and not args.no_configs3 and not args.only_configs3:
        m3 = measure(cfg_for(3), args, rank, world, local, "configs3")
        r3 = {"workload": desc3, "value": m3["E"] * m3["steps"] / m3["dt"], "unit": "events/s", "steps": m3["steps"],
              "ms_per_step": 1e3 * m3["dt"] / m3["steps"], "events_per_gpu_per_step": m3["E"], "losses_last_step": m3["out"]}
        if m3["recs"]:
            kernel_report(r3, m3, args)
        res["configs3"] = r3
        m4 = measure(cfg_for(4), argparse.Namespace(**dict(vars(args), no_kernel_timing=True)), rank, world, local, "configs4")
        res["configs4"] = {"workload": "BASELINE configs[4] on ONE GPU: configs[1] with OCP e4m3 MFMA operands (per-slice weight scale, per-tile "
                                       "activation scale, fp32 accumulate; block-scaled K = 128 instruction v_mfma_scale_f32_16x16x128_f8f6f4 with "
                                       "unit block scales) in the forward AND dgrad launches of the C = 128 3x3 convolutions and of the C = 64 ones "
                                       "with >= 1000 tile-blocks; tensors in HBM stay bf16, wgrad bf16", "value": m4["E"] * m4["steps"] / m4["dt"], "unit": "events/s",
                           "steps": m4["steps"], "ms_per_step": 1e3 * m4["dt"] / m4["steps"], "dtype": "fp8 (e4m3) operands / bf16 tensors",
                           "losses_last_step": m4["out"], "tolerance": "tests/test_networks_gpu.py::test_fp8_conv_path_forward_and_step_tolerance"}
    if world == 1 and args.full and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(cfg_for(1), args.cpu_baseline)
    print(json.dumps(res))
    sys.stdout.flush()
    if dist.is_initialized():
        parallel.shutdown()
    # Normal interpreter exit (round 3 left through os._exit after one run had died with SIGSEGV behind its record): every
    # measure() has released its graphs / streams through train.close() while the HIP runtime was alive, the CPU leg's
    # intra-op pool is parked, and faulthandler would print the Python stack of any fault that is left.


if __name__ == "__main__":
    main()
