"""Stand-alone timing of the conv1x1_tile launches of the 256x768 train step at N = 40 (development aid), with the prologue / mask / residual
the step uses (the shape tags of `bench.py --full --shape-tags`):
    python tools/tile1x1_ab.py [iters]            one JSON line per shape: the time per launch (us) of THIS process's library
    python tools/tile1x1_ab.py --edges [iters]    the launcher's two map-size floors: each edge shape under flags 0 (what the dispatch picks,
                                                  conv_gather there) and CONV_FORCE_TILE, alternated over five rounds in this process
    python tools/tile1x1_ab.py --summarize DIR    DIR/parent_r*.jsonl against DIR/new_r*.jsonl: per shape the per-round values, median and
                                                  spread (max - min) of each build, and `kept`: new median < parent median - parent spread
CB_LIB selects another build of the library (tools/conv_ab_bench.py): a comparison alternates the two builds in FRESH processes, one
output file per process and round."""
import glob
import json
import os
import statistics
import sys

# (Cin, Cout, H, W of the output, pooled source, BatchNorm prologue, ReLU, residual: None | same | up | pool, mask)
SHAPES = [
    (256, 64, 32, 96, 0, 0, 1, None, 0), (256, 64, 32, 96, 0, 0, 0, None, 1), (64, 256, 32, 96, 0, 0, 0, "same", 1),
    (64, 256, 32, 96, 0, 1, 1, "up", 0), (128, 256, 32, 96, 0, 0, 0, "same", 0), (128, 128, 32, 96, 0, 0, 0, "same", 0),
    (256, 32, 32, 96, 0, 0, 0, None, 0), (256, 128, 32, 96, 0, 0, 0, None, 0),
    (256, 64, 16, 48, 0, 1, 1, None, 0), (64, 256, 16, 48, 0, 0, 0, "same", 1), (128, 256, 16, 48, 0, 1, 1, "up", 0),
    (256, 256, 8, 24, 0, 0, 0, "same", 0), (128, 512, 8, 24, 0, 0, 0, "same", 1),
    (64, 256, 32, 96, 1, 0, 1, "pool", 0), (128, 128, 32, 96, 1, 0, 0, None, 0), (32, 128, 64, 192, 1, 0, 1, "pool", 0),
]
# below the floors of conv1x1_tile_launch: Cin = 512 on the 8x24 maps (M < 16384 && Cin > 256) and the 4x12 maps (M < 4096)
EDGES = [
    (512, 128, 8, 24, 0, 0, 1, None, 0), (512, 128, 8, 24, 0, 0, 0, None, 0), (512, 128, 8, 24, 0, 0, 0, None, 1),     # (a1: 8*24 % 128 != 0, never this kernel)
    (512, 128, 4, 12, 0, 0, 0, None, 0), (128, 512, 4, 12, 0, 0, 0, "same", 1),
]
N = 40


def tag(s):
    ci, co, h, w, pooled, aff, relu, res, mask = s
    return f"ci{ci} co{co} {h}x{w} rs{2 if pooled else 0} a{aff} r{relu} res{ {None: 0, 'same': 1, 'up': 2, 'pool': 3}[res] }{' mask' if mask else ''}"


def summarize(d):
    def load(prefix):
        rounds = {}
        for f in sorted(glob.glob(os.path.join(d, prefix + "_r*.jsonl"))):
            for line in open(f):
                if line.startswith("{"):
                    r = json.loads(line)
                    rounds.setdefault(r["shape"], []).append(r["us"])
        return rounds
    p, n = load("parent"), load("new")
    for shape in p:
        a, b = p[shape], n.get(shape, [])
        if not b:
            continue
        sp = max(a) - min(a)
        print(json.dumps({"shape": shape, "parent_us": a, "new_us": b, "parent_median": round(statistics.median(a), 2),
                          "new_median": round(statistics.median(b), 2), "parent_spread": round(sp, 2), "new_spread": round(max(b) - min(b), 2),
                          "kept": statistics.median(b) < statistics.median(a) - sp}))


if len(sys.argv) > 2 and sys.argv[1] == "--summarize":
    summarize(sys.argv[2])
    sys.exit(0)

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "iea-gan_amd"), root]
import torch
import _hip as H
if os.environ.get("CB_LIB"):
    H.LIB_PATH = os.environ["CB_LIB"]
import ops

args = [a for a in sys.argv[1:] if not a.startswith("--")]
edges = "--edges" in sys.argv
iters = int(args[0]) if args else 200
H.require_gpu()
dev = "cuda:0"
BF = torch.bfloat16
fn = H.lib().ieagan_conv_forward
st = H.stream()
torch.manual_seed(0)


def desc(s, flags):
    """(descriptor, the tensors it points to)"""
    ci, co, h, w, pooled, aff, relu, res, mask = s
    hs, ws = (2 * h, 2 * w) if pooled else (h, w)
    kpad = ops._kpad(ci)
    t = dict(x=torch.randn(N, hs, ws, ci, device=dev).to(BF), w=(torch.randn(co, kpad, device=dev) * 0.05).to(BF), bias=torch.randn(co, device=dev),
             out=torch.empty(N, h, w, co, device=dev, dtype=BF))
    if aff:
        t["sc"], t["sh"] = 1 + 0.1 * torch.randn(N, ci, device=dev), 0.1 * torch.randn(N, ci, device=dev)
    if mask:
        t["mk"] = torch.randn(N, h, w, co, device=dev).to(BF)
    ra_rs = {None: 0, "same": 0, "up": 1, "pool": 2}[res]
    if res is not None:
        rh, rw = {"same": (h, w), "up": (h // 2, w // 2), "pool": (2 * h, 2 * w)}[res]
        t["ra"] = torch.randn(N, rh, rw, co, device=dev).to(BF)
    src = H.src_desc(t["x"], ci, hs, ws, 2 if pooled else 0, t.get("sc"), t.get("sh"), ci if aff else 0, bool(relu))
    d = H.ConvDesc(N, h, w, ci, co, 1, kpad, src, H.ptr(t["w"]), H.ptr(t["bias"]), H.ptr(t.get("ra")), co if res else 0, co if res else 0, ra_rs, 1.0,
                   None, 0, H.ptr(t.get("mk")), H.ptr(t["out"]), None, 0, flags, None, None, 0, 0, 0)
    return d, t


def warm(d, what):
    for _ in range(20):
        rc = fn(d, st)
        if rc != 0:
            raise RuntimeError(f"{what}: ieagan_conv_forward failed ({rc}): {H.lib().ieagan_last_error().decode()}")
    torch.cuda.synchronize()


def timed(d):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(d, st)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


lib = os.path.basename(os.path.dirname(os.path.dirname(os.path.abspath(H.LIB_PATH)))) + "/" + os.path.basename(H.LIB_PATH)
if not edges:
    for s in SHAPES:
        d, keep = desc(s, 0)
        warm(d, tag(s))
        print(json.dumps({"shape": tag(s), "N": N, "lib": lib, "iters": iters, "us": round(timed(d), 2)}), flush=True)
else:
    for s in EDGES:
        (da, ka), (db, kb) = desc(s, 0), desc(s, H.CONV_FORCE_TILE)
        warm(da, tag(s))
        warm(db, tag(s) + " forced")
        ta, tb = [], []
        for _ in range(5):
            ta.append(timed(da))
            tb.append(timed(db))
        sp = max(ta) - min(ta)
        print(json.dumps({"edge": tag(s), "N": N, "lib": lib, "dispatch_us": [round(t, 2) for t in ta], "forced_tile_us": [round(t, 2) for t in tb],
                          "dispatch_median": round(statistics.median(ta), 2), "forced_tile_median": round(statistics.median(tb), 2),
                          "dispatch_spread": round(sp, 2), "move_edge": statistics.median(tb) < statistics.median(ta) - sp}), flush=True)
