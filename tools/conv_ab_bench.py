"""Same-process A/B timing of one 3x3 C = 64 conv launch under two values of ieagan_conv_desc.flags (development aid):
    python tools/conv_ab_bench.py FLAGS_A FLAGS_B N H W [rounds] [iters]
e.g. 32 16 = conv3x3_ws64 (forced) against conv3x3_lds.  The two forms alternate round by round on identical operands; per variant
the script prints one JSON line with the per-round times (us), their median and the spread (max - min) of each form.
Variants: relu (bare-ReLU forward), ccbn (BatchNorm prologue + ReLU + statistics), up (the same on an up-sampled source), mask (ReLU-mask
dgrad), bnb (BatchNorm-backward dgrad).  CB_LIB selects another build of the library, CB_VARIANTS a comma-separated subset."""
import json
import os
import statistics
import sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "iea-gan_amd"), root]
import torch
import _hip as H
if os.environ.get("CB_LIB"):
    H.LIB_PATH = os.environ["CB_LIB"]
import ops

fa, fb, N, Hh, Ww = map(int, sys.argv[1:6])
rounds = int(sys.argv[6]) if len(sys.argv) > 6 else 5
iters = int(sys.argv[7]) if len(sys.argv) > 7 else 100
want = os.environ.get("CB_VARIANTS", "relu,ccbn,up,mask,bnb").split(",")
H.require_gpu()
dev = "cuda:0"
C = 64
kpad = ops._kpad(9 * C)
torch.manual_seed(0)
w = (torch.randn(C, kpad, device=dev) * 0.05).to(torch.bfloat16)
bias = torch.randn(C, device=dev)
out = torch.empty(N, Hh, Ww, C, device=dev, dtype=torch.bfloat16)
x = torch.randn(N, Hh, Ww, C, device=dev).to(torch.bfloat16)
xh = torch.randn(N, Hh // 2, Ww // 2, C, device=dev).to(torch.bfloat16)
mk = torch.randn(N, Hh, Ww, C, device=dev).to(torch.bfloat16)
sc, sh = 1 + 0.1 * torch.randn(N, C, device=dev), 0.1 * torch.randn(N, C, device=dev)
stats = torch.zeros(32, 2, C, device=dev)
acc = torch.zeros(N, 8, 2, C, device=dev)


def desc(variant, flags):
    aff = variant in ("ccbn", "up")
    src = H.src_desc(xh if variant == "up" else x, C, Hh // 2 if variant == "up" else Hh, Ww // 2 if variant == "up" else Ww,
                     1 if variant == "up" else 0, sc if aff else None, sh if aff else None, C if aff else 0, variant in ("relu", "ccbn", "up"))
    bnb = variant == "bnb"
    return H.ConvDesc(N, Hh, Ww, C, C, 9, kpad, src, H.ptr(w), None if bnb else H.ptr(bias), None, 0, 0, 0, 1.0, None, 0,
                      H.ptr(mk) if variant in ("mask", "bnb") else None, H.ptr(out), H.ptr(acc) if bnb else (H.ptr(stats) if aff else None),
                      1 if bnb else 0, flags, H.ptr(sc) if bnb else None, H.ptr(sh) if bnb else None, C if bnb else 0, int(bnb))


fn = H.lib().ieagan_conv_forward
st = H.stream()


def timed(d):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn(d, st)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


for v in want:
    da, db = desc(v, fa), desc(v, fb)
    for d in (da, db):
        for _ in range(10):
            rc = fn(d, st)
            if rc != 0:
                raise RuntimeError(f"{v}: ieagan_conv_forward failed ({rc}): {H.lib().ieagan_last_error().decode()}")
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(da))
        tb.append(timed(db))
    print(json.dumps({"variant": v, "N": N, "H": Hh, "W": Ww, "flags_a": fa, "flags_b": fb, "lib": os.path.basename(H.LIB_PATH),
                      "a_us": [round(t, 2) for t in ta], "b_us": [round(t, 2) for t in tb],
                      "a_median": round(statistics.median(ta), 2), "b_median": round(statistics.median(tb), 2),
                      "a_spread": round(max(ta) - min(ta), 2), "b_spread": round(max(tb) - min(tb), 2)}), flush=True)
