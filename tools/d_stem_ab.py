"""Two builds of the library on identical seeded d_stem operands, each in a fresh process (development aid):
    DS_LIB=/path/to/libieagan_hip.so python tools/d_stem_ab.py run OUT.pt [time]
    python tools/d_stem_ab.py compare A.pt B.pt [A_AGAIN.pt]
``run`` calls ieagan_d_stem_fwd and ieagan_d_stem_bwd (and ieagan_d_stem_dimg where the build has it) at the cases of
tests/test_d_stem_gpu.py and stores every output; with ``time`` it also times the launches at 40 x 256 x 768 (hip events, median of
rounds).  Without DS_LIB (the tree's own build) it also runs and times the separate launches ieagan_d_stem_dimg replaces (conv1's dgrad
+ conv_Cto1).  ``compare`` prints one JSON line: h1 / p0 / sc bit for bit, the largest relative difference max|a - b| / max|a| of the
atomic-accumulated weight gradients, -- given a second run of build A -- the run-to-run difference of A alone next to it, and d img of
the fused kernel against the separate launches."""
import ctypes as C
import json
import os
import statistics
import sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(root, "iea-gan_amd"), os.path.join(root, "tests"), root]
import torch

CASES = [(1, 8, 32), (1, 8, 64), (2, 24, 96), (5, 128, 320), (7, 128, 320)]
BF16 = torch.bfloat16


def run(out_path, timed):
    import _hip as H
    import d_stem_reference as R
    path = os.environ.get("DS_LIB", H.LIB_PATH)
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)           # not H.lib(): an older build lacks the newer entry points
    entries = [e for e in ("ieagan_d_stem_fwd", "ieagan_d_stem_bwd", "ieagan_d_stem_dimg") if hasattr(lib, e)]
    for e in entries:
        getattr(lib, e).argtypes = [C.POINTER(H.DStemDesc), C.c_void_p] if e != "ieagan_d_stem_dimg" else [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p]
    dev = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    res = {"lib": path, "entries": entries}

    def operands(n, h, w):
        i = R.inputs(n, h, w)
        return {k: (v.to(BF16) if k in ("w1", "wsc", "w1_bwd", "dh1", "dp0") else v).to(dev).contiguous() for k, v in i.items()}

    def launch(d, n, h, w):
        o = dict(h1=torch.empty(n, h, w, 16, dtype=BF16, device=dev), p0=torch.empty(n, h // 2, w // 2, 32, dtype=BF16, device=dev),
                 sc=torch.empty(n, h // 2, w // 2, 32, dtype=BF16, device=dev), dw_in=torch.zeros(9, 32, device=dev),
                 db_in=torch.zeros(32, 32, device=dev), dw1=torch.zeros(16, 32, device=dev), db1=torch.zeros(32, 16, device=dev),
                 dimg=torch.empty(n, h, w, device=dev))
        p = lambda t: t.data_ptr()
        desc = H.DStemDesc(p(d["img"]), n, h, w, p(d["w_in"]), p(d["b_in"]), p(d["w1"]), p(d["b1"]), p(d["wsc"]), p(d["bsc"]), p(o["h1"]), p(o["p0"]),
                           p(o["sc"]), p(d["dh1"]), p(d["dp0"]), p(d["w1_bwd"]), p(o["dw_in"]), p(o["db_in"]), p(o["dw1"]), p(o["db1"]))
        calls = {"ieagan_d_stem_fwd": lambda: lib.ieagan_d_stem_fwd(desc, st), "ieagan_d_stem_bwd": lambda: lib.ieagan_d_stem_bwd(desc, st),
                 "ieagan_d_stem_dimg": lambda: lib.ieagan_d_stem_dimg(p(d["dh1"]), p(d["dp0"]), p(d["w1_bwd"]), p(d["w_in"]), p(o["dimg"]), n, h, w, st)}
        if "DS_LIB" not in os.environ:               # the separate launches d_stem_dimg replaces (the kernels are the same in both builds)
            import types
            import ops
            dh0 = torch.empty(n, h, w, 32, dtype=BF16, device=dev)
            o["dimg_separate"] = torch.empty(n, h, w, device=dev)
            b = types.SimpleNamespace(rec=types.SimpleNamespace(kpad2=32, w_bwd=d["w1_bwd"]), N=n, Hc=h, Wc=w, Cout=16, Cin=32, taps=1)

            def separate():
                ops._dgrad(b, d["dh1"], 16, dh0, link=(d["dp0"], 32, 32), link_rs=1, link_scale=0.25)
                return H.lib().ieagan_conv_Cto1(p(dh0), None, None, 0, 0, p(d["w_in"]), None, p(o["dimg_separate"]), 0, n, h, w, 32, 1, st)
            calls["separate_dimg"] = separate
        return o, calls

    if "DS_LIB" not in os.environ:
        entries.append("separate_dimg")
    for n, h, w in CASES:
        d = operands(n, h, w)
        o, calls = launch(d, n, h, w)
        for e in entries:
            rc = calls[e]()
            assert rc == 0, (e, rc)
        torch.cuda.synchronize()
        if "ieagan_d_stem_dimg" not in entries:
            o.pop("dimg")
        res[f"{n}x{h}x{w}"] = {k: v.cpu() for k, v in o.items()}
    if timed:
        n, h, w = 40, 256, 768
        d = operands(n, h, w)
        o, calls = launch(d, n, h, w)
        times = {}
        for e in entries:
            fn, per = calls[e], []
            for _ in range(7):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) * 1e3 / 20)
            times[e] = {"us_rounds": [round(t, 1) for t in per], "us_median": round(statistics.median(per), 1)}
        res["time_40x256x768"] = times
        print(json.dumps({"lib": path, "time_40x256x768": times}))
    torch.save(res, out_path)


def compare(pa, pb, pa2=None):
    a, b = torch.load(pa), torch.load(pb)
    a2 = torch.load(pa2) if pa2 else None
    rel = lambda u, v: ((u.double() - v.double()).abs().max() / u.double().abs().max().clamp_min(1e-30)).item()
    out = {"a": a["lib"], "b": b["lib"], "cases": {}}
    for n, h, w in CASES:
        k = f"{n}x{h}x{w}"
        r = {"bit_identical": {t: bool(torch.equal(a[k][t].view(torch.int16), b[k][t].view(torch.int16))) for t in ("h1", "p0", "sc")}}
        for t in ("dw_in", "db_in", "dw1", "db1"):
            red = (lambda x: x.sum(0)) if t.startswith("db") else (lambda x: x)
            r[t] = {"a_vs_b": rel(red(a[k][t]), red(b[k][t]))}
            if a2 is not None:
                r[t]["a_vs_a_again"] = rel(red(a[k][t]), red(a2[k][t]))
        for x in (a, b):
            if "dimg_separate" in x[k]:
                r["dimg_fused_vs_separate"] = rel(x[k]["dimg_separate"], x[k]["dimg"])
        out["cases"][k] = r
    for k in ("time_40x256x768",):
        if k in a and k in b:
            out[k] = {"a": a[k], "b": b[k]}
    print(json.dumps(out))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], len(sys.argv) > 3 and sys.argv[3] == "time")
    else:
        compare(*sys.argv[2:5])
