"""Timing of descriptor matching: sfmba_match_descriptors (one launch of k_match) from its own
`kernel_us` (profile = 1: HIP events round the launch) on 8 images x 8192 descriptors, D = 128, all 28 pairs u > v, in
form A (integers 0..255) and in form B (RootSIFT-like fp32 rows), against a PyTorch-ROCm baseline that computes the same
thing on the same device: per pair `torch.mm` of the descriptors (fp16 for form A, fp32 for form B, and fp32 on the form-A
data as well: the fp16 product of 0..255 values overflows fp16, so that baseline's output is unusable and only its time is
of interest), the norms added, `topk(2, largest=False)`; HIP events round the 28 pairs.  Every figure is the median of
ROUNDS warm calls; min and max are the scatter.  No speed threshold is attached.

Each step (one form of one implementation) runs in a child process of its own under a time limit; the first step that
fails ends the run.  Usage: python tools/match_timing.py [--out profiles/match_timing.txt]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

N_IMAGES, N_DESC, D, ROUNDS = 8, 8192, 128, 9
STEP_SECONDS = 180
PEAK = {"A": 2.5e15, "B": 157.3e12}             # fp16 and fp32 MFMA, dense, FLOP/s (MI355X_MICROARCH.md, spec)
STEPS = ("sfmba-A", "torch-A", "torch-A32", "sfmba-B", "torch-B")


def descriptors(form):
    rng = np.random.default_rng(7)
    if form == "A":
        return [rng.integers(0, 256, size=(N_DESC, D)).astype(np.uint8) for _ in range(N_IMAGES)]
    import match_ref as mr
    return [mr.rootsift_rows(rng, N_DESC, D).astype(np.float32) for _ in range(N_IMAGES)]


def step_sfmba(form):
    import sfmba
    be = sfmba.Backend(0)
    descs = descriptors(form)
    assert be.set_descriptors(descs) == (1 if form == "A" else 2)
    m = be.match_descriptors(None, profile=1)                     # warm-up: code object, buffers
    us = [be.match_descriptors(None, profile=1).kernel_us for _ in range(ROUNDS)]
    be.close()
    return dict(us=us, good=int(m.edge_good.sum()), queries=int(m.query_ptr[-1]))


def step_torch(form, dtype_name):
    import torch
    dt = getattr(torch, dtype_name)
    dev = torch.device("cuda:0")
    descs = [torch.from_numpy(d.astype(np.float32)).to(dev) for d in descriptors(form)]
    low = [d.to(dt) for d in descs]
    edges = [(u, v) for u in range(N_IMAGES) for v in range(N_IMAGES) if u > v]

    def batch():
        out = []
        for u, v in edges:
            dot = torch.mm(low[u], low[v].t()).float()
            d2 = (descs[u] * descs[u]).sum(1)[:, None] + (descs[v] * descs[v]).sum(1)[None, :] - 2.0 * dot
            out.append(torch.topk(d2, 2, dim=1, largest=False))
        return out
    batch()
    torch.cuda.synchronize()
    us = []
    for _ in range(ROUNDS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = batch()
        b.record()
        torch.cuda.synchronize()
        us.append(1e3 * a.elapsed_time(b))
    finite = all(bool(torch.isfinite(o.values).all()) for o in out)
    return dict(us=us, finite=finite)


def run_step(name):
    if name == "sfmba-A":
        return step_sfmba("A")
    if name == "sfmba-B":
        return step_sfmba("B")
    if name == "torch-A":
        return step_torch("A", "float16")
    if name == "torch-A32":
        return step_torch("A", "float32")
    if name == "torch-B":
        return step_torch("B", "float32")
    raise SystemExit(f"unknown step {name}")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        print("RESULT " + json.dumps(run_step(sys.argv[2])), flush=True)
        return
    out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
    results = {}
    for name in STEPS:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True,
                               timeout=STEP_SECONDS)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {name} ran into its time limit of {STEP_SECONDS} s; nothing more is started")
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            raise SystemExit(f"step {name} failed with exit status {p.returncode}; nothing more is started")
        results[name] = json.loads(line[-1][7:])
    pairs = N_IMAGES * (N_IMAGES - 1) // 2
    flop = 2.0 * pairs * N_DESC * N_DESC * D
    med = {k: float(np.median(v["us"])) for k, v in results.items()}
    lines = [f"descriptor matching: {N_IMAGES} images x {N_DESC} descriptors, D = {D}, all {pairs} pairs u > v "
             f"({flop / 1e9:.1f} GFLOP of dot products), median of {ROUNDS} warm calls [min .. max], microseconds"]
    label = {"sfmba-A": "k_match, form A (fp16 MFMA, exact)", "torch-A": "torch.mm fp16 + norms + topk(2)",
             "torch-A32": "torch.mm fp32 + norms + topk(2), form-A data", "sfmba-B": "k_match, form B (fp32 MFMA)",
             "torch-B": "torch.mm fp32 + norms + topk(2)"}
    for name in STEPS:
        v = np.array(results[name]["us"])
        extra = ""
        if name.startswith("sfmba"):
            form = name[-1]
            rate = flop / (1e-6 * med[name])
            extra = (f"   {rate / 1e12:8.1f} TFLOP/s = {100 * rate / PEAK[form]:.1f} % of the {'fp16' if form == 'A' else 'fp32'} MFMA peak; "
                     f"{results[name]['good']} of {results[name]['queries']} queries pass the ratio test")
        elif not results[name]["finite"]:
            extra = "   (its distances overflow: the output is not usable)"
        lines.append(f"  {label[name]:46s} {med[name]:12.1f} [{v.min():12.1f} .. {v.max():12.1f}]{extra}")
    for ours, base in (("sfmba-A", "torch-A"), ("sfmba-A", "torch-A32"), ("sfmba-B", "torch-B")):
        r = med[base] / med[ours]
        lines.append(f"  {label[ours]}: {r:.2f} x the speed of {label[base]}" + ("" if r >= 1 else "  -- SLOWER than the baseline"))
    text = "\n".join(lines)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")


main()
