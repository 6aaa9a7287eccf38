"""dev: what the mixed sampler costs beside the plain one, at the headline dimensions (B = 64, Tc = 20, |V| = 12000, R = 128 decode rows).

    python tools/mix_sample_timing.py [--pairs 3] [--calls 200] [--parent-tree /a/built/checkout/of/the/parent/commit]

Alternating pairs of fresh processes: `model.sample(video, 1, True)` (with --parent-tree: that checkout's package and library) and
`model.mix_sample(video, caption, 0.9, with_greedy=True)` on this tree's library.  Both decode 128 rows with the per-step launches; the mixed
call adds Tc - 1 word-select launches.  Each process warms up, then times `--calls` calls between two device events; the last line is one
JSON object with every run and the two medians."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, TC, V = 64, 20, 12000


def one_side(side, calls, tree):
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    import s2vt_amd
    from s2vt_amd import model as M
    mdl = M.Video_Caption_Generator(1536, V, 500, 1000, B, 0, 5, TC, seed=3, multisample=1)
    rng = np.random.default_rng(1)
    video = torch.as_tensor(np.abs(rng.standard_normal((B, 5, 1536)) * 0.5).astype(np.float32)).cuda()
    cap = torch.as_tensor(rng.integers(2, V, (B, TC)).astype(np.int32)).cuda()
    call = (lambda i: mdl.sample(video, 1, True, seed=5 + i)) if side == "sample" else (lambda i: mdl.mix_sample(video, cap, 0.9, True, seed=5 + i))
    for i in range(10):
        call(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        call(i)
    e1.record()
    torch.cuda.synchronize()
    print(json.dumps({"side": side, "ms_per_call": e0.elapsed_time(e1) / calls, "calls": calls, "tree": os.path.dirname(os.path.abspath(s2vt_amd.__file__))}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3); ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--parent-tree"); ap.add_argument("--side", choices=("sample", "mix")); ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.side:
        return one_side(a.side, a.calls, a.tree)
    runs = {"sample": [], "mix": []}
    for _ in range(a.pairs):
        for side in ("sample", "mix"):
            tree = os.path.abspath(a.parent_tree) if side == "sample" and a.parent_tree else ROOT
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--calls", str(a.calls), "--tree", tree], check=True,
                                 capture_output=True, text=True, timeout=300).stdout
            rec = json.loads(out.strip().splitlines()[-1])
            runs[side].append(rec["ms_per_call"])
            print(rec, flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    print(json.dumps({"runs": runs, "median_ms": med, "extra_us_per_word_select_launch": (med["mix"] - med["sample"]) * 1000.0 / (TC - 1)}))


if __name__ == "__main__":
    main()
