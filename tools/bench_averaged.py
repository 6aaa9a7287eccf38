#!/usr/bin/env python
"""Step time of averaged-embedding training (Video_Caption_Generator.averaged_update) against scheduled-sampling training
(scheduled_update) and the teacher-forced cross-entropy step (xe_update(q1=False)) at the `xe` workload's shape: BASELINE configs[1],
B = 64, Tc = 20, |V| = 12000, bench.py's synthetic inputs (the statements of its make_step).

    python tools/bench_averaged.py [--steps 100] [--warmup 10] [--pairs 3] [--only averaged|scheduled|xe] [--optimizer sgd|adam]

The three steps run in ONE process in alternating rounds (averaged, scheduled, xe, averaged, ...), each block of --steps steps bracketed
by device synchronisation, so clock and thermal drift hit all alike; one JSON line with every block's ms per step, the medians and the
spread (max - min over a kind's blocks, as a share of its median).  The averaged step takes the script's rule (--optimizer sgd: SGD behind
the per-variable clip; adam: Adam behind the global clip), the scheduled step the same optimizer behind its global clip.  The xe step
unrolls all Tc steps here (active_steps=None), as the other two must.  The averaged step has the scheduled step's launch count per decode
step, writes one extra [N, E] block per step, scatters twice, and with sgd replaces one update launch by one per variable.
--only: one kind alone, no pairing -- the body of a `rocprofv3 --kernel-trace --stats` run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("averaged", "scheduled", "xe")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--only", choices=KINDS)
    ap.add_argument("--optimizer", choices=("adam", "sgd"), default="sgd")
    a = ap.parse_args()

    import numpy as np
    import torch
    import bench
    import s2vt_amd
    from s2vt_amd import model as M
    from s2vt_amd import ops
    s2vt_amd.lib()
    dev = torch.device("cuda")
    B = 64
    TC, TV, D, E, H, V = bench.TC, bench.TV, bench.D, bench.E, bench.H, bench.V

    def make():
        return M.Video_Caption_Generator(D, V, E, H, B, 0, TV, TC, device=dev, seed=1234, multisample=1)
    # bench.py's synthetic inputs of the xe workload: the same generator seeds, drawn by the same statements
    g = torch.Generator().manual_seed(1234)
    video = (torch.randn(B, TV, D, generator=g) * 0.5).abs().to(dev)
    rng = np.random.default_rng(1234)
    ln = 1 + np.minimum(rng.poisson(6, B), TC - 2)
    cap = rng.integers(2, V, (B, TC)).astype(np.int32)
    for j in range(B):
        cap[j, ln[j]:] = 0
    gt = torch.as_tensor(cap).to(dev)
    is_eos = (gt == 0)
    gt_mask = ((torch.cumsum(is_eos.int(), 1) - is_eos.int()) == 0).float()

    models = {k: make() for k in KINDS}
    clip = "per_variable" if a.optimizer == "sgd" else "global"
    steps = {
        "averaged": lambda m: m.averaged_update(video, gt, gt_mask, lr=1e-3, clip_norm=10.0, clip=clip, optimizer=a.optimizer),
        "scheduled": lambda m: m.scheduled_update(video, gt, lr=1e-3, true_word_prob=0.5, clip_norm=10.0, optimizer=a.optimizer),
        "xe": lambda m: m.xe_update(video, gt, gt_mask, lr=1e-3, clip_norm=10.0, q1=False, smoothing=0.0, active_steps=None, live_mask=None),
    }
    kinds = [a.only] if a.only else list(KINDS)

    def block(kind, n):
        m = models[kind]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            st = steps[kind](m)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, st

    for k in kinds:
        block(k, a.warmup)
    out = {k: [] for k in kinds}
    last = {}
    for _ in range(a.pairs if not a.only else 1):
        for k in kinds:
            ms, last[k] = block(k, a.steps)
            out[k].append(round(ms, 4))
    med = {k: statistics.median(v) for k, v in out.items()}
    line = {"tool": "bench_averaged", "B": B, "Tc": TC, "V": V, "steps": a.steps, "warmup": a.warmup, "optimizer": a.optimizer, "clip": clip,
            "ms_per_step": out, "median_ms": {k: round(v, 4) for k, v in med.items()},
            "spread_pct": {k: round(100.0 * (max(v) - min(v)) / med[k], 2) for k, v in out.items()},
            "last_loss": {k: float(last[k].loss) for k in kinds}, "last_mask_sum": {k: float(last[k].mask_sum) for k in kinds},
            "chain_timeouts": int(ops.chain_timeouts())}
    if not a.only:
        line["averaged_over_scheduled"] = round(med["averaged"] / med["scheduled"], 3)
        line["averaged_over_xe"] = round(med["averaged"] / med["xe"], 3)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
