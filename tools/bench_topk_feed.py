#!/usr/bin/env python
"""Step time of top-k score-weighted embedding training (Video_Caption_Generator.topk_feed_update) against averaged-embedding training
(averaged_update) at the `xe` workload's shape: BASELINE configs[1], B = 64, Tc = 20, |V| = 12000, bench.py's synthetic inputs (the
statements of its make_step).

    python tools/bench_topk_feed.py [--steps 100] [--warmup 10] [--pairs 3] [--k 5] [--only topk|averaged] [--optimizer sgd|adam] [--parts]

Both steps run in ONE process in alternating rounds (topk, averaged, topk, ...), each block of --steps steps bracketed by device
synchronisation, so clock and thermal drift hit both alike; one JSON line with every block's ms per step, the medians and the spread
(max - min over a kind's blocks, as a share of its median).  Both take the same update rule (--optimizer sgd: SGD behind the per-variable
clip, the scripts' train(); adam: Adam behind the global clip).  The top-k step has the averaged step's forward launch count (its mix kernel
in place of the mean kernel); its backward unrolls LSTM2's recurrence into Tv + Tc per-step launches with the mix backward between the
decode steps, where the averaged step has one persistent recurrence, and always takes the fp32 products.
--parts also times the top-k step's forward and backward on their own (ops.topk_feed_fwd, then softmax + ops.topk_feed_bptt_bwd on its
workspace) and reports the backward's share per unrolled LSTM2 step, (backward - averaged backward) / (Tv + Tc).
--only: one kind alone, no pairing -- the body of a `rocprofv3 --kernel-trace --stats` run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("topk", "averaged")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--only", choices=KINDS)
    ap.add_argument("--optimizer", choices=("adam", "sgd"), default="sgd")
    ap.add_argument("--parts", action="store_true")
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
        "topk": lambda m: m.topk_feed_update(video, gt, gt_mask, k=a.k, lr=1e-3, clip_norm=10.0, clip=clip, optimizer=a.optimizer),
        "averaged": lambda m: m.averaged_update(video, gt, gt_mask, lr=1e-3, clip_norm=10.0, clip=clip, optimizer=a.optimizer),
    }
    kinds = [a.only] if a.only else list(KINDS)

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, out

    for k in kinds:
        timed(lambda: steps[k](models[k]), a.warmup)
    out = {k: [] for k in kinds}
    last = {}
    for _ in range(a.pairs if not a.only else 1):
        for k in kinds:
            ms, last[k] = timed(lambda: steps[k](models[k]), a.steps)
            out[k].append(round(ms, 4))
    med = {k: statistics.median(v) for k, v in out.items()}
    line = {"tool": "bench_topk_feed", "B": B, "Tc": TC, "Tv": TV, "V": V, "k": a.k, "steps": a.steps, "warmup": a.warmup, "optimizer": a.optimizer,
            "clip": clip, "ms_per_step": out, "median_ms": {k: round(v, 4) for k, v in med.items()},
            "spread_pct": {k: round(100.0 * (max(v) - min(v)) / med[k], 2) for k, v in out.items()},
            "last_loss": {k: float(last[k].loss) for k in kinds}, "last_mask_sum": {k: float(last[k].mask_sum) for k in kinds}}
    if not a.only:
        line["topk_over_averaged"] = round(med["topk"] / med["averaged"], 3)
    if a.parts:
        # forward and backward of each kind alone, on one model's variables (no update between the calls: the same work every time)
        m = models["topk"]
        vid, sid = m._row_ids(B, 1, 0)
        p, gr = m.store.params, m.store.grads
        parts = {}
        f = ops.topk_feed_fwd(m.dims, p, video, gt, gt_mask, B, a.k, 1.0, 0.9, 7, vid, sid)
        parts["topk_fwd"], f = timed(lambda: ops.topk_feed_fwd(m.dims, p, video, gt, gt_mask, B, a.k, 1.0, 0.9, 7, vid, sid), a.steps)
        dl0 = f["logits"].clone()
        ops.softmax_nll_fwd_bwd(dl0, f["target_tm"], f["coef_tm"], 0.0)
        dl = dl0.clone()

        def topk_bwd():
            dl.copy_(dl0)                                        # (the backward completes dlogits in place)
            ops.topk_feed_bptt_bwd(m.dims, p, gr, video, B, dl, f["ws"], f["scratch"], a.k, 0.9, 7, vid, sid)
        parts["topk_bwd_with_copy"], _ = timed(topk_bwd, a.steps)
        parts["dlogits_copy"], _ = timed(lambda: dl.copy_(dl0), a.steps)
        fa = ops.averaged_fwd(m.dims, p, video, gt, gt_mask, B, 1.0, 0.9, 7, vid, sid)
        parts["averaged_fwd"], fa = timed(lambda: ops.averaged_fwd(m.dims, p, video, gt, gt_mask, B, 1.0, 0.9, 7, vid, sid), a.steps)
        da = fa["logits"].clone()
        ops.softmax_nll_fwd_bwd(da, fa["target_tm"], fa["coef_tm"], 0.0)
        parts["averaged_bwd_fp32"], _ = timed(lambda: ops.averaged_bptt_bwd(m.dims, p, gr, video, B, da, fa["ws"], fa["scratch"], 0.9, 7, vid, sid,
                                                                           products="fp32"), a.steps)
        parts["topk_bwd"] = parts["topk_bwd_with_copy"] - parts["dlogits_copy"]
        parts["unrolled_lstm2_bwd_us_per_step"] = 1e3 * (parts["topk_bwd"] - parts["averaged_bwd_fp32"]) / (TV + TC)
        line["parts_ms"] = {k: round(v, 4) for k, v in parts.items()}
    line["chain_timeouts"] = int(ops.chain_timeouts())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
