#!/usr/bin/env python
"""Time of one ROUGE-L reward call: the device kernel (reward.RougeL.score_ids_device = s2vt_rouge_l_score, one launch) against the host
library (score_ids = s2vt_rouge_score) with 1 and 16 threads, in one process, on a synthetic corpus with MSVD's statistics.

    python tools/bench_rouge.py [--calls 200] [--host-calls 10] [--warmup 20] [--blocks 5] [--out FILE.jsonl]

Corpus: 1200 videos, max(1, Poisson(41)) references each, reference lengths max(1, round(N(7, 3))) words, tokens uniform over a 12000-word
vocabulary.  Candidates: the `rl_msvd` workload's lengths (bench.py: 1 + min(Poisson(6), Tc - 2) words, then <eos> = 0), tokens from the
same vocabulary, videos drawn uniformly.  Shapes: 384 rows x Tc 20 (the `rl` workload: B 64 x K 5 samples + B greedy rows) and 2304 rows x
Tc 35 (`rl_ref`: B 256 x K 8 + B).

The kinds run in alternating blocks (device, device queued, host x1, host x16, device, ...), every shape warmed up first.  A device block
is `--calls` back-to-back calls between two events on the stream: from an idle stream this is bound by the host's enqueue (the wrapper's
allocation and the ctypes call), what a caller pays who does nothing else.  A queued block enqueues the same calls behind a plug of matrix
products that keeps the GPU busy meanwhile (`plug_held_every_block` says it did): the kernels' own time plus the boundary between two
dependent launches, what a training step pays, where the launches sit behind the teacher-forced forward.  A host block is `--host-calls`
calls under a host clock.  One JSON line per shape: every block's microseconds per call, the medians, the spread
(max - min over a kind's blocks as a share of its median), and whether the device and the host scores are bit-equal on the timed inputs.
LCS work does not depend on how many words match, so uniform tokens time the same table a trained policy's captions would."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"rl": (384, 20), "rl_ref": (2304, 35)}
V, N_VIDEOS = 12000, 1200


def corpus(rng):
    words = [f"w{i}" for i in range(V)]
    wordtoix = {w: i for i, w in enumerate(words)}
    refs = []
    for _ in range(N_VIDEOS):
        n = max(1, int(rng.poisson(41)))
        lens = [max(1, int(round(x))) for x in rng.normal(7.0, 3.0, n)]
        refs.append([" ".join(words[int(t)] for t in rng.integers(2, V, size=l)) for l in lens])
    return refs, wordtoix


def candidates(rng, N, Tc):
    import numpy as np
    ln = 1 + np.minimum(rng.poisson(6, N), Tc - 2)
    ids = rng.integers(2, V, (N, Tc)).astype(np.int32)
    for j in range(N):
        ids[j, ln[j]:] = 0
    return ids, rng.integers(0, N_VIDEOS, size=N).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--host-calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--plug", type=int, default=3, help="8192^3 fp32 matrix products in front of a queued block (the GPU stays busy while the host enqueues)")
    ap.add_argument("--out")
    a = ap.parse_args()

    import numpy as np
    import torch
    import s2vt_amd
    from s2vt_amd import reward
    s2vt_amd.lib()
    assert torch.cuda.is_available(), "bench_rouge.py times the device kernel: it needs a GPU"
    rng = np.random.default_rng(1234)
    refs, wordtoix = corpus(rng)
    n_refs = sum(len(r) for r in refs)
    dev = reward.RougeL(refs, wordtoix, device="cuda")
    host = {1: reward.RougeL(refs, wordtoix, n_threads=1), 16: reward.RougeL(refs, wordtoix, n_threads=16)}
    plug = torch.randn(8192, 8192, device="cuda")
    plug_out = torch.empty_like(plug)
    lines = []
    for name, (N, Tc) in SHAPES.items():
        ids, vrow = candidates(rng, N, Tc)
        ids_d, vrow_d = torch.as_tensor(ids).cuda(), torch.as_tensor(vrow).cuda()

        def device_block(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                out = dev.score_ids_device(ids_d, vrow_d)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n, out

        def queued_block(n):
            """The same n launches enqueued while the GPU is still busy with a plug of matrix products: between the two events the stream
            never waits for the host, so this is the kernels' own time plus the boundary between two dependent launches."""
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(a.plug):
                torch.mm(plug, plug, out=plug_out)
            e0.record()
            for _ in range(n):
                dev.score_ids_device(ids_d, vrow_d)
            e1.record()
            busy = not e0.query()                       # the plug was still running when the last launch had been enqueued
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / n, busy

        def host_block(t, n):
            t0 = time.perf_counter()
            for _ in range(n):
                out = host[t].score_ids(ids, vrow)
            return (time.perf_counter() - t0) * 1e6 / n, out

        device_block(a.warmup)
        for t in host:
            host_block(t, 2)
        queued_block(a.warmup)
        us = {"device": [], "device_queued": [], "host_1": [], "host_16": []}
        plug_held = True
        for _ in range(a.blocks):
            d, out_d = device_block(a.calls)
            us["device"].append(round(d, 3))
            q, busy = queued_block(a.calls)
            us["device_queued"].append(round(q, 3))
            plug_held = plug_held and busy
            for t in host:
                h, out_h = host_block(t, a.host_calls)
                us[f"host_{t}"].append(round(h, 3))
        med = {k: statistics.median(v) for k, v in us.items()}
        same = bool(np.array_equal(out_d.cpu().numpy().view(np.uint32), out_h.view(np.uint32)))
        cells = int(sum((ids[j] != 0).sum() * sum(len(s.split()) for s in refs[int(vrow[j])]) for j in range(N)))
        lines.append({"tool": "bench_rouge", "shape": name, "rows": N, "Tc": Tc, "videos": N_VIDEOS, "references": n_refs, "lcs_cells": cells,
                      "calls_per_block": a.calls, "host_calls_per_block": a.host_calls, "warmup": a.warmup, "us_per_call": us,
                      "median_us": {k: round(v, 3) for k, v in med.items()},
                      "spread_pct": {k: round(100.0 * (max(v) - min(v)) / med[k], 2) for k, v in us.items()},
                      "host_1_over_device": round(med["host_1"] / med["device"], 2), "host_16_over_device": round(med["host_16"] / med["device"], 2),
                      "host_16_over_device_queued": round(med["host_16"] / med["device_queued"], 2),
                      "plug_held_every_block": plug_held, "bit_equal": same, "mean_score": round(float(out_h.mean()), 5)})
    for l in lines:
        print(json.dumps(l))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
