"""What the residual S2VT captioner (residual_tf_s2vt.py; Video_Caption_Generator(residual=True)) costs against the plain one, in one
build and one process.  A measurement tool, not a test (bench.py has no such workload).

    python tools/bench_residual.py [--shapes rl multitask] [--reps 10] [--rounds 6]

Full dimensions (d = 1536, H = 1000, E = 500, |V| = 12000, Tv = 5, Tc = 20).  Shapes: rl = B 64, K 5 (384 sampler rows, 320 unrolled rows),
multitask = B 32, K 1 (64 sampler rows: the window in which a plain model's decode runs as ONE persistent launch, which a residual model
leaves for per-step launches -- DESIGN.md section 5f).  Per shape, alternating plain / residual inside every round after a warm-up:
  sample   sample(video, K, with_greedy=True) alone
  step     that sampler call followed by reinforce_update on the ids it returned (mask on the device, fixed rewards, lr = 0 so that every
           repetition does the same work, LSTM1's trajectory reused from the sampler pass)
Prints one JSON line per shape: the median over rounds of the per-call milliseconds, the per-decode-step difference of the sampler call
in microseconds, and the plain model's own round-to-round spread."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SHAPES = {"rl": (64, 5), "multitask": (32, 1)}
D, V, E, H, TV, TC = 1536, 12000, 500, 1000, 5, 20


def timed(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", choices=sorted(SHAPES), default=["rl", "multitask"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    a = ap.parse_args()
    import torch
    from s2vt_amd import model as M
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    for shape in a.shapes:
        B, K = SHAPES[shape]
        rng = np.random.default_rng(5)
        video = torch.as_tensor((np.abs(rng.standard_normal((B, TV, D))) * 0.5).astype(np.float32)).cuda()
        r = torch.as_tensor(rng.uniform(0, 1, K * B).astype(np.float32)).cuda()
        b = torch.as_tensor(np.tile(rng.uniform(0, 1, B), K).astype(np.float32)).cuda()
        fns = {}
        for tag, residual in (("plain", False), ("residual", True)):
            mdl = M.Video_Caption_Generator(D, V, E, H, B, 0, TV, TC, seed=11, multisample=K, residual=residual)

            def sample(mdl=mdl):
                return mdl.sample(video, K, True, seed=7)

            def step(mdl=mdl):
                mdl.set_step(0)
                s, _ = mdl.sample(video, K, True, seed=7)
                mdl.reinforce_update(video, s, None, r, b, lr=0.0, reuse_sampler_state=True)
            fns[f"sample_{tag}"], fns[f"step_{tag}"] = sample, step
        for fn in fns.values():                                             # warm-up (workspaces, attributes)
            fn(); fn()
        t = {n: [] for n in fns}
        for _ in range(a.rounds):
            for n, fn in fns.items():
                t[n].append(timed(fn, a.reps))
        med = {n: float(np.median(v)) for n, v in t.items()}
        out = {"shape": shape, "B": B, "K": K, "sampler_rows": (K + 1) * B, "unrolled_rows": K * B, "reps": a.reps, "rounds": a.rounds,
               "ms": {n: round(v, 4) for n, v in med.items()},
               "sample_us_per_decode_step_residual_minus_plain": round((med["sample_residual"] - med["sample_plain"]) * 1e3 / TC, 2),
               "step_ms_residual_minus_plain": round(med["step_residual"] - med["step_plain"], 4),
               "plain_round_spread_ms": {n: round(float(max(t[n]) - min(t[n])), 4) for n in ("sample_plain", "step_plain")}}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
