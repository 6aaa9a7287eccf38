"""The two LSTM1 recurrences of the bidirectional captioner (bidirection_tf_s2vt.py): one persistent launch for both directions
(csrc/bidir.hip) against one persistent recurrence per direction -- three persistent launches, the backward direction's carried
partial being a suffix, which the plain recurrence takes in two calls -- in one build and one process.  A measurement tool, not a test
(bench.py has no such workload).

    python tools/bench_bidirection.py [--rows 32 64] [--reps 20] [--pairs 5]

The script's cell: H = 1000, E = 500, T = Tv + Tc = 25 + 35 = 60 chain steps; the forward direction continues from the hoisted frame
products at its first 25 steps, the backward direction at its last 25, read backwards.  Both forms are timed in the same call,
alternating, `pairs` times after a warm-up, with device events around `reps` back-to-back calls.  Prints one JSON line per row count:
the median microseconds per call and per chain step of each form, the difference, and the spread (max - min over the pairs) of each
form -- the one-launch form counts as faster only where the difference exceeds both spreads.

Then the whole XE step of the script (bidirection.Video_Caption_Generator.xe_update: forward, loss, backward, per-variable clip, SGD with
lr = 0 so that every repetition does the same work) with LSTM1's forward in each form, the same way: d = 1024, Tv = 25, Tc = 35, batch 32 as
in bidirection_tf_s2vt.py:233-246, |V| = 12000 (the script's vocabulary file is not distributed; 12000 is this project's synthetic
vocabulary), and the greedy decode of the same batch (s2vt_bidir_decode_greedy, one fused cell launch + one pick launch per decode
step).  --no-step leaves both out.

--beam K: beside the greedy decode, the beam search of the same batch at beam K (bidirection_beam.Beam_Caption_Generator.beam_search:
s2vt_bidir_beam_encode once, then per decode step one index launch, one gathered-state cell launch, the vocabulary product and the top-k
on up to B * K rows, with one host-to-device and one device-to-host copy and the host's heap bookkeeping in between): wall-clock ms per
beam_search call (the search synchronises every step, so device events would not see the host's share), and ms per s2vt_bidir_beam_step
call on B * K rows including its two copies.  The untrained model never emits <eos>, so every video runs all Tc steps: the long case."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

E, H, TV, TC = 500, 1000, 25, 35
FORMS = {"per_direction": 2, "one_launch": 1}      # per_direction: one persistent recurrence per direction = THREE launches (the backward one is cut at step Tc)


def timed_us(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", type=int, default=[32, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--step-reps", type=int, default=3)
    ap.add_argument("--beam", type=int, default=0, help="also time beam search at this beam width (0: off)")
    a = ap.parse_args()
    assert a.pairs >= 3
    import torch
    from s2vt_amd import ops
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    T = TV + TC
    for M in a.rows:
        rng = np.random.default_rng(5)

        def dev(x):
            return torch.as_tensor(x.astype(np.float32)).cuda()
        lim = float(np.sqrt(6.0 / (E + H + 4 * H)))
        dirs = []
        for k in range(2):
            W = dev(rng.uniform(-lim, lim, (E + H, 4 * H))); b = dev(rng.uniform(-.02, .02, 4 * H))
            xp = dev(rng.standard_normal((TV, M, 4 * H)) * 0.3)
            z = torch.zeros(M, H, device="cuda")
            dirs.append(ops.lstm_dir(W, E, b, z, z, T, cinit=xp, cinit_t0=TC if k else 0, reverse=bool(k)))
        fns = {n: (lambda p=p: ops.lstm_birecurrence_fwd(dirs[0], dirs[1], persistent=p)) for n, p in FORMS.items()}
        for fn in fns.values():                                             # warm-up (attributes, workspaces)
            fn(); fn()
        t = {n: [] for n in fns}
        for _ in range(a.pairs):
            for n, fn in fns.items():
                t[n].append(timed_us(fn, a.reps))
        assert ops.chain_timeouts() == 0
        med = {n: float(np.median(v)) for n, v in t.items()}
        out = {"rows": M, "H": H, "E": E, "T": T, "reps": a.reps, "pairs": a.pairs,
               "us_per_call": {n: round(v, 1) for n, v in med.items()},
               "us_per_step": {n: round(v / T, 2) for n, v in med.items()},
               "spread_us": {n: round(float(max(v) - min(v)), 1) for n, v in t.items()},
               "per_direction_minus_one_us": round(med["per_direction"] - med["one_launch"], 1)}
        print(json.dumps(out), flush=True)
    if a.no_step:
        return
    from s2vt_amd import bidirection
    D, V, B = 1024, 12000, 32
    rng = np.random.default_rng(6)
    mdl = bidirection.Video_Caption_Generator(D, V, E, H, B, T, TV, TC, seed=11)
    video = torch.as_tensor((np.abs(rng.standard_normal((B, TV, D))) * 0.5).astype(np.float32)).cuda()
    cap = torch.as_tensor(rng.integers(2, V, (B, TC)).astype(np.int32)).cuda()
    lens = rng.integers(4, TC + 1, B)
    mask = torch.as_tensor((np.arange(TC)[None, :] < lens[:, None]).astype(np.float32)).cuda()
    fns = {n: (lambda p=p: mdl.xe_update(video, cap, mask, lr=0.0, step=0, persistent=p)) for n, p in FORMS.items()}
    for fn in fns.values():
        fn()
    t = {n: [] for n in fns}
    for _ in range(a.pairs):
        for n, fn in fns.items():
            t[n].append(timed_us(fn, a.step_reps) / 1e3)
    assert ops.chain_timeouts() == 0
    med = {n: float(np.median(v)) for n, v in t.items()}
    print(json.dumps({"xe_step": True, "B": B, "d": D, "V": V, "H": H, "E": E, "Tv": TV, "Tc": TC, "reps": a.step_reps, "pairs": a.pairs,
                      "ms_per_step": {n: round(v, 3) for n, v in med.items()},
                      "spread_ms": {n: round(float(max(v) - min(v)), 3) for n, v in t.items()},
                      "per_direction_minus_one_ms": round(med["per_direction"] - med["one_launch"], 3)}), flush=True)
    dec = lambda: mdl.build_sampler(video)
    dec(); dec()
    td = [timed_us(dec, a.step_reps) / 1e3 for _ in range(a.pairs)]
    print(json.dumps({"greedy_decode": True, "B": B, "Tc": TC, "ms_per_call": round(float(np.median(td)), 3), "spread_ms": round(max(td) - min(td), 3),
                      "us_per_decode_step_incl_encode": round(float(np.median(td)) * 1e3 / TC, 1)}), flush=True)

    if a.beam > 0:
        import time
        from s2vt_amd import bidirection_beam
        K = a.beam
        bm = bidirection_beam.Beam_Caption_Generator(D, V, E, H, B, T, TV, TC, params={n: v.cpu().numpy() for n, v in mdl.p.items()})
        vhost = video.cpu().numpy()

        def wall_ms(fn, reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / reps
        search = lambda: bm.beam_search(vhost, K, 0.0, B)
        res = search(); search()
        ts = [wall_ms(search, a.step_reps) for _ in range(a.pairs)]
        # one step on all B * K rows (parents = the rows' own videos' first hypotheses: any valid map costs the same)
        dec = bm._beam_decoder(B, K)
        dec.encode(bm.store.params, video)
        rows0 = np.array([np.arange(B), np.zeros(B), np.ones(B)], np.int32)
        dec.step(bm.store.params, 0, rows0, K)
        R = B * K
        rows = np.array([np.arange(R) % B, np.arange(R) % B, rng.integers(2, V, R)], np.int32)
        one = lambda: dec.step(bm.store.params, 1, rows, K)
        one(); one()
        tp = [wall_ms(one, 20) for _ in range(a.pairs)]
        assert ops.chain_timeouts() == 0
        print(json.dumps({"beam_search": True, "beam": K, "B": B, "Tc": TC, "rows_per_step": R, "steps_run": max(len(s) for s, _, _ in res),
                          "ms_per_call": round(float(np.median(ts)), 3), "spread_ms": round(max(ts) - min(ts), 3),
                          "ms_per_step_call": round(float(np.median(tp)), 4), "step_spread_ms": round(max(tp) - min(tp), 4)}), flush=True)


if __name__ == "__main__":
    main()
