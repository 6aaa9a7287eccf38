"""The self-critical REINFORCE step of the bidirectional captioner: LSTM1's side shared by a video's samples against the plain drivers on the
tiled feature block, and the sampler call alone.  A measurement tool, not a test (bench.py has no such workload).

    python tools/bench_bidirection_rl.py [--B 32] [--K 5] [--pairs 6] [--reps 10] [--eos-bias 0]

The script's dimensions (d = 1024, H = 1000, E = 500, Tv = 25, Tc = 35, |V| = 12000).  One sample() call provides the ids (N = K * B rows);
then, alternating inside every one of --pairs rounds in ONE process (the two forms share whatever the box is doing), timed with device
events around --reps calls:
  shared   reinforce_update(share_lstm1=True):  s2vt_bidir_teacher_forced_fwd_rows / s2vt_bidir_bptt_bwd_rows -- LSTM1, its input products
           and the 2H input rows of lstm2_W (hoist, weight gradient, data gradient) on B rows per step
  tiled    reinforce_update(share_lstm1=False): s2vt_bidir_teacher_forced_fwd / s2vt_bidir_bptt_bwd on the K-times tiled block
both with the mask derived on the device, fixed rewards (no host scorer in the timing) and lr = 0 (the variables stay, so every repetition
does the same work), and
  sample   sample(video, K, with_greedy=True) alone, (K + 1) * B decode rows.
Prints one JSON line: the per-pair times, their medians, the spread between repeats (the larger of the two forms' max - min over the pairs),
the gain tiled - shared, and the verdict by the project's rule -- a gain counts only when it exceeds five times the spread, else it is
"within spread" -- and the largest relative difference of the two forms' gradients (the same sums in different orders)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, reps):
    """milliseconds per call between two device events around `reps` calls"""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--eos-bias", type=float, default=0.0, help="added to embed_word_b[0]: > 0 makes samples end early (the unroll is not cut short)")
    a = ap.parse_args()
    assert a.pairs >= 5, "at least five pairs: the verdict rests on the spread between them"
    import torch
    import s2vt_amd
    from s2vt_amd import bidirection_rl
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    D, H, E, Tv, Tc, V = 1024, 1000, 500, 25, 35, 12000
    mdl = bidirection_rl.Reinforce_Caption_Generator(D, V, E, H, a.B, Tv + Tc, Tv, Tc, seed=11, multisample=a.K)
    with torch.no_grad():
        mdl.p["embed_word_b"][0] += a.eos_bias
    rng = np.random.default_rng(5)
    video = torch.as_tensor((np.abs(rng.standard_normal((a.B, Tv, D))) * 0.5).astype(np.float32)).cuda()
    N = a.K * a.B
    r = torch.as_tensor(rng.uniform(0, 1, N).astype(np.float32)).cuda()
    b = torch.as_tensor(np.tile(rng.uniform(0, 1, a.B), a.K).astype(np.float32)).cuda()
    sample = lambda: mdl.sample(video, a.K, True, seed=7)
    ids, _ = sample()
    step = lambda share: mdl.reinforce_update(video, ids, None, r, b, lr=0.0, share_lstm1=share)
    shared, tiled = (lambda: step(True)), (lambda: step(False))
    grads = {}
    for name, fn in (("shared", shared), ("tiled", tiled)):            # warm-up of both forms (workspaces), and their gradients
        mdl.set_step(0)
        fn()
        grads[name] = mdl.store.grad[:mdl.store.numel].clone()
    diff = float((grads["shared"] - grads["tiled"]).abs().max() / grads["tiled"].abs().max())
    t = {"shared": [], "tiled": [], "sample": []}
    for fn in (shared, tiled, sample):                                  # one untimed round in the timed order: the first pass behind the other form's
        timed(fn, a.reps)                                              # warm-up re-reads everything it evicted
    for _ in range(a.pairs):
        t["shared"].append(timed(shared, a.reps)); t["tiled"].append(timed(tiled, a.reps)); t["sample"].append(timed(sample, a.reps))
    mdl.check_health()
    med = {n: float(np.median(v)) for n, v in t.items()}
    spread = max(max(t[n]) - min(t[n]) for n in ("shared", "tiled"))
    gain = med["tiled"] - med["shared"]
    verdict = "within spread" if abs(gain) <= 5 * spread else ("shared faster" if gain > 0 else "shared slower")
    rnd = lambda v: [round(x, 3) for x in v]
    stamp = {"s2vt_version": s2vt_amd.lib().s2vt_version(), "torch": torch.__version__, "hip": torch.version.hip, "device": torch.cuda.get_device_name(0)}
    print(json.dumps({"B": a.B, "K": a.K, "rows": N, "Tv": Tv, "Tc": Tc, "H": H, "E": E, "V": V, "pairs": a.pairs, "reps": a.reps, "eos_bias": a.eos_bias,
                      "update_shared_ms": rnd(t["shared"]), "update_tiled_ms": rnd(t["tiled"]), "sample_ms": rnd(t["sample"]),
                      "median_ms": {n: round(x, 3) for n, x in med.items()}, "spread_ms": round(spread, 3), "gain_ms": round(gain, 3), "verdict": verdict,
                      "grad_max_rel_diff_shared_vs_tiled": diff, "build": stamp}), flush=True)


if __name__ == "__main__":
    main()
