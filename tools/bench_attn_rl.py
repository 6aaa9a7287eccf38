"""The self-critical REINFORCE step of the temporal-attention captioner: shared image blocks against the tiled feature block, and the
sampler call alone.  A measurement tool, not a test (bench.py has no such workload).

    python tools/bench_attn_rl.py [--B 64] [--K 5] [--frames 5 32] [--reps 10] [--rounds 4] [--eos-bias 0] [--stop-at-eos]

Full dimensions (d = 1536, H = 1000, |V| = 12000, Tc = 20).  Per frame count one sample() call provides the ids (N = K * B rows); then,
alternating over --rounds in ONE process (the two forms share whatever the box is doing):
  shared   reinforce_update(share_image_blocks=True):  the S rows of a video read its one [Tv, H] block (s2vt_attn_*_rows)
  tiled    reinforce_update(share_image_blocks=False): the plain entry points on the K-times tiled feature block
both with the mask derived on the device, fixed rewards (no host scorer in the timing), all Tc steps unrolled, lr = 0 (the variables
stay, so every repetition does the same work), and
  sample   sample(video, K, with_greedy=True) alone, (K + 1) * B rows.
Also reports the largest relative difference of the two forms' gradients (they are the same sums in different orders).  Prints one JSON
line per frame count.

--stop-at-eos: instead of the above, the early-exit sampler against the plain one, alternating inside every round in the same process:
  sample / sample_eos   sample(video, K, True) and sample(..., stop_at_eos=True) alone
  step / step_eos       that sampler call followed by reinforce_update (shared blocks, all Tc steps unrolled) on the ids it returned
with the mean length of the sampled rows (first <eos> included) that the run saw and the build's version / flags; give an --eos-bias that makes it realistic (MSVD
captions average about 7 words).  The live launches' tiles: S2VT_ATTN_EOS_STORE_CFG / S2VT_ATTN_EOS_LSTM_CFG / S2VT_ATTN_EOS_PICK_CFG."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--K", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--eos-bias", type=float, default=0.0, help="added to embed_word_b[0]: > 0 makes samples end early (the unroll is not cut short here)")
    ap.add_argument("--stop-at-eos", action="store_true", help="time the sampler call and sampler + update with and without the early-exit sampler, interleaved")
    a = ap.parse_args()
    import torch
    from s2vt_amd import attention as A
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    for Tv in a.frames:
        mdl = A.Attention_Caption_Generator(1536, 12000, 1000, a.B, Tv, 20, 0.9, seed=11)
        with torch.no_grad():
            mdl.p["embed_word_b"][0] += a.eos_bias
        rng = np.random.default_rng(5)
        video = torch.as_tensor((np.abs(rng.standard_normal((a.B, Tv, 1536))) * 0.5).astype(np.float32)).cuda()
        N = a.K * a.B
        r = torch.as_tensor(rng.uniform(0, 1, N).astype(np.float32)).cuda()
        b = torch.as_tensor(np.tile(rng.uniform(0, 1, a.B), a.K).astype(np.float32)).cuda()
        sample = lambda: mdl.sample(video, a.K, True, seed=7)
        ids, _ = sample()
        if a.stop_at_eos:
            from s2vt_amd import hostglue
            sample_eos = lambda: mdl.sample(video, a.K, True, seed=7, stop_at_eos=True)
            update = lambda s: mdl.reinforce_update(video, s, None, r, b, lr=0.0, active_steps=None, share_image_blocks=True)
            step, step_eos = (lambda: update(sample()[0])), (lambda: update(sample_eos()[0]))
            ref, got = ids.cpu().numpy(), sample_eos()[0].cpu().numpy()
            mask = hostglue.masks_from_ids(ref).astype(bool)
            assert np.array_equal(got[mask], ref[mask]) and (got[~mask] == 0).all(), "the early-exit sampler's ids differ up to the first <eos>"
            fns = {"sample": sample, "sample_eos": sample_eos, "step": step, "step_eos": step_eos}
            for fn in fns.values():                                         # warm-up (workspaces)
                mdl.set_step(0)
                fn()
            t = {n: [] for n in fns}
            for _ in range(a.rounds):
                for n, fn in fns.items():
                    t[n].append(timed(fn, a.reps))
            mdl.check_health()
            import s2vt_amd
            stamp = {"s2vt_version": s2vt_amd.lib().s2vt_version(), "build_flags": s2vt_amd.lib().s2vt_build_flags(), "torch": torch.__version__,
                     "hip": torch.version.hip, "device": torch.cuda.get_device_name(0)}
            print(json.dumps({"frames": Tv, "B": a.B, "K": a.K, "sampler_rows": (a.K + 1) * a.B, "Tc": 20, "eos_bias": a.eos_bias, "build": stamp,
                              "mean_sampled_length": round(float(mask.sum(1).mean()), 2), "rows_without_eos": int((~(ref == 0).any(1)).sum()),
                              "eos_cfg": {k: os.environ.get(k) for k in ("S2VT_ATTN_EOS_STORE_CFG", "S2VT_ATTN_EOS_LSTM_CFG", "S2VT_ATTN_EOS_PICK_CFG")},
                              "ms": {n: [round(x * 1e3, 3) for x in v] for n, v in t.items()},
                              "median_ms": {n: round(float(np.median(v)) * 1e3, 3) for n, v in t.items()}}), flush=True)
            del mdl
            torch.cuda.empty_cache()
            continue
        step = lambda share: mdl.reinforce_update(video, ids, None, r, b, lr=0.0, active_steps=None, share_image_blocks=share)
        shared, tiled = (lambda: step(True)), (lambda: step(False))
        grads = {}
        for name, fn in (("shared", shared), ("tiled", tiled)):        # warm-up of both forms (workspaces), and their gradients
            mdl.set_step(0)
            fn()
            grads[name] = mdl.store.grad[:mdl.store.numel].clone()
        diff = float((grads["shared"] - grads["tiled"]).abs().max() / grads["tiled"].abs().max())
        t = {"shared": [], "tiled": [], "sample": []}
        for _ in range(a.rounds):
            t["shared"].append(timed(shared, a.reps)); t["tiled"].append(timed(tiled, a.reps)); t["sample"].append(timed(sample, a.reps))
        mdl.check_health()
        ms = lambda v: [round(x * 1e3, 3) for x in v]
        med = {n: round(float(np.median(v)) * 1e3, 3) for n, v in t.items()}
        print(json.dumps({"frames": Tv, "B": a.B, "K": a.K, "rows": N, "Tc": 20, "update_shared_ms": ms(t["shared"]), "update_tiled_ms": ms(t["tiled"]),
                          "sample_ms": ms(t["sample"]), "median_ms": med, "grad_max_rel_diff_shared_vs_tiled": diff}), flush=True)
        del mdl
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
