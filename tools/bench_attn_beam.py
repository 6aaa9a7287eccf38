"""Beam search of the temporal-attention captioner against its yardstick, the greedy decode loop.  A measurement tool, not a test.

    python tools/bench_attn_beam.py [--B 64] [--beams 3 5] [--frames 5 32] [--lnf 0.5] [--reps 5] [--rounds 3]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python tools/bench_attn_beam.py --only beam --frames 32 --beams 5 --rounds 1

Full dimensions (d = 1536, H = 1000, V = 12000, Tc = 20), weights scaled as tools/make_beam_fixtures.py scales them so that beams
compete; with the default --eos-bias no caption ends early, so every search runs all Tc steps at k * B rows from step 1 on.  Per
(frames, beam) it times, alternating over --rounds:
  beam      Attention_Caption_Generator.beam_search on B videos (encode + Tc steps + host bookkeeping, synchronous per step);
  greedy_B  s2vt_attn_decode_greedy on the same B videos (one enqueue, no host exchange);
  greedy_kB s2vt_attn_decode_greedy on k * B rows, the video block tiled k times: the arithmetic volume of the beam search without
            the gather, the top-k or the per-step host exchange.
and splits a beam step into device time (events around the library call) and the rest.  Prints one JSON line per (frames, beam).
--only beam | greedy_kB runs that path alone a few times: the body of a profiler run."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_beam import TimedDecoder  # noqa: E402


def build_model(Tv, B, eos_bias):
    import torch
    from s2vt_amd import attention as A
    mdl = A.Attention_Caption_Generator(1536, 12000, 1000, B, Tv, 20, 0.9, seed=11)
    with torch.no_grad():
        mdl.p["embed_word_W"].mul_(30.0); mdl.p["lstm3_W"].mul_(6.0); mdl.p["Wemb"].mul_(20.0)
        mdl.p["embed_word_b"][0] += eos_bias
    return mdl


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
    ap.add_argument("--beams", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--frames", type=int, nargs="+", default=[5, 32])
    ap.add_argument("--lnf", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eos-bias", type=float, default=-50.0)
    ap.add_argument("--only", choices=("beam", "greedy_kB"), default=None)
    a = ap.parse_args()
    import torch
    from s2vt_amd import ops
    from s2vt_amd.beam_generator import BatchedBeamSearch
    assert torch.cuda.is_available(), "needs a GPU: there is no CPU path to time"
    for Tv in a.frames:
        mdl = build_model(Tv, a.B, a.eos_bias)
        rng = np.random.default_rng(5)
        scale = np.linspace(0.2, 2.0, a.B, dtype=np.float32)[:, None, None]
        video = torch.as_tensor((np.abs(rng.standard_normal((a.B, Tv, 1536))) * scale * 0.5).astype(np.float32)).cuda()
        for k in a.beams:
            tiled = video.repeat(k, 1, 1).contiguous()
            gen = BatchedBeamSearch(mdl, k, a.lnf)
            beam = lambda: gen.generate(video)
            greedy_b = lambda: ops.attn_decode_greedy(mdl.dims, mdl.store.params, video)
            greedy_kb = lambda: ops.attn_decode_greedy(mdl.dims, mdl.store.params, tiled)
            if a.only:
                fn = beam if a.only == "beam" else greedy_kb
                fn()
                print(json.dumps({"only": a.only, "frames": Tv, "beam": k, "ms": round(timed(fn, a.reps) * 1e3, 3)}), flush=True)
                continue
            res = beam(); greedy_b(); greedy_kb()                               # warm-up of every shape (allocates the decoder)
            t = {"beam": [], "greedy_B": [], "greedy_kB": []}
            for _ in range(a.rounds):                                           # alternating: the three share whatever the box is doing
                t["beam"].append(timed(beam, a.reps)); t["greedy_B"].append(timed(greedy_b, a.reps)); t["greedy_kB"].append(timed(greedy_kb, a.reps))
            td = TimedDecoder(gen._dec)
            gen._dec = td
            t_all = timed(beam, a.reps)
            lens = [len(s) for s, _, _ in res]
            ms = lambda v: [round(x * 1e3, 3) for x in v]
            med = {n: float(np.median(v)) for n, v in t.items()}
            steps = td.calls / a.reps
            print(json.dumps({
                "frames": Tv, "beam": k, "B": a.B, "lnf": a.lnf, "Tc": 20,
                "beam_ms": ms(t["beam"]), "greedy_B_ms": ms(t["greedy_B"]), "greedy_kB_ms": ms(t["greedy_kB"]),
                "beam_steps_per_search": steps,
                "per_step_ms": {"beam": round(med["beam"] / steps * 1e3, 4), "greedy_B": round(med["greedy_B"] / 20 * 1e3, 4),
                                "greedy_kB": round(med["greedy_kB"] / 20 * 1e3, 4)},
                "beam_step_ms_device": round(td.dev / td.calls * 1e3, 4), "beam_step_ms_call": round(td.wall / td.calls * 1e3, 4),
                "beam_step_ms_host_bookkeeping_and_encode": round((t_all * a.reps - td.wall) / td.calls * 1e3, 4),
                "caption_len_min_mean_max": [min(lens), round(float(np.mean(lens)), 2), max(lens)],
            }), flush=True)
        del mdl
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
