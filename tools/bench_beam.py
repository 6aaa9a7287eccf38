"""Videos per second of beam-search decoding: the per-video BeamSearchGenerator against the batched BatchedBeamSearch (one library
call per decode step for every live hypothesis of the batch).  A measurement tool, not a test.

    python tools/bench_beam.py [--B 64] [--beams 3 5] [--lnf 0.0] [--reps 3] [--per-video-videos 16]

BASELINE configs[2] dimensions (d = 1536, E = 500, H = 1000, V = 12000, Tv = 5, Tc = 20), weights scaled as
tools/make_beam_fixtures.py scales them so that beams compete and finish at different steps.  For the batched path it also splits
the time of a decode step into the device work (hipEvents around the step's launches), the rest of the library call (index copy
in, result copy out, launch overhead) and the host bookkeeping (the BestK heaps).  Prints one JSON line per beam size."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build_model(eos_bias):
    import torch
    from s2vt_amd import model as M
    mdl = M.Video_Caption_Generator(1536, 12000, 500, 1000, 64, 0, 5, 20, seed=11)
    p = mdl.store.p
    with torch.no_grad():
        p["embed_word_W"].mul_(30.0); p["lstm1_W"].mul_(6.0); p["lstm2_W"].mul_(6.0); p["Wemb"].mul_(20.0)
        p["embed_word_b"][0] += eos_bias
    return mdl


class TimedDecoder:
    """Wraps ops.BeamDecoder.step: wall time of each call and device time of its launches."""

    def __init__(self, dec):
        self.dec, self.calls, self.wall, self.dev = dec, 0, 0.0, 0.0
        self.max_B = dec.max_B

    def encode(self, *a):
        return self.dec.encode(*a)

    def step(self, *a, **kw):
        import torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = self.dec.step(*a, **kw)                  # ends with the device-to-host copy: synchronous
        e1.record()
        self.wall += time.perf_counter() - t0
        e1.synchronize()
        self.dev += e0.elapsed_time(e1) / 1e3
        self.calls += 1
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--beams", type=int, nargs="+", default=[3, 5])
    ap.add_argument("--lnf", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eos-bias", type=float, default=20.0)
    ap.add_argument("--per-video-videos", type=int, default=16, help="videos timed on the per-video path (it is slow)")
    a = ap.parse_args()
    import torch
    from s2vt_amd.beam_generator import BatchedBeamSearch, BeamSearchGenerator
    mdl = build_model(a.eos_bias)
    rng = np.random.default_rng(5)
    scale = np.linspace(0.2, 2.0, a.B, dtype=np.float32)[:, None, None]
    video = torch.as_tensor((np.abs(rng.standard_normal((a.B, 5, 1536))) * scale).astype(np.float32)).cuda()
    for k in a.beams:
        # per-video path
        gen1 = BeamSearchGenerator(mdl, k, a.lnf)
        gen1.generate(video[:1])                                              # warm-up
        nv = min(a.per_video_videos, a.B)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(nv):
            gen1.generate(video[j:j + 1])
        torch.cuda.synchronize()
        t_pv = (time.perf_counter() - t0) / nv
        # batched path
        gen = BatchedBeamSearch(mdl, k, a.lnf)
        res = gen.generate(video)                                             # warm-up (allocates the decoder)
        timed = TimedDecoder(gen._dec)
        gen._dec = timed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            gen.generate(video)
        torch.cuda.synchronize()
        t_b = (time.perf_counter() - t0) / a.reps
        steps = timed.calls / a.reps
        lens = [len(s) for s, _, _ in res]
        print(json.dumps({
            "beam": k, "B": a.B, "lnf": a.lnf, "eos_bias": a.eos_bias,
            "per_video_videos_per_s": round(1.0 / t_pv, 2), "per_video_ms_per_video": round(t_pv * 1e3, 3),
            "batched_videos_per_s": round(a.B / t_b, 2), "batched_ms_per_batch": round(t_b * 1e3, 3),
            "speedup": round(t_pv * a.B / t_b, 2),
            "batched_steps_per_batch": steps,
            "step_ms_device": round(timed.dev / timed.calls * 1e3, 4),
            "step_ms_call": round(timed.wall / timed.calls * 1e3, 4),
            "step_ms_host_bookkeeping_and_encode": round((t_b * a.reps - timed.wall) / timed.calls * 1e3, 4),
            "caption_len_min_mean_max": [min(lens), round(float(np.mean(lens)), 2), max(lens)],
        }), flush=True)


if __name__ == "__main__":
    main()
