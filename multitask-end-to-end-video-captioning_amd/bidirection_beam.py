"""Beam-search evaluation for the bidirectional S2VT captioner: build_generator(beam_size, length_normalization_factor) of
final_beam_search.py:201-294 applied to bidirection_tf_s2vt.py's model, which is how the reference's test scripts report their numbers.
That script has greedy decoding only, so bidirection.Video_Caption_Generator keeps refusing beam_search; the search lives in this subclass
of the REINFORCE class, whose checkpoints -- and the XE class's -- it loads (restore / train_common.optimistic_restore).

No word ever enters LSTM1: both LSTM1 directions and [fw ; bw] @ W2[:2H] depend on the video only, so every hypothesis of a video shares
them (s2vt_bidir_beam_encode, once per batch).  A decode step (s2vt_bidir_beam_step) is one fused LSTM2 cell launch on the live
hypothesis rows -- its gathered-state form: Wemb rows by word, h / c by parent row, the hoisted partial by video, read in place through
index arrays -- then the vocabulary product and the top-k with its log-normaliser.  The caption bookkeeping (the reference's TopN heaps) is
beam_generator.BatchedBeamSearch's, shared with the other captioners."""
from __future__ import annotations

import numpy as np
import torch

from . import bidirection, bidirection_rl, ops


class Beam_Caption_Generator(bidirection_rl.Reinforce_Caption_Generator):
    """bidirection_rl.Reinforce_Caption_Generator (same constructor) + beam_search and what train_common.beam_eval reads."""

    def _beam_decoder(self, B, beam):
        """The device half of beam_generator.BatchedBeamSearch for this model: encode(params, video) / step(params, t, rows, k)."""
        return ops.BidirBeamDecoder(self._dims(), B, beam, self.device)

    def beam_search(self, video, beam_size=3, length_normalization_factor=0.0, batch_size=64):
        """Beam search over a block of videos [n, Tv, dim_image], batch_size videos at once (beam_generator.BatchedBeamSearch over
        ops.BidirBeamDecoder).  Returns [(sentence ids, logprob, score)] * n, as model.Video_Caption_Generator.beam_search: the best caption
        of each video, cut after its <eos> = 0 when it has one.  A video decodes to the same bits whatever batch it is in."""
        from .beam_generator import BatchedBeamSearch
        gen = BatchedBeamSearch(self, beam_size, length_normalization_factor)
        n = video.shape[0] if hasattr(video, "shape") else len(video)
        out = []
        for a in range(0, n, batch_size):
            out += gen.generate(video[a:a + batch_size])
        return out

    def build_generator(self, video=None, beam_size=None, length_normalization_factor=0.0):
        """Without beam_size: bidirection.Video_Caption_Generator.build_generator, unchanged (the script's greedy graph).  With it
        (final_beam_search.py:201's arguments), for one video [1, Tv, D]: (video, sentence [Tc] int32 -- the best beam caption padded with
        <eos> = 0 --, probs = [])."""
        if beam_size is None:
            return super().build_generator(video)
        if video is None:
            raise ValueError("build_generator(beam_size=...) decodes a given video: pass video [1, Tv, D]")
        if video.shape[0] != 1:
            raise ValueError("build_generator(beam_size=...) decodes one video [1, Tv, D], got %d; beam_search takes a block" % video.shape[0])
        sent, _, _ = self.beam_search(video, int(beam_size), length_normalization_factor, 1)[0]
        Tc = self.n_caption_lstm_step
        ids = np.zeros(Tc, np.int32)
        ids[:min(len(sent), Tc)] = sent[:Tc]
        return video, torch.as_tensor(ids).to(self.device), []


Session = bidirection_rl.Session
TF_NAMES, VARIABLES = bidirection.TF_NAMES, bidirection.VARIABLES
