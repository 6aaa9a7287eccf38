"""Self-critical reward on token ids: ctypes binding of libs2vt_host.so (include/s2vt_host.h).

Stands where the reference calls evaluate_captions_cider(ref_decoded, decoded) (cider_evaluation.py:60-87,
driven at reinforcement_multisampling_tf_s2vt.py:784-803): r for the K*B sampled captions, b for the B
greedy captions, both against ALL ground-truth captions of the row's video.  CiderD is that reward; RougeL is what the same call returns in
the scripts that start with `from rouge_evaluation import *` (ROUGE-L), on the host (libs2vt_host.so) and on the device (libs2vt_hip.so).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def host_lib():
    global _LIB
    if _LIB is None:
        path = os.environ.get("S2VT_HOST_LIB") or os.path.join(_HERE, "libs2vt_host.so")   # S2VT_HOST_LIB: the sanitizer build (tests)
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with __graft_entry__.build()")
        L = C.CDLL(path)
        L.s2vt_cider_create.restype = C.c_void_p
        L.s2vt_cider_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.s2vt_cider_destroy.restype = None
        L.s2vt_cider_destroy.argtypes = [C.c_void_p]
        L.s2vt_cider_score.restype = C.c_int
        L.s2vt_cider_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
        L.s2vt_cider_num_videos.restype = C.c_int32
        L.s2vt_cider_num_videos.argtypes = [C.c_void_p]
        L.s2vt_rouge_create.restype = C.c_void_p
        L.s2vt_rouge_create.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.s2vt_rouge_destroy.restype = None
        L.s2vt_rouge_destroy.argtypes = [C.c_void_p]
        L.s2vt_rouge_score.restype = C.c_int
        L.s2vt_rouge_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_int32]
        _LIB = L
    return _LIB


def tokenize_refs(refs_by_video, wordtoix):
    """Reference strings -> (tokens int32, offsets int64, video_of_ref int32).  Words outside the model
    vocabulary get private ids >= len(wordtoix): they take part in n-grams and document frequencies exactly
    as their strings would, and can never equal a generated token."""
    oov = {}
    base = max(wordtoix.values()) + 1
    toks, offs, vids = [], [0], []
    for v, refs in enumerate(refs_by_video):
        for s in refs:
            for w in s.split():
                i = wordtoix.get(w)
                if i is None:
                    i = oov.setdefault(w, base + len(oov))
                toks.append(i)
            offs.append(len(toks))
            vids.append(v)
    return np.asarray(toks, np.int32), np.asarray(offs, np.int64), np.asarray(vids, np.int32)


class CiderD:
    """CIDEr-D scorer over a fixed reference corpus (one document per video)."""

    def __init__(self, refs_by_video, wordtoix, n_threads: int = 0):
        toks, offs, vids = tokenize_refs(refs_by_video, wordtoix)
        self.n_threads = n_threads
        self._h = host_lib().s2vt_cider_create(toks.ctypes.data, offs.ctypes.data, vids.ctypes.data, len(vids), len(refs_by_video))
        if not self._h:
            raise ValueError("s2vt_cider_create failed (empty corpus or bad indices)")

    def score_ids(self, ids, video_of_row, eos_id: int = 0):
        """ids [N, Tc] int32 (numpy or CPU tensor) -> float32 [N] rewards."""
        ids = np.ascontiguousarray(np.asarray(ids), dtype=np.int32)
        vr = np.ascontiguousarray(np.asarray(video_of_row), dtype=np.int32)
        out = np.empty(ids.shape[0], np.float32)
        rc = host_lib().s2vt_cider_score(self._h, ids.ctypes.data, ids.shape[0], ids.shape[1], eos_id, vr.ctypes.data,
                                         out.ctypes.data, self.n_threads)
        if rc != 0:
            raise ValueError("s2vt_cider_score: bad arguments (video index out of range?)")
        return out

    def close(self):
        if self._h:
            host_lib().s2vt_cider_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RougeL:
    """ROUGE-L scorer over a fixed reference corpus: the reward of the reference's rouge_* scripts (`from rouge_evaluation import *`,
    reinforce_multitask_e2e_attribute_loss.py:18 -- their evaluate_captions_cider returns pycocoevalcap's Rouge, beta = 1.2, one candidate
    against all references of its video).  The arithmetic contract is DESIGN.md §3: score_ids (the host library) and score_ids_device
    (one HIP launch on ids that never leave the GPU) give the same float32 bits.
    device: upload the corpus once for score_ids_device (None: host scoring only)."""

    def __init__(self, refs_by_video, wordtoix, beta: float = 1.2, device=None, n_threads: int = 0):
        for v, refs in enumerate(refs_by_video):
            if len(refs) == 0:
                raise ValueError(f"RougeL: video {v} has no references")
        toks, offs, vids = tokenize_refs(refs_by_video, wordtoix)
        self.n_threads = n_threads
        self.beta2 = float(beta) ** 2
        self.n_videos = len(refs_by_video)
        self._h = host_lib().s2vt_rouge_create(toks.ctypes.data, offs.ctypes.data, vids.ctypes.data, len(vids), self.n_videos)
        if not self._h:
            raise ValueError("s2vt_rouge_create failed (empty corpus or bad indices)")
        self._dev = None
        if device is not None:
            import torch
            if int(offs[-1]) >= 2 ** 31:
                raise ValueError("RougeL: the device corpus holds at most 2^31 - 1 tokens")
            # tokenize_refs walks the videos in order: the references are already sorted by video
            video_refs = np.concatenate([[0], np.cumsum(np.bincount(vids, minlength=self.n_videos))]).astype(np.int32)
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to(device)
            self._dev = (up(toks if len(toks) else np.zeros(1, np.int32)), up(offs), up(video_refs), len(vids))

    def score_ids(self, ids, video_of_row, eos_id: int = 0):
        """ids [N, Tc] int32 (numpy or CPU tensor) -> float32 [N] rewards."""
        ids = np.ascontiguousarray(np.asarray(ids), dtype=np.int32)
        vr = np.ascontiguousarray(np.asarray(video_of_row), dtype=np.int32)
        out = np.empty(ids.shape[0], np.float32)
        rc = host_lib().s2vt_rouge_score(self._h, ids.ctypes.data, ids.shape[0], ids.shape[1], eos_id, vr.ctypes.data, self.beta2,
                                         out.ctypes.data, self.n_threads)
        if rc != 0:
            raise ValueError("s2vt_rouge_score: bad arguments (video index out of range?)")
        return out

    def score_ids_device(self, ids, video_of_row, eos_id: int = 0, want_pr: bool = False):
        """ids [N, Tc] int32 device tensor (rows may be a strided view of a wider buffer), video_of_row [N] int32 device tensor -> float32 [N]
        device tensor (with want_pr: also [N, 2] float64 = p, r), queued on the current stream.  A video index outside the corpus gives
        NaN in that row (the host cannot see it)."""
        if self._dev is None:
            raise RuntimeError("RougeL was built without `device`: no corpus on the GPU for score_ids_device")
        from . import ops
        toks, offs, video_refs, n_refs = self._dev
        return ops.rouge_l_score(toks, offs, video_refs, n_refs, ids, video_of_row, self.beta2, eos_id=eos_id, want_pr=want_pr)

    def close(self):
        if self._h:
            host_lib().s2vt_rouge_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


REWARDS = ("cider", "rouge")
METRIC_KEY = {"cider": "ciderD", "rouge": "rougeL"}      # the key an epoch's mean test score is reported under


def make_scorer(kind, refs_by_video, wordtoix, device=None):
    """The reward of a REINFORCE driver: "cider" (CIDEr-D on the host, the default) or "rouge" (ROUGE-L; with `device` also on the GPU)."""
    if kind == "cider":
        return CiderD(refs_by_video, wordtoix)
    if kind == "rouge":
        return RougeL(refs_by_video, wordtoix, device=device)
    raise ValueError(f"reward must be one of {REWARDS}, got {kind!r}")
