"""Beam-search captions for a test set from a checkpoint (the test() of final_beam_search.py:504-545 / e2e_beam_search.py, batched):

    python -m s2vt_amd.beam_eval --checkpoint CKPT --test-sents SENTS --test-feats FEATS --vocab VOCAB \
        [--beam 3] [--lnf 0.0] [--batch-size 64] [--n-caption-lstm-step 35] [--out captions.txt] [--model auto|s2vt|attention|bidirectional]
        [--topk-feed [--topk-k 5]]

The checkpoint is loaded with optimistic_restore (an .npz dump or a TensorFlow checkpoint); the model's dimensions are read from
its variables, Tv from the feature file.  The model class is read off the variable names too: a checkpoint that holds embed_att_Wa
is the temporal-attention captioner (original_attention.py:64-86), one that holds the forward LSTM1 cell of bidirection_tf_s2vt.py's
static_bidirectional_rnn (bidirection.TF_NAMES["lstm1_fw_W"]) the bidirectional captioner -- an XE or a REINFORCE checkpoint of it --, any
other the S2VT model; --model overrides the detection.  Writes one `video_id<TAB>sentence` line per test video, as the reference does (the
caption cut at its first <eos>, <bos> / <eos> dropped), and prints the mean CIDEr-D against the test set's references.

--topk-feed decodes an S2VT checkpoint greedily by build_generator of sum_generate_words_tf_s2vt.py:221-275 instead: LSTM2 is fed the
weighted sum of the embeddings of its own top-k words, weights and emitted word from the unshifted softmax (Video_Caption_Generator.
generate_topk_feed) -- what a checkpoint of train_xe --topk-feed was trained to be decoded with.  Beam search over that soft feed is not
implemented: --beam and --lnf are not read."""
from __future__ import annotations

import argparse
import sys


def caption_text(ids, ixtoword) -> str:
    """The reference's output sentence (final_beam_search.py:531-539): the words up to and including the first <eos>, joined,
    with <bos> and <eos> removed.  (Without an <eos>, the reference's np.argmax(... == '<eos>') + 1 keeps only the first word;
    here the whole caption is kept.)"""
    words = []
    for t in ids:
        w = ixtoword[int(t)]
        if w == "<eos>":
            break
        if w != "<bos>":
            words.append(w)
    return " ".join(words)


def write_captions(path, captions) -> None:
    """captions: iterable of (video_id, sentence text) -> `video_id<TAB>sentence` lines (final_beam_search.py:540-545)."""
    with open(path, "w") as f:
        for vid, text in captions:
            f.write(f"{vid}\t{text}\n")


def read_captions(path) -> dict:
    out = {}
    with open(path) as f:
        for line in f:
            vid, _, text = line.rstrip("\n").partition("\t")
            out[vid] = text
    return out


def model_kind(variable_names, choice="auto") -> str:
    """"attention", "bidirectional" or "s2vt" for a checkpoint's variable names (any iterable of names, e.g. the dict read_checkpoint
    returns): embed_att_Wa exists only in the temporal-attention captioner, the forward LSTM1 cell of a bidirectional_rnn scope only in the
    bidirectional one.  `choice` other than "auto" wins."""
    if choice != "auto":
        if choice not in ("s2vt", "attention", "bidirectional"):
            raise ValueError(f"model: {choice!r} (auto, s2vt, attention or bidirectional)")
        return choice
    names = set(variable_names)
    if "embed_att_Wa" in names:
        return "attention"
    from .tfckpt import BIDIRECTION_TF_NAMES
    return "bidirectional" if BIDIRECTION_TF_NAMES["lstm1_fw_W"] in names else "s2vt"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--test-sents", required=True); ap.add_argument("--test-feats", required=True)
    ap.add_argument("--vocab", required=True)
    ap.add_argument("--beam", type=int, default=3); ap.add_argument("--lnf", type=float, default=0.0)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--n-caption-lstm-step", type=int, default=35)
    ap.add_argument("--out", default="beam_captions.txt")
    ap.add_argument("--model", choices=("auto", "s2vt", "attention", "bidirectional"), default="auto")
    ap.add_argument("--residual", action="store_true", help="decode as the residual captioner of residual_tf_s2vt.py (an S2VT checkpoint "
                    "does not say which script trained it)")
    ap.add_argument("--topk-feed", action="store_true", help="greedy decoding by the generator of sum_generate_words_tf_s2vt.py (S2VT checkpoints)")
    ap.add_argument("--topk-k", type=int, default=5, metavar="K", help="with --topk-feed: the number of words in the mix, 1..8")
    a = ap.parse_args(argv)
    if a.topk_feed and (a.residual or a.model not in ("auto", "s2vt") or not 1 <= a.topk_k <= 8):
        ap.error("--topk-feed decodes a plain S2VT checkpoint with 1 <= --topk-k <= 8")

    from . import hostglue, reward, tfckpt
    from . import model as M
    from .train_common import Corpus, beam_eval, greedy_eval, optimistic_restore
    corpus = Corpus(a.test_sents, a.test_feats, vocabulary_file=a.vocab)
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(corpus.vocabulary)
    raw = tfckpt.read_checkpoint(a.checkpoint)
    V, E = raw["Wemb"].shape
    D = raw["encode_image_W"].shape[0]
    H = raw["embed_word_W"].shape[0]
    if V != len(wordtoix):
        raise SystemExit(f"checkpoint vocabulary has {V} words, {a.vocab} gives {len(wordtoix)}")
    Tv = corpus.features.features.shape[1]
    Tc = a.n_caption_lstm_step
    kind = model_kind(raw, a.model)
    if a.topk_feed and kind != "s2vt":
        raise SystemExit(f"--topk-feed is an S2VT generator; this checkpoint is a {kind} model")
    if kind == "attention":
        from . import attention as A
        if a.residual:
            raise SystemExit("--residual is an S2VT variant; this checkpoint is an attention model")
        model = A.Attention_Caption_Generator(D, V, E, a.batch_size, Tv, Tc, 1.0, bias_init_vector=None)    # dim_hidden = Wemb.shape[1] (:65)
    elif kind == "bidirectional":
        from . import bidirection_beam as BB
        if a.residual:
            raise SystemExit("--residual is an S2VT variant; this checkpoint is a bidirectional model")
        model = BB.Beam_Caption_Generator(D, V, E, H, a.batch_size, Tv + Tc, Tv, Tc, bias_init_vector=None)
    else:
        model = M.Video_Caption_Generator(D, V, E, H, a.batch_size, Tv + Tc, Tv, Tc, bias_init_vector=None, residual=a.residual)
    optimistic_restore(model, a.checkpoint)
    scorer = reward.CiderD(corpus.index.refs_by_video(), wordtoix)
    if a.topk_feed:
        decoded, cider = greedy_eval(model, corpus, ixtoword, scorer, a.batch_size, decode=lambda f: model.generate_topk_feed(f, k=a.topk_k))
        write_captions(a.out, [(v, caption_text([wordtoix[w] for w in decoded[v].split()], ixtoword)) for v in corpus.index.video_ids])
        print(f"top-{a.topk_k} feed, greedy: {len(decoded)} videos, mean CIDEr-D {cider:.4f} -> {a.out}")
        return 0
    decoded, cider = beam_eval(model, corpus, ixtoword, scorer, a.batch_size, a.beam, a.lnf)
    write_captions(a.out, [(v, caption_text([wordtoix[w] for w in decoded[v].split()], ixtoword)) for v in corpus.index.video_ids])
    print(f"beam {a.beam} lnf {a.lnf}: {len(decoded)} videos, mean CIDEr-D {cider:.4f} -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
