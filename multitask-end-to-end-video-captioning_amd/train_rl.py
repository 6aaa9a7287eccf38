"""Self-critical REINFORCE driver: the counterpart of train() in reinforcement_multisampling_tf_s2vt.py
:602-880 on the HIP path.

Step of the reference                                   | here
--------------------------------------------------------+---------------------------------------------------
9 sess.run of the sampler graphs (:743-753), each       | model.sample(video, K, with_greedy=True): ONE call,
  re-encoding the batch, vstack on the host (:757-764)  |   one encode, rows already sample-major
decode_captions_masks: ids -> strings + mask (:783-784) | mask on the device (s2vt_caption_mask), no strings
get_captions scan + evaluate_captions_cider x2 (:787-803| reward.CiderD.score_ids on the int32 ids (C++ inverted index, ~3 ms,
  pyciderevalcap on strings)                            |   under the GPU's teacher-forced forward); references indexed once
the rouge_* scripts' `from rouge_evaluation import *`   | --reward rouge: reward.RougeL.score_ids_device on the sampler's own tensors (one HIP launch
  (evaluate_captions_cider returns ROUGE-L there)       |   each for r and b, the baseline tiled on the device); the epoch reports rougeL
features tiled x8 on the host (:779-782)                | never tiled: rows address video n % B
sess.run([train_op, sum_loss]) (:823)                   | model.reinforce_update (forward with dropout, reward-scaled
                                                        |   NLL, BPTT, all-reduce, clip 5, Adam, lr 1e-6 * 0.5^(step//1000))
single GPU (:21)                                        | one process per GPU: `python -m torch.distributed.run --nproc-per-node N
                                                        |   -m s2vt_amd.train_rl ...`; batch_size stays the GLOBAL batch
"""
from __future__ import annotations

import argparse
import random
import time

import numpy as np

from . import hostglue, reward
from .train_common import (Config, Corpus, DataParallel, StepLog, epoch_batches, greedy_eval, learning_rate, lookahead, optimistic_restore,
                           reward_scorers, run_step, save_checkpoint, save_checkpoint_checked)


def rl_config(**kw):
    base = dict(start_learning_rate=1e-6, decay_steps=1000, clip_norm=5.0, batch_size=256, multisample=8,
                model_name="reinforce_multisample_model")
    base.update(kw)
    return Config(**base)


def multilabel_eval(model, corpus, labels, batch_size, threshold=0.5):
    """The multilabel evaluation of the multitask scripts' test loop (reinforce_multitask_e2e_attribute_loss.py:1042-1073): scores of
    evaluate_multilabel on every video of `corpus` against its bag-of-words labels -> sensitivity / specificity / harmmean / precision / f1."""
    tot = np.zeros(6, np.int64)
    vids = corpus.index.video_ids
    for a in range(0, len(vids), batch_size):
        ids = vids[a:a + batch_size]
        scores = model.attribute_scores(corpus.features.batch(ids)).cpu().numpy()
        tot += np.asarray(hostglue.get_metrics(scores, labels[[corpus.index.row[v] for v in ids]], threshold), np.int64)
    tp, tn, fp, fn, cp, cn = (int(x) for x in tot)
    if tp == 0 or tn == 0:                      # (the reference's harmonic mean divides by them: an untrained head may have neither)
        return {"true_positive": tp, "true_negative": tn, "false_positive": fp, "false_negative": fn, "count_pos": cp, "count_neg": cn}
    return dict(hostglue.multilabel_summary(tp, tn, fp, fn, cp, cn), true_positive=tp, true_negative=tn, false_positive=fp, false_negative=fn)


def train(cfg: Config, train_corpus: Corpus, test_corpus: Corpus | None = None, model=None, restore=None, log=print, resume=None,
          attr_vocabulary=None, grad_precision=None):
    """attr_vocabulary (list of attribute words; None = the plain REINFORCE script): the multitask scripts on precomputed features
    (BASELINE configs[3]).  Labels = bag of words over all ground-truth captions of a video (get_multilabel, reinforce_multitask_e2e_attribute_loss.py
    :874-893), the model gets the attribute head (label_dim = len(attr_vocabulary), alpha = cfg.alpha) and the objective becomes
    -(1 - alpha) PG / sum(mask) + alpha BCE / (A B) (..._loss.py:957); with cfg.lambda_loss > 0 the ground-truth XE term of ..._s2vt.py:850 is mixed in
    (model.mixed_update: the batch's own sentences as ground truth, every variable decayed as that script's predicate does).  Each epoch also reports
    the multilabel metrics of the script's test loop (:1042-1073).
    cfg.batch_size is the GLOBAL batch (the reference's batch_size).  Under torch.distributed.run every rank walks the
    same shuffled epoch, takes its shard of each batch (videos [lo, hi) of the global batch, global indices in the noise
    counters), scores its own captions, and the gradient bucket is all-reduced inside reinforce_update; rank 0 logs and
    writes checkpoints.
    cfg.mix_baseline = P (None: off): the step of reinforce_multitask_e2e_attribute_by_groudtruth_greedy_s2vt.py:957-979 -- the GREEDY caption is the
    policy's sample and the baseline is the reward of a mixed decode, a greedy decode fed the batch's own ground-truth sentence word by word with
    probability P / 1.00001 (model.mix_sample; one call decodes both from one encode, coins keyed by the global video index).  The update runs on
    the greedy ids with their own mask: model.mixed_update when cfg.lambda_loss > 0 (that script's objective, :850), reinforce_update otherwise.
    One caption per video: cfg.multisample must be 1.  restore: variables of an earlier model (optimistic, :667 -- the step counter of an XE checkpoint
    does not match this script's 'g_step', Adam's slots do); resume: a checkpoint of THIS driver, counters included."""
    import torch
    from . import model as M
    par = DataParallel(model.device if model is not None else None)
    if not par.chief:
        log = lambda *_: None
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(train_corpus.vocabulary)
    K = cfg.multisample
    mix_p = cfg.mix_baseline
    if mix_p is not None:
        if K != 1:
            raise ValueError(f"mix_baseline: the greedy caption is the one sample per video (reinforce_multitask_e2e_attribute_by_groudtruth_greedy_s2vt.py"
                             f":957-979), so multisample / --samples must be 1, got {K}")
        if not 0.0 <= float(mix_p) <= 1.0:
            raise ValueError(f"mix_baseline is a probability in [0, 1], got {mix_p!r}")
        if cfg.stop_at_eos:
            raise ValueError("mix_baseline: the mixed decode has no early-exit form; drop stop_at_eos")
    B = par.per_rank(cfg.batch_size)
    multitask = attr_vocabulary is not None
    if model is None:
        model = M.Video_Caption_Generator(cfg.dim_image, len(wordtoix), cfg.word_dim, cfg.lstm_dim, B,
                                          cfg.n_video_lstm_step + cfg.n_caption_lstm_step, cfg.n_video_lstm_step,
                                          cfg.n_caption_lstm_step, bias_init_vector=None, seed=cfg.seed, multisample=K, device=par.device,
                                          label_dim=len(attr_vocabulary) if multitask else 0, alpha=cfg.alpha if multitask else 0.0,
                                          residual=cfg.residual)
    if mix_p is not None and getattr(model, "residual", False):
        raise ValueError("mix_baseline is not implemented for a residual model (residual=True / --residual)")
    if grad_precision is not None:
        model.grad_precision = grad_precision          # (None: the model's default, S2VT_GRAD_PRECISION)
    par.attach(model)
    labels = test_labels = None
    if multitask:
        def label_matrix(corpus):
            lab = hostglue.get_multilabel(corpus.index.by_video, attr_vocabulary)
            return np.stack([lab[v] for v in corpus.index.video_ids]).astype(np.float32)
        labels = label_matrix(train_corpus)
        test_labels = label_matrix(test_corpus) if test_corpus is not None else None
    if restore:
        log(f"restored: {optimistic_restore(model, restore, step_names=('g_step',))}")
    if resume:
        log(f"resumed: {optimistic_restore(model, resume)} at step {model.global_step}")
    scorer, test_scorer, metric = reward_scorers(cfg, train_corpus.index.refs_by_video(),
                                                 test_corpus.index.refs_by_video() if test_corpus is not None else None, wordtoix, model.device)
    on_device = cfg.reward == "rouge"           # the reward is scored on the sampler's own tensors: the advantage never waits for the host
    rng = random.Random(cfg.seed)
    caps = train_corpus.captions
    history = []
    steplog = StepLog(cfg.step_log if par.chief else None)
    if test_corpus is not None:
        log(f"before train: {metric} {greedy_eval(model, test_corpus, ixtoword, test_scorer, B, par)[1]}")
    def prepare(gidx):
        """Host side of one step: this rank's shard of the batch, its features on their way to the GPU (one copy, shared by
        sample + update), the reward tables' rows of its videos."""
        idx, lo = par.shard(gidx)
        vid = caps[idx, 0]
        rows = np.asarray([train_corpus.index.row[v] for v in vid], np.int32)
        out = dict(lo=lo, video=model._dev(train_corpus.features.batch(vid), torch.float32), rows=rows)
        if on_device:
            out["rows_dev"] = model._dev(rows, torch.int32)
            out["rows_dev_k"] = out["rows_dev"].repeat(K)                  # [K*B], sample-major like the ids
        if multitask:
            out["labels"] = model._dev(labels[rows], torch.float32)
        if (multitask and cfg.lambda_loss > 0) or mix_p is not None:
            # the batch's own sentences are the ground truth of the XE term (..._s2vt.py:977-983) and the words the mixed decode is fed
            gt, gm = hostglue.sentence_padding_toix(caps[idx, 1].tolist(), wordtoix, cfg.n_caption_lstm_step)
            out["gt"], out["gmask"] = np.asarray(gt, np.int32), np.asarray(gm, np.float32)
        return out

    for epoch in range(cfg.n_epochs):
        losses, adv = [], []
        batches = (g for it, g in enumerate(epoch_batches(len(caps), cfg.batch_size, rng)) if not (cfg.max_steps_per_epoch and it >= cfg.max_steps_per_epoch))
        cur, pending, t0 = None, None, time.time()
        for it, (gidx, gnext) in enumerate(lookahead(batches)):
            if cur is None:
                cur = prepare(gidx)
            video, rows, lo = cur["video"], cur["rows"], cur["lo"]
            rb, nxt = {}, {}

            def step():
                samples, greedy_words = model.sample(video, K, True, seed=cfg.seed + 7919 * (model.global_step + 1), video_base=lo, stop_at_eos=cfg.stop_at_eos)
                s_host, g_host = samples.cpu().numpy(), greedy_words.cpu().numpy()
                model.check_health()            # the ids just came to the host: a starved sampler recurrence is caught before it is scored

                def rewards():                  # runs on the host while the GPU does the teacher-forced forward
                    if on_device:               # two launches behind the forward, on the sampler's own tensors; the baseline is tiled on the device
                        rb["r"] = scorer.score_ids_device(samples, cur["rows_dev_k"])
                        rb["b"] = scorer.score_ids_device(greedy_words, cur["rows_dev"])
                        return rb["r"], rb["b"].repeat(K)
                    rb["r"] = scorer.score_ids(s_host, np.tile(rows, K))                 # [K*B], sample-major like the ids
                    rb["b"] = scorer.score_ids(g_host, rows)                            # [B]
                    return rb["r"], hostglue.tile_baseline(rb["b"], K)
                # the ids are on the host anyway: behind the longest sample (its first <eos> included) every position of the
                # batch is masked, and the update does not unroll those steps
                eos = s_host == 0
                steps = int(np.where(eos.any(1), eos.argmax(1) + 1, s_host.shape[1]).max())
                if multitask and cfg.lambda_loss > 0:
                    r_, b_ = rewards()
                    return model.mixed_update(video, samples, hostglue.masks_from_ids(s_host), r_, b_, cur["gt"], cur["gmask"],
                                              lr=learning_rate(cfg, model.global_step), lambda_loss=cfg.lambda_loss, clip_norm=cfg.clip_norm, video_base=lo,
                                              true_labels=cur["labels"], decay_all=True, reuse_sampler_state=True)
                if multitask:
                    return model.reinforce_update(video, samples, None, None, None, lr=learning_rate(cfg, model.global_step),
                                                  clip_norm=cfg.clip_norm, video_base=lo, reuse_sampler_state=True, reward_fn=rewards,
                                                  active_steps=steps, live_mask=hostglue.masks_from_ids(s_host), true_labels=cur["labels"])
                return model.reinforce_update(video, samples, None, None, None, lr=learning_rate(cfg, model.global_step),
                                              clip_norm=cfg.clip_norm, video_base=lo, reuse_sampler_state=True, reward_fn=rewards,
                                              active_steps=steps, live_mask=hostglue.masks_from_ids(s_host))

            def step_mix():         # ..._by_groudtruth_greedy_s2vt.py:957-979: r = reward(greedy), b = reward(mixed decode), the update on the greedy ids
                mix, greedy_words = model.mix_sample(video, cur["gt"], mix_p, True, seed=cfg.seed + 7919 * (model.global_step + 1), video_base=lo)
                m_host, g_host = mix.cpu().numpy(), greedy_words.cpu().numpy()
                model.check_health()
                if on_device:
                    rb["r"], rb["b"] = scorer.score_ids_device(greedy_words, cur["rows_dev"]), scorer.score_ids_device(mix, cur["rows_dev"])
                else:
                    rb["r"], rb["b"] = scorer.score_ids(g_host, rows), scorer.score_ids(m_host, rows)
                g_mask = hostglue.masks_from_ids(g_host)
                labels_ = cur["labels"] if multitask else None
                if cfg.lambda_loss > 0:
                    return model.mixed_update(video, greedy_words, g_mask, rb["r"], rb["b"], cur["gt"], cur["gmask"], lr=learning_rate(cfg, model.global_step),
                                              lambda_loss=cfg.lambda_loss, clip_norm=cfg.clip_norm, video_base=lo, true_labels=labels_, decay_all=multitask)
                return model.reinforce_update(video, greedy_words, g_mask, rb["r"], rb["b"], lr=learning_rate(cfg, model.global_step), clip_norm=cfg.clip_norm,
                                              video_base=lo, true_labels=labels_)

            def overlap():          # while the GPU runs the update: the next batch, and the previous step's log lines
                if gnext is not None:
                    nxt.update(prepare(gnext))
                if pending is not None:
                    pending()
            st, loss = run_step(model, step if mix_p is None else step_mix, log, overlap=overlap)
            r, b = rb["r"], rb["b"]
            losses.append(loss)
            if not on_device:
                adv.append(float(r.mean() - b.mean()))
            t1 = time.time()

            def pending(it=it, loss=loss, lr=learning_rate(cfg, model.global_step), step=model.global_step, rm=None if on_device else float(r.mean()),
                        bm=None if on_device else float(b.mean()), secs=t1 - t0, r=r, b=b):
                if on_device:                   # device-resident rewards: their means are read when the log line is written, not in the step
                    rm, bm = float(r.mean()), float(b.mean())
                    adv.append(rm - bm)
                log(f"idx: {it * cfg.batch_size} rate: {lr:g} Epoch: {epoch} loss: {loss:.5f} r: {rm:.4f} b: {bm:.4f} Elapsed time: {secs:.3f}")
                steplog.write(kind="step", epoch=epoch, step=step, lr=lr, loss=loss, reward=rm, baseline=bm, seconds=secs)
            t0, cur = t1, (nxt if gnext is not None else None)
        if pending is not None:
            pending()
        entry = {"epoch": epoch, "loss": float(np.mean(losses)) if losses else None, "r_minus_b": float(np.mean(adv)) if adv else None}
        if test_corpus is not None:
            _, entry[metric] = greedy_eval(model, test_corpus, ixtoword, test_scorer, B, par)
            if multitask:
                entry["multilabel"] = multilabel_eval(model, test_corpus, test_labels, B)
        ck = save_checkpoint_checked(model, cfg, epoch, step_name="g_step", chief=par.chief)
        if par.chief:
            entry["checkpoint"] = ck
        history.append(entry)
        steplog.write(kind="epoch", residual=bool(cfg.residual), **entry)
        log(f"Epoch {epoch} is done: {entry}")
    steplog.close()
    return model, history


def train_bidirectional(cfg: Config, train_corpus: Corpus, test_corpus: Corpus | None = None, model=None, restore=None, resume=None, log=print):
    """The loop of train() on the bidirectional captioner (bidirection_rl.Reinforce_Caption_Generator): per step model.sample (K multinomial
    captions + the greedy one, LSTM1 once per video), CIDEr-D of both on the host under the queued teacher-forced forward, model.reinforce_update
    (LSTM1's side of the forward and the backward on B rows), a step-log record; per epoch a checkpoint `<model_name>-<epoch>` under the TF
    names with Adam's slots and the counter as g_step.  restore: an XE checkpoint of train_xe --bidirectional (variables only, the counters start at
    zero as the reference's optimistic restore leaves them); resume: a checkpoint of THIS driver.  One process, one GPU: data parallel is not
    built for this model.  Returns (model, history)."""
    import os
    import torch
    from . import bidirection_rl
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("--bidirectional trains in one process: data parallel is not built for the bidirectional captioner")
    if cfg.residual or cfg.mix_baseline is not None or cfg.stop_at_eos:
        raise ValueError("the bidirectional captioner has no residual form, no mixed baseline and no early-exit sampler")
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(train_corpus.vocabulary)
    K, B = cfg.multisample, cfg.batch_size
    if model is None:
        model = bidirection_rl.Reinforce_Caption_Generator(cfg.dim_image, len(wordtoix), cfg.word_dim, cfg.lstm_dim, B, cfg.n_video_lstm_step + cfg.n_caption_lstm_step,
                                                           cfg.n_video_lstm_step, cfg.n_caption_lstm_step, bias_init_vector=None, seed=cfg.seed, multisample=K)
    if restore:
        model.restore(restore)
        log(f"restored: {restore}")
    if resume:
        model.restore(resume)
        log(f"resumed: {resume} at step {model.global_step}")
    scorer, test_scorer, metric = reward_scorers(cfg, train_corpus.index.refs_by_video(),
                                                 test_corpus.index.refs_by_video() if test_corpus is not None else None, wordtoix, model.device)
    on_device = cfg.reward == "rouge"
    rng = random.Random(cfg.seed)
    caps = train_corpus.captions
    history = []
    steplog = StepLog(cfg.step_log)
    if test_corpus is not None:
        log(f"before train: {metric} {greedy_eval(model, test_corpus, ixtoword, test_scorer, B)[1]}")
    for epoch in range(cfg.n_epochs):
        losses, adv = [], []
        for it, idx in enumerate(epoch_batches(len(caps), B, rng)):
            if cfg.max_steps_per_epoch and it >= cfg.max_steps_per_epoch:
                break
            t0 = time.time()
            vid = caps[idx, 0]
            rows = np.asarray([train_corpus.index.row[v] for v in vid], np.int32)
            video = model._dev(train_corpus.features.batch(vid), torch.float32)
            lr = learning_rate(cfg, model.global_step)
            rb = {}

            def step():
                samples, greedy_words = model.sample(video, K, True, seed=cfg.seed + 7919 * (model.global_step + 1))
                s_host, g_host = samples.cpu().numpy(), greedy_words.cpu().numpy()
                model.check_health()            # the ids just came to the host: a starved recurrence is caught before it is scored

                def rewards():                  # runs on the host while the GPU does the teacher-forced forward
                    if on_device:               # two launches on the sampler's own tensors, the baseline tiled on the device
                        rows_dev = model._dev(rows, torch.int32)
                        rb["r"] = scorer.score_ids_device(samples, rows_dev.repeat(K))
                        rb["b"] = scorer.score_ids_device(greedy_words, rows_dev)
                        return rb["r"], rb["b"].repeat(K)
                    rb["r"] = scorer.score_ids(s_host, np.tile(rows, K))                 # [K*B], sample-major like the ids
                    rb["b"] = scorer.score_ids(g_host, rows)                            # [B]
                    return rb["r"], hostglue.tile_baseline(rb["b"], K)
                return model.reinforce_update(video, samples, None, None, None, lr=lr, clip_norm=cfg.clip_norm, reward_fn=rewards)
            st, loss = run_step(model, step, log)
            if not np.isfinite(loss):
                raise FloatingPointError(f"bidirectional captioner, REINFORCE step {model.global_step}: the loss is {loss}")
            rm, bm = float(rb["r"].mean()), float(rb["b"].mean())
            losses.append(loss); adv.append(rm - bm)
            secs = time.time() - t0
            log(f"idx: {it * B} rate: {lr:g} Epoch: {epoch} loss: {loss:.5f} r: {rm:.4f} b: {bm:.4f} Elapsed time: {secs:.3f}")
            steplog.write(kind="step", epoch=epoch, step=model.global_step, lr=lr, loss=loss, reward=rm, baseline=bm, seconds=secs)
        entry = {"epoch": epoch, "loss": float(np.mean(losses)) if losses else None, "r_minus_b": float(np.mean(adv)) if adv else None}
        if test_corpus is not None:
            _, entry[metric] = greedy_eval(model, test_corpus, ixtoword, test_scorer, B)
        model.check_health()
        os.makedirs(cfg.model_path, exist_ok=True)
        entry["checkpoint"] = os.path.join(cfg.model_path, f"{cfg.model_name}-{epoch}")
        model.save(entry["checkpoint"], tf_version=2)          # the REINFORCE script's Saver writes V2 (reinforcement_multisampling_tf_s2vt.py:661)
        history.append(entry)
        steplog.write(kind="epoch", bidirectional=True, **entry)
        log(f"Epoch {epoch} is done: {entry}")
    steplog.close()
    return model, history


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-sents", required=True); ap.add_argument("--train-feats", required=True)
    ap.add_argument("--test-sents"); ap.add_argument("--test-feats")
    ap.add_argument("--vocab", required=True); ap.add_argument("--restore"); ap.add_argument("--resume")
    ap.add_argument("--epochs", type=int, default=30); ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--samples", type=int, default=8); ap.add_argument("--model-path", default="./new_multisamp_reinforcement_models")
    ap.add_argument("--stop-at-eos", action="store_true", help="samples leave the decode loop at their first <eos> (same update, shorter sampler loop)")
    ap.add_argument("--attr-vocab", help="multitask scripts: file with one attribute word per line (label_dim = its length)")
    ap.add_argument("--alpha", type=float, default=0.05); ap.add_argument("--lambda-loss", type=float, default=0.0)
    ap.add_argument("--mix-baseline", type=float, metavar="P", help="the greedy caption is the policy's sample and the baseline is the reward of a greedy "
                    "decode fed ground-truth words with probability P / 1.00001 (reinforce_multitask_e2e_attribute_by_groudtruth_greedy_s2vt.py:957-979; "
                    "0.9 there); needs --samples 1; with --lambda-loss > 0 the update is that script's mixed objective")
    ap.add_argument("--residual", action="store_true", help="the residual captioner of residual_tf_s2vt.py: out1 + out2 into the vocabulary projection")
    ap.add_argument("--grad-precision", choices=("fp32", "bf16"), help="the backward's gradient contractions on bf16 operands (non-parity "
                    "fast mode, DESIGN.md §3); default: S2VT_GRAD_PRECISION, else fp32")
    ap.add_argument("--bidirectional", action="store_true", help="the bidirectional captioner of bidirection_tf_s2vt.py (d = 1024, Tv = 25) under this "
                    "script's self-critical stage: LSTM1 runs once per video, the samples share it (train_bidirectional); --restore takes a "
                    "train_xe --bidirectional checkpoint")
    ap.add_argument("--reward", choices=reward.REWARDS, default="cider", help="the self-critical reward: CIDEr-D on the host (default), or ROUGE-L as the "
                    "rouge_* scripts and reinforce_multitask_e2e_attribute_loss.py optimise it, scored on the device from the sampler's own tensors")
    a = ap.parse_args(argv)
    if a.bidirectional:
        if a.residual or a.mix_baseline is not None or a.stop_at_eos or a.attr_vocab or a.grad_precision:
            ap.error("--bidirectional does not combine with --residual, --mix-baseline, --stop-at-eos, --attr-vocab or --grad-precision")
        cfg = rl_config(dim_image=1024, n_video_lstm_step=25, n_caption_lstm_step=35, n_epochs=a.epochs, batch_size=a.batch_size, multisample=a.samples,
                        model_path=a.model_path, model_name="reinforce_bimodel", reward=a.reward)
        tr = Corpus(a.train_sents, a.train_feats, vocabulary_file=a.vocab)
        te = Corpus(a.test_sents, a.test_feats, vocabulary=tr.vocabulary) if a.test_sents and a.test_feats else None
        train_bidirectional(cfg, tr, te, restore=a.restore, resume=a.resume)
        return
    cfg = rl_config(n_epochs=a.epochs, batch_size=a.batch_size, multisample=a.samples, model_path=a.model_path, stop_at_eos=a.stop_at_eos,
                    alpha=a.alpha, lambda_loss=a.lambda_loss, mix_baseline=a.mix_baseline, residual=a.residual, reward=a.reward)
    tr = Corpus(a.train_sents, a.train_feats, vocabulary_file=a.vocab)
    te = Corpus(a.test_sents, a.test_feats, vocabulary=tr.vocabulary) if a.test_sents and a.test_feats else None
    attr = [l.strip() for l in open(a.attr_vocab)] if a.attr_vocab else None
    train(cfg, tr, te, restore=a.restore, resume=a.resume, attr_vocabulary=attr, grad_precision=a.grad_precision)


if __name__ == "__main__":
    main()
