"""Training driver of the temporal-attention captioner: the counterpart of train() in original_attention.py:383-520 on the HIP path.

    python -m s2vt_amd.train_attention --train-sents S --train-feats F --test-sents S2 --test-feats F2 --vocab V [--frames 32]

Per step the reference runs sess.run([train_op, tf_loss]) on build_model (cross entropy on the ground-truth caption + the alpha
regulariser, clip 10, Adam, lr 1e-4 halved every 10000 steps, :430-441); here that is Attention_Caption_Generator.xe_update.  Every
epoch: greedy captions of the test videos through the sampler graph (:483-497) and a checkpoint under the TF variable names (:519).
One process per GPU under torch.distributed.run for data parallel (every rank walks the same shuffled epoch and takes its shard).

    python -m s2vt_amd.train_attention ... --reinforce --samples 5 --restore XE_CHECKPOINT

is the CIDEr fine-tuning stage the reinforcement_* scripts apply to their models, on this one: the loop of train_rl.train -- K multinomial
samples + the greedy caption per video in one sampler call, CIDEr-D on the ids (reward.py) on the host under the queued teacher-forced
forward, then Attention_Caption_Generator.reinforce_update (clip 5, lr 1e-6 halved every 1000 steps unless the config says otherwise)."""
from __future__ import annotations

import argparse
import random
import time

import numpy as np
import torch

from . import hostglue, reward
from .train_common import (Config, Corpus, DataParallel, StepLog, beam_eval, epoch_batches, greedy_eval, learning_rate, lookahead,
                           optimistic_restore, reward_scorers, run_step, save_checkpoint_checked)


def attention_config(**kw):
    """original_attention.py:293-311: dim_hidden 1000, 35 caption steps, 20 epochs, lr 1e-4 / 10000 steps, clip 10."""
    base = dict(start_learning_rate=1e-4, decay_steps=10000, clip_norm=10.0, batch_size=64, n_epochs=20, n_caption_lstm_step=35,
                model_path="./attention_models", model_name="attention_model")
    base.update(kw)
    return Config(**base)


def reinforce_config(**kw):
    """The REINFORCE stage's "Train Parameters" (reinforcement_multisampling_tf_s2vt.py:505-517) on this model's dimensions."""
    return attention_config(**dict(dict(start_learning_rate=1e-6, decay_steps=1000, clip_norm=5.0, model_name="attention_reinforce_model"), **kw))


def train(cfg: Config, train_corpus: Corpus, test_corpus: Corpus | None = None, model=None, log=print, resume=None, m=0.5, beta=10.0,
          eval_beam=0, eval_lnf=0.0, reinforce=False, samples=5, restore=None):
    """cfg.batch_size is the GLOBAL batch; cfg.lstm_dim is dim_hidden (the word embedding has the same width, :65).  eval_beam > 0:
    the per-epoch evaluation decodes with a beam of that size and length normalisation eval_lnf (train_common.beam_eval) instead of
    greedily.
    reinforce: the self-critical stage instead of cross entropy -- per step `samples` multinomial captions and the greedy one per video
    (model.sample, global video indices in the noise counters), CIDEr-D of both against the training references, and
    model.reinforce_update with reward = the samples' scores and baseline = the greedy caption's; logging, checkpoints and the
    per-epoch evaluation are the same.  cfg.stop_at_eos: the sampler's early-exit mode (model.sample(stop_at_eos=True)) -- same update.
    restore: variables (and Adam slots) of an XE checkpoint, the step counter starting at 0; resume: a checkpoint of this driver,
    counters included."""
    from . import attention as A
    par = DataParallel(model.device if model is not None else None)
    if not par.chief:
        log = lambda *_: None
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(train_corpus.vocabulary)
    B = par.per_rank(cfg.batch_size)
    if model is None:
        model = A.Attention_Caption_Generator(cfg.dim_image, len(wordtoix), cfg.lstm_dim, B, cfg.n_video_lstm_step, cfg.n_caption_lstm_step, 0.9,
                                              bias_init_vector=None, m=m, beta=beta, seed=cfg.seed, device=par.device)
    par.attach(model)
    if restore:
        log(f"restored: {optimistic_restore(model, restore, step_names=('g_step',))}")
    if resume:
        log(f"resumed: {optimistic_restore(model, resume)} at step {model.global_step}")
    K = int(samples)
    on_device = reinforce and cfg.reward == "rouge"     # the reward is scored on the sampler's own tensors (reward.RougeL.score_ids_device)
    if reinforce:
        train_scorer, scorer, metric = reward_scorers(cfg, train_corpus.index.refs_by_video(),
                                                      test_corpus.index.refs_by_video() if test_corpus is not None else None, wordtoix, model.device)
    else:
        scorer = reward.CiderD(test_corpus.index.refs_by_video(), wordtoix) if test_corpus is not None else None
        train_scorer, metric = None, "ciderD"
    rng = random.Random(cfg.seed)
    caps = train_corpus.captions
    history = []
    steplog = StepLog(cfg.step_log if par.chief else None)

    def prepare(gidx):
        idx, lo = par.shard(gidx)
        vid = caps[idx, 0]
        if reinforce:
            out = dict(lo=lo, feats=model._dev(train_corpus.features.batch(vid), torch.float32),
                       rows=np.asarray([train_corpus.index.row[v] for v in vid], np.int32))
            if on_device:
                out["rows_dev"] = model._dev(out["rows"], torch.int32)
                out["rows_dev_k"] = out["rows_dev"].repeat(K)              # [K*B], sample-major like the ids
            return out
        g_ind, g_mask = hostglue.sentence_padding_toix(caps[gidx, 1].tolist(), wordtoix, cfg.n_caption_lstm_step)
        g_mask = np.asarray(g_mask, np.float32)
        return dict(lo=lo, ind=np.asarray(g_ind, np.int32)[lo:lo + len(idx)], mask=g_mask[lo:lo + len(idx)],
                    steps=model.active_steps(g_mask), feats=model._dev(train_corpus.features.batch(vid), torch.float32))

    for epoch in range(cfg.n_epochs):
        losses = []
        batches = (g for it, g in enumerate(epoch_batches(len(caps), cfg.batch_size, rng)) if not (cfg.max_steps_per_epoch and it >= cfg.max_steps_per_epoch))
        cur, pending, t0 = None, None, time.time()
        for it, (gidx, gnext) in enumerate(lookahead(batches)):
            if cur is None:
                cur = prepare(gidx)
            nxt = {}

            def overlap():          # while the GPU runs this step: the next batch, and the previous step's log lines
                if gnext is not None:
                    nxt.update(prepare(gnext))
                if pending is not None:
                    pending()
            b = cur
            rb = {}

            def rl_step():
                sampled, greedy = model.sample(b["feats"], K, True, seed=cfg.seed + 7919 * (model.global_step + 1), video_base=b["lo"],
                                               stop_at_eos=cfg.stop_at_eos)
                s_host, g_host = sampled.cpu().numpy(), greedy.cpu().numpy()

                def rewards():              # on the host while the GPU runs the teacher-forced forward
                    if on_device:           # two launches behind the forward; the baseline is tiled on the device
                        rb["r"] = train_scorer.score_ids_device(sampled, b["rows_dev_k"])
                        rb["b"] = train_scorer.score_ids_device(greedy, b["rows_dev"])
                        return rb["r"], rb["b"].repeat(K)
                    rb["r"] = train_scorer.score_ids(s_host, np.tile(b["rows"], K))      # [K*B], sample-major like the ids
                    rb["b"] = train_scorer.score_ids(g_host, b["rows"])                  # [B]
                    return rb["r"], hostglue.tile_baseline(rb["b"], K)
                # the ids are on the host anyway: behind the longest sample (its first <eos> included) every position is masked
                eos = s_host == 0
                steps = int(np.where(eos.any(1), eos.argmax(1) + 1, s_host.shape[1]).max())
                return model.reinforce_update(b["feats"], sampled, None, None, None, lr=learning_rate(cfg, model.global_step), clip_norm=cfg.clip_norm,
                                              video_base=b["lo"], reward_fn=rewards, active_steps=steps)
            if reinforce:
                st, loss = run_step(model, rl_step, log, overlap=overlap)
            else:
                st, loss = run_step(model, lambda: model.xe_update(b["feats"], b["ind"], b["mask"], lr=learning_rate(cfg, model.global_step),
                                                                   clip_norm=cfg.clip_norm, video_base=b["lo"], active_steps=b["steps"]),
                                    log, overlap=overlap)
            losses.append(loss)
            t1 = time.time()
            rm, bm = (float(rb["r"].mean()), float(rb["b"].mean())) if reinforce and not on_device else (None, None)

            def pending(it=it, loss=loss, lr=learning_rate(cfg, model.global_step), step=model.global_step, secs=t1 - t0, rm=rm, bm=bm, rb=rb):
                if on_device:               # device-resident rewards: their means are read when the log line is written, not in the step
                    rm, bm = float(rb["r"].mean()), float(rb["b"].mean())
                if reinforce:
                    log(f"idx: {it * cfg.batch_size} rate: {lr:g} Epoch: {epoch} loss: {loss:.5f} r: {rm:.4f} b: {bm:.4f} Elapsed time: {secs:.3f}")
                    steplog.write(kind="step", epoch=epoch, step=step, lr=lr, loss=loss, reward=rm, baseline=bm, seconds=secs)
                    return
                log(f"idx: {it * cfg.batch_size} rate: {lr:g} Epoch: {epoch} loss: {loss:.5f} Elapsed time: {secs:.3f}")
                steplog.write(kind="step", epoch=epoch, step=step, lr=lr, loss=loss, seconds=secs)
            t0, cur = t1, (nxt if gnext is not None else None)
        if pending is not None:
            pending()
        entry = {"epoch": epoch, "loss": float(np.mean(losses)) if losses else None}
        if test_corpus is not None:
            if eval_beam > 0:
                _, entry[metric] =beam_eval(model, test_corpus, ixtoword, scorer, B, eval_beam, eval_lnf, par)
            else:
                _, entry[metric] =greedy_eval(model, test_corpus, ixtoword, scorer, B, par)
        ck = save_checkpoint_checked(model, cfg, epoch, step_name="g_step" if reinforce else "Variable", chief=par.chief)
        if par.chief:
            entry["checkpoint"] = ck
        history.append(entry)
        steplog.write(kind="epoch", **entry)
        log(f"Epoch {epoch} is done: {entry}")
    steplog.close()
    return model, history


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-sents", required=True); ap.add_argument("--train-feats", required=True)
    ap.add_argument("--test-sents"); ap.add_argument("--test-feats")
    ap.add_argument("--vocab", required=True); ap.add_argument("--resume")
    ap.add_argument("--epochs", type=int, default=20); ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--frames", type=int, default=5, help="n_video_lstm_steps (the feature file's frames per video; up to 64)")
    ap.add_argument("--model-path", default="./attention_models")
    ap.add_argument("--eval-beam", type=int, default=0, help="per-epoch evaluation with a beam of this size (1..16) instead of greedy decoding")
    ap.add_argument("--eval-lnf", type=float, default=0.0, help="length normalisation factor of the evaluation beam search")
    ap.add_argument("--reinforce", action="store_true", help="the self-critical REINFORCE stage (CIDEr-D reward) instead of cross entropy")
    ap.add_argument("--samples", type=int, default=5, help="multinomial samples per video and step of --reinforce (K)")
    ap.add_argument("--restore", help="--reinforce: the XE checkpoint to start from (variables and Adam slots; the step counter starts at 0)")
    ap.add_argument("--stop-at-eos", action="store_true", help="samples leave the decode loop at their first <eos> (same update, shorter sampler loop)")
    ap.add_argument("--reward", choices=reward.REWARDS, default="cider", help="--reinforce: CIDEr-D on the host (default) or ROUGE-L scored on the device")
    a = ap.parse_args(argv)
    if a.reward != "cider" and not a.reinforce:
        ap.error("--reward belongs to --reinforce")
    make =reinforce_config if a.reinforce else attention_config
    cfg = make(n_epochs=a.epochs, batch_size=a.batch_size, model_path=a.model_path, n_video_lstm_step=a.frames, stop_at_eos=a.stop_at_eos, reward=a.reward,
               model_name=f"batch_size{a.batch_size}_beta10_m05_{a.frames}img_attention_{'reinforce_' if a.reinforce else ''}model")
    tr = Corpus(a.train_sents, a.train_feats, vocabulary_file=a.vocab)
    te = Corpus(a.test_sents, a.test_feats, vocabulary=tr.vocabulary) if a.test_sents and a.test_feats else None
    train(cfg, tr, te, resume=a.resume, eval_beam=a.eval_beam, eval_lnf=a.eval_lnf, reinforce=a.reinforce, samples=a.samples, restore=a.restore)


if __name__ == "__main__":
    main()
