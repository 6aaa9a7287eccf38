"""Cross-entropy training driver: the counterpart of train() in tf_s2vt.py:404-560 on the HIP path.

    python -m s2vt_amd.train_xe --train-sents S --train-feats F --test-sents S2 --test-feats F2 --vocab V

Per step the reference runs sess.run([train_op, tf_loss]) on build_model (label-smoothed XE with the Q1
batch-mean rule, weight decay, clip 10, Adam, lr 1e-3 halved every 5000 steps); here that is
Video_Caption_Generator.xe_update.  One process per GPU under torch.distributed.run for data parallel.

--bidirectional trains the bidirectional captioner of bidirection_tf_s2vt.py by that script's rule (train_bidirectional: SGD, clip_by_norm 10 per
variable, lr 0.01 halved every 10000 steps).

--scheduled-sampling P trains as generate_words_tf_s2vt.py does instead (Video_Caption_Generator.scheduled_update): the unroll decodes and
a per-row coin feeds the ground-truth word with probability P / 1.00001 (the script writes P = 0.5), or, with --ss-k K, with the inverse
sigmoid schedule K / (K + exp(step / K)) of its commented line :134; --optimizer sgd is that script's GradientDescentOptimizer.

--averaged-embedding trains as average_generate_words_tf_s2vt.py does (Video_Caption_Generator.averaged_update): the unroll decodes and
LSTM2 is fed the mean of the ground-truth word's and the model's own argmax's embedding, with that script's rule -- SGD behind
tf.clip_by_norm 10 per variable, loss_weight 20, lr halved every 40000 steps -- unless --optimizer adam is given (Adam behind the global clip).

--topk-feed [--topk-k 5] trains as sum_generate_words_tf_s2vt.py does (Video_Caption_Generator.topk_feed_update): the unroll decodes and
LSTM2 is fed the weighted sum of the embeddings of the model's own top-k words, the weights those k logits over their sum and
differentiated; the same update rule with lr halved every 20000 steps.  The per-epoch evaluation decodes with that script's generator."""
from __future__ import annotations

import argparse
import random
import time

import numpy as np
import torch

from . import hostglue, reward
from .train_common import (Config, Corpus, DataParallel, StepLog, epoch_batches, greedy_eval, learning_rate, lookahead, optimistic_restore,
                           run_step, save_checkpoint, save_checkpoint_checked)


def train(cfg: Config, train_corpus: Corpus, test_corpus: Corpus | None = None, model=None, log=print, resume=None,
          grad_precision=None, scheduled_sampling=None, ss_k=None, optimizer="adam", averaged_embedding=False, topk_feed=None):
    """topk_feed: k -- topk_feed_update with that many words in the mix instead of xe_update, under averaged_embedding's optimizer rules and
    loss_weight; the epoch's evaluation then decodes with generate_topk_feed(k).
    averaged_embedding: averaged_update instead of xe_update (optimizer "sgd": behind the per-variable clip, the script's train();
    "adam": behind the global clip); a model built here then takes the script's loss_weight = 20.
    scheduled_sampling: None = cross entropy; a probability = scheduled sampling with that true-word probability (ss_k: the inverse
    sigmoid schedule on the step counter instead).  Its mask comes from the model's own picks, so a batch in which every row emits <eos>
    at step 0 has sum(mask) = 0 and a 0/0 loss, as in the reference: the run stops there, before another checkpoint is written.
    cfg.batch_size is the GLOBAL batch; data parallel as in train_rl.train (shards of each shuffled batch, Q1's per-step
    mask sums and the gradient bucket all-reduced inside xe_update, rank 0 logs and saves)."""
    from . import model as M
    par = DataParallel(model.device if model is not None else None)
    if not par.chief:
        log = lambda *_: None
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(train_corpus.vocabulary)
    B = par.per_rank(cfg.batch_size)
    if model is None:
        model = M.Video_Caption_Generator(cfg.dim_image, len(wordtoix), cfg.word_dim, cfg.lstm_dim, B,
                                          cfg.n_video_lstm_step + cfg.n_caption_lstm_step, cfg.n_video_lstm_step,
                                          cfg.n_caption_lstm_step, bias_init_vector=None, seed=cfg.seed, device=par.device,
                                          residual=cfg.residual, **({"loss_weight": 20} if averaged_embedding or topk_feed is not None else {}))
    if topk_feed is not None and (averaged_embedding or scheduled_sampling is not None or getattr(model, "residual", False)):
        raise ValueError("top-k feed training does not combine with averaged embeddings, scheduled sampling or a residual model")
    if scheduled_sampling is not None and getattr(model, "residual", False):
        raise ValueError("scheduled sampling is not implemented for a residual model (residual=True / --residual)")
    if averaged_embedding and (scheduled_sampling is not None or getattr(model, "residual", False)):
        raise ValueError("averaged-embedding training does not combine with scheduled sampling or a residual model")
    if grad_precision is not None:
        model.grad_precision = grad_precision          # (None: the model's default, S2VT_GRAD_PRECISION)
    par.attach(model)
    if resume:
        log(f"resumed: {optimistic_restore(model, resume)} at step {model.global_step}")
    scorer = reward.CiderD(test_corpus.index.refs_by_video(), wordtoix) if test_corpus is not None else None
    rng = random.Random(cfg.seed)
    caps = train_corpus.captions
    history = []
    steplog = StepLog(cfg.step_log if par.chief else None)
    def prepare(gidx):
        """Host side of one step: this rank's shard of the batch, padded captions, features staged for the copy to the GPU."""
        idx, lo = par.shard(gidx)
        vid = caps[idx, 0]
        # the GLOBAL batch is padded (64 short strings) so that every rank knows its longest caption: the steps behind
        # it are all padding on every rank and are not unrolled (Q1's batch mean couples the ranks at a live step)
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
            if topk_feed is not None:
                update = lambda: model.topk_feed_update(b["feats"], b["ind"], b["mask"], k=topk_feed, lr=learning_rate(cfg, model.global_step),
                                                        clip_norm=cfg.clip_norm, clip="per_variable" if optimizer == "sgd" else "global",
                                                        optimizer=optimizer, video_base=b["lo"])
            elif averaged_embedding:
                update = lambda: model.averaged_update(b["feats"], b["ind"], b["mask"], lr=learning_rate(cfg, model.global_step),
                                                       clip_norm=cfg.clip_norm, clip="per_variable" if optimizer == "sgd" else "global",
                                                       optimizer=optimizer, video_base=b["lo"])
            elif scheduled_sampling is None:
                update = lambda: model.xe_update(b["feats"], b["ind"], b["mask"], lr=learning_rate(cfg, model.global_step),
                                                 clip_norm=cfg.clip_norm, video_base=b["lo"], active_steps=b["steps"])
            else:
                prob = scheduled_sampling if ss_k is None else model.inverse_sigmoid_prob(ss_k, model.global_step)
                update = lambda: model.scheduled_update(b["feats"], b["ind"], lr=learning_rate(cfg, model.global_step), true_word_prob=prob,
                                                        clip_norm=cfg.clip_norm, optimizer=optimizer, video_base=b["lo"])
            st, loss = run_step(model, update, log, overlap=overlap)
            if scheduled_sampling is not None and not np.isfinite(loss):
                raise FloatingPointError(f"scheduled sampling, step {model.global_step}: the loss is {loss} -- the mask is empty (every row "
                                         "emitted <eos> at step 0, sum(mask) = 0) or the update diverged; the variables are not usable "
                                         "from here on and no further checkpoint is written")
            losses.append(loss)
            t1 = time.time()

            def pending(it=it, loss=loss, lr=learning_rate(cfg, model.global_step), step=model.global_step, secs=t1 - t0):
                log(f"idx: {it * cfg.batch_size} rate: {lr:g} Epoch: {epoch} loss: {loss:.5f} Elapsed time: {secs:.3f}")
                steplog.write(kind="step", epoch=epoch, step=step, lr=lr, loss=loss, seconds=secs)
            t0, cur = t1, (nxt if gnext is not None else None)
        if pending is not None:
            pending()
        entry = {"epoch": epoch, "loss": float(np.mean(losses)) if losses else None}
        if test_corpus is not None:
            decode = (lambda f: model.generate_topk_feed(f, k=topk_feed)) if topk_feed is not None else None
            _, entry["ciderD"] = greedy_eval(model, test_corpus, ixtoword, scorer, B, par, decode=decode)
        ck = save_checkpoint_checked(model, cfg, epoch, step_name="Variable", chief=par.chief, tf_version=1)   # the XE script's saver writes V1 (tf_s2vt.py:440)      # tf_s2vt.py:441: the unnamed counter
        if par.chief:
            entry["checkpoint"] = ck
        history.append(entry)
        steplog.write(kind="epoch", residual=bool(cfg.residual), **entry)
        log(f"Epoch {epoch} is done: {entry}")
    steplog.close()
    return model, history


def train_bidirectional(cfg: Config, train_corpus: Corpus, model=None, log=print, resume=None):
    """train() of bidirection_tf_s2vt.py (:336-428) on the bidirectional captioner (bidirection.Video_Caption_Generator): per step
    sess.run([train_op, tf_loss]) there is xe_update here -- plain softmax cross-entropy x mask x loss_weight (20) / sum(mask) + weight decay,
    GradientDescentOptimizer behind tf.clip_by_norm(grad, cfg.clip_norm) PER VARIABLE, lr = cfg.start_learning_rate * 0.5^(step // cfg.decay_steps)
    (the script: 0.01, 10000) -- and a version-1 checkpoint `<model_name>-<epoch>` under the TF names per epoch.  One process, one GPU (the
    script is; data parallel is not built for this model).  Returns (model, history)."""
    import os
    from . import bidirection
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("--bidirectional trains in one process: data parallel is not built for the bidirectional captioner")
    wordtoix, ixtoword = hostglue.preProBuildWordVocab(train_corpus.vocabulary)
    B = cfg.batch_size
    if model is None:
        model = bidirection.Video_Caption_Generator(cfg.dim_image, len(wordtoix), cfg.word_dim, cfg.lstm_dim, B, cfg.n_video_lstm_step + cfg.n_caption_lstm_step,
                                                    cfg.n_video_lstm_step, cfg.n_caption_lstm_step, bias_init_vector=None, seed=cfg.seed)
    if resume:
        model.restore(resume)
        log(f"resumed: {resume} at step {model.global_step}")
    model.global_step = getattr(model, "global_step", 0)
    rng = random.Random(cfg.seed)
    caps = train_corpus.captions
    history = []
    steplog = StepLog(cfg.step_log)
    dev = model.device
    for epoch in range(cfg.n_epochs):
        losses = []
        for it, idx in enumerate(epoch_batches(len(caps), B, rng)):
            if cfg.max_steps_per_epoch and it >= cfg.max_steps_per_epoch:
                break
            t0 = time.time()
            ind, mask = hostglue.sentence_padding_toix(caps[idx, 1].tolist(), wordtoix, cfg.n_caption_lstm_step)
            feats = torch.as_tensor(np.asarray(train_corpus.features.batch(caps[idx, 0], pinned=False), np.float32)).to(dev)
            lr = learning_rate(cfg, model.global_step)
            step = model.global_step
            loss = model.xe_update(feats, torch.as_tensor(np.asarray(ind, np.int32)).to(dev), torch.as_tensor(np.asarray(mask, np.float32)).to(dev),
                                   lr=lr, clip_norm=cfg.clip_norm, seed=cfg.seed + 104729 * step)
            if not np.isfinite(loss):
                raise FloatingPointError(f"bidirectional captioner, step {step}: the loss is {loss}")
            losses.append(loss)
            secs = time.time() - t0
            log(f"idx: {it * B} rate: {lr:g} Epoch: {epoch} loss: {loss:.5f} Elapsed time: {secs:.3f}")
            steplog.write(kind="step", epoch=epoch, step=step + 1, lr=lr, loss=loss, seconds=secs)
        os.makedirs(cfg.model_path, exist_ok=True)
        ck = os.path.join(cfg.model_path, f"{cfg.model_name}-{epoch}")
        model.save(ck, tf_version=1)                                  # :368, :426: Saver(write_version=1), global_step = epoch
        entry = {"epoch": epoch, "loss": float(np.mean(losses)) if losses else None, "checkpoint": ck}
        history.append(entry)
        steplog.write(kind="epoch", bidirectional=True, **entry)
        log(f"Epoch {epoch} is done: {entry}")
    steplog.close()
    return model, history


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-sents", required=True); ap.add_argument("--train-feats", required=True)
    ap.add_argument("--test-sents"); ap.add_argument("--test-feats")
    ap.add_argument("--vocab", required=True); ap.add_argument("--resume")
    ap.add_argument("--epochs", type=int, default=30); ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--model-path", default="./new_s2vt_models")
    ap.add_argument("--grad-precision", choices=("fp32", "bf16"), help="the backward's gradient contractions on bf16 operands (non-parity "
                    "fast mode, DESIGN.md §3); default: S2VT_GRAD_PRECISION, else fp32")
    ap.add_argument("--scheduled-sampling", type=float, metavar="P", help="scheduled-sampling training (generate_words_tf_s2vt.py): feed the "
                    "ground-truth word with probability P / 1.00001, the model's own argmax otherwise (the script writes 0.5)")
    ap.add_argument("--ss-k", type=float, metavar="K", help="with scheduled sampling: P = K / (K + exp(step / K)) (the script's k_value = 5000)")
    ap.add_argument("--residual", action="store_true", help="the residual captioner of residual_tf_s2vt.py: out1 + out2 into the vocabulary projection")
    ap.add_argument("--bidirectional", action="store_true", help="the bidirectional captioner of bidirection_tf_s2vt.py with its own training rule: "
                    "plain SGD, tf.clip_by_norm 10 per variable, lr 0.01 halved every 10000 steps, loss_weight 20, batch 32, d = 1024, Tv = 25 "
                    "(train_bidirectional)")
    ap.add_argument("--averaged-embedding", action="store_true", help="averaged-embedding training (average_generate_words_tf_s2vt.py): feed the "
                    "mean of the ground-truth word's and the model's own argmax's embedding; SGD behind tf.clip_by_norm 10 per variable, loss_weight "
                    "20, lr halved every 40000 steps, unless --optimizer adam")
    ap.add_argument("--topk-feed", action="store_true", help="top-k score-weighted embedding training (sum_generate_words_tf_s2vt.py): feed the "
                    "weighted sum of the embeddings of the model's own top-k words; SGD behind tf.clip_by_norm 10 per variable, loss_weight 20, lr "
                    "halved every 20000 steps, unless --optimizer adam")
    ap.add_argument("--topk-k", type=int, default=5, metavar="K", help="with --topk-feed: the number of words in the mix, 1..8 (the script's 5)")
    ap.add_argument("--optimizer", choices=("adam", "sgd"), help="sgd: the scheduled-sampling script's GradientDescentOptimizer; default adam, "
                    "with --averaged-embedding / --topk-feed sgd")
    a = ap.parse_args(argv)
    if a.topk_feed and (a.averaged_embedding or a.scheduled_sampling is not None or a.ss_k is not None or a.bidirectional or a.residual):
        ap.error("--topk-feed does not combine with --averaged-embedding, --scheduled-sampling, --ss-k, --bidirectional or --residual")
    if a.topk_feed and not 1 <= a.topk_k <= 8:
        ap.error("--topk-k must lie in 1..8")
    if a.topk_feed and a.grad_precision == "bf16":
        ap.error("--topk-feed has the fp32 gradient products only")
    if a.averaged_embedding and (a.scheduled_sampling is not None or a.ss_k is not None or a.bidirectional or a.residual):
        ap.error("--averaged-embedding does not combine with --scheduled-sampling, --ss-k, --bidirectional or --residual")
    if a.optimizer is None:
        a.optimizer = "sgd" if a.averaged_embedding or a.topk_feed else "adam"
    if a.ss_k is not None and a.scheduled_sampling is None:
        a.scheduled_sampling = 0.5
    if a.bidirectional:
        if a.scheduled_sampling is not None or a.residual or a.grad_precision or a.optimizer != "adam":
            ap.error("--bidirectional has one training rule (the script's); it does not combine with --scheduled-sampling, --residual, --grad-precision or --optimizer")
        # the script's "Train Parameters" (bidirection_tf_s2vt.py:233-252)
        cfg = Config(dim_image=1024, n_video_lstm_step=25, n_caption_lstm_step=35, n_epochs=a.epochs, batch_size=a.batch_size, start_learning_rate=0.01,
                     decay_steps=10000, clip_norm=10.0, model_path=a.model_path, model_name="bimodel")
        train_bidirectional(cfg, Corpus(a.train_sents, a.train_feats, vocabulary_file=a.vocab), resume=a.resume)
        return
    if a.optimizer != "adam" and a.scheduled_sampling is None and not a.averaged_embedding and not a.topk_feed:
        ap.error("--optimizer sgd is wired for --scheduled-sampling, --averaged-embedding and --topk-feed only")
    cfg = Config(n_epochs=a.epochs, batch_size=a.batch_size, model_path=a.model_path, model_name=f"batch_size{a.batch_size}_s2vt_model",
                 residual=a.residual, **({"decay_steps": 40000} if a.averaged_embedding else {"decay_steps": 20000} if a.topk_feed else {}))
    # (average_generate_words_tf_s2vt.py:366-367: 40000; sum_generate_words_tf_s2vt.py:429-431: 20000)
    tr = Corpus(a.train_sents, a.train_feats, vocabulary_file=a.vocab)
    te = Corpus(a.test_sents, a.test_feats, vocabulary=tr.vocabulary) if a.test_sents and a.test_feats else None
    train(cfg, tr, te, resume=a.resume, grad_precision=a.grad_precision, scheduled_sampling=a.scheduled_sampling, ss_k=a.ss_k,
          optimizer=a.optimizer, averaged_embedding=a.averaged_embedding, topk_feed=a.topk_k if a.topk_feed else None)


if __name__ == "__main__":
    main()
