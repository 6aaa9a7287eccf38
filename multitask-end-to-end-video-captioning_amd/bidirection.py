"""The bidirectional S2VT captioner of bidirection_tf_s2vt.py:48-216, forward side: LSTM1 is a static_bidirectional_rnn over the Tv
frames and then the Tc zero paddings, LSTM2 reads [fw ; bw ; embed ; h2] (kernel [(2H + E) + H, 4H]), no word ever enters LSTM1.

What is here: the variables and their initialisers, the teacher-forced logits of build_model (:85-165), build_generator (:167-216,
B = 1, unshifted softmax then argmax; the `break` at :214 never fires on a graph) and a batched greedy sampler with the same
arithmetic per row.  The model runs in the library (csrc/bidir.hip: s2vt_bidir_teacher_forced_fwd / s2vt_bidir_bptt_bwd /
s2vt_bidir_decode_greedy on a caller-owned workspace); this class owns the variables and the script's surface.  What the drivers do:
  1. frame embedding (s2vt_gemm), its products with the input rows of both LSTM1 kernels (time-major rows through rowidx);
  2. both LSTM1 recurrences in one call (s2vt_lstm_birecurrence_fwd: one persistent launch at <= 64 rows) -- the backward direction's
     history stays in chain-step order (slot k + 1 = the state after time T-1-k) and every consumer reads it through rowidx;
  3. [fw ; bw (; embed)] @ W2[:2H (+ E)] hoisted for all T steps; LSTM2 continues each chain from it (same bits);
  4. the vocabulary projection and the pick.
Training: build_model's loss (:150-165; plain softmax cross-entropy x mask x loss_weight / sum(mask) + 5e-5 l2 on the variables without
'bias' in their name) and its gradients from the library's order-free pieces -- s2vt_gemm_tn / s2vt_gemm_nt with the same rowidx for
the backward direction, one s2vt_lstm_recurrence_bwd per cell -- then tf.clip_by_norm(grad, 10) PER VARIABLE (each variable its own
squared-norm slot of s2vt_grad_finalize / s2vt_sgd_guarded) and plain gradient descent (:369-375).  Wemb's gradient is dense (TF 1.1's
clip_by_norm converts the IndexedSlices; recalled, TF is not vendored).  Anything the script has no graph for raises ValueError."""
from __future__ import annotations

import numpy as np
import torch

from . import ops, tfckpt

VARIABLES = ("Wemb", "encode_image_W", "encode_image_b", "lstm1_fw_W", "lstm1_fw_b", "lstm1_bw_W", "lstm1_bw_b", "lstm2_W", "lstm2_b",
             "embed_word_W", "embed_word_b")
TF_NAMES = tfckpt.BIDIRECTION_TF_NAMES      # variable -> TF 1.1 checkpoint name (the table and its caveat: tfckpt.py)
assert tuple(TF_NAMES) == VARIABLES
LSTM2_DROP_CODE0 = 2 * 256          # the DropoutWrapper stream of LSTM2 (layer * 256 + step), as in the plain captioner


def param_shapes(dim_image, n_words, word_dim, lstm_dim):
    D, V, E, H = dim_image, n_words, word_dim, lstm_dim
    return {"Wemb": (V, E), "encode_image_W": (D, E), "encode_image_b": (E,), "lstm1_fw_W": (E + H, 4 * H), "lstm1_fw_b": (4 * H,),
            "lstm1_bw_W": (E + H, 4 * H), "lstm1_bw_b": (4 * H,), "lstm2_W": (2 * H + E + H, 4 * H), "lstm2_b": (4 * H,),
            "embed_word_W": (H, V), "embed_word_b": (V,)}


def init_reference(shapes, seed):
    """bidirection_tf_s2vt.py:64-83 and TF's defaults: U(-0.1, 0.1), Glorot-uniform for the three BasicLSTMCell kernels, zero biases."""
    rng = np.random.default_rng(seed)
    p = {}
    for n in VARIABLES:
        s = shapes[n]
        if len(s) == 1:
            p[n] = np.zeros(s, np.float32)
        else:
            a = float(np.sqrt(6.0 / (s[0] + s[1]))) if n.startswith("lstm") else 0.1
            p[n] = rng.uniform(-a, a, s).astype(np.float32)
    return p


def _no_graph(what):
    raise ValueError(f"bidirection_tf_s2vt.py has no graph for {what}")


class Video_Caption_Generator:
    """The script's constructor (bidirection_tf_s2vt.py:49-50).  params: name -> array for every name in VARIABLES (default: the
    reference initialisers from `seed`)."""

    def __init__(self, dim_image, n_words, word_dim, lstm_dim, batch_size, n_lstm_steps, n_video_lstm_step, n_caption_lstm_step,
                 bias_init_vector=None, loss_weight=20, decay_value=0.00005, dropout_rate=0.9, seed=0, params=None, device="cuda"):
        self.dim_image, self.n_words, self.word_dim, self.lstm_dim = dim_image, n_words, word_dim, lstm_dim
        self.batch_size, self.n_lstm_steps = batch_size, n_lstm_steps
        self.n_video_lstm_step, self.n_caption_lstm_step = n_video_lstm_step, n_caption_lstm_step
        self.loss_weight, self.decay_value, self.dropout_rate = loss_weight, decay_value, dropout_rate
        shapes = param_shapes(dim_image, n_words, word_dim, lstm_dim)
        if params is None:
            params = init_reference(shapes, seed)
            if bias_init_vector is not None:
                params["embed_word_b"] = np.asarray(bias_init_vector, np.float32)
        self.p = {}
        for n in VARIABLES:
            t = torch.as_tensor(np.ascontiguousarray(params[n], np.float32)).to(device)
            assert tuple(t.shape) == shapes[n], (n, tuple(t.shape), shapes[n])
            self.p[n] = t
        self.device = device

    # ---- checkpoints in TF's formats and names (tfckpt.py); the script's Saver writes version 1 (:368)
    def save(self, path, tf_version=1):
        from . import tfckpt
        sd = {TF_NAMES[n]: self.p[n].detach().cpu().numpy() for n in VARIABLES}
        sd["Variable"] = np.asarray(getattr(self, "global_step", 0), np.int32)          # train()'s unnamed global_step (:369)
        (tfckpt.write_checkpoint_v1 if tf_version == 1 else tfckpt.write_checkpoint_v2)(path, sd)

    def restore(self, path):
        from . import tfckpt
        sd = tfckpt.read_checkpoint(path)
        for n in VARIABLES:
            a = np.asarray(sd[TF_NAMES[n]], np.float32)
            assert a.shape == tuple(self.p[n].shape), (n, a.shape)
            self.p[n].copy_(torch.as_tensor(a))
        if "Variable" in sd:
            self.global_step = int(sd["Variable"])

    # ---- the library's drivers (csrc/bidir.hip: s2vt_bidir_*), one workspace per batch size
    def _dims(self):
        return ops.make_dims(self.dim_image, self.n_words, self.word_dim, self.lstm_dim, self.n_video_lstm_step, self.n_caption_lstm_step)

    def _params(self):
        if getattr(self, "_cparams", None) is None:
            self._cparams = ops.make_bidir_params(self.p)
        return self._cparams

    def _workspace(self, B, dev):
        ws = getattr(self, "_ws", {})
        if B not in ws:
            ws[B] = ops.bidir_workspace(self._dims(), B, dev)
        self._ws = ws
        return ws[B]

    def teacher_forced_logits(self, video, caption, keep=None, seed=0, video_id=None, sample_id=None, persistent=-1):
        """build_model's logits (:113-156), time-major [Tc * B, V]: row t * B + b (s2vt_bidir_teacher_forced_fwd).  keep: LSTM2's
        DropoutWrapper (default: the constructor's dropout_rate); the noise is the library's Philox stream keyed by (seed, video id, sample
        id, LSTM2's codes).  persistent: the form of the LSTM1 call (s2vt_lstm_birecurrence_fwd)."""
        dev = video.device
        B = video.shape[0]
        keep = float(self.dropout_rate if keep is None else keep)
        if keep < 1.0 and video_id is None:
            video_id, sample_id = torch.arange(B, device=dev, dtype=torch.int32), torch.zeros(B, device=dev, dtype=torch.int32)
        self._noise = (keep, seed, video_id, sample_id)
        return ops.bidir_teacher_forced_fwd(self._dims(), self._params(), video.contiguous(), caption.to(torch.int32).contiguous(), self._workspace(B, dev),
                                            keep, seed, video_id, sample_id, persistent)

    def build_sampler(self, video, unshifted_softmax=False, video_base=0, want_logits=False, persistent=-1):
        """Batched greedy decode, build_generator's arithmetic per row (s2vt_bidir_decode_greedy): ids int32 [B, Tc] (and the logits
        [B, Tc, V]).  unshifted_softmax: pick argmax(exp(l) / sum(exp(l))) as :211-212 write it instead of argmax(l)."""
        return ops.bidir_decode_greedy(self._dims(), self._params(), video.contiguous(), unshifted_softmax, video_base, want_logits, persistent)

    def build_generator(self, video=None):
        """bidirection_tf_s2vt.py:167-216 for one video [1, Tv, D]: (video, sentence [Tc] int32, probs = [] as the script leaves it).
        Without a video: the script's call (:448) -- placeholders for Session.run."""
        if video is None:
            return _Node("gen_video"), _Node("sentence"), []
        assert video.shape[0] == 1
        return video, self.build_sampler(video, unshifted_softmax=True)[0], []

    # ---- build_model's loss and tf.gradients (:150-165), the per-variable clip and the SGD step of train() (:369-375)
    def decayed(self, name):
        """quirk Q3: weight decay on every variable without 'bias' in its TF name -- all but the three BasicLSTMCell biases"""
        return name not in ("lstm1_fw_b", "lstm1_bw_b", "lstm2_b")

    def l2_term(self):
        return float(sum((self.p[n].double() ** 2).sum() for n in VARIABLES if self.decayed(n))) * 0.5 * self.decay_value

    def loss_and_grads(self, video, caption, mask, keep=None, seed=0, video_id=None, sample_id=None, persistent=-1):
        """(loss as a host float, {name: d loss / d variable} fp32, before any clip).  loss = loss_weight * sum(xent * mask) / sum(mask) +
        decay_value * sum l2_loss(decayed variables); Wemb's gradient is dense.  The per-variable squared norms are left in self._sumsq."""
        p, dev = self.p, video.device
        B = video.shape[0]
        video = video.contiguous()
        caption = caption.to(torch.int32).contiguous()
        logits = self.teacher_forced_logits(video, caption, keep, seed, video_id, sample_id, persistent)
        if getattr(self, "_want_probs", False):
            self._probs = logits.clone()
        keep, seed, video_id, sample_id = self._noise
        coef, target, msum = ops.xe_prep(mask.contiguous(), caption, self.loss_weight, B, False)
        nll, _ = ops.softmax_nll_fwd_bwd(logits, target, coef, 0.0)         # logits <- coef * (softmax - onehot)
        loss_t, gscale = torch.empty(1, device=dev), torch.empty(1, device=dev)
        ops.step_scalars(coef, nll, msum, msum, loss=loss_t, gscale=gscale)
        g = {n: torch.zeros_like(p[n]) for n in VARIABLES}
        ops.bidir_bptt_bwd(self._dims(), self._params(), ops.make_bidir_params(g), video, logits, self._workspace(B, dev), keep, seed, video_id, sample_id)
        # 1 / sum(mask) and the weight decay, one squared norm per variable
        self._sumsq = torch.zeros(len(VARIABLES), device=dev)
        for i, n in enumerate(VARIABLES):
            ops.grad_finalize(g[n].view(-1), p[n].view(-1), gscale, self.decay_value if self.decayed(n) else 0.0, self._sumsq[i:i + 1])
        return float(loss_t) + self.l2_term(), g

    def xe_update(self, video, caption, mask, lr=None, clip_norm=10.0, step=None, **kw):
        """One step of train() (:369-375): GradientDescentOptimizer on tf.clip_by_norm(grad, clip_norm) PER VARIABLE, lr = 0.01 * 0.5^(step // 10000)
        unless given.  Returns the loss before the update."""
        self.global_step = getattr(self, "global_step", 0) if step is None else int(step)
        lr = 0.01 * 0.5 ** (self.global_step // 10000) if lr is None else lr
        loss, g = self.loss_and_grads(video, caption, mask, **kw)
        self.apply_clipped(g, lr, clip_norm)
        self.global_step += 1
        return loss

    def apply_clipped(self, g, lr, clip_norm=10.0, sumsq=None):
        sumsq = self._sumsq if sumsq is None else sumsq
        for i, n in enumerate(VARIABLES):
            ops.sgd(self.p[n].view(-1), g[n].view(-1), sumsq[i:i + 1], clip_norm, lr, self.global_step + 1 if hasattr(self, "global_step") else 1)

    def minimize(self, *args, optimizer="sgd", clip="per_variable", learning_rate=None, clip_norm=10.0, **kw):
        """minimize(video, caption, mask): one step now.  minimize(tf_loss [, learning_rate]) with build_model()'s loss (or its whole tuple): the
        script's train_op (:372-375) for Session.run.  Only the script's optimizer exists: plain SGD behind the per-variable clip."""
        if optimizer != "sgd" or clip != "per_variable":
            _no_graph(f"optimizer={optimizer!r}, clip={clip!r}")
        if args and isinstance(args[0], (_Node, tuple)):
            if len(args) > 1:
                learning_rate = args[1]
            self._train = (learning_rate, float(clip_norm))
            return _Node("train_op")
        return self.xe_update(*args, clip_norm=clip_norm, **kw)

    # ---- the script's graph surface: build_model's 5-tuple (:165), exponential_decay (:370), Session.run
    def build_model(self):
        return _Node("loss"), _Node("video"), _Node("caption"), _Node("caption_mask"), [_Node("probs", i) for i in range(self.n_caption_lstm_step)]

    def exponential_decay(self, start_learning_rate, decay_steps=10000, decay_rate=0.5):
        """tf.train.exponential_decay(start, global_step, decay_steps, decay_rate, staircase=True)"""
        self._lr = (float(start_learning_rate), int(decay_steps), float(decay_rate))
        return _Node("learning_rate")

    def learning_rate(self):
        start, steps, rate = getattr(self, "_lr", (0.01, 10000, 0.5))
        return start * rate ** (getattr(self, "global_step", 0) // steps)


    def sample(self, *a, **k):
        _no_graph("multinomial sampling")

    def reinforce_update(self, *a, **k):
        _no_graph("REINFORCE")

    def build_mix_sample(self, *a, **k):
        _no_graph("build_mix_sample")

    def scheduled_update(self, *a, **k):
        _no_graph("scheduled sampling")

    def beam_search(self, *a, **k):
        _no_graph("beam search")


class _Node:
    """what build_model / build_generator hand out in place of TF tensors: a key for Session.run's fetches and feed_dict"""

    def __init__(self, kind, index=None):
        self.kind, self.index = kind, index


class Session:
    """sess.run(fetches, feed_dict) over the nodes above: a train_op among the fetches runs one xe_update (dropout noise keyed by the step
    count); loss / probs alone run the same pass and apply nothing; `sentence` runs build_generator."""

    def __init__(self, model, dropout_seed=0):
        self.model, self.dropout_seed = model, dropout_seed

    def run(self, fetches, feed_dict=None):
        m = self.model
        single = isinstance(fetches, _Node)
        fl = [fetches] if single else list(fetches)
        feed = {k.kind: v for k, v in (feed_dict or {}).items()}
        dev = m.device
        out = {}
        kinds = {f.kind for f in fl}
        if "sentence" in kinds:
            video = torch.as_tensor(np.asarray(feed["gen_video"], np.float32)).to(dev)
            out["sentence"] = m.build_generator(video)[1].cpu().numpy().astype(np.int64)
        if kinds & {"loss", "probs", "train_op"}:
            video = torch.as_tensor(np.asarray(feed["video"], np.float32)).to(dev)
            caption = torch.as_tensor(np.asarray(feed["caption"], np.int32)).to(dev)
            mask = torch.as_tensor(np.asarray(feed["caption_mask"], np.float32)).to(dev)
            step = getattr(m, "global_step", 0)
            m.global_step = step
            m._want_probs = "probs" in kinds
            loss, g = m.loss_and_grads(video, caption, mask, seed=self.dropout_seed + 104729 * step)
            m._want_probs = False
            out["loss"] = np.float32(loss)
            if "probs" in kinds:
                B = video.shape[0]
                out["probs"] = m._probs.view(m.n_caption_lstm_step, B, m.n_words).cpu().numpy()
            if "train_op" in kinds:
                lr_node, clip_norm = m._train
                lr = m.learning_rate() if isinstance(lr_node, _Node) or lr_node is None else float(lr_node)
                m.apply_clipped(g, lr, clip_norm)
                m.global_step = step + 1
                out["train_op"] = None
        if "learning_rate" in kinds:
            out["learning_rate"] = m.learning_rate()
        res = [out[f.kind][f.index] if f.kind == "probs" else out[f.kind] for f in fl]
        return res[0] if single else res
