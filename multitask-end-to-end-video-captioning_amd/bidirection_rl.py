"""Self-critical REINFORCE for the bidirectional S2VT captioner: the stage every reinforcement_* script applies to its model
(reinforcement_multisampling_tf_s2vt.py:227-339 the graphs, :633-652 the train_op), on bidirection_tf_s2vt.py's model.  That script stops at
cross entropy, so bidirection.Video_Caption_Generator keeps refusing what it has no graph for; the stage lives in this subclass.

No word ever enters LSTM1: both LSTM1 directions, their histories and [fw ; bw] @ W2[:2H] depend on the video only.  The K samples of a
video share all of it, forward (s2vt_bidir_sample, s2vt_bidir_teacher_forced_fwd_rows) and backward (s2vt_bidir_bptt_bwd_rows: LSTM2's
pre-activation gradients are summed over a video's samples without atomics, and everything in front of LSTM2 runs on B rows).  Rows are
sample-major -- row s * B + j is sample s of video j -- and the feature block is never tiled.

The variables live in one model.ParamStore (flat buffers for the variables, the gradients and Adam's two moments, TF names from
bidirection.TF_NAMES), so the checkpoint helpers of train_common work on this class as on the others."""
from __future__ import annotations

import numpy as np
import torch

from . import bidirection, ops, tfckpt
from .bidirection import TF_NAMES, VARIABLES
from .model import Output, ParamStore, Placeholder, StepStats
from .model import Session as _GraphSession


class Reinforce_Caption_Generator(bidirection.Video_Caption_Generator):
    """bidirection.Video_Caption_Generator (same constructor) + sample / reinforce_update and their graph surface.  multisample: K of the
    REINFORCE graphs (build_loss's feed is the K-times tiled feature block, as the reference feeds it)."""

    def __init__(self, *args, multisample=1, **kw):
        super().__init__(*args, **kw)
        self.device = torch.device(self.device)
        self.multisample = int(multisample)
        shapes = bidirection.param_shapes(self.dim_image, self.n_words, self.word_dim, self.lstm_dim)
        self.store = ParamStore(shapes, self.device, order=VARIABLES, tf_names=TF_NAMES, params_factory=ops.make_bidir_params)
        for n in VARIABLES:
            self.store.p[n].copy_(self.p[n])
        self.p, self.g = self.store.p, self.store.g
        self._cparams = self.store.params
        self.global_step = 0
        self.adam_t = 0
        self.world_size, self.rank = 1, 0
        seed = int(kw.get("seed", args[12] if len(args) > 12 else 0))
        self.sample_seed, self.dropout_seed = seed, seed + 1
        self._gscale = torch.ones(1, dtype=torch.float32, device=self.device)
        self._applied = torch.zeros(1, dtype=torch.int32, device=self.device)   # step number of the last Adam update the device APPLIED
        self._row_ids_cache, self._rows_ws = {}, {}

    # ------------------------------------------------------------------------------------------ utilities
    def _dev(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype).contiguous()

    def _row_ids(self, B, video_base=0, rep=1):
        """(video_id, sample_id) of rep * B sample-major rows: row s * B + j is sample s of video video_base + j."""
        key = (B, int(video_base), int(rep))
        hit = self._row_ids_cache.get(key)
        if hit is None:
            if len(self._row_ids_cache) > 64:
                self._row_ids_cache.clear()
            vid = (torch.arange(B, dtype=torch.int32, device=self.device) + video_base).repeat(rep)
            sid = torch.arange(rep, dtype=torch.int32, device=self.device).repeat_interleave(B)
            hit = self._row_ids_cache[key] = (vid.contiguous(), sid.contiguous())
        return hit

    def _rows_workspace(self, B, S):
        if (B, S) not in self._rows_ws:
            if len(self._rows_ws) > 4:
                self._rows_ws.clear()
            self._rows_ws[(B, S)] = ops.bidir_rows_workspace(self._dims(), B, S, self.device)
        return self._rows_ws[(B, S)]

    def set_step(self, global_step, adam_t=None):
        self.global_step = int(global_step)
        self.adam_t = int(global_step if adam_t is None else adam_t)
        self._applied.fill_(self.adam_t)

    def check_health(self):
        """Raise S2VTChainTimeout if a persistent recurrence gave up a grid-wide wait since the last recover() (a host-memory read)."""
        if ops.chain_fault():
            from ._lib import S2VTChainTimeout
            raise S2VTChainTimeout("a persistent recurrence timed out (is another process running persistent kernels on this GPU?); "
                                   "the variables are intact: call recover() and repeat the step")

    def recover(self, disable_persistent=True):
        """After S2VTChainTimeout: synchronise, rewind the step counters to the last update the device applied, acknowledge the fault and
        switch to per-step launches (same bits).  Returns (step counter, updates skipped)."""
        torch.cuda.synchronize(self.device)
        applied = int(self._applied.item())
        ops.chain_ack(disable_persistent)
        lost = max(0, self.adam_t - applied)
        self.adam_t -= lost
        self.global_step -= lost
        return self.global_step, lost

    # ------------------------------------------------------------------------------------------ checkpoints
    def save(self, path, tf_version=1):
        """The variables under the TF names, and what a Saver created after the optimizer keeps beside them (model.ParamStore.state_dict):
        `<var>/Adam`, `<var>/Adam_1`, beta1_power, beta2_power, adam_t, and the step counter as g_step (the REINFORCE script's name)."""
        sd = self.store.state_dict(global_step=self.global_step, adam_t=self.adam_t, step_name="g_step", counter_dtype=np.int32)
        sd.pop("global_step", None)
        arrays = {k: np.asarray(v) for k, v in sd.items()}
        (tfckpt.write_checkpoint_v1 if tf_version == 1 else tfckpt.write_checkpoint_v2)(path, arrays)

    def restore(self, path):
        """A checkpoint of this class: variables, moments, adam_t and g_step.  An XE checkpoint of bidirection.Video_Caption_Generator.save
        (no g_step, no slots) restores optimistically: the variables load, the moments and both counters start at zero."""
        sd = dict(tfckpt.read_checkpoint(path))
        sd.pop("Variable", None)                           # the XE script's counter is not this graph's
        for n in VARIABLES:
            a = np.asarray(sd[TF_NAMES[n]])
            assert a.shape == tuple(self.p[n].shape), (n, a.shape)
        if "g_step" not in sd:
            sd = {TF_NAMES[n]: sd[TF_NAMES[n]] for n in VARIABLES}
            ops.zero_(self.store.m, self.store.v)
        self.store.load_state_dict(sd)
        step = self.store.restored_step or 0
        t = self.store.restored_adam_t
        self.set_step(step, step if t is None else t)

    # ------------------------------------------------------------------------------------------ the stage
    def sample(self, video, K=0, with_greedy=True, seed=None, video_base=0, stop_at_eos=False):
        """K multinomial captions per video (+ the greedy caption): (sampled [K*B, Tc], greedy [B, Tc]) int32 device tensors, sample-major
        rows -- the contract of model.Video_Caption_Generator.sample.  One LSTM1 pass, one hoisted partial and LSTM2's encode steps for the B
        videos, the decode steps on (K + greedy) * B rows that continue from their video's slice; Gumbel-max over Philox with counters
        (video_base + j, s, step); no dropout, <bos> at step 0, no host round trip.  K = 0: (None, greedy ids [B, Tc])."""
        if stop_at_eos:
            raise ValueError("the bidirectional captioner's sampler has no early-exit form: stop_at_eos is not available")
        video = self._dev(video, torch.float32)
        if K == 0:
            assert with_greedy
        return ops.bidir_sample(self._dims(), self.store.params, video, int(K), self.sample_seed if seed is None else seed, video_base, with_greedy)

    def _pg_forward(self, video, cap, keep, video_base, share):
        """The teacher-forced logits of the N = S * B sample rows: LSTM1's side on the B videos, or (share False) the plain driver on the
        S-times tiled feature block -- the same chains, bit-identical logits."""
        B, N = video.shape[0], cap.shape[0]
        assert N % B == 0 and N >= B, (N, B)
        S = N // B
        vid, sid = self._row_ids(B, video_base, S)
        seed = self.dropout_seed + 104729 * self.global_step
        if share:
            ws, feats = self._rows_workspace(B, S), video
            logits = ops.bidir_teacher_forced_fwd_rows(self._dims(), self.store.params, video, cap, ws, keep, seed, vid, sid)
        else:
            feats = video.repeat(S, 1, 1).contiguous() if S > 1 else video
            ws = self._workspace(N, self.device)
            logits = ops.bidir_teacher_forced_fwd(self._dims(), self.store.params, feats, cap, ws, keep, seed, vid, sid)
        return dict(logits=logits, ws=ws, feats=feats, S=S, B=B, N=N, vid=vid, sid=sid, seed=seed, keep=keep)

    def reinforce_update(self, video, sampled, mask, rewards, baseline, lr, clip_norm=5.0, keep=None, video_base=0, reward_fn=None,
                         share_lstm1=True, beta1=0.9, beta2=0.999, eps=1e-8):
        """One self-critical REINFORCE step (build_loss + train_op of reinforcement_multisampling_tf_s2vt.py:227-292, 633-652, on this model):
        video [B, Tv, D], sampled [N, Tc] ids with N = S * B sample-major rows, rewards / baseline [N].  The objective is

            - sum_{n,t} lp[n,t] mask[n,t] (r[n] - b[n]) / sum(mask)

        (no loss_weight and no weight decay, as in that script); lp = the log-probability of the sampled word under the teacher-forced pass
        with LSTM2's DropoutWrapper (keep; None: the model's dropout_rate -- quirk Q4), noise ids video_base + n % B and n // B.  mask None:
        derived from the ids on the device (1 up to and including the first <eos> = 0).  reward_fn: callable() -> (rewards, baseline),
        evaluated on the host AFTER the forward has been queued.  Then 1 / sum(mask), one squared norm per variable summed to the global
        norm, clip_by_global_norm(clip_norm) and TF-form Adam (quirk Q6).  Wemb's gradient is dense.  The gradients stay readable in self.g
        (scaled by 1 / sum(mask), before any clip).  share_lstm1 False: the same update through the plain drivers on the tiled block (the A/B
        switch; profiles/NOTES.md)."""
        keep = float(self.dropout_rate if keep is None else keep)
        video = self._dev(video, torch.float32)
        cap = self._dev(sampled, torch.int32)
        if mask is None:
            mask, target, msum = ops.caption_mask(cap)
        else:
            mask = self._dev(mask, torch.float32)
            target, msum = cap.t().contiguous().view(-1), mask.sum().reshape(1)
        c = self._pg_forward(video, cap, keep, video_base, share_lstm1)
        r, b = reward_fn() if reward_fn is not None else (rewards, baseline)
        coef = ops.pg_coef(mask, self._dev(r, torch.float32), self._dev(b, torch.float32), 1.0)
        nll, _ = ops.softmax_nll_fwd_bwd(c["logits"], target, coef, 0.0)          # logits <- coef * (softmax - onehot)
        st = self.store
        ops.zero_(st.grad)
        if share_lstm1:
            ops.bidir_bptt_bwd_rows(self._dims(), st.params, st.grads, video, c["S"], c["logits"], c["ws"], keep, c["seed"], c["vid"], c["sid"])
        else:
            ops.bidir_bptt_bwd(self._dims(), st.params, st.grads, c["feats"], c["logits"], c["ws"], keep, c["seed"], c["vid"], c["sid"])
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        ops.step_scalars(coef, nll, msum, msum, loss=loss, gscale=self._gscale)
        self._sumsq = torch.zeros(len(VARIABLES), dtype=torch.float32, device=self.device)       # one squared-norm slot per variable ...
        for i, n in enumerate(VARIABLES):
            ops.grad_finalize(self.g[n].view(-1), self.p[n].view(-1), self._gscale, 0.0, self._sumsq[i:i + 1])
        sumsq = self._sumsq.sum().reshape(1)                                                      # ... summed to the global norm
        self.global_step += 1
        self.adam_t += 1
        for n in VARIABLES:
            ops.adam_tf(self.p[n].view(-1), self.g[n].view(-1), st._view(st.m, n).view(-1), st._view(st.v, n).view(-1), sumsq, clip_norm, lr,
                        self.adam_t, beta1, beta2, eps, applied_step=self._applied)
        out = StepStats(loss[0], sumsq, msum[0])
        out.mask = mask
        return out

    # ------------------------------------------------------------------------------------------ the graph surface
    def placeholder(self, name, shape=(None,), dtype=np.float32):
        """tf.placeholder: `rewards` / `base_line` of reinforcement_multisampling_tf_s2vt.py:628-629."""
        return Placeholder(name, shape, dtype)

    def build_multinomial_sampler(self):
        """(sampled_captions, video): one multinomial caption per video (reinforcement_multisampling_tf_s2vt.py:294-339).  Every run draws
        from a fresh Philox stream (the TF op is stateful too); the stream is a function of the model's seed and the run count."""
        video = Placeholder("video", (self.batch_size, self.n_video_lstm_step, self.dim_image), np.float32)
        state = {"calls": 0}

        def fn(v):
            state["calls"] += 1
            s, _ = self.sample(v, 1, False, seed=self.sample_seed + 7919 * state["calls"])
            return {"sampled_captions": s.cpu().numpy().astype(np.int64)}
        return Output("sampled_captions", fn, [video]), video

    def _untile(self, v, N):
        """build_loss's video feed -> the B distinct videos on the device.  The reference feeds the feature block tiled K times, rows
        k*B + j = video j (reinforcement_multisampling_tf_s2vt.py:779-782): with multisample = K > 1 and N % K == 0 such a feed is
        recognised (compared on the host when it arrives there; a device tensor is taken at the feed contract's word) and the K copies
        are never made on the device.  Any other [N, ...] block is N videos."""
        K = self.multisample
        host = None if isinstance(v, torch.Tensor) else np.asarray(v, np.float32)
        n = (v if host is None else host).shape[0]
        if n == N and K > 1 and N % K == 0:
            B = N // K
            if host is not None:
                hb = host.reshape(K, B, -1)
                if all(np.array_equal(hb[0], hb[k]) for k in range(1, K)):
                    return self._dev(host[:B], torch.float32)
            else:
                return v[:B].to(device=self.device, dtype=torch.float32).contiguous()
        return self._dev(v if host is None else host, torch.float32)

    def build_loss(self):
        """(loss, video, caption, caption_mask) as reinforcement_multisampling_tf_s2vt.py:227-292 on this model: the reference returns the dense
        [N, Tc, V] tensor log_softmax * onehot * mask, which has one non-zero per (n, t) -- the fetch here is the [N, Tc] array of those
        values, lp * mask."""
        N, Tc = self.batch_size * self.multisample, self.n_caption_lstm_step
        video = Placeholder("video", (N, self.n_video_lstm_step, self.dim_image), np.float32)
        caption = Placeholder("caption", (N, Tc), np.int32)
        caption_mask = Placeholder("caption_mask", (N, Tc), np.float32)

        def fn(v, c, m):
            c = self._dev(c, torch.int32); m = self._dev(m, torch.float32)
            f = self._pg_forward(self._untile(v, c.shape[0]), c, float(self.dropout_rate), 0, True)
            zero = torch.zeros(f["logits"].shape[0], dtype=torch.float32, device=self.device)
            _, lp = ops.softmax_nll_fwd_bwd(f["logits"], c.t().contiguous().view(-1), zero, 0.0)
            return {"loss": (lp.view(Tc, -1).t() * m).cpu().numpy()}
        loss = Output("loss", fn, [video, caption, caption_mask])
        loss.graph = {"kind": "build_loss"}
        return loss, video, caption, caption_mask

    def reinforce_train_op(self, build_loss_outputs, rewards, base_line, learning_rate, clip_norm=5.0):
        """(train_op, sum_loss) of reinforcement_multisampling_tf_s2vt.py:641-652:
            norm = sum(loss_masks); sum_loss = -sum(loss * (rewards - base_line)) / norm;
            clip_by_global_norm(tf.gradients(sum_loss), 5); Adam.apply_gradients(global_step).
        Fed as there (:821-823): {loss_masks, loss_captions, loss_features (the K-times tiled block), rewards, base_line}.  sum_loss
        fetched beside train_op is the pre-update value the update differentiated."""
        video, caption, caption_mask = build_loss_outputs[1:4]
        lr = learning_rate.value if hasattr(learning_rate, "value") else (lambda: float(learning_rate))
        inputs = [video, caption, caption_mask, rewards, base_line]

        def fn(v, c, m, r, b):
            r = np.asarray(r, np.float32).reshape(-1); b = np.asarray(b, np.float32).reshape(-1)
            st = self.reinforce_update(self._untile(v, np.shape(c)[0]), c, m, r, b, lr(), clip_norm=clip_norm)
            return {"train_op": None, "sum_loss": float(st.loss)}
        return Output("train_op", fn, inputs), Output("sum_loss", fn, inputs)


class Session(bidirection.Session):
    """bidirection.Session, which also runs the REINFORCE graphs above (model.Output fetches, fed through model.Placeholder keys)."""

    def run(self, fetches, feed_dict=None):
        fl = fetches if isinstance(fetches, (list, tuple)) else [fetches]
        if any(isinstance(f, Output) for f in fl):
            return _GraphSession(self.model).run(fetches, feed_dict)
        return super().run(fetches, feed_dict)
