"""The residual model's beam search on the GPU (s2vt_beam_encode / s2vt_beam_step with S2VT_MODEL_RESIDUAL): every step's logits bit for
bit against the CPU restatement's unroll of each hypothesis' prefix, and the model surface (batched beam search against the per-video
generator, which sums in s2vt_lstm_cell_fwd_res)."""
import numpy as np
import pytest

import residual_cases as RC

pytestmark = pytest.mark.gpu
BEAM = 3


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", ["small-odd", "one-tile"])
def test_beam_step_logits_equal_the_unroll_of_each_prefix(gpu, oracle, name):
    p, d, video = RC.case(oracle, name)
    B, Tc, V = video.shape[0], d.n_caption_lstm_step, d.n_words
    dims = gpu.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step, residual=True)
    dp = {k: _dev(v) for k, v in p.items()}                              # (held: the struct has raw pointers)
    params = gpu.make_params(dp)
    dec = gpu.BeamDecoder(dims, B, BEAM)
    dec.encode(params, _dev(video))
    # step 0: one row per video, fed <bos>; from step 1 on BEAM hypotheses per video (video-major), each continuing ANOTHER row of its
    # video's group with that row's k-th best word, so the parent gather is not the identity
    vid = np.arange(B, dtype=np.int32)
    parent = np.zeros(B, np.int32)
    word = np.ones(B, np.int32)
    prefix = np.zeros((B, Tc), np.int32)                                   # the words fed at steps 1 .. t (column t - 1)
    differs = 0
    for t in range(Tc):
        R = len(vid)
        ids, logp, logits = dec.step(params, t, np.stack([vid, parent, word]), BEAM, want_logits=True)
        ref = RC.residual_teacher_forced(oracle, p, d, video[vid], prefix)[:, t]
        assert np.array_equal(logits.cpu().numpy(), ref), t
        differs += not np.array_equal(ref, RC.residual_teacher_forced(oracle, p, d, video[vid], prefix, residual=False)[:, t])
        order = np.argsort(-ref, axis=1, kind="stable")[:, :BEAM]
        assert np.array_equal(ids, order), t
        if t + 1 == Tc:
            break
        nvid = np.repeat(np.arange(B, dtype=np.int32), BEAM)
        k = np.tile(np.arange(BEAM), B)
        nparent = (nvid if t == 0 else nvid * BEAM + (k + 1) % BEAM).astype(np.int32)
        nword = ids[nparent, k].astype(np.int32)
        nprefix = prefix[nparent].copy()
        nprefix[:, t] = nword
        vid, parent, word, prefix = nvid, nparent, nword, nprefix
        assert R in (B, B * BEAM)
    assert differs == Tc                                                   # every step's logits are not the plain model's


def test_model_beam_search_equals_the_per_video_generator(gpu, oracle):
    import torch
    from s2vt_amd import model as M
    from s2vt_amd import residual
    p, d, video = RC.case(oracle, "small-odd")
    p = dict(p)
    p["embed_word_b"] = p["embed_word_b"].copy()
    p["embed_word_b"][0] += np.float32(1.0)                                # some captions end early
    args = (d.dim_image, d.n_words, d.word_dim, d.lstm_dim, 1, 0, d.n_video_lstm_step, d.n_caption_lstm_step)
    mdl = residual.Video_Caption_Generator(*args)
    plain = M.Video_Caption_Generator(*args)
    assert mdl.residual and not plain.residual
    mdl.store.load(p); plain.store.load(p)
    Tc = d.n_caption_lstm_step
    sess = M.Session(mdl)
    other = 0
    for k, lnf in ((1, 0.0), (3, 0.0), (3, 0.5)):
        got = mdl.beam_search(video, k, lnf, batch_size=4)                  # chunks of 4, 1
        vp, sent, _ = mdl.build_generator(beam_size=k, length_normalization_factor=lnf)
        base = plain.beam_search(video, k, lnf, batch_size=4)
        for j in range(video.shape[0]):
            ref = [int(w) for w in sess.run(sent, {vp: video[j:j + 1]})]
            ids = [0] * Tc
            ids[:len(got[j][0])] = got[j][0]
            if k > 1:
                assert ids == ref, (k, lnf, j)
            else:                                                           # beam 1 == greedy up to its <eos>
                assert got[j][0] == ref[:len(got[j][0])], (k, j)
            other += got[j][0] != base[j][0]
    assert other > 0
    # the greedy generator and its unshifted-softmax form against the restatement
    (_, rg), (_, pg) = RC.residual_sample(oracle, p, d, video, 0, 0), RC.residual_sample(oracle, p, d, video, 0, 0, residual=False)
    assert not np.array_equal(rg, pg)
    for quirk in (False, True):
        vp, sent, _ = mdl.build_generator(unshifted_softmax=quirk)
        for j in range(video.shape[0]):
            assert [int(w) for w in sess.run(sent, {vp: video[j:j + 1]})] == rg[j].tolist(), (quirk, j)
