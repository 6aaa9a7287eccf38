"""The opt-in early-exit sampler of the temporal-attention captioner (s2vt_attn_sample_ex, S2VT_SAMPLE_STOP_AT_EOS; model.sample(...,
stop_at_eos=True)): rows that have emitted <eos> leave the decode loop -- every step's query projection, attention step, LSTM3, output
layer and vocabulary pick run on the compact list of rows still sampling, whose length only the device knows.  Ids up to and including
a row's first <eos> must be bit-identical to the plain sampler's, ids behind it 0; the masks -- and so the REINFORCE update -- are the
same.  embed_word_b[0] is raised so that rows end early (a random-initialised model never stops).

Shapes are (D, V, H, Tv, Tc, B, K) as in test_gpu_attn_reinforce.py; the reference ids are drawn once per (shape, bias, seed) by the
plain sampler and shared."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_attn_reinforce import _assert_mask_exercised

pytestmark = pytest.mark.gpu

#            D,   V,     H,   Tv, Tc, B,  K      <eos> bias
SMALL = [((48, 131, 32, 5, 6, 5, 3), 3.0),
         ((40, 97, 36, 32, 4, 7, 2), 3.0),       # H % 16 != 0: the scalar tiles and the scalar attention path, at the 32-frame chunk
         ((48, 131, 32, 5, 8, 100, 3), 3.0)]     # R = 400: several scan chunks of the live list, past 256 rows
TIMED = ((1536, 12000, 1000, 5, 20, 64, 5), 7.5)   # the measured shape: the real vector tiles; lengths as in test_gpu_stop_at_eos.py
SEEDS = (11, 12)


def _oracle():
    from oracle import s2vt_oracle
    s2vt_oracle.lib()
    return s2vt_oracle


@functools.lru_cache(maxsize=None)
def _inputs(shape, bias):
    D, V, H, Tv, Tc, B, K = shape
    if H >= 1000:          # the timed shape: the class's own initialisation (what tools/bench_attn_rl.py times)
        return None, np.abs(np.random.default_rng(5).standard_normal((B, Tv, D)) * 0.5).astype(np.float32)
    orc = _oracle()
    d = orc.Dims(dim_image=D, n_words=V, word_dim=0, lstm_dim=H, n_video_lstm_step=Tv, n_caption_lstm_step=Tc, label_dim=0)
    p = orc.init_attention_params(d, 1234)
    p["embed_word_b"][0] = bias
    return p, np.random.default_rng(7).standard_normal((B, Tv, D)).astype(np.float32)


def _model(shape, bias, **kw):
    import torch
    from s2vt_amd import attention as A
    D, V, H, Tv, Tc, B, K = shape
    p, video = _inputs(shape, bias)
    m = A.Attention_Caption_Generator(D, V, H, B, Tv, Tc, 0.9, **kw)
    if p is not None:
        m.load(p)
    else:
        with torch.no_grad():
            m.store.p["embed_word_b"][0] += bias
    return m, video


@functools.lru_cache(maxsize=None)
def _reference_once(shape, bias, seed, video_base=0):
    m, video = _model(shape, bias)
    s, g = m.sample(video, shape[6], True, seed=seed, video_base=video_base)
    return s.cpu().numpy(), g.cpu().numpy()


def _reference(shape, bias, seed, video_base=0):
    """(ids [K*B, Tc], greedy [B, Tc]) of the plain sampler: drawn once, every test gets its own copy."""
    s, g = _reference_once(shape, bias, seed, video_base)
    return s.copy(), g.copy()


def _mask(ids):
    from s2vt_amd import hostglue
    return hostglue.masks_from_ids(np.asarray(ids)).astype(bool)


def _assert_equal_up_to_first_eos(got, ref, what=""):
    mask = _mask(ref)                                         # up to and including the first <eos>
    assert 0 < mask.sum() < mask.size, what                   # the test must see rows that stop early
    assert np.array_equal(got[mask], ref[mask]), what         # identical where the objective looks
    assert (got[~mask] == 0).all(), what                      # and <eos> behind it
    assert np.array_equal(_mask(got), mask), what


# ------------------------------------------------------------------------------------------------- 1. ids up to the first <eos>
@pytest.mark.parametrize("shape,bias", SMALL + [TIMED], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_ids_equal_up_to_first_eos(gpu, shape, bias):
    D, V, H, Tv, Tc, B, K = shape
    m, video = _model(shape, bias)
    for seed in SEEDS:
        s_ref, g_ref = _reference(shape, bias, seed)
        # conditions on the inputs (the reference ids), not measurements
        lens = _mask(s_ref).sum(1)
        print(f"\n{shape} bias {bias} seed {seed}: sampled length mean {lens.mean():.2f} min {lens.min()} max {lens.max()}, "
              f"{int((~(s_ref == 0).any(1)).sum())} of {len(s_ref)} rows without <eos>")
        if (shape, bias) != TIMED:
            _assert_mask_exercised(_mask(s_ref).astype(np.float32))                  # at least a quarter of the rows end before Tc
        assert (~(s_ref == 0).any(1)).any(), "no reference row reaches Tc without <eos>"
        s, g = m.sample(video, K, True, seed=seed, stop_at_eos=True)
        assert s.shape == (K * B, Tc) and g.shape == (B, Tc) and s.dtype == g.dtype == __import__("torch").int32
        _assert_equal_up_to_first_eos(s.cpu().numpy(), s_ref, "sample block")
        _assert_equal_up_to_first_eos(g.cpu().numpy(), g_ref, "greedy block")
    assert gpu.chain_timeouts() == 0


# ------------------------------------------------------------------------------------------------- 2. empty live list
def test_every_row_finished_before_the_last_steps(gpu):
    """A bias so large that every row has its <eos> at least two steps before Tc: the last steps run with a device count of 0."""
    shape, bias = SMALL[0][0], 9.0
    D, V, H, Tv, Tc, B, K = shape
    m, video = _model(shape, bias)
    s_ref, g_ref = _reference(shape, bias, SEEDS[0])
    for ref in (s_ref, g_ref):
        assert (_mask(ref).sum(1) <= Tc - 2).all(), _mask(ref).sum(1)
    s, g = m.sample(video, K, True, seed=SEEDS[0], stop_at_eos=True)
    _assert_equal_up_to_first_eos(s.cpu().numpy(), s_ref)
    _assert_equal_up_to_first_eos(g.cpu().numpy(), g_ref)
    assert gpu.chain_timeouts() == 0
    s2, g2 = m.sample(video, K, True, seed=SEEDS[0])                                 # a following plain call is unharmed
    assert np.array_equal(s2.cpu().numpy(), s_ref) and np.array_equal(g2.cpu().numpy(), g_ref)


# ------------------------------------------------------------------------------------------------- 3. variants
@pytest.mark.parametrize("shape,bias", SMALL[:2], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_variants_greedy_only_no_greedy_and_video_base(gpu, shape, bias):
    import torch
    D, V, H, Tv, Tc, B, K = shape
    m, video = _model(shape, bias)
    s_ref, g_ref = _reference(shape, bias, SEEDS[0])
    # K = 0 with the greedy block: the greedy decoder up to the first <eos>
    ids0, _ = gpu.attn_decode_greedy(m.dims, m.store.params, m._dev(video, torch.float32))
    none, g0 = m.sample(video, 0, True, stop_at_eos=True)
    assert none is None
    _assert_equal_up_to_first_eos(g0.cpu().numpy(), ids0.cpu().numpy(), "K = 0")
    # without the greedy block: None, and the same sample ids as with it
    s_with, _ = m.sample(video, K, True, seed=SEEDS[0], stop_at_eos=True)
    s_with = s_with.cpu().numpy()
    s_only, no_g = m.sample(video, K, False, seed=SEEDS[0], stop_at_eos=True)
    assert no_g is None and np.array_equal(s_only.cpu().numpy(), s_with)
    _assert_equal_up_to_first_eos(s_with, s_ref)
    # a video_base of its own: the noise counters go through the live list
    base = 5
    sb_ref, gb_ref = _reference(shape, bias, SEEDS[0], base)
    assert not np.array_equal(sb_ref, s_ref)
    sb, gb = m.sample(video, K, True, seed=SEEDS[0], video_base=base, stop_at_eos=True)
    _assert_equal_up_to_first_eos(sb.cpu().numpy(), sb_ref, "video_base")
    _assert_equal_up_to_first_eos(gb.cpu().numpy(), gb_ref, "video_base, greedy")


# ------------------------------------------------------------------------------------------------- 4. the update is the same
def test_update_is_the_same_update(gpu):
    """reinforce_update on the early-exit sampler's ids == on the plain sampler's ids (same mask, same positions)."""
    shape, bias = SMALL[1]
    D, V, H, Tv, Tc, B, K = shape
    a, video = _model(shape, bias)
    b, _ = _model(shape, bias)
    rng = np.random.default_rng(2)
    r = (rng.random(K * B) * 2).astype(np.float32); bl = np.tile((rng.random(B) * 2).astype(np.float32), K)
    sa, _ = a.sample(video, K, True, seed=9)
    sb, _ = b.sample(video, K, True, seed=9, stop_at_eos=True)
    mask = _mask(sa.cpu().numpy())
    assert 0 < mask.sum() < mask.size and not np.array_equal(sa.cpu().numpy(), sb.cpu().numpy())
    a.reinforce_update(video, sa, None, r, bl, lr=1e-2, keep=0.9, share_image_blocks=True)
    b.reinforce_update(video, sb, None, r, bl, lr=1e-2, keep=0.9, share_image_blocks=True)
    worst = float((a.store.theta - b.store.theta).abs().max())
    print(f"\nmax |dtheta| between the two updates: {worst:.3e}")
    assert worst <= 1e-6


# ------------------------------------------------------------------------------------------------- 5. guard bands
@pytest.mark.parametrize("B,K", [(7, 2), (24, 3)])        # 21 rows; 96 rows with the greedy block (72 sampled: past the 64-row boundary)
def test_outputs_inside_guard_bands(gpu, B, K):
    import torch
    from guardband import SENTINEL32, Guarded
    shape, bias = (48, 131, 32, 5, 6, B, K), 3.0
    D, V, H, Tv, Tc = shape[:5]
    m, video = _model(shape, bias)
    s_ref, g_ref = _reference(shape, bias, SEEDS[0])
    L = __import__("s2vt_amd").lib()
    vd = m._dev(video, torch.float32)
    nbytes = L.s2vt_attn_sample_workspace_bytes(ctypes.byref(m.dims), B, K, 1)
    ws = gpu.workspace(nbytes, vd.device, "attn_sample")
    ids = Guarded(K * B, Tc, dtype=torch.int32, lead=65, name="ids_out")         # dense [rows, Tc] windows pre-filled with the sentinel
    gr = Guarded(B, Tc, dtype=torch.int32, lead=67, tail=70, name="greedy_out")
    ids.reset(); gr.reset()
    rc = L.s2vt_attn_sample_ex(ctypes.byref(m.dims), ctypes.byref(m.store.params), ctypes.c_void_p(vd.data_ptr()), B, K, 1, SEEDS[0], 0,
                               1, ids.ptr, gr.ptr,      # flags = S2VT_SAMPLE_STOP_AT_EOS
                               ctypes.c_void_p(ws.data_ptr()), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0
    ids.assert_intact(); gr.assert_intact()
    assert not (ids.bits() == SENTINEL32).any() and not (gr.bits() == SENTINEL32).any(), "an element of the outputs was not written"
    _assert_equal_up_to_first_eos(ids.numpy(), s_ref)
    _assert_equal_up_to_first_eos(gr.numpy(), g_ref)


# ------------------------------------------------------------------------------------------------- 6. driver
def test_driver_passes_the_flag_and_takes_the_same_step(gpu, tmp_path):
    import torch
    from s2vt_amd import attention as A, hostglue, train_attention, train_common as tc
    from test_gpu_train_drivers import _corpus
    rng = np.random.default_rng(0)
    sents, feats, vocab = _corpus(tmp_path, "attrleos", rng, n_videos=8)
    corpus = tc.Corpus(sents, feats, vocabulary=vocab)
    wordtoix, _ = hostglue.preProBuildWordVocab(corpus.vocabulary)
    quiet = lambda *_: None

    def cfg(name, **kw):
        return train_attention.reinforce_config(dim_image=24, lstm_dim=32, n_video_lstm_step=3, n_caption_lstm_step=8, n_epochs=1, batch_size=4,
                                                max_steps_per_epoch=1, start_learning_rate=1e-3, model_path=str(tmp_path / name), model_name=name, **kw)

    def fresh():
        return A.Attention_Caption_Generator(24, len(wordtoix), 32, 4, 3, 8, 0.9, seed=cfg("x").seed, device=f"cuda:{torch.cuda.current_device()}")
    m0 = fresh()
    with torch.no_grad():
        m0.store.p["embed_word_b"][0] += 3.0                      # rows end early: 17 words, logits within +-0.4 -> P(<eos>) ~ 1/2 per step
    _, hist = train_attention.train(cfg("start"), corpus, None, model=m0, log=quiet, reinforce=True, samples=2)
    ck = hist[-1]["checkpoint"]
    out = {}
    for flag in (False, True):
        m = fresh()
        seen = []
        plain_sample = m.sample

        def recording_sample(*a, _seen=seen, _f=plain_sample, **kw):
            res = _f(*a, **kw)
            _seen.append((kw.get("stop_at_eos", False), res[0].cpu().numpy()))
            return res
        m.sample = recording_sample
        model, _ = train_attention.train(cfg(f"run{int(flag)}", stop_at_eos=flag), corpus, None, model=m, log=quiet, reinforce=True, samples=2,
                                         resume=ck)
        assert model.global_step == 2
        assert [f for f, _ in seen] == [flag], seen
        out[flag] = (model.store.theta.clone(), seen[0][1])
    ref_ids, eos_ids = out[False][1], out[True][1]
    mask = _mask(ref_ids)
    assert 0 < mask.sum() < mask.size
    _assert_equal_up_to_first_eos(eos_ids, ref_ids)
    assert float((out[False][0] - out[True][0]).abs().max()) <= 1e-6
