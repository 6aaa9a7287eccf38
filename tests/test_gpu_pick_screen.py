"""The sampler's screened vocabulary pick (s2vt_sample_screened, csrc/pick_screen.hip) through the C ABI: token ids against the fp32
pick (s2vt_sample) and the oracle, ties and near-ties, the survivor counters (the screen is live, and no survivor is dropped), and the
error bound of the split-bf16 product the margin is built on.

Every sampler call runs on exact-size, guarded scratch blocks that a call on other inputs has dirtied beforehand."""
import ctypes as C

import numpy as np
import pytest

from guardband import GuardedWorkspace

pytestmark = pytest.mark.gpu

SMALL = (32, 300, 16, 136, 2, 6)           # V = 300: a 44-column tile edge; K = 136 padded to 192
WIDE = (32, 2000, 24, 264, 2, 4)
# dims (D, V, E, H, Tv, Tc), B, K, seed, video_base
ID_CASES = [
    pytest.param(SMALL, 13, 4, 7, 0, id="R65"),                  # one row past a 64-row tile
    pytest.param(WIDE, 48, 2, 11, 5, id="R144-video_base"),
    pytest.param(SMALL, 65, 2, 3, 0, id="R195"),                 # three rows past 192
]


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _case(oracle, dims, B, pseed=1):
    d = oracle.Dims(*dims, label_dim=0)
    p = oracle.init_params(d, seed=pseed)
    rng = np.random.default_rng(100 + B)
    video = np.abs(rng.standard_normal((B, d.n_video_lstm_step, d.dim_image)) * 0.5).astype(np.float32)
    return d, p, video


class _Sampler:
    """Both entry points on guarded scratch blocks of exactly the queried sizes, dirtied by a screened call on other inputs."""

    def __init__(self, gpu, d, p, video, B, K):
        import s2vt_amd
        self.L, self.gpu, self.B, self.K = s2vt_amd.lib(), gpu, B, K
        self.dims = gpu.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step)
        self.Tc, self.V = d.n_caption_lstm_step, d.n_words
        self.video = _dev(video)
        self.rows = (K + 1) * B
        nb = self.L.s2vt_sample_workspace_bytes(C.byref(self.dims), B, K, 1)
        sb = self.L.s2vt_sample_screen_workspace_bytes(C.byref(self.dims), B, K, 1)
        assert nb > 0 and sb > 0 and sb % 256 == 0
        self.ws, self.sws = GuardedWorkspace(nb, name="sampler workspace"), GuardedWorkspace(sb, name="screen scratch")
        self.set_params(p)
        self.screened(seed=991, video=_dev(video[::-1] * 0.7))          # dirt: a real call on other inputs

    def set_params(self, p):
        self._keep = {k: _dev(v) for k, v in p.items()}
        self.params = self.gpu.make_params(self._keep)

    def _ids(self):
        import torch
        return torch.full((self.rows, self.Tc), -7, dtype=torch.int32, device="cuda")

    def _split(self, ids):
        import torch
        torch.cuda.synchronize()
        self.ws.assert_intact()
        self.sws.assert_intact()
        a = ids.cpu().numpy()
        return a[:self.K * self.B], a[self.K * self.B:]

    def screened(self, seed, video_base=0, video=None):
        ids = self._ids()
        v = self.video if video is None else video
        rc = self.L.s2vt_sample_screened(C.byref(self.dims), C.byref(self.params), C.c_void_p(v.data_ptr()), self.B, self.K, 1, seed, video_base,
                                         C.c_void_p(ids.data_ptr()), self.ws.ptr, self.ws.nbytes, self.sws.ptr, self.sws.nbytes, None)
        assert rc == 0, rc
        return self._split(ids)

    def plain(self, seed, video_base=0):
        ids = self._ids()
        rc = self.L.s2vt_sample(C.byref(self.dims), C.byref(self.params), C.c_void_p(self.video.data_ptr()), self.B, self.K, 1, seed, video_base,
                                C.c_void_p(ids.data_ptr()), self.ws.ptr, self.ws.nbytes, None)
        assert rc == 0, rc
        return self._split(ids)

    def counters(self):
        """(survivors summed over rows and steps, most survivors of one row, rows that took every column) of the last screened call."""
        head = self.sws.window[:16].cpu().numpy()
        return int(head[:8].view(np.uint64)[0]), int(head[8:12].view(np.uint32)[0]), int(head[12:16].view(np.uint32)[0])


@pytest.mark.parametrize("dims,B,K,seed,video_base", ID_CASES)
def test_ids_equal_the_fp32_pick_and_the_oracle(gpu, oracle, dims, B, K, seed, video_base):
    d, p, video = _case(oracle, dims, B)
    s = _Sampler(gpu, d, p, video, B, K)
    got_s, got_g = s.screened(seed, video_base)
    total, most, every = s.counters()
    ref_s, ref_g = s.plain(seed, video_base)
    assert np.array_equal(got_g, ref_g), "greedy ids differ from s2vt_sample's"
    assert np.array_equal(got_s, ref_s), "sampled ids differ from s2vt_sample's"
    orc_s, orc_g = oracle.sample_captions(p, d, video, K=K, seed=seed, video_base=video_base)
    assert np.array_equal(got_g, orc_g), "greedy ids differ from the oracle's"
    assert np.array_equal(got_s, orc_s), "sampled ids differ from the oracle's"
    # the screen is live: a path that silently resolved every column would show V survivors per row (measured here: 1.9 - 2.9)
    mean = total / (s.rows * s.Tc)
    print(f"survivors per row: mean {mean:.3f}, most {most}; rows that took every column: {every}")
    assert 1.0 <= mean <= 8.0 and every == 0


def test_duplicated_columns_pick_the_lowest_index(gpu, oracle):
    d, p, video = _case(oracle, SMALL, 13)
    p["embed_word_W"][:, 1::2] = p["embed_word_W"][:, 0::2]
    s = _Sampler(gpu, d, p, video, 13, 4)
    got_s, got_g = s.screened(5)
    _, most, _ = s.counters()
    ref_s, ref_g = s.plain(5)
    assert np.array_equal(got_g, ref_g) and np.array_equal(got_s, ref_s)
    assert (got_g % 2 == 0).all(), "an argmax row took the higher of two equal columns"
    assert most >= 2


def test_near_ties_resolve_as_the_fp32_pick(gpu, oracle):
    d, p, video = _case(oracle, SMALL, 13)
    W = p["embed_word_W"]
    for j in range(1, 4):                                     # groups of four columns, 2^-20 apart: all of the winning group survive
        W[:, j::4] = W[:, 0::4] * np.float32(1.0 + j * 2.0 ** -20)
    s = _Sampler(gpu, d, p, video, 13, 4)
    got_s, got_g = s.screened(9)
    _, most, every = s.counters()
    ref_s, ref_g = s.plain(9)
    assert np.array_equal(got_g, ref_g) and np.array_equal(got_s, ref_s)
    assert most >= 4 and every == 0


def test_zero_weights_keep_every_column_and_pick_id_zero(gpu, oracle):
    B, K = 33, 1
    d, p, video = _case(oracle, SMALL, B)
    p["embed_word_W"][:] = 0.0
    p["embed_word_b"][:] = 0.25
    s = _Sampler(gpu, d, p, video, B, K)
    got_s, got_g = s.screened(2)
    total, most, every = s.counters()
    ref_s, ref_g = s.plain(2)
    assert np.array_equal(got_g, ref_g) and np.array_equal(got_s, ref_s)
    assert (got_g == 0).all()
    assert most == s.V and every == 0                         # an argmax row: all V keys are equal, none may be dropped
    assert total >= B * s.Tc * s.V


@pytest.mark.parametrize("R,H,V", [(65, 136, 300), (144, 1000, 2000)])
def test_split_product_error_is_inside_the_margin(gpu, R, H, V):
    """max |L~ - L| / (|h| |w|) <= C / 8 with C = 2^-10 (K <= 1024), L~ from the split-bf16 entries, L from the fp32 chain (s2vt_gemm)."""
    import torch
    import s2vt_amd
    from s2vt_amd import _lib
    L = s2vt_amd.lib()
    rng = np.random.default_rng(R + H)
    h = rng.uniform(-1.0, 1.0, (R, H)).astype(np.float32)
    W = rng.uniform(-0.1, 0.1, (H, V)).astype(np.float32)
    hd, Wd = _dev(h), _dev(W)
    Hp = (H + 63) // 64 * 64
    P = lambda t: C.c_void_p(t.data_ptr())
    hh, hl = (torch.empty((R, Hp), dtype=torch.int16, device="cuda") for _ in range(2))
    Wh, Wl = (torch.empty((V, Hp), dtype=torch.int16, device="cuda") for _ in range(2))
    assert L.s2vt_cast_bf16_split(P(hd), H, None, R, H, 0, P(hh), P(hl), Hp, 0, None, None, None, 0, None, 0, None) == 0
    assert L.s2vt_cast_bf16_split(P(Wd), V, None, H, V, 1, P(Wh), P(Wl), Hp, Hp, None, None, None, 0, None, 0, None) == 0
    approx = torch.empty((R, V), dtype=torch.float32, device="cuda")
    assert L.s2vt_gemm_bf16x3_nt(P(hh), P(hl), Hp, P(Wh), P(Wl), Hp, P(approx), V, R, V, Hp, 0, None, 0, None) == 0
    exact = torch.empty((R, V), dtype=torch.float32, device="cuda")
    seg = _lib.Operand(hd.data_ptr(), None, H, H, 0, 0)
    assert L.s2vt_gemm(C.byref(seg), 1, P(Wd), V, None, None, 0, P(exact), V, R, V, 0, -1, None) == 0
    torch.cuda.synchronize()
    scale = np.linalg.norm(h.astype(np.float64), axis=1)[:, None] * np.linalg.norm(W.astype(np.float64), axis=0)[None, :]
    ratio = float((np.abs(approx.cpu().numpy().astype(np.float64) - exact.cpu().numpy()) / scale).max())
    print(f"R={R} H={H} V={V}: max |L~ - L| / (|h||w|) = {ratio:.3e} = {ratio / 2.0 ** -10:.3e} of C")
    assert ratio <= 2.0 ** -10 / 8
