"""The residual model's samplers on the GPU (s2vt_sample / s2vt_sample_ex with S2VT_MODEL_RESIDUAL): token ids against the CPU
restatement of tests/residual_cases.py, on cases shown there to differ from the plain model's decode."""
import numpy as np
import pytest

import residual_cases as RC

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _gpu_case(gpu, p, d, residual=True):
    dims = gpu.make_dims(d.dim_image, d.n_words, d.word_dim, d.lstm_dim, d.n_video_lstm_step, d.n_caption_lstm_step, residual=residual)
    dp = {k: _dev(v) for k, v in p.items()}
    params = gpu.make_params(dp)
    params._keep = dp                      # the struct holds raw pointers: keep the tensors alive with it
    return dims, params


@pytest.mark.parametrize("name,K,seed,video_base", RC.SAMPLE_CASES)
def test_sampled_and_greedy_ids_equal_the_restatement(gpu, oracle, name, K, seed, video_base):
    import torch
    res, plain = RC.decodes(oracle, name, seed, K, video_base=video_base)
    RC.assert_visible(name, res, plain)
    p, d, video = RC.case(oracle, name)
    dims, params = _gpu_case(gpu, p, d)
    s, g = gpu.sample(dims, params, _dev(video), K, seed=seed, video_base=video_base)
    torch.cuda.synchronize()
    assert np.array_equal(g.cpu().numpy(), res[1]), "greedy ids"
    assert np.array_equal(s.cpu().numpy(), res[0]), "sampled ids"


def test_without_the_greedy_block_and_greedy_alone(gpu, oracle):
    p, d, video = RC.case(oracle, "one-tile")
    dims, params = _gpu_case(gpu, p, d)
    (rs, rg), _ = RC.decodes(oracle, "one-tile", RC.SAMPLER_SEEDS[0])
    s, g = gpu.sample(dims, params, _dev(video), 2, seed=RC.SAMPLER_SEEDS[0], with_greedy=False)
    assert g is None and np.array_equal(s.cpu().numpy(), rs)
    _, g = gpu.sample(dims, params, _dev(video), 0, seed=RC.SAMPLER_SEEDS[0])
    assert np.array_equal(g.cpu().numpy(), rg)


@pytest.mark.parametrize("name", list(RC.EOS_BIAS))
def test_stop_at_eos_equals_the_full_decode_up_to_each_first_eos(gpu, oracle, name):
    seed = RC.SAMPLER_SEEDS[0]
    (rs, rg), _ = RC.decodes(oracle, name, seed, eos=True)
    ref = np.concatenate([rs, rg])
    first = RC.first_eos(ref)
    Tc = ref.shape[1]
    assert (first < Tc - 1).any() and (first == Tc).any()                       # rows do end early, and some never do
    p, d, video = RC.case(oracle, name)
    dims, params = _gpu_case(gpu, RC.with_eos_bias(p, name), d)
    s, g = gpu.sample(dims, params, _dev(video), RC.K_SAMPLES, seed=seed)
    full = np.concatenate([s.cpu().numpy(), g.cpu().numpy()])
    assert np.array_equal(full, ref)
    s, g = gpu.sample(dims, params, _dev(video), RC.K_SAMPLES, seed=seed, stop_at_eos=True)
    got = np.concatenate([s.cpu().numpy(), g.cpu().numpy()])
    want = ref.copy()
    for r, f in enumerate(first):
        want[r, f:] = 0
    assert np.array_equal(got, want)
