"""Sampler cases at the edges of the persistent decode loop's window (csrc/decode_loop.hip, csrc/decode4.hip) -- a plain helper
module, shared by tests/test_sampler_cases_cpu.py (the inputs discriminate: oracle only) and tests/test_gpu_decode_loop_edges.py.

With oracle.init_params alone (U(-0.1, 0.1) / Glorot) the logits are almost flat: the greedy caption is one constant id and a multinomial
pick is decided by the noise and the bias, so a kernel that dropped its K tail, its padded embedding group or a hidden unit would still
draw the oracle's ids.  build() therefore scales the weights that carry the decode state (embed_word_W, lstm2_W, Wemb) and gives every
video a magnitude of its own; MUTANTS are the parameter edits that stand for such a kernel, and the CPU test requires that each of them
changes the oracle's ids at every case."""
from collections import namedtuple

import numpy as np

D_IMAGE, TV = 24, 2

# scales = (embed_word_W, lstm2_W, Wemb), chosen per case so that tests/test_sampler_cases_cpu.py holds; vmax = magnitude of the last video (the first has 0.2)
Case = namedtuple("Case", "V E H Tc B K with_greedy tiny scales vmax", defaults=(False, (30.0, 4.0, 10.0), 10.0))


def case_id(c):
    return f"V{c.V}-E{c.E}-H{c.H}-Tc{c.Tc}-B{c.B}-K{c.K}-g{int(c.with_greedy)}"


def rows(c):
    return (c.K + (1 if c.with_greedy else 0)) * c.B


# ---- (K + with_greedy) * B <= 64 rows: decode_loop_kernel<1>, the product path
CASES = [
    Case(8, 1, 132, 1, 16, 1, True, tiny=True),          # smallest corner: one column tile, one step, eg = 1, hgp = 16
    Case(16, 1, 132, 2, 16, 0, True, tiny=True, scales=(10.0, 8.0, 30.0)),       # all-argmax, a single hand-off
    Case(52, 5, 136, 3, 16, 3, True),                    # V straddles the 48-column workgroup boundary, R = 64 from B = 16
    Case(48, 16, 140, 4, 32, 1, True),                   # exactly one workgroup of columns, E = one full group, H % 16 = 12
    Case(100, 17, 144, 3, 48, 0, True),                  # B = 48 (one MFMA wave idle), E one past a group, H % 16 = 0
    Case(200, 7, 260, 3, 64, 0, True),                   # hgp = 24: six stages, 64 greedy rows
    Case(12288, 3, 132, 2, 16, 1, True),                 # every pick workgroup full
    Case(12284, 129, 260, 3, 32, 1, True),               # partial last column tile in the last workgroup, E one past 128
    Case(1000, 33, 1004, 3, 16, 2, True),                # H % 16 = 12 at 63 k-groups
    Case(1000, 128, 1008, 2, 32, 1, True, scales=(30.0, 4.0, 30.0)),   # the H ceiling, E = 128 (no padded embedding group)
    Case(300, 12, 500, 3, 16, 3, False, scales=(30.0, 8.0, 10.0)),     # with_greedy = 0: noise_rows == R
    Case(300, 12, 500, 3, 32, 2, False),
]

# ---- 257-384 rows: the opt-in forms (S2VT_DECLOOP=2: decode_loop_kernel<5> / <6>; S2VT_DEC4=1: decode4.hip)
BIG_CASES = [
    Case(200, 5, 132, 2, 16, 16, True),                  # R = 272: five row tiles per part
    Case(200, 9, 260, 2, 48, 6, True),                   # R = 336: six
]
DEC4_ONLY_CASES = [
    Case(200, 5, 136, 2, 100, 2, True),                  # R = 300, B no multiple of 16 (the persistent loop refuses it)
]


def params(c, oracle):
    """init_params with random biases, the state-carrying weights scaled by c.scales."""
    d = oracle.Dims(D_IMAGE, c.V, c.E, c.H, TV, c.Tc, 0)
    p = oracle.init_params(d, seed=3)
    rng = np.random.default_rng(9)
    for k in ("lstm1_b", "lstm2_b", "encode_image_b"):
        p[k] = rng.uniform(-.1, .1, p[k].shape).astype(np.float32)
    p["embed_word_b"] = rng.uniform(-.5, .5, c.V).astype(np.float32)
    s_out, s_w2, s_emb = c.scales
    p["embed_word_W"] = (p["embed_word_W"] * np.float32(s_out)).astype(np.float32)
    p["lstm2_W"] = (p["lstm2_W"] * np.float32(s_w2)).astype(np.float32)
    p["Wemb"] = (p["Wemb"] * np.float32(s_emb)).astype(np.float32)
    return d, p


def build(c, oracle):
    """-> (Dims, parameters, video [B, TV, D_IMAGE], seed, video_base).  Video j has magnitude 0.2 .. c.vmax (ascending in j): the encoder
    state, and with it the logits, differ from row to row."""
    d, p = params(c, oracle)
    rng = np.random.default_rng(c.B * 131 + c.H)
    video = np.abs(rng.standard_normal((c.B, TV, D_IMAGE)) * 0.5)
    video = (video * np.linspace(0.2, c.vmax, c.B)[:, None, None]).astype(np.float32)
    return d, p, video, 2024 + c.V, 10


# ---- oracle mutants: what a kernel that dropped part of its contraction would compute
def _tail(H):
    return H - (H % 16 or 16)


def _copy(p):
    return {k: v.copy() for k, v in p.items()}


def _hev(p):
    H = p["embed_word_W"].shape[0]
    return H, p["lstm2_W"].shape[0] - 2 * H


def drop_out_tail_group(p):
    """embed_word_W loses the last (partial) k-group of the vocabulary product."""
    q = _copy(p); H, _ = _hev(p)
    q["embed_word_W"][_tail(H):H] = 0
    return q


def drop_out_last_unit(p):
    q = _copy(p); H, _ = _hev(p)
    q["embed_word_W"][H - 1] = 0
    return q


def drop_recurrent_tail_group(p):
    """lstm2_W loses the recurrent rows of the last (partial) k-group."""
    q = _copy(p); H, E = _hev(p)
    q["lstm2_W"][H + E + _tail(H):2 * H + E] = 0
    return q


def drop_recurrent_last_row(p):
    q = _copy(p); H, E = _hev(p)
    q["lstm2_W"][2 * H + E - 1] = 0
    return q


def drop_embedding_last_column(p):
    q = _copy(p); _, E = _hev(p)
    q["Wemb"][:, E - 1] = 0
    return q


def drop_last_unit_gates(p):
    """the four gate columns of hidden unit H - 1 of LSTM2."""
    q = _copy(p); H, _ = _hev(p)
    for g in range(4):
        q["lstm2_W"][:, g * H + H - 1] = 0
    return q


MUTANTS = [drop_out_tail_group, drop_out_last_unit, drop_recurrent_tail_group, drop_recurrent_last_row, drop_embedding_last_column,
           drop_last_unit_gates]


def run_oracle(c, oracle, mutant=None):
    """The oracle's (sampled, greedy) ids of a case, on the parameters as built or as a mutant leaves them."""
    d, p, video, seed, base = build(c, oracle)
    if mutant is not None:
        p = mutant(p)
    return oracle.sample_captions(p, d, video, c.K, seed=seed, video_base=base, with_greedy=c.with_greedy)


def ids_changed(a, b):
    """Number of ids that differ between two (sampled, greedy) results."""
    return sum(int((x != y).sum()) for x, y in zip(a, b) if x is not None)
