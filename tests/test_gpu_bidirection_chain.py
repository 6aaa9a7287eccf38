"""Both LSTM1 directions of the bidirectional captioner in one call (csrc/bidir.hip, s2vt_lstm_birecurrence_fwd) against
(1) one direction at a time through s2vt_lstm_recurrence_fwd on per-step launches -- C, H and gates of both directions
BIT-identical -- and (2) the CPU oracle's BasicLSTMCell steps at the small shapes.

The one-launch form serves M <= 64; above that, and on per-step launches, a direction whose carried partial is not a
prefix is cut in two calls at the window's first step.  Covered: M = 1, 5, 16, 17, 32, 64 (one launch) and 65, 150 (fallback);
H = 32, 64 (8 k-groups) and 992 (64 k-groups, the last ones partly empty); the window as a prefix, a suffix read backwards
(the backward direction's frames), in the middle, over every step and absent; persistent 1 / 0 / -1 and 2 (one persistent recurrence per direction, by name); twice back to back
(every polled word and both state images are re-zeroed per call)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _dir_case(rng, M, E, H, T, win):
    W = rng.uniform(-.3, .3, (E + H, 4 * H)).astype(np.float32); b = rng.uniform(-.5, .5, 4 * H).astype(np.float32)
    h0 = rng.uniform(-1, 1, (M, H)).astype(np.float32); c0 = rng.standard_normal((M, H)).astype(np.float32)
    cinit = None if win is None else rng.standard_normal((win[1], M, 4 * H)).astype(np.float32)
    return W, b, h0, c0, cinit


# a window is (first chain step, steps, read last slice first) or None
CASES = [  # M, E, H, T, forward direction's window, backward direction's window
    (1, 4, 32, 5, (0, 2, False), (3, 2, True)),
    (5, 8, 64, 8, (0, 3, False), (5, 3, True)),
    (16, 8, 64, 6, None, None),
    (17, 4, 32, 5, (1, 2, False), (0, 5, True)),            # in the middle; over every step
    (64, 12, 64, 7, (0, 7, False), (2, 5, False)),
    (64, 500, 992, 6, (0, 2, False), (4, 2, True)),          # the script's cell, frames then padding / padding then frames
    (32, 500, 992, 4, None, (1, 3, True)),
    (65, 8, 64, 5, (0, 2, False), (3, 2, True)),             # above 64 rows: one recurrence per direction
    (150, 8, 32, 4, (0, 1, False), (1, 3, True)),
    (150, 16, 992, 3, (0, 1, False), (2, 1, True)),
]


def _reference(gpu, d, E, T, win):
    """one direction as s2vt_lstm_recurrence_fwd calls on per-step launches: steps ahead of the window without a partial,
    then from the window's first step with the partial as a prefix"""
    import torch
    W, b, h0, c0, cinit = d
    dW, db = _dev(W), _dev(b)
    t0, steps, rev = win if win is not None else (0, 0, False)
    if cinit is not None and rev:
        cinit = cinit[::-1].copy()
    Cs, Hs, Gs = [_dev(c0)[None]], [_dev(h0)[None]], []
    if t0 > 0:
        C, Hh, G, _ = gpu.lstm_recurrence_fwd(dW, E, db, _dev(h0), _dev(c0), t0, persistent=0)
        Cs.append(C[1:]); Hs.append(Hh[1:]); Gs.append(G)
    C, Hh, G, _ = gpu.lstm_recurrence_fwd(dW, E, db, Hs[-1][-1], Cs[-1][-1], T - t0, cinit=None if cinit is None else _dev(cinit),
                                          cinit_steps=steps, persistent=0)
    Cs.append(C[1:]); Hs.append(Hh[1:]); Gs.append(G)
    return torch.cat(Cs), torch.cat(Hs), torch.cat(Gs)


def _oracle_dir(oracle, d, E, T, win):
    W, b, h0, c0, cinit = d
    M, H = h0.shape
    t0, steps, rev = win if win is not None else (0, 0, False)
    c, h = c0, h0
    Cs, Hs, Gs = [c0], [h0], []
    for t in range(T):
        z = np.zeros((M, 4 * H), np.float32)
        if cinit is not None and t0 <= t < t0 + steps:
            z = cinit[steps - 1 - (t - t0) if rev else t - t0].copy()         # the carried partial starts the chain
        oracle.gemm_chain(np.ascontiguousarray(h), np.ascontiguousarray(W[E:]), z)
        oracle.bias_add(z, b)
        c, h, _, g = oracle.lstm_pointwise(z, c, None, 1.0, want_gates=True)
        Cs.append(c); Hs.append(h); Gs.append(g)
    return np.stack(Cs), np.stack(Hs), np.stack(Gs)


@pytest.mark.parametrize("M,E,H,T,wf,wb", CASES)
def test_both_directions_equal_one_recurrence_each(gpu, oracle, M, E, H, T, wf, wb):
    import torch
    rng = np.random.default_rng(1000 * M + H + T)
    dirs = [_dir_case(rng, M, E, H, T, w) for w in (wf, wb)]
    refs = [_reference(gpu, d, E, T, w) for d, w in zip(dirs, (wf, wb))]
    forms = (1, 2, 0, -1) if M <= 64 else (2, 0, -1)
    for persistent in forms:
        for rep in range(2 if persistent == 1 else 1):                      # back to back: nothing stale from the previous call
            desc = [gpu.lstm_dir(_dev(W), E, _dev(b), _dev(h0), _dev(c0), T, cinit=None if ci is None else _dev(ci),
                                 cinit_t0=0 if w is None else w[0], reverse=bool(w and w[2]))
                    for (W, b, h0, c0, ci), w in zip(dirs, (wf, wb))]
            got = gpu.lstm_birecurrence_fwd(desc[0], desc[1], persistent=persistent)
            assert gpu.chain_timeouts() == 0
            for which, r, g in zip(("fw", "bw"), refs, got):
                for name, rr, gg in zip(("C", "H", "gates"), r, g):
                    assert torch.equal(rr, gg), (which, name, persistent, rep)
    if H <= 64:
        for which, d, w, g in zip(("fw", "bw"), dirs, (wf, wb), got):
            for name, rr, gg in zip(("C", "H", "gates"), _oracle_dir(oracle, d, E, T, w), g):
                assert np.array_equal(rr, gg.cpu().numpy()), (which, name)


def test_one_launch_form_refuses_shapes_it_cannot_hold(gpu):
    import torch
    rng = np.random.default_rng(3)

    def pair(M, E, H, T):
        out = []
        for _ in range(2):
            W, b, h0, c0, _ = _dir_case(rng, M, E, H, T, None)
            out.append(gpu.lstm_dir(_dev(W), E, _dev(b), _dev(h0), _dev(c0), T))
        return out
    fw, bw = pair(65, 8, 64, 2)
    with pytest.raises(RuntimeError, match="bad argument"):
        gpu.lstm_birecurrence_fwd(fw, bw, persistent=1)                      # 65 rows: a fifth row tile
    fw, bw = pair(3, 8, 6, 2)
    with pytest.raises(RuntimeError, match="bad argument"):
        gpu.lstm_birecurrence_fwd(fw, bw, persistent=1)                      # H = 6 is not a multiple of 4
    (C, _, _), _ = gpu.lstm_birecurrence_fwd(fw, bw, persistent=-1)          # auto: per-step launches
    assert C.shape == (3, 3, 6) and bool(torch.isfinite(C).all())
    assert gpu.chain_timeouts() == 0


@pytest.mark.parametrize("M,persistent", [(5, 1), (64, 1), (65, -1), (5, 0)])
def test_histories_stay_inside_their_windows(gpu, M, persistent):
    """all six outputs in guard bands (tests/guardband.py), the carried partials and the index-free inputs too: nothing is written
    outside [T+1, M, H] / [T, M, 4H], nothing is read outside the partials' windows (a NaN read would poison the states)"""
    import ctypes as C
    import torch
    from guardband import Guarded
    from s2vt_amd import _lib
    E, H, T = 8, 64, 6
    rng = np.random.default_rng(M)
    dirs, refs, keep = [], [], []
    for k, win in enumerate(((0, 2, False), (4, 2, True))):
        d = _dir_case(rng, M, E, H, T, win)
        refs.append(_reference(gpu, d, E, T, win))
        W, b, h0, c0, cinit = d
        gW, gb = Guarded.of(W, name="W"), Guarded.of(b, name="b")
        gci = Guarded.of(cinit.reshape(win[1] * M, 4 * H), name="cinit")
        gC, gH = Guarded((T + 1) * M, H, name="C_hist"), Guarded((T + 1) * M, H, name="H_hist")
        gG = Guarded(T * M, 4 * H, name="gates")
        gC.view[:M].copy_(_dev(c0)); gH.view[:M].copy_(_dev(h0))
        s = _lib.LstmDir()
        s.W, s.kw0, s.b = gW.view.data_ptr(), E, gb.view.data_ptr()
        s.cinit = gci.view.data_ptr() + (4 * (win[1] - 1) * M * 4 * H if win[2] else 0)
        s.cinit_tstride = -M * 4 * H if win[2] else M * 4 * H
        s.ldcinit, s.cinit_t0, s.cinit_steps = 4 * H, win[0], win[1]
        s.C_hist, s.H_hist, s.gates = gC.view.data_ptr(), gH.view.data_ptr(), gG.view.data_ptr()
        dirs.append(s); keep.append((gW, gb, gci, gC, gH, gG))
    L = _lib.lib()
    nb = L.s2vt_lstm_birecurrence_scratch_bytes(H)
    ws = gpu.workspace(nb, "cuda", "bichain")
    rc = L.s2vt_lstm_birecurrence_fwd(C.byref(dirs[0]), C.byref(dirs[1]), M, H, T, persistent, C.c_void_p(ws.data_ptr()), ws.numel(),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert gpu.chain_timeouts() == 0
    for (gW, gb, gci, gC, gH, gG), (rC, rH, rG) in zip(keep, refs):
        for g in (gW, gb, gci, gC, gH, gG):
            g.assert_intact()
        assert np.array_equal(gC.numpy().reshape(T + 1, M, H), rC.cpu().numpy())
        assert np.array_equal(gH.numpy().reshape(T + 1, M, H), rH.cpu().numpy())
        assert np.array_equal(gG.numpy().reshape(T, M, 4 * H), rG.cpu().numpy())
