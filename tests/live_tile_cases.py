"""Inputs and the oracle's expected outputs for the live-row forms of the single-op calls (s2vt_gemm_live, s2vt_lstm_cell_fwd_live,
s2vt_vocab_pick_live) -- a plain helper module, shared by tests/test_live_tile_cases_cpu.py (the cases discriminate: oracle only) and
tests/test_gpu_live_tiles.py.

A launch is described by a capacity of R rows, a list `live` and a count n: it computes the rows live[0 .. min(n, R)) of the caller's
arrays (`live` absent: rows 0 .. min(n, R) - 1) and neither reads nor writes another row.

Poison, so that a wrong row shows by VALUE and never by a fault:
  - every per-row input of a row that is not live holds NaN (plain operands, Cinit); its noise ids hold POISON_ID (another Philox stream),
    its gather index points at the table's last row, which holds NaN and which no live row uses; a row of a broadcast block (rowmod) that
    no live row maps to holds NaN;
  - the entries of `live` behind the count hold DEAD, one dedicated row: a valid index, never live, its inputs NaN;
  - every output row holds SENTINEL bits before the launch (tests/guardband.py) and the rows that are not live must still hold them after.
No index is out of range anywhere.

Lists.  "holes": the first n of LISTABLE (ascending; every row r with r % 8 == 0 is a hole, row 0 among them, so that the list differs
from the identity from its first entry on), then DEAD up to R entries.  LISTABLE has 131 rows: every count up to one past the largest
tile's 128 rows.  A list of R distinct rows of [0, R) is 0 .. R - 1 and nothing else, so at the counts R and R + EXTRA (the clamp) the
"holes" list IS that list, DEAD and the holes are live, and a list is told from no list only by the launch taking its rows through it.
"null": no list.

Half-built kernels (MUTANTS), restated in numpy by launch(): the list ignored (identity map); the list applied to the inputs but not to the
outputs; the count ignored (all R entries processed); one entry behind the count used (`m <= n`).  Where a mutant computes what the
contract asks for, no expected output can reject it: with no list the first two ARE the contract; at n == 0 they launch nothing, as the
contract does; at n >= R all four are the contract.  distinguishable() states exactly that, test_live_tile_cases_cpu.py pins it and
requires every case the GPU tests use to reject every distinguishable mutant -- all four at each of the counts 1, BM - 1, BM, BM + 1 of
the "holes" list."""
import numpy as np

from guardband import SENTINEL32

R = 150
DEAD = 72                                            # the dedicated row: a hole, NaN inputs, what `live` holds behind the count
LISTABLE = np.array([r for r in range(R) if r % 8], np.int32)
EXTRA = 7                                            # the count above R
POISON_ID = 999331                                   # video / sample id of a row that is not live
B = 5                                                # cell cases: videos the state and the residual operand are broadcast over
DROP_SEED, DROP_CODE = 77, 258
PICK_SEED, PICK_STEP = (5 << 32) | 2024, 5
LISTS = ("holes", "null")
CORRECT, IDENTITY, INPUTS_ONLY, COUNT_IGNORED, BEHIND_COUNT = "correct", "identity map", "outputs not mapped", "count ignored", "entry behind the count"
MUTANTS = (IDENTITY, INPUTS_ONLY, COUNT_IGNORED, BEHIND_COUNT)

# (K or E, N or H or V) per table and path, as the issue lists them
STORE_SHAPES = {"scalar": (7, 5), "vector": (76, 132), "vector-deep": (168, 260)}
STORE_SPLIT = {7: (2, 2, 3), 76: (24, 20, 32), 168: (64, 36, 68)}        # K = broadcast + gathered + plain segment (multiples of 4 on the vector path)
CELL_SHAPES = {"scalar": (3, 20), "vector": (12, 64), "vector-deep": (36, 132)}      # K = E + H: 23, 76 (fewer chunks than the deepest ring), 168 (more than any)
PICK_SHAPES = {"scalar": (20, 97), "vector": (64, 260), "vector-deep": (132, 388)}
STORE_VARIANTS = ("nobias", "bias", "bias+tanh")
CELL_VARIANTS = ((1.0, False), (1.0, True), (0.9, False), (0.9, True))               # (keep, residual form)
STORE_MOD, STORE_TABLE = 7, 23
TIE_ROW, NEG_ROW = 1, 2                               # pick cases: live from n = 2 ("holes") / n = 3 ("null") on; TIE_ROW is the one row of n = 1


def counts(bm):
    """The counts of a tile of bm rows."""
    return sorted({0, 1, bm - 1, bm, bm + 1, R, R + EXTRA})


def live_list(kind, n):
    """-> (the R entries of `live` or None, the rows that are live, ascending)."""
    assert kind in LISTS and n >= 0
    if kind == "null":
        return None, np.arange(min(n, R), dtype=np.int32)
    if n >= R:
        return np.arange(R, dtype=np.int32), np.arange(R, dtype=np.int32)
    assert n <= len(LISTABLE), "a list with holes has no more than len(LISTABLE) rows"
    lst = np.full(R, DEAD, np.int32)
    lst[:n] = LISTABLE[:n]
    return lst, LISTABLE[:n].copy()


def distinguishable(kind, n):
    """The mutants that do NOT compute what the contract asks for at this list and count (module docstring)."""
    if n >= R:
        return ()
    if kind == "null" or n == 0:
        return (COUNT_IGNORED, BEHIND_COUNT)
    return MUTANTS


def launch(per_row, lst, n, variant=CORRECT):
    """What the output arrays hold after a launch, as uint32 bits: per_row[name][r] = what a kernel computes for caller row r from the
    case's inputs.  variant: the contract, or one of MUTANTS."""
    cnt = min(n, R)
    if variant == COUNT_IGNORED:
        cnt = R
    if variant == BEHIND_COUNT:
        cnt = min(cnt + 1, R)
    m = np.arange(cnt)
    src = m if (lst is None or variant == IDENTITY) else lst[m]
    dst = m if variant == INPUTS_ONLY else src
    out = {}
    for name, a in per_row.items():
        a = np.ascontiguousarray(a).reshape(R, -1)
        o = np.full(a.shape, SENTINEL32, np.uint32)
        o[dst] = (a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32))[src]
        out[name] = o
    return out


def _nan_rows(a, live, mod=0):
    """A copy with NaN in every row no live row uses (mod > 0: a broadcast block, row r % mod)."""
    a = a.copy()
    used = np.zeros(a.shape[0], bool)
    used[(live % mod) if mod > 0 else live] = True
    a[~used] = np.nan
    return a


def _poison_ids(ids, live):
    out = np.full_like(ids, POISON_ID)
    out[live] = ids[live]
    return out


_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- store tiles: C = act([A0[r % 7] ; Tab[idx[r]] ; A2[r]] @ W (+ bias)) continuing Cinit[r]
def store_clean(path):
    def make():
        K, N = STORE_SHAPES[path]
        k0, k1, k2 = STORE_SPLIT[K]
        rng = np.random.default_rng(K * 1000 + N)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        tab = f(STORE_TABLE, k1)
        tab[-1] = np.nan                                                   # the row a non-live row's index points at
        return dict(A0=f(STORE_MOD, k0), Tab=tab, idx=rng.integers(0, STORE_TABLE - 1, R).astype(np.int32), A2=f(R, k2), W=f(K, N), bias=f(N),
                    Cinit=f(R, N), k=(k0, k1, k2), N=N)
    return _cached(("store", path), make)


def store_inputs(path, live):
    c = dict(store_clean(path))
    c["A0"] = _nan_rows(c["A0"], live, STORE_MOD)
    c["A2"] = _nan_rows(c["A2"], live)
    c["Cinit"] = _nan_rows(c["Cinit"], live)
    idx = np.full(R, STORE_TABLE - 1, np.int32)
    idx[live] = c["idx"][live]
    c["idx"] = idx
    return c


def store_per_row(oracle, c, variant):
    k0, k1, k2 = c["k"]
    C = c["Cinit"].copy()
    oracle.gemm_chain(np.ascontiguousarray(c["A0"][np.arange(R) % STORE_MOD]), c["W"][:k0], C)
    oracle.gemm_chain(c["Tab"], c["W"][k0:k0 + k1], C, rowidx=c["idx"])
    oracle.gemm_chain(c["A2"], c["W"][k0 + k1:], C)
    if variant != "nobias":
        oracle.bias_add(C, c["bias"])
    if variant.endswith("tanh"):
        C = oracle.det_tanh(C)
    return {"C": C}


def store_expected(oracle, path, variant):
    """The oracle's C of all R rows from the clean inputs (rows are independent: a live row's expected value does not depend on the list)."""
    return _cached(("store-exp", path, variant), lambda: store_per_row(oracle, store_clean(path), variant))


# ---- cell tiles: one BasicLSTMCell step, x[r] per row, the state and the residual operand of B videos broadcast (row r % B)
def cell_clean(path):
    def make():
        E, H = CELL_SHAPES[path]
        rng = np.random.default_rng(E * 1000 + H)
        return dict(W=rng.uniform(-.3, .3, (E + H, 4 * H)).astype(np.float32), b=rng.uniform(-.5, .5, 4 * H).astype(np.float32),
                    x=rng.standard_normal((R, E)).astype(np.float32), c=rng.standard_normal((B, H)).astype(np.float32),
                    h=rng.uniform(-1, 1, (B, H)).astype(np.float32), res=rng.standard_normal((B, H)).astype(np.float32),
                    vid=(100 + np.arange(R)).astype(np.int32), sid=(np.arange(R) % 4).astype(np.int32), E=E, H=H)
    return _cached(("cell", path), make)


def cell_inputs(path, live):
    c = dict(cell_clean(path))
    c["x"] = _nan_rows(c["x"], live)
    for k in ("c", "h", "res"):
        c[k] = _nan_rows(c[k], live, B)
    c["vid"], c["sid"] = _poison_ids(c["vid"], live), _poison_ids(c["sid"], live)
    return c


def cell_per_row(oracle, c, keep, residual):
    rows = np.arange(R) % B
    mask = None if keep >= 1 else oracle.dropout_mask(DROP_SEED, c["vid"], c["sid"], DROP_CODE, keep, c["H"])
    cn, hn, out, gates, _ = oracle.lstm1_step({"lstm1_W": c["W"], "lstm1_b": c["b"]}, c["x"], np.ascontiguousarray(c["c"][rows]),
                                              np.ascontiguousarray(c["h"][rows]), mask, keep, want_gates=True)
    if residual:
        out = (out + c["res"][rows]).astype(np.float32)                   # one fp32 addition
    return {"c_new": cn, "h_new": hn, "out": out, "gates": gates}


def cell_expected(oracle, path, keep, residual):
    return _cached(("cell-exp", path, keep, residual), lambda: cell_per_row(oracle, cell_clean(path), keep, residual))


# ---- pick tiles: logits = out2[r] @ W + b, one token per row (greedy for sample id -1, a Gumbel-max draw otherwise)
def pick_clean(path):
    def make():
        H, V = PICK_SHAPES[path]
        rng = np.random.default_rng(H * 1000 + V)
        o2 = rng.uniform(-1, 1, (R, H)).astype(np.float32)
        W = rng.uniform(-1, 1, (H, V)).astype(np.float32)
        b = rng.uniform(-.5, .5, V).astype(np.float32)
        sid = (np.arange(R) % 4 - 1).astype(np.int32)                      # -1 (greedy), 0, 1, 2
        # TIE_ROW: logits == b exactly, whose maximum 0.75 sits at column 3 and at the last column but one (another column tile of every
        # tile narrower than V - 4 columns): the lowest index wins
        o2[TIE_ROW] = 0
        b[[3, V - 2]] = 0.75
        # NEG_ROW: every logit below -9 (W[0] <= -1, |b| <= 0.75): a packed word whose key must still beat the zeroed word
        W[0] = -1 - np.abs(W[0])
        o2[NEG_ROW] = 0
        o2[NEG_ROW, 0] = 10
        sid[[TIE_ROW, NEG_ROW]] = -1
        return dict(o2=o2, W=W, b=b, vid=(100 + np.arange(R)).astype(np.int32), sid=sid, H=H, V=V)
    return _cached(("pick", path), make)


def pick_inputs(path, live):
    c = dict(pick_clean(path))
    c["o2"] = _nan_rows(c["o2"], live)
    c["vid"], c["sid"] = _poison_ids(c["vid"], live), _poison_ids(c["sid"], live)
    return c


def pick_per_row(oracle, c):
    logits = oracle.xw_plus_b(c["o2"], c["W"], c["b"])
    return {"logits": logits, "token": oracle.pick_tokens(logits, c["vid"], c["sid"], PICK_STEP, PICK_SEED)}


def pick_expected(oracle, path):
    return _cached(("pick-exp", path), lambda: pick_per_row(oracle, pick_clean(path)))

