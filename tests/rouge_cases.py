"""ROUGE-L as the reference's reward applies it (pycocoevalcap's Rouge, beta = 1.2, one candidate against ALL references of its video),
restated on STRINGS from the arithmetic of DESIGN.md §3, and the seeded cases the host library (csrc_host/rouge.cpp) and the device
kernel (csrc/rouge.hip) are compared with bit for bit.

    l_j   = LCS(c, r_j)                                  the classic table, on split(" ") tokens
    p     = max_j float(l_j) / float(len c)
    r     = max_j float(l_j) / float(len r_j)            p and r may come from different references
    score = 0.0 if p == 0 or r == 0 else ((1 + b2) * p * r) / (r + b2 * p),   b2 = beta ** 2

Python floats are IEEE doubles and the interpreter fuses nothing, so every line above is one rounding, in this order.

The bridge to ids: the references go through reward.tokenize_refs (out-of-vocabulary words get private ids), the candidate of a row is
ixtoword of its ids BEFORE the first <eos> = 0 joined by blanks ("" for an empty one: "".split(" ") is one empty token that matches
nothing, so p = r = 0).

A plain module (no fixtures, no conftest): tests import it and share expected(name), computed once per case."""
import functools

import numpy as np

BETA = 1.2
CASES = ("tiny", "ragged", "long", "repeat")


def lcs_len(a, b):
    """The classic LCS table on two token lists."""
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for k, y in enumerate(b):
            cur.append(prev[k] + 1 if x == y else max(prev[k + 1], cur[k]))
        prev = cur
    return prev[len(b)]


def multiset_overlap(a, b):
    """NOT ROUGE-L: the bag-of-words overlap a wrong scorer might compute (order ignored).  The cases must tell it from lcs_len."""
    ca = {}
    for x in a:
        ca[x] = ca.get(x, 0) + 1
    n = 0
    for y in b:
        if ca.get(y, 0) > 0:
            ca[y] -= 1
            n += 1
    return n


def rouge_l(candidate: str, references, beta: float = BETA, overlap=lcs_len):
    """(score, p, r, [l_j]) of one candidate string against its video's reference strings."""
    c = candidate.split(" ")
    ls = [overlap(c, ref.split(" ")) for ref in references]
    p = max(float(l) / float(len(c)) for l in ls)
    r = max(float(l) / float(len(ref.split(" "))) for l, ref in zip(ls, references))
    b2 = beta ** 2
    score = 0.0 if p == 0 or r == 0 else ((1 + b2) * p * r) / (r + b2 * p)
    return score, p, r, ls


def candidate_string(row, ixtoword, eos_id=0, cut=True):
    """decode_captions (rouge_evaluation.py:122-143): the words before the first <eos>.  cut=False keeps the whole row (NOT the rule)."""
    words = []
    for i in row:
        if cut and int(i) == eos_id:
            break
        words.append(ixtoword[int(i)])
    return " ".join(words)


def vocabulary(V):
    """wordtoix / ixtoword of a model vocabulary of V ids: <eos> = 0, w1 .. w(V-1)."""
    ixtoword = {0: "<eos>"}
    for i in range(1, V):
        ixtoword[i] = f"w{i}"
    return {w: i for i, w in ixtoword.items()}, ixtoword


def _ref(rng, V, length):
    """A reference of `length` words over a vocabulary three words wider than the model's (w(V) .. w(V+2) are out of vocabulary)."""
    return " ".join(f"w{int(i)}" for i in rng.integers(1, V + 3, size=length))


def _ids_of(ref, wordtoix):
    return [wordtoix[w] for w in ref.split(" ")]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(ids [N, Tc] int32, video_of_row [N] int32, refs_by_video, wordtoix, ixtoword, V, forced {label: row})."""
    # (`repeat`: at |V| = 4 a quarter of the uniform rows start with <eos> and score 0, so the share of rows strictly inside (0, 1) hovers
    #  around two thirds -- 33 to 52 of 65 over seeds 14..39; 22 is one that leaves 47 and 12 rows on which a bag-of-words overlap differs)
    rng = np.random.default_rng({"tiny": 11, "ragged": 12, "long": 13, "repeat": 22}[name])
    forced = {}
    if name == "tiny":
        N, Tc, V = 1, 1, 3
        refs = [[_ref(rng, V, 1)]]
    elif name == "ragged":
        N, Tc, V = 130, 8, 12
        counts = [1, 64, 65, 130, 3, 2, 7]
        refs = [[_ref(rng, V, int(rng.integers(1, 15))) for _ in range(c)] for c in counts]
        refs[3][0] = _ref(rng, V, 14)                          # the longest length is present
        refs[1][5] = _ref(rng, V, 1)                           # and the shortest
        refs[4][0] = "w3 w7 w2 w9 w5"                          # in-vocabulary, for the row that carries it behind its <eos>
        refs[4][1] = "w11 w11 w1"
        refs[4][2] = "w10 w8"
        refs[6][2] = "w4 w4 w6 w1 w2 w8"                       # in-vocabulary, for the row that equals a reference
    elif name == "long":
        N, Tc, V = 3, 128, 30
        refs = [[_ref(rng, V, int(n)) for n in (200, 57, 131)], [_ref(rng, V, int(rng.integers(50, 201))) for _ in range(5)]]
    elif name == "repeat":
        N, Tc, V = 65, 5, 4
        refs = [[_ref(rng, V, int(rng.integers(1, 7))) for _ in range(int(c))] for c in (2, 4, 3)]
    else:
        raise KeyError(name)
    wordtoix, ixtoword = vocabulary(V)
    ids = rng.integers(0, V, size=(N, Tc)).astype(np.int32)             # uniform over the vocabulary: <eos> = 0 falls where it may
    vrow = rng.integers(0, len(refs), size=N).astype(np.int32)
    if name == "ragged":
        ids[0, 0] = 0                                                    # starts with <eos>: m = 0, score 0.0
        forced["empty"] = 0
        ids[1] = rng.integers(1, V, size=Tc)                             # no <eos> at all: m = Tc
        forced["no_eos"] = 1
        ids[2] = [6, 0] + _ids_of(refs[4][0], wordtoix) + [0]            # a full reference of its video BEHIND the first <eos>: must not count
        vrow[2] = 4
        forced["behind_eos"] = 2
        ids[3] = _ids_of(refs[6][2], wordtoix) + [0, 5]                  # equals a reference: exactly 1.0
        vrow[3] = 6
        forced["equal"] = 3
        vrow[4:11] = np.arange(7)                                        # every video is scored, the ones with 1, 64, 65 and 130 references too
    if name == "long":
        ids[1] = rng.integers(1, V, size=Tc)                             # a candidate without <eos>: length 128
        forced["no_eos"] = 1
    return dict(name=name, ids=ids, video_of_row=vrow, refs_by_video=refs, wordtoix=wordtoix, ixtoword=ixtoword, V=V, forced=forced)


def score_rows(c, beta=BETA, overlap=lcs_len, cut=True):
    """The restatement on every row of a case: (scores float64 [N], pr float64 [N, 2], [per-reference l_j lists])."""
    scores, pr, ls = [], [], []
    for row, v in zip(c["ids"], c["video_of_row"]):
        s, p, r, l = rouge_l(candidate_string(row, c["ixtoword"], cut=cut), c["refs_by_video"][int(v)], beta, overlap)
        scores.append(s); pr.append((p, r)); ls.append(l)
    return np.asarray(scores, np.float64), np.asarray(pr, np.float64).reshape(-1, 2), ls


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement of a case at beta = 1.2, computed once and shared: dict(score float64, f32 = float32(score), pr, ls).  Read only."""
    s, pr, ls = score_rows(case(name))
    out = dict(score=s, f32=s.astype(np.float32), pr=pr, ls=ls)
    for a in (out["score"], out["f32"], out["pr"]):
        a.setflags(write=False)
    return out
