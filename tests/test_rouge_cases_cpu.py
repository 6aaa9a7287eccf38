"""The ROUGE-L restatement (tests/rouge_cases.py) against hand values, and the seeded cases' power to discriminate: a spread of scores,
p and r from different references, and a scorer that replaces LCS by a bag-of-words overlap or forgets the "before the first <eos>"
rule gets caught.  No GPU, no native code.

The spread is asked where the case's size allows it: two thirds of the rows strictly inside (0, 1) at `ragged`, `long` and `repeat`
(`tiny` is one row); 20 distinct scores, an exact 0.0 and an exact 1.0 at `ragged`, which forces such rows."""
import numpy as np
import pytest

import rouge_cases as RC


def test_hand_values():
    s, p, r, ls = RC.rouge_l("a b c d", ["a c d e f"])
    assert ls == [3] and p == 0.75 and r == 0.6 and s == 0.6535714285714286
    s, p, r, ls = RC.rouge_l("a b c", ["a b c x y z w", "a q"])
    assert ls == [3, 1] and p == 1.0 and r == 0.5 and s == 0.6288659793814433          # p from the first reference, r from the second
    assert RC.rouge_l("x y z", ["q", "x y z", "x y"])[0] == 1.0                       # equal to one reference: exactly 1.0
    assert RC.rouge_l("", ["a b"])[:3] == (0.0, 0.0, 0.0)                              # "".split(" ") is one empty token
    assert RC.rouge_l("a", ["b"])[0] == 0.0
    assert RC.lcs_len("a b a b".split(), "b a b a".split()) == 3 and RC.multiset_overlap("a b a b".split(), "b a b a".split()) == 4


def test_case_shapes():
    t = RC.case("tiny")
    assert t["ids"].shape == (1, 1) and len(t["refs_by_video"]) == 1 and len(t["refs_by_video"][0]) == 1 and len(t["refs_by_video"][0][0].split(" ")) == 1
    g = RC.case("ragged")
    assert g["ids"].shape == (130, 8) and g["V"] == 12 and [len(r) for r in g["refs_by_video"]] == [1, 64, 65, 130, 3, 2, 7]
    lens = {len(s.split(" ")) for refs in g["refs_by_video"] for s in refs}
    assert min(lens) == 1 and max(lens) == 14
    assert set(range(7)) <= set(g["video_of_row"].tolist())
    f = g["forced"]
    assert g["ids"][f["empty"], 0] == 0 and (g["ids"][f["no_eos"]] != 0).all()
    l = RC.case("long")
    assert l["ids"].shape == (3, 128) and l["V"] == 30 and (l["ids"][l["forced"]["no_eos"]] != 0).all()
    assert max(len(s.split(" ")) for refs in l["refs_by_video"] for s in refs) == 200
    r = RC.case("repeat")
    assert r["ids"].shape == (65, 5) and r["V"] == 4
    for name in RC.CASES:                                          # the reference vocabulary is wider than the model's: some words are OOV
        c = RC.case(name)
        words = {w for refs in c["refs_by_video"] for s in refs for w in s.split(" ")}
        assert name == "tiny" or any(w not in c["wordtoix"] for w in words)


@pytest.mark.parametrize("name", RC.CASES)
def test_score_spread(name):
    e = RC.expected(name)
    s = e["score"]
    assert ((s >= 0.0) & (s <= 1.0)).all() and len(s) == len(RC.case(name)["ids"])
    inside = int(((s > 0.0) & (s < 1.0)).sum())
    print(name, "rows", len(s), "strictly inside (0, 1):", inside, "distinct:", len(set(s.tolist())), "zeros:", int((s == 0).sum()), "ones:", int((s == 1).sum()))
    if name != "tiny":
        assert 3 * inside >= 2 * len(s)
    if name == "ragged":
        assert len(set(s.tolist())) >= 20 and (s == 0.0).any() and (s == 1.0).any()
        f = RC.case(name)["forced"]
        assert s[f["empty"]] == 0.0 and s[f["equal"]] == 1.0 and s[f["behind_eos"]] == 0.0 and s[f["no_eos"]] > 0.0
    assert np.array_equal(e["f32"], s.astype(np.float32))


def test_p_and_r_from_different_references():
    c, e = RC.case("ragged"), RC.expected("ragged")
    split = 0
    for row, v, ls in zip(c["ids"], c["video_of_row"], e["ls"]):
        refs = c["refs_by_video"][int(v)]
        if max(ls) == 0:
            continue
        ratios = [l / len(s.split(" ")) for l, s in zip(ls, refs)]
        best_p = {j for j, l in enumerate(ls) if l == max(ls)}
        best_r = {j for j, x in enumerate(ratios) if x == max(ratios)}
        split += not (best_p & best_r)
    assert split >= 1


def test_cases_tell_lcs_from_a_bag_of_words():
    for name in ("repeat", "ragged"):
        wrong = RC.score_rows(RC.case(name), overlap=RC.multiset_overlap)[0]
        assert (wrong != RC.expected(name)["score"]).any(), name


def test_cases_tell_the_eos_rule():
    c, e = RC.case("ragged"), RC.expected("ragged")
    wrong = RC.score_rows(c, cut=False)[0]
    assert (wrong != e["score"]).any() and wrong[c["forced"]["behind_eos"]] > 0.0 == e["score"][c["forced"]["behind_eos"]]
