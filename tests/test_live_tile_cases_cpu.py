"""The cases of tests/live_tile_cases.py discriminate -- a condition on the INPUTS and expected outputs of tests/test_gpu_live_tiles.py,
checked on the CPU oracle alone: at every (table shape, variant, list, count) the GPU tests launch, the expected output arrays differ
from what each half-built kernel of live_tile_cases.MUTANTS would leave behind, wherever that kernel does not compute the contract itself
(live_tile_cases.distinguishable, pinned here).  The counts come from the tile tables through s2vt_tile_info, which needs no GPU."""
import numpy as np
import pytest

import live_tile_cases as lc


def _tile_rows(kind):
    import s2vt_amd
    from s2vt_amd import ops
    s2vt_amd.lib()
    return sorted({ops.tile_info(kind, i)["rows"] for i in range(ops.tile_count(kind))})


def _all_counts(kind):
    return sorted({n for bm in _tile_rows(kind) for n in lc.counts(bm)})


def test_lists_are_what_the_contract_allows():
    assert len(lc.LISTABLE) >= 129 and lc.DEAD not in lc.LISTABLE and 0 <= lc.DEAD < lc.R
    for kind in (0, 1, 2):
        rows = _tile_rows(kind)
        assert max(rows) + 1 <= len(lc.LISTABLE) and lc.R > max(rows), "two row tiles of the largest tile, every count listable"
        for n in _all_counts(kind):
            lst, live = lc.live_list("holes", n)
            assert len(lst) == lc.R and lst.min() >= 0 and lst.max() < lc.R                 # no out-of-range index, behind the count either
            k = min(n, lc.R)
            assert np.array_equal(lst[:k], live) and np.all(np.diff(live) > 0)              # distinct, ascending
            assert np.all(lst[k:] == lc.DEAD) and (n >= lc.R or lc.DEAD not in live)
            assert lc.live_list("null", n)[0] is None and len(lc.live_list("null", n)[1]) == k


def test_where_a_mutant_is_the_contract_itself():
    """Pinned, so that no case is dropped silently: all four mutants are distinguishable wherever a list with holes has a row, the two
    count mutants wherever the count is below R."""
    for n in range(0, lc.R + lc.EXTRA + 1):
        want_null = (lc.COUNT_IGNORED, lc.BEHIND_COUNT) if n < lc.R else ()
        assert lc.distinguishable("null", n) == want_null
        if n <= len(lc.LISTABLE) or n >= lc.R:
            want = lc.MUTANTS if 1 <= n < lc.R else want_null
            assert lc.distinguishable("holes", n) == want
    # and the restatement agrees: a mutant that is not distinguishable leaves exactly the contract's bits (on any per-row values)
    per_row = {"v": np.arange(lc.R * 3, dtype=np.float32).reshape(lc.R, 3)}
    for kind in lc.LISTS:
        for n in (0, 1, 5, 64, 129, lc.R, lc.R + lc.EXTRA):
            lst, _ = lc.live_list(kind, n)
            good = lc.launch(per_row, lst, n)["v"]
            for mut in lc.MUTANTS:
                same = np.array_equal(lc.launch(per_row, lst, n, mut)["v"], good)
                assert same == (mut not in lc.distinguishable(kind, n)), (kind, n, mut)


def _check(kind, expected, per_row_of, what):
    """expected: name -> [R, w] clean oracle outputs.  per_row_of(live) -> name -> [R, w] outputs from the inputs poisoned for `live`."""
    for lname in lc.LISTS:
        for n in _all_counts(kind):
            lst, live = lc.live_list(lname, n)
            per_row = per_row_of(live)
            # the contract on the poisoned inputs = the clean expected rows on the live rows, SENTINEL elsewhere: the GPU tests' expectation
            want = lc.launch(expected, lst, n)
            got = lc.launch(per_row, lst, n)
            for name in want:
                assert np.array_equal(want[name], got[name]), (what, lname, n, name)
                dead = np.ones(lc.R, bool); dead[live] = False
                assert np.all(want[name][dead] == lc.SENTINEL32) and not np.any(np.all(want[name][live] == lc.SENTINEL32, axis=1))
            for mut in lc.distinguishable(lname, n):
                bad = lc.launch(per_row, lst, n, mut)
                assert all(not np.array_equal(bad[name], want[name]) for name in want), (what, lname, n, mut)


@pytest.mark.parametrize("path", list(lc.STORE_SHAPES))
@pytest.mark.parametrize("variant", lc.STORE_VARIANTS)
def test_store_cases_reject_every_mutant(oracle, path, variant):
    _check(0, lc.store_expected(oracle, path, variant), lambda live: lc.store_per_row(oracle, lc.store_inputs(path, live), variant), (path, variant))


@pytest.mark.parametrize("path", list(lc.CELL_SHAPES))
@pytest.mark.parametrize("keep,residual", lc.CELL_VARIANTS)
def test_cell_cases_reject_every_mutant(oracle, path, keep, residual):
    _check(1, lc.cell_expected(oracle, path, keep, residual), lambda live: lc.cell_per_row(oracle, lc.cell_inputs(path, live), keep, residual),
           (path, keep, residual))
    if keep < 1:                                     # the mask is the caller row's: rows differ in their masks, and dropout changes `out`
        c = lc.cell_clean(path)
        mask = oracle.dropout_mask(lc.DROP_SEED, c["vid"], c["sid"], lc.DROP_CODE, keep, c["H"])
        assert len({m.tobytes() for m in mask}) > lc.R // 2 and 0 < mask.mean() < 1
    if residual:
        assert not np.array_equal(lc.cell_expected(oracle, path, keep, True)["out"], lc.cell_expected(oracle, path, keep, False)["out"])


@pytest.mark.parametrize("path", list(lc.PICK_SHAPES))
def test_pick_cases_reject_every_mutant(oracle, path):
    exp = lc.pick_expected(oracle, path)
    _check(2, exp, lambda live: lc.pick_per_row(oracle, lc.pick_inputs(path, live)), path)
    c = lc.pick_clean(path)
    # the tie row: two equal maxima, the lower index is the token; the all-negative row; both greedy; the other rows draw many tokens
    row = exp["logits"][lc.TIE_ROW]
    assert np.array_equal(np.flatnonzero(row == row.max()), [3, c["V"] - 2]) and exp["token"][lc.TIE_ROW] == 3
    assert exp["logits"][lc.NEG_ROW].max() < 0 and c["sid"][lc.TIE_ROW] == c["sid"][lc.NEG_ROW] == -1
    assert (c["sid"] >= 0).sum() > lc.R // 2 and (c["sid"] == -1).sum() > lc.R // 8 and len(np.unique(exp["token"])) > 20
    # the tokens depend on the noise ids of the caller's row: another row's ids change most of the sampled tokens
    shifted = oracle.pick_tokens(exp["logits"], np.roll(c["vid"], 1), c["sid"], lc.PICK_STEP, lc.PICK_SEED)
    assert (shifted != exp["token"])[c["sid"] >= 0].mean() > 0.5
