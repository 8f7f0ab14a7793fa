"""What the GPU tests of amd_ivf_add's own assignment (test_gpu_add_assign.py) require of their data, asserted from the reference
alone (the CPU oracle over add_assign_cases.py): the tie cases tie exactly as often as they say, the gate cases hold vectors whose two
best centroids an approximate ranking could confuse, the non-finite cases meet both outcomes of the reference's heap, and no list
stays empty by accident.  The list model itself is held to a vector-by-vector restatement."""
import numpy as np
import pytest

import add_assign_cases as ac


def rel_gap(D):
    """per row: |best - second best| relative to the larger magnitude"""
    D = D.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(D[:, 0] - D[:, 1]) / np.maximum(np.abs(D[:, 0]), np.abs(D[:, 1]))


def test_gate_terms():
    assert not ac.takes_pick(255, 68) and ac.takes_pick(256, 68) and ac.takes_pick(256, 4096)
    assert not ac.takes_pick(257, 67) and not ac.takes_pick(257, 4097)
    assert {(n, nl) for _, _, n, nl in ac.GATE_CASES} == {(n, nl) for n in (255, 256, 257) for nl in (67, 68, 4096, 4097)}
    assert {ac.gate_case(*a).cen.shape[1] for a in ac.GATE_CASES if ac.takes_pick(a[2], a[3])} == {4, 8, 30, 64}


@pytest.mark.parametrize("kind,metric,n,nlist", ac.GATE_CASES)
def test_gate_cases_hold_near_ties(oracle, kind, metric, n, nlist):
    c = ac.gate_case(kind, metric, n, nlist)
    (x, ids), = c.adds
    assert x.shape == (n, c.cen.shape[1]) and c.cen.shape[0] == nlist and ids is None and np.isfinite(x).all()
    if kind == "bytes":
        assert np.array_equal(x, np.floor(x)) and x.min() >= 0 and x.max() <= 255
    D, _ = oracle.knn(metric, x, c.cen, 2)
    g = rel_gap(D)
    close = int(((g < 0.01) & (D[:, 0] != D[:, 1])).sum())
    print(c.name, "d", x.shape[1], "within 1 %:", close, "exactly tied:", int((D[:, 0] == D[:, 1]).sum()))
    assert close >= 1
    assert int((D[:, 0] == D[:, 1]).sum()) < n // 2  # (most rankings are the picked path's to answer)


@pytest.mark.parametrize("metric,count,where", ac.TIE_CASES)
def test_tie_cases_tie_exactly_as_often_as_they_say(oracle, metric, count, where):
    c = ac.tie_case(metric, count, where)
    (x, _), = c.adds
    assert x.shape == (ac.TIE_N, ac.TIE_D) and ac.takes_pick(*x.shape[:1], len(c.cen))
    D, I = oracle.knn(metric, x, c.cen, 2)
    tied = np.nonzero(D[:, 0] == D[:, 1])[0]
    assert len(tied) == count == c.tied
    assert (tied[0] == 0) if where == "first" else (tied[-1] == ac.TIE_N - 1)
    assert count == 1 or (0 < tied[-1] < ac.TIE_N - 1 if where == "first" else 0 < tied[0] < ac.TIE_N - 1)
    # both kinds of tie: between the duplicated centroids (0 = 1) and between two distinct ones (2 and 3, or any under a zero vector)
    pairs = {tuple(sorted(p)) for p in I[tied].tolist()}
    assert np.array_equal(c.cen[0], c.cen[1]) and not np.array_equal(c.cen[2], c.cen[3])
    if count > 1:
        assert (0, 1) in pairs and len(pairs - {(0, 1)}) >= 1, pairs
    if metric == 0:
        assert (x[tied] == 0).all(axis=1).sum() == 1  # the all-zero vector
    assert np.array_equal(x[tied], np.floor(x[tied])) and np.abs(x[tied]).max() < 64  # small integers: exact distances
    assert ac.model_of(c).sizes()[1] == 0  # (of the duplicated centroids the reference's heap names the first: list 1 stays empty)
    assert (count + 7) // 8 * 8 - count == {1: 7, 7: 1, 8: 0, 9: 7}[count]      # copies that pad the flagged list


def test_zero_table_ties_everywhere(oracle):
    c = ac.zero_table_case()
    (x, _), = c.adds
    D, _ = oracle.knn(0, x, c.cen, 2)
    assert not c.cen.any() and (D == 0).all() and c.tied == len(x) == ac.TIE_N
    assert (ac.model_of(c).sizes() == 0).sum() == ac.TIE_NLIST - 1  # (the heap names one list for every vector)


def test_nonfinite_cases_meet_both_outcomes(oracle):
    stored_any, skipped_any = False, False
    for metric, n in ac.NONFINITE_CASES:
        c = ac.nonfinite_case(metric, n)
        (x, _), = c.adds
        bad = ~np.isfinite(x).all(axis=1)
        assert 5 <= bad.sum() <= 6 and bad[0] and bad[n - 1] and np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        assert (x == 0).all(axis=1).sum() == 1
        keys = ac.expected_keys(metric, x, c.cen)
        assert (keys[~bad] >= 0).all()
        print(c.name, "keys of the non-finite vectors:", keys[bad])
        if metric == 1:
            assert (keys[bad] == -1).all()  # every distance NaN or +inf: the heap admits none
        else:
            assert (keys[bad] == -1).any() and (keys[bad] >= 0).any()
        stored_any |= bool((keys[bad] >= 0).any())
        skipped_any |= bool((keys[bad] == -1).any())
        m = ac.model_of(c)
        assert m.ntotal == n and m.sizes().sum() == int((keys >= 0).sum())
        # the default ids of the vectors behind a skipped one are their positions
        got = np.sort(np.concatenate([m.ids(l) for l in range(m.nlist)]))
        assert np.array_equal(got, np.nonzero(keys >= 0)[0])
    assert stored_any and skipped_any


def test_nonfinite_bytes_cases_leave_byte_lists():
    for n in (300, 17):
        c = ac.nonfinite_bytes_case(n)
        (x, _), = c.adds
        keys = ac.expected_keys(1, x, c.cen)
        bad = ~np.isfinite(x).all(axis=1)
        assert bad.sum() == 3 and np.array_equal(keys < 0, bad) and np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        stored = x[~bad]
        assert np.array_equal(stored, np.floor(stored)) and stored.min() >= 0 and stored.max() <= 255
        assert np.array_equal(c.cen, np.floor(c.cen)) and c.cen.min() >= 0 and c.cen.max() <= 255  # (the journal variant's seed rows)


def test_no_list_stays_empty_by_accident():
    for c in ac.small_cases().values():
        sizes = ac.model_of(c).sizes()
        if not c.empty_ok:
            assert sizes.min() > 0, (c.name, int((sizes == 0).sum()))
        assert sizes.sum() > 0 and ac.model_of(c).ntotal == sum(len(x) for x, _ in c.adds)


def test_ids_case():
    for metric in (1, 0):
        c = ac.ids_case(metric)
        assert [len(x) for x, _ in c.adds] == [300, 5, 256, 40] and [i is None for _, i in c.adds] == [True, True, True, False]
        own = c.adds[3][1]
        assert (np.diff(own) < 0).any() and (np.diff(own) > 0).any() and (own > 1 << 32).sum() >= 10 and (own < 1 << 32).sum() >= 10
        assert len(np.unique(own)) == len(own) and own.min() >= 561  # (no id of the first three adds again)
        m = ac.model_of(c)
        got = np.sort(np.concatenate([m.ids(l) for l in range(m.nlist)]))
        assert np.array_equal(got, np.sort(np.concatenate([np.arange(561), own]))) and m.ntotal == 601


def test_model_equals_a_vector_by_vector_restatement():
    """IndexIVFFlat::add_core, one vector at a time, over a case with skipped vectors and one with ids of its own"""
    for c in (ac.nonfinite_case(0, 17), ac.ids_case(1)):
        nlist, d = c.cen.shape
        codes, ids, ntotal = [[] for _ in range(nlist)], [[] for _ in range(nlist)], 0
        for x, xids in c.adds:
            keys = ac.expected_keys(c.metric, x, c.cen)
            for i in range(len(x)):
                if keys[i] >= 0:
                    codes[keys[i]].append(x[i])
                    ids[keys[i]].append(int(xids[i]) if xids is not None else ntotal + i)
            ntotal += len(x)
        m = ac.model_of(c)
        assert m.ntotal == ntotal
        for l in range(nlist):
            assert np.array_equal(m.ids(l), np.array(ids[l], np.int64))
            assert np.array_equal(ac.bits(m.codes(l)), ac.bits(np.array(codes[l], np.float32).reshape(-1, d)))
        xb, assign, fid = m.flat()
        assert len(xb) == len(assign) == len(fid) == m.sizes().sum() and (np.diff(assign) >= 0).all()


def test_block_case_spans_two_blocks():
    for metric, nlist in ac.BLOCK_CASES:
        c = ac.block_case(metric, nlist)
        (x, _), = c.adds
        assert x.shape == (ac.ADD_BLOCK + 3, 4) and np.array_equal(x, np.floor(x)) and 0 <= x.min() and x.max() <= 255
        assert ac.takes_pick(ac.ADD_BLOCK, nlist) == (nlist == 68) and not ac.takes_pick(3, nlist)
        keys = ac.block_keys(metric, nlist)
        assert keys.min() >= 0 and (c.empty_ok or np.bincount(keys, minlength=nlist).min() > 0)


def test_seed_rows_let_the_journal_apply():
    c = ac.tie_case(1, 7, "first")
    s = ac.seed_rows(c)
    assert len(s) > 4 * ac.TIE_N and np.isfinite(s).all()
    q = ac.finite_queries(ac.nonfinite_case(0, 17))
    assert np.isfinite(q).all() and 0 < len(q) <= 32
