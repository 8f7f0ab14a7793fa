"""A search's result does not depend on what its handle searched before.

The engine keeps three kinds of history per handle ("Device-chained rounds"): the item counts every round of the previous search
of the same signature planned, by which the chained rounds size their scan grids without a look at the device (+ 12 %); the row
space the last adaptive search of the signature wanted; and workspaces that only grow, so that after a large search they hold its
masks, rows, logs and items.  The signature is made of n, the first round's probes, nprobe, k and the kind of search -- not of the
queries, the lists they probe or the lists' contents.  Every test here keeps ONE handle through a sequence of searches that share
a signature and differ in work, and holds every step to the pinned oracle bit for bit (ids, distances, statistics), computed per
step from lists built in handle_history_cases.py.  amd_ivf_last_round_hints proves the path: `hinted` scan launches sized from
history, `short` of them on a grid smaller than their work (the workgroups must stride over the count on the device, ItemWalk).

Notes on what the code does where the plan of these tests said otherwise:
  * fp32 lists are planned in blocks of 32 queries (scan_qblock), so scan_shape_of never returns 8 for them: "crowd" (every query
    on the same eight big lists, 160 = 5 x 32 queries a list) is tile shape 4 only, "spread" (no list probed by more than 8
    queries, the other probes absent) tile shape 1 only.  Byte lists have one item form, counted where shape 8 is.
  * a round's segments are n x (probes of the round), whatever the keys: at a fixed nprobe the keep-bit kernel's grid, sized from
    the segments of the previous search, is never short.  Its walk is reached where there is NO history: the grid is then sized for
    64 probes a query, and the last steps of the selector sequence search 72 (the reference's -1 padding behind eight real keys) in
    one round.
  * max_codes acts in the selection, not in the planning: the step that caps it plans the same items and returns fewer results.
No form of the matrix came out unhinted; none was removed."""
import numpy as np
import pytest

import handle_history_cases as hc
from handle_history_cases import K, N, NPROBE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@pytest.fixture(scope="module")
def expect(oracle):
    """the oracle's results, computed once per world and query set (handle_history_cases caches them, read-only)"""
    return hc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want, what):
    D, I = got
    assert D.shape == want[0].shape and np.array_equal(I, want[1]), what
    assert np.array_equal(bits(D), bits(want[0])), what


def open_handle(capi, w, options=()):
    h = capi.Handle(w["d"], hc.NLIST, w["metric"], 0)
    for key, value in options:
        h.set_option(key, value)
    h.set_centroids(w["cen"])
    h.set_lists_from_assign(w["xb"], w["assign"])
    return h


def step(h, form, name, what, n=N, store_pairs=False, max_codes=0, want=None, on=None):
    """one search_preassigned of query set `name` on `on` (default h) against the oracle -> (hinted, short)"""
    kind, d, metric = form
    on = on if on is not None else h
    xq, keys, dis = hc.query_set(kind, d, metric, name, n)
    eD, eI, est = want if want is not None else hc.expected(kind, d, metric, name, n, store_pairs, max_codes)
    on.stats(reset=True)
    got = on.search_preassigned(xq, K, keys, dis, store_pairs=store_pairs, max_codes=max_codes)
    st = on.stats()
    hints = on.last_round_hints()
    print("[history]", what, name, "hinted/short", hints, "filter", on.last_filter(), "passes", on.last_timing()["rounds"])
    same(got, (eD, eI), (what, name))
    assert [st["nlist"], st["ndis"], st["nheap_updates"]] == list(est), (what, name, st, est)
    assert h.scan_arith() == hc.KINDS[kind], (what, name)
    return hints


def too_small(hints, what):
    assert hints[0] > 0 and hints[1] > 0, (what, hints, "no scan ran on a grid smaller than its work")


def oversized(hints, what):
    assert hints[0] > 0 and hints[1] == 0, (what, hints)


# ------------------------------------------------------------------------------------------------------------------------------
# the forms sequences 1 and 2 run through
# ------------------------------------------------------------------------------------------------------------------------------
def _forms():
    out = []
    for pipe in (0, 3, 7):
        for rounds in (1, 2):
            out.append(("bytes", N, (("scan_pipelined", pipe), ("fixed_rounds", rounds))))
    out.append(("bytes", N, (("scan_pipelined", 7), ("fixed_rounds", 2), ("select", 0))))
    out.append(("bytes", 256, (("fixed_rounds", 2), ("row_lists", 1))))
    for lanes in (0, 1):
        for filt in (0, 1, 2):
            for rounds in (1, 2):
                out.append(("float", N, (("lanes", lanes), ("filter", filt), ("fixed_rounds", rounds))))
    out.append(("float", N, (("lanes", 1), ("filter", 2), ("fixed_rounds", 2), ("select", 0))))
    for rounds in (1, 2):
        out.append(("smallint", N, (("fixed_rounds", rounds),)))
    # both dimensions and both metrics, dealt over the forms of every kind in turn
    return [(kind, (24, 128)[i % 2], (1, 0)[(i // 2) % 2], n, opts) for i, (kind, n, opts) in enumerate(out)]


FORMS = _forms()


def form_id(f):
    kind, d, metric, n, opts = f
    return "-".join([kind, f"d{d}", "L2" if metric else "IP", f"n{n}"] + [f"{k}{v}" for k, v in opts])


def through_filter(kind, opts):
    o = dict(opts)
    return kind != "bytes" and o.get("filter", 2) != 0 and o.get("fixed_rounds") == 2


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_light_heavy_light_heavy(capi, expect, form):
    """sequence 1.  "light" probes small lists only (a few dozen items a round), "heavy" big lists only (ten to forty times as
    many).  heavy after light: every scan of the step runs on a grid sized for light's items -- fails if a workgroup ended after its
    first item or tile, or walked with a wrong stride or end.  light after heavy: an oversized grid whose surplus workgroups must
    find nothing, over workspaces that still hold heavy's rows, masks and admission logs -- fails if a kernel read a word this
    search did not write"""
    kind, d, metric, n, opts = form
    h = open_handle(capi, hc.world(kind, d, metric), opts)
    f = (kind, d, metric)
    tag = form_id(form)
    step(h, f, "light", tag, n)
    for rep in range(2):
        hints = step(h, f, "heavy", tag, n)
        too_small(hints, (tag, rep))
        if through_filter(kind, opts):
            assert h.last_filter()[0] >= 1, tag
        if rep == 0:
            hints = step(h, f, "light", tag, n)
            oversized(hints, tag)
            if through_filter(kind, opts):
                assert h.last_filter()[0] >= 1, tag
    h.close()


@pytest.mark.parametrize("form", FORMS, ids=form_id)
def test_spread_crowd_spread(capi, expect, form):
    """sequence 2.  scan_shape_of gives a block of r queries on a list tile shape 1 for r <= 8, 2 for r <= 16, 4 for r <= 32.
    "spread": every list is probed by at most 8 queries (handle_history_cases.spread_lists asserts it), so every item of an fp32
    round has shape 1 and the other shapes' counts are 0.  "crowd": all queries probe the same eight big lists, 160 (256) = 5 (8)
    full blocks of 32 a list: shape 4 only.  crowd after spread: shape 4's hint is 0 under a valid history, its launch is
    resident_grid(1) -- one workgroup a CU, 256 -- for 8 lists x 5 blocks x 13..32 tiles, and must stride; shape 1 gets spread's grid
    and must find nothing.  spread after crowd: the reverse.  Byte lists have one item form: the sequence is a second pair of
    unequal item counts for them.  No counter tells which shape strode; both steps must at least have been sized from history"""
    kind, d, metric, n, opts = form
    h = open_handle(capi, hc.world(kind, d, metric), opts)
    f = (kind, d, metric)
    tag = form_id(form)
    step(h, f, "spread", tag, n)
    hints = step(h, f, "crowd", tag, n)
    assert hints[0] > 0, (tag, hints)
    hints = step(h, f, "spread", tag, n)
    assert hints[0] > 0, (tag, hints)
    h.close()


# one byte form and one float form for sequences 3 to 7
BYTE_FORM = ("bytes", 128, 1, (("fixed_rounds", 2),))
FLOAT_FORM = ("float", 24, 0, (("fixed_rounds", 2),))
FLOAT_FORM_L2 = ("float", 24, 1, (("fixed_rounds", 2),))


def short_id(f):
    return "-".join([f[0], f"d{f[1]}", "L2" if f[2] else "IP"])


@pytest.mark.parametrize("incremental", [1, 0])
@pytest.mark.parametrize("form", [BYTE_FORM, FLOAT_FORM], ids=short_id)
def test_same_call_after_the_lists_changed(capi, expect, form, incremental):
    """sequence 3.  The same queries and keys three times; in between the sixteen probed lists grow about fifty-fold (amd_ivf_add)
    and shrink back (byte form: amd_ivf_remove_ids of the added ids, which all sit at their lists' ends, so every list is what it
    was; float form: amd_ivf_update_lists with the old sizes).  The hint signature does not see the lists: the second search runs
    on the first one's grids, the third on the second one's.  Fails like sequence 1, and if a derived copy of the lists (byte
    fragments, lane order, fp16 / fp32 filter copies) kept rows of the grown lists after they shrank"""
    kind, d, metric, opts = form
    w = hc.world(kind, d, metric)
    h = open_handle(capi, w, (("incremental", incremental),) + opts)
    f = (kind, d, metric)
    tag = (short_id(form), incremental)
    step(h, f, "light", tag)
    rows, ids, lists = hc.growth(kind, d, metric)
    h.add(rows, ids, lists)
    too_small(step(h, f, "light", tag, want=hc.expected_grown(kind, d, metric, "light")), tag)
    if kind == "bytes":
        assert h.remove_ids(ids) == len(ids)
    else:
        h.update_lists(w["sizes"], np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros((0, d), np.float32))
    assert h.ntotal == len(w["xb"])
    oversized(step(h, f, "light", tag), tag)
    h.close()


@pytest.mark.parametrize("form", [BYTE_FORM, FLOAT_FORM], ids=short_id)
def test_store_pairs_and_max_codes_between_steps(capi, expect, form):
    """sequence 4.  store_pairs and max_codes are no part of the signature: a search that returns (list, position) pairs, or stops a
    query's ranking after max_codes vectors (the reference's loop leaves mid-ranking: 300 vectors are less than any big list), runs
    on the grids of the plain search before it, and the plain search after it on theirs"""
    kind, d, metric, opts = form
    h = open_handle(capi, hc.world(kind, d, metric), opts)
    f = (kind, d, metric)
    tag = short_id(form)
    step(h, f, "light", tag)
    too_small(step(h, f, "heavy", tag, store_pairs=True), tag)
    oversized(step(h, f, "light", tag, max_codes=20), tag)
    too_small(step(h, f, "heavy", tag, max_codes=300), tag)
    step(h, f, "heavy", tag)
    step(h, f, "light", tag, store_pairs=True)
    h.close()


def selected_step(h, s, form, name, sel_name, what):
    kind, d, metric = form
    xq, keys, dis = hc.query_set(kind, d, metric, name)
    eD, eI, est = hc.expected_selected(kind, d, metric, name, sel_name)
    _, _, plain = hc.expected(kind, d, metric, name) if name != "wide" else (None, None, None)
    h.stats(reset=True)
    got = h.search_preassigned_selected(s, xq, K, keys, dis)
    st = h.stats()
    hints = h.last_round_hints()
    print("[history]", what, name, sel_name, "hinted/short", hints)
    same(got, (eD, eI), (what, name, sel_name))
    # (as tests/test_gpu_selector.py: the heap updates are the filtered lists', the distances computed the parent's)
    assert st["nheap_updates"] == est[2], (what, name, sel_name)
    if plain is not None:
        assert st["ndis"] == plain[1], (what, name, sel_name)
    return hints


@pytest.mark.parametrize("form", [BYTE_FORM, FLOAT_FORM], ids=short_id)
def test_selected_and_unselected_searches_alternate(capi, expect, form):
    """sequence 5.  A search under a sparse selector (one id in fifty), the plain search of the same shape, searches under a dense
    one (nine in ten): the expected values are the oracle's over the lists with the non-members removed.  Fails if a plain search
    read keep bits the selected one before it left in the mask words, or a selected one missed rows.  The last three steps search 72
    probes a query in one round -- eight real keys and the reference's -1 padding: on a signature without history the keep-bit
    kernel's grid holds 64 rows a query, so the rows of the last eighteen queries are reached only by the stride of its walk"""
    kind, d, metric, opts = form
    w = hc.world(kind, d, metric)
    h = open_handle(capi, w, opts)
    f = (kind, d, metric)
    tag = short_id(form)
    from test_gpu_subset import id_bits
    nwords = (len(w["xb"]) + 63) // 64 + 2
    sels = {nm: h.selector(capi.SUBSET_ID_BITS, 0, 0, id_bits(np.nonzero(hc.selector_members(w, nm))[0], nwords)) for nm in ("sparse", "dense")}
    selected_step(h, sels["sparse"], f, "light", "sparse", tag)
    too_small(step(h, f, "heavy", tag), tag)
    hints = selected_step(h, sels["dense"], f, "heavy", "dense", tag)
    assert hints[0] > 0, (tag, hints)
    oversized(selected_step(h, sels["dense"], f, "light", "dense", tag), tag)
    too_small(selected_step(h, sels["sparse"], f, "heavy", "sparse", tag), tag)
    h.set_option("fixed_rounds", 1)
    selected_step(h, sels["dense"], f, "wide", "dense", tag)
    selected_step(h, sels["sparse"], f, "wide", "sparse", tag)
    selected_step(h, sels["dense"], f, "wide", "dense", tag)
    for s in sels.values():
        s.close()
    h.close()


@pytest.mark.parametrize("form", [BYTE_FORM, FLOAT_FORM], ids=short_id)
def test_owner_and_clone_interleaved(capi, expect, form):
    """sequence 6.  Hints belong to a context, the lists and the row-space history to the index: heavy on the owner, light and then
    heavy on a clone (the clone's grids come from ITS light search: too small), light on the owner (its grids from its own heavy
    one).  Fails if a clone took its hints from the owner's workspace or counters"""
    kind, d, metric, opts = form
    h = open_handle(capi, hc.world(kind, d, metric), opts)
    c = h.clone()
    f = (kind, d, metric)
    tag = short_id(form)
    step(h, f, "heavy", tag)
    step(h, f, "light", tag, on=c)
    too_small(step(h, f, "heavy", tag, on=c), tag)
    oversized(step(h, f, "light", tag), tag)
    c.close()
    h.close()


@pytest.mark.parametrize("form", [BYTE_FORM, FLOAT_FORM_L2], ids=short_id)
def test_tickets_on_one_context(capi, expect, form):
    """sequence 7.  Asynchronous depth 1: one internal context serves every ticket.  Three resident ranges of the same length --
    light, heavy, light -- each ranked by the engine (L2: handle_history_cases.query_set asserts that the reference's ranking of a
    light (heavy) query holds small (big) lists only), each waited for.  The heavy ticket's diagnostics must report hints that were
    too small"""
    kind, d, metric, opts = form
    h = open_handle(capi, hc.world(kind, d, metric), opts)
    allx, want = hc.expected_ranked(kind, d, metric, ("light", "heavy", "light2"))
    h.set_queries(allx)
    h.set_async_depth(1)
    for i, nm in enumerate(("light", "heavy", "light2")):
        D, I, _, diag = h.wait(h.submit_search_resident(i * N, N, K, NPROBE))
        print("[history] tickets", short_id(form), nm, diag)
        same((D, I), want[i], (short_id(form), nm))
        if nm == "heavy":
            assert diag["hinted_launches"] > 0 and diag["short_hints"] > 0, diag
        if nm == "light2":
            assert diag["hinted_launches"] > 0 and diag["short_hints"] == 0, diag
    assert h.scan_arith() == hc.KINDS[kind]
    h.close()


@pytest.mark.parametrize("kind", ["bytes", "float"])
def test_adaptive_easy_hard_easy(capi, expect, kind):
    """sequence 8.  amd_ivf_search_adaptive over three resident ranges of one length: "easy" (stored vectors, require_acc 0.5),
    "hard" (points half way between clusters, 0.99), easy again.  Short rounds ("round_first" 2, "round_grow" 1.5, "round_inc" 2)
    make the hard batch run rounds the easy one before it never planned: beyond the recorded history (no hint at all), and inside it
    with hints far too small; the third batch finds hints for rounds it does not reach.  my_nprobe, D, I, t_recalls and the
    statistics are the oracle's at every step"""
    w = hc.adaptive_world(kind)
    h = capi.Handle(w["d"], hc.A_NLIST, 1, 0)
    for key, value in (("round_first", 2), ("round_grow", 1.5), ("round_inc", 2)):
        h.set_option(key, value)
    h.set_centroids(w["cen"])
    h.set_lists_from_assign(w["xb"], w["assign"])
    h.set_interdis(None)
    h.set_tuner(hc.A_K, w["traces"], capi.arcos_table())
    h.set_queries(w["xq"])
    passes = []
    for stp in range(3):
        eD, eI, est, e_np, e_rec, gtD = hc.expected_adaptive(kind, stp)
        my_np = np.zeros(3 * hc.A_N, dtype=np.uint64)
        t_rec = np.zeros(3 * hc.A_N, dtype=np.float32)
        h.stats(reset=True)
        D, I = h.search_adaptive(stp * hc.A_N, hc.A_N, hc.A_QUERY_TOPK, hc.A_MULTIPLER, hc.A_STD_M, w["req"], my_np, t_rec, gt_D=gtD)
        st = h.stats()
        passes.append(h.last_timing()["rounds"])
        print("[history] adaptive", kind, stp, "passes", passes[-1], "hinted/short", h.last_round_hints(), "nprobe max", int(e_np.max()))
        rows = slice(stp * hc.A_N, (stp + 1) * hc.A_N)
        assert np.array_equal(my_np[rows].astype(np.int64), e_np), (kind, stp)
        same((D, I), (eD, eI), (kind, stp))
        assert np.array_equal(bits(t_rec[rows]), bits(e_rec)), (kind, stp)
        assert [st["nlist"], st["ndis"], st["nheap_updates"]] == list(est), (kind, stp)
        assert h.scan_arith() == w["arith"]
    assert passes[1] > passes[0] and passes[1] > passes[2], passes
    h.close()
