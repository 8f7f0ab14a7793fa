"""The adaptive (error-bounded) search over float lists through MANY filter rounds: scan_filter_kernel / scan_filter_wide_kernel ->
rescore_kernel -> select_sorted_kernel<.., MASKED, TUNE> round after round, with thresholds that move between the rounds and queries
that stop in mid-search, against the pinned CPU oracle.  test_gpu_filter.py and test_gpu_filter_bound.py meet the filter in one
threshold round of a fixed-nprobe search; test_gpu_random_adaptive.py meets the adaptive rule under the default schedule, where
most queries end in the dense round.  Here the round schedule -- which cannot change a result -- is set so that a 64-list index
plans up to 8 rounds (12 at 256 lists) instead of 1 or 2, and every case asserts from the oracle's my_nprobe that it did:
last_filter()[0] >= rounds - 1 and last_timing()["rounds"] >= rounds (adaptive_filter_cases.py: how the schedule in effect is
derived, and why the first round is set through AUNCEL_AMD_FILTER_FIRST beside the "round_first" option).

Every expected value is the oracle's (oracle.search_preassigned(.., tuner=..) over oracle.knn's ranking): my_nprobe, I, the bits
of D and of t_recalls, and [nlist, ndis, nheap_updates].

  1. every filter kernel form under the adaptive rule, 1 / 2 / 4 query blocks an item, both copies the filter streams
  2. four schedules, one result; the filter rounds follow the schedule
  3. bounds mixed per query: stops at 1, 2, 3, 5 and 8 probes in one call; profile, both selections, both stream widths
  4. exact and one-ulp copies spread over the lists: every round meets candidates on or next to the current threshold
  5. rows that all round one way in fp16: the fp16 constant under thresholds that shrink round after round
  6. inner product on unit-norm data; a list shorter than K is the reference's error
  7. the other adaptive entry points over the same rounds
  8. queries without a usable fp16 scale"""
import ctypes as C

import numpy as np
import pytest

import adaptive_filter_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from auncel_amd import capi
    capi.lib()
    return capi


@pytest.fixture(params=[2, 1], ids=["fp16", "fp32"])
def form(request, monkeypatch):
    monkeypatch.setenv("AUNCEL_AMD_FILTER", str(request.param))
    return request.param


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_handle(capi, c):
    h = capi.Handle(c.d, c.nlist, c.metric, 0)
    h.set_centroids(c.cen)
    h.set_lists_from_assign(c.xb, c.assign)
    h.set_interdis(None)
    h.set_tuner(c.K, c.traces, capi.arcos_table())
    h.set_queries(c.xq)
    return h


def set_schedule(h, monkeypatch, schedule):
    first, grow, inc = ac.SCHEDULES[schedule]
    if first is None:
        monkeypatch.delenv("AUNCEL_AMD_FILTER_FIRST", raising=False)
    else:
        monkeypatch.setenv("AUNCEL_AMD_FILTER_FIRST", str(first))  # (the option alone is overridden: adaptive_filter_cases.py)
    for key, v in (("round_first", first), ("round_grow", grow), ("round_inc", inc)):
        h.set_option(key, v)


def adaptive_x(capi, h, c, query_topk, my_np, t_rec, gtD, profile):
    nq = len(c.xq)
    D, I = np.empty((nq, c.K), np.float32), np.empty((nq, c.K), np.int64)
    f32p, u64p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
    xq, req, gt = (np.ascontiguousarray(a, dtype=np.float32) for a in (c.xq, c.req, gtD))
    rc = capi.lib().amd_ivf_search_adaptive_x(
        h._h, C.c_size_t(nq), xq.ctypes.data_as(f32p), C.c_size_t(0), C.c_size_t(query_topk), C.c_float(c.multipler), C.c_float(c.std_m),
        req.ctypes.data_as(f32p), gt.ctypes.data_as(f32p), int(profile), 0, my_np.ctypes.data_as(u64p), t_rec.ctypes.data_as(f32p),
        D.ctypes.data_as(f32p), I.ctypes.data_as(i64p))
    if rc != 0:
        raise capi.EngineError(rc, capi.lib().amd_ivf_last_error().decode())
    return D, I


def run_and_compare(capi, oracle, monkeypatch, key, c, query_topk, schedule="one_probe", profile=False, entry="resident", h=None):
    """one adaptive call under `schedule` against the oracle -> (filter rounds, planning passes, the floor of the latter)"""
    ref = ac.reference(oracle, capi.arcos_table(), key, c, query_topk, profile)
    nq = len(c.xq)
    own = h is None
    if own:
        h = make_handle(capi, c)
    set_schedule(h, monkeypatch, schedule)
    my_np, t_rec = np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.float32)
    h.stats(reset=True)
    if entry == "resident":
        D, I = h.search_adaptive(0, nq, query_topk, c.multipler, c.std_m, c.req, my_np, t_rec, gt_D=ref.gtD, profile=profile)
    elif entry == "host":
        D, I = adaptive_x(capi, h, c, query_topk, my_np, t_rec, ref.gtD, profile)
    else:
        D, I = h.search_adaptive_pre(c.xq, 0, ref.ck, ref.cd, query_topk, c.multipler, c.std_m, c.req, my_np, t_rec, gt_D=ref.gtD,
                                     profile=profile)
    launches, kept = h.last_filter()
    passes = int(h.last_timing()["rounds"])
    st = h.stats()
    floor = ac.rounds_floor(schedule, c.K, c.sizes, c.nlist, ref.my_nprobe)
    tag = (key, query_topk, schedule, entry, profile)
    bad = np.nonzero((I != ref.I).any(axis=1) | (bits(D) != bits(ref.D)).any(axis=1))[0]
    print(tag, "filter rounds", launches, "kept", kept, "planning passes", passes, "floor", floor, "wrong queries", bad.size)
    assert np.array_equal(my_np.astype(np.int64), ref.my_nprobe), tag
    assert np.array_equal(I, ref.I), (tag, "queries", bad[:8])
    assert np.array_equal(bits(D), bits(ref.D)), (tag, "queries", bad[:8])
    assert np.array_equal(bits(t_rec), bits(ref.t_recalls)), tag
    assert [st["nlist"], st["ndis"], st["nheap_updates"]] == ref.stats, tag
    assert passes >= floor, (tag, "the call planned fewer rounds than its last query needs")
    assert launches >= floor - 1, (tag, "rounds behind the first did not go through the filter")
    if own:
        h.close()
    return launches, passes, floor


# ------------------------------------------------------------------------------------------ 1. every filter kernel form
def check_forms(capi, oracle, monkeypatch, d, query_topk):
    most = 0
    for layout in range(len(ac.FORM_LAYOUTS)):
        _, _, floor = run_and_compare(capi, oracle, monkeypatch, ("form", d, layout), ac.form_case(d, layout), query_topk)
        most = max(most, floor)
    assert most >= 8  # (6 or more planning passes: the cases are built to reach nlist / 8 = 8)


@pytest.mark.parametrize("query_topk", [1, 10])
@pytest.mark.parametrize("d", ac.FORM_D)
def test_every_filter_form_under_the_adaptive_rule(capi, oracle, monkeypatch, form, d, query_topk):
    check_forms(capi, oracle, monkeypatch, d, query_topk)


@pytest.mark.parametrize("query_topk", [1, 10])
@pytest.mark.parametrize("d", ac.FORM_NARROW_D)
def test_the_one_wave_form_under_the_adaptive_rule(capi, oracle, monkeypatch, form, d, query_topk):
    monkeypatch.setenv("AUNCEL_AMD_FILTER_NARROW", "1")
    check_forms(capi, oracle, monkeypatch, d, query_topk)


# ------------------------------------------------------------------------------------------ 2. schedule invariance
@pytest.mark.parametrize("metric", [ac.L2, ac.IP])
def test_the_schedule_changes_the_rounds_and_nothing_else(capi, oracle, monkeypatch, metric):
    """the default schedule, one probe a round, 3 probes then doubling, one large round: each equals the oracle, so all are equal;
    the rounds run are what the schedule says -- at least the floor, and never as many as the next finer schedule's floor allows
    to tell apart (rounds are enqueued two at a time, so a call may run one more than it needs)"""
    c = ac.schedule_case(metric)
    h = make_handle(capi, c)
    seen = {}
    for schedule in ("default", "one_probe", "three_two", "one_round"):
        seen[schedule] = run_and_compare(capi, oracle, monkeypatch, ("schedule", metric), c, 10, schedule=schedule, h=h)
    h.close()
    floors = {s: v[2] for s, v in seen.items()}
    assert floors["one_probe"] >= 8 and floors["three_two"] == 3 and floors["one_round"] == 1
    assert seen["one_probe"][0] > seen["three_two"][0] >= seen["one_round"][0]
    assert seen["one_round"][0] <= 1 and seen["one_round"][1] <= 2  # (nothing left after the one round, and its speculative second)
    assert seen["three_two"][0] <= floors["three_two"] + 1


# ------------------------------------------------------------------------------------------ 3. queries that stop at different rounds
@pytest.mark.parametrize("profile", [False, True])
@pytest.mark.parametrize("select", ["sorted", "heap"])
@pytest.mark.parametrize("nld", ["16", "32"])
def test_queries_stop_at_different_rounds_of_one_call(capi, oracle, monkeypatch, nld, select, profile):
    monkeypatch.setenv("AUNCEL_AMD_REPLAY_NLD", nld)
    monkeypatch.setenv("AUNCEL_AMD_SELECT", select)
    _, _, floor = run_and_compare(capi, oracle, monkeypatch, "mixed", ac.mixed_case(), 10, profile=profile)
    assert floor == ac.MIXED_NLIST // 8


# ------------------------------------------------------------------------------------------ 4. thresholds that shrink onto candidates
@pytest.mark.parametrize("d", ac.COPIES_D)
def test_thresholds_shrink_onto_exact_and_one_ulp_copies(capi, oracle, monkeypatch, d):
    _, _, floor = run_and_compare(capi, oracle, monkeypatch, ("copies", d), ac.copies_case(d), ac.COPIES_K)
    assert floor == ac.COPIES_NLIST // 8


# ------------------------------------------------------------------------------------------ 5. the bound under shrinking thresholds
@pytest.mark.parametrize("d", ac.BOUND_D)
def test_the_fp16_bound_under_shrinking_thresholds(capi, oracle, monkeypatch, d):
    """the fp16 copy (the default); test_adaptive_filter_cases_cpu.py holds that the fp32 form's constant behind the same keep rule
    drops, in every round from the second on, entries the heap admits"""
    monkeypatch.setenv("AUNCEL_AMD_FILTER", "2")
    _, _, floor = run_and_compare(capi, oracle, monkeypatch, ("bound", d), ac.bound_case(d), ac.BOUND_K)
    assert floor == ac.BOUND_NLIST // 8


def test_the_fp16_bound_in_the_one_wave_form(capi, oracle, monkeypatch):
    monkeypatch.setenv("AUNCEL_AMD_FILTER", "2")
    monkeypatch.setenv("AUNCEL_AMD_FILTER_NARROW", "1")
    run_and_compare(capi, oracle, monkeypatch, ("bound", 136), ac.bound_case(136), ac.BOUND_K)


# ------------------------------------------------------------------------------------------ 6. inner product
@pytest.mark.parametrize("query_topk", ["one", "K"])
@pytest.mark.parametrize("d,K", ac.IP_CASES)
def test_inner_product_on_unit_norm_data(capi, oracle, monkeypatch, d, K, query_topk):
    run_and_compare(capi, oracle, monkeypatch, ("ip", d, K), ac.ip_case(d, K), 1 if query_topk == "one" else K)


def test_a_list_shorter_than_k_is_the_references_error(capi, oracle, monkeypatch):
    c = ac.ip_case(64, 10, True)
    with pytest.raises(RuntimeError):
        ac.reference(oracle, capi.arcos_table(), "ip short", c, 10)
    gtD, _ = oracle.knn(c.metric, c.xq, c.xb, c.K, nthreads=8)
    h = make_handle(capi, c)
    set_schedule(h, monkeypatch, "one_probe")
    nq = len(c.xq)
    with pytest.raises(capi.EngineError):
        h.search_adaptive(0, nq, 10, c.multipler, c.std_m, c.req, np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.float32), gt_D=gtD)
    h.close()


# ------------------------------------------------------------------------------------------ 7. the other entry points
@pytest.mark.parametrize("entry", ["resident", "host", "pre"])
def test_the_adaptive_entry_points_run_the_same_rounds(capi, oracle, monkeypatch, entry):
    _, _, floor = run_and_compare(capi, oracle, monkeypatch, "entry", ac.entry_case(), 10, entry=entry, profile=True)
    assert floor == 8


def test_two_tickets_over_adjacent_resident_ranges(capi, oracle, monkeypatch):
    """submit_adaptive / wait: the halves of the resident queries as two searches in flight equal the oracle's rows of the whole
    call.  (A ticket reports its planning passes; the filter rounds of the engine's own contexts are not readable from the handle.)"""
    c = ac.entry_case()
    ref = ac.reference(oracle, capi.arcos_table(), "entry", c, 10, True)
    nq = len(c.xq)
    cut = nq // 2 + 3
    h = make_handle(capi, c)
    set_schedule(h, monkeypatch, "one_probe")
    my_np, t_rec = np.zeros(nq, dtype=np.uint64), np.zeros(nq, dtype=np.float32)
    h.stats(reset=True)
    tickets = [h.submit_adaptive(a, b - a, 10, c.multipler, c.std_m, c.req, my_np, t_rec, gt_D=ref.gtD, profile=True)
               for a, b in ((0, cut), (cut, nq))]
    for t, (a, b) in zip(tickets, ((0, cut), (cut, nq))):
        D, I, timing, _ = h.wait(t)
        floor = ac.rounds_floor("one_probe", c.K, c.sizes, c.nlist, ref.my_nprobe[a:b])
        print("ticket", (a, b), "planning passes", timing["rounds"], "floor", floor)
        assert np.array_equal(I, ref.I[a:b]) and np.array_equal(bits(D), bits(ref.D[a:b])), (a, b)
        assert timing["rounds"] >= floor >= 8
    assert np.array_equal(my_np.astype(np.int64), ref.my_nprobe)
    assert np.array_equal(bits(t_rec), bits(ref.t_recalls))
    st = h.stats()
    assert [st["nlist"], st["ndis"], st["nheap_updates"]] == ref.stats
    h.close()


# ------------------------------------------------------------------------------------------ 8. scale edge
def test_queries_without_a_usable_fp16_scale(capi, oracle, monkeypatch, form):
    _, _, floor = run_and_compare(capi, oracle, monkeypatch, "scale", ac.scale_case(), 10)
    assert floor == 8
