"""The grid axis of the full-panel passes on the device: every constructed case of tests/grid_cases.py (grid counts around the
64-grid blocks, renormalisation placed grid by grid, no-variant runs, grids with specials, thinned columns at the ends and across
a block edge, planted ties) through every kernel family that accepts it, against the fp64 CPU oracle.

Each family is held to the bar the suite already holds it to:

  * fp32 state (default handle; single-pass entry and qa_fullpass_batch): dosage 2e-4, c rtol 1e-4, alpha / beta / gamma as
    test_dosage_pass_matches_oracle states them, lists identical; the oracle under always_normalize = True
  * k_fwd64 + k_bwd64 + k_topk (thin pass; single-pass entry and qa_fullpass_batch): lists identical with values to 1e-9, c and
    alpha at the thinned grids rtol 1e-9 (test_headline_gpu.py)
  * k_fwd64 + k_bwd64d (qa_panel_set_dosage_precision(64); dosage-only call and qa_fullpass_batch): dosage 1e-10, c rtol 1e-12
    (test_fp64_dosage_kernels_match_oracle)
  * the picker fused into k_bwd64 (HipBackend.fullpass_reads_batch at top_width = K_top, 8 and 64, and the select= form): `top`
    with its order and `cnt` identical to tests.oracle_backend.OracleBackend on the same reads; the float `top_val` is the
    rounding of the oracle's value, 2.4e-7 relative (one float rounding, 6e-8, of a value that agrees to 1e-9)
  * validation mode (qa_panel_set_sum_order(1); single-pass entry): bit-identical, as test_validation_mode_headline_size

tests/test_grid_cases_cpu.py holds every case to a separation of 1e-6 between unequal gammas among the ranks compared here, so no
comparison branches on the device's result, and nothing is skipped."""
import ctypes as C

import numpy as np
import pytest

from tests import grid_cases as GC
from tests.fullpass_calls import batch as _batch, lists_equal as _lists_equal, single as _single
from tests.util import check_best_haps

pytestmark = pytest.mark.gpu

NAMES = GC.case_names()
TIE_NAMES = [c.name for c in GC.all_cases() if "list_len" in c.claims]
DOSAGE_ATOL = 2e-4
MIN_GL = GC.MIN_GL


@pytest.fixture(scope="module")
def device_panel():
    """One device panel per host panel, for the whole module."""
    from quilt_amd.native import DevicePanel
    held = {}

    def get(panel):
        if id(panel) not in held:
            held[id(panel)] = DevicePanel(panel)
        return held[id(panel)]
    yield get
    for dev in held.values():
        dev.close()


@pytest.mark.parametrize("from_rhb", [False, True])
def test_one_grid_panel_needs_no_transition_matrix(from_rhb, device_panel):
    """nGrids == 1: transMatRate_t is 2 x 0 (include/quilt_amd.h), and a C caller's empty array may be NULL -- both panel
    constructors take it, and the passes give what they give with numpy's empty array, bit for bit."""
    import copy
    from quilt_amd.native import DevicePanel
    c = GC.case("grids_G1_T32_dh8")
    bare = copy.copy(c.panel)
    bare.transMatRate_t = None
    dev = DevicePanel.from_rhb(bare, nMaxDH=c.panel.nMaxDH) if from_rhb else DevicePanel(bare)
    try:
        for kw in (dict(dosage=True), dict(dosage=False, alpha=True)):
            want, got = _single(device_panel(c.panel), c, **kw), _single(dev, c, **kw)
            assert np.array_equal(got["c"], want["c"]) and _lists_equal(got["best_haps_stuff_list"], want["best_haps_stuff_list"])
            if kw["dosage"]:
                assert np.array_equal(got["dosage"], want["dosage"])
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 state
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fp32_state_passes(name, device_panel):
    c = GC.case(name)
    dev = device_panel(c.panel)
    ref = GC.oracle_ref(c, "full")
    got = _single(dev, c, dosage=True, alpha=True, gamma=True, beta=True, always_normalize=True)
    assert np.abs(got["dosage"] - ref["dosage"]).max() <= DOSAGE_ATOL
    np.testing.assert_allclose(got["gamma_t"].sum(axis=0), 1.0, atol=1e-4)
    np.testing.assert_allclose(got["gamma_t"], ref["gamma_t"], atol=2e-5, rtol=2e-3)
    np.testing.assert_allclose(got["alphaHat_t"], ref["alphaHat_t"], atol=1e-6, rtol=2e-3)
    np.testing.assert_allclose(got["betaHat_t"], ref["betaHat_t"], atol=1e-30, rtol=2e-3)
    np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-4)
    check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
    # the batched entry: the same kernels without the K x G outputs, the lists from the ranking passes beside them
    lazy = GC.oracle_ref(c, "dosage")
    dosage, lists = _batch(dev, [c], [1])
    assert np.abs(dosage[0] - lazy["dosage"]).max() <= DOSAGE_ATOL
    check_best_haps(lists[0], lazy["best_haps"])


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 ranking passes: k_fwd64 + k_bwd64 + k_topk
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_ranking_passes(name, device_panel):
    c = GC.case(name)
    dev = device_panel(c.panel)
    ref = GC.oracle_ref(c, "thin", 1, c.always_normalize)
    got = _single(dev, c, dosage=False, alpha=True, always_normalize=c.always_normalize)
    check_best_haps(got["best_haps_stuff_list"], ref["best_haps"], exact=True)
    np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-9)
    for g in c.thin_grids:
        np.testing.assert_allclose(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g], rtol=1e-9, atol=1e-300)
    if "list_len" in c.claims:
        assert {len(e["top_matches"]) for e in got["best_haps_stuff_list"]} == {c.claims["list_len"]}
    _, lists = _batch(dev, [c], [0])
    check_best_haps(lists[0], GC.oracle_ref(c, "thin")["best_haps"], exact=True)


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 dosage passes: k_fwd64 + k_bwd64d
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fp64_dosage_passes(name, device_panel):
    c = GC.case(name)
    dev = device_panel(c.panel)
    dev.set_dosage_precision(64)
    try:
        ref = GC.oracle_ref(c, "dosage", 1, c.always_normalize)
        got = _single(dev, c, dosage=True, always_normalize=c.always_normalize)   # no K x G output: the dosage-only call
        assert np.abs(got["dosage"] - ref["dosage"]).max() <= 1e-10
        np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-12)
        check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
        lazy = GC.oracle_ref(c, "dosage")
        dosage, lists = _batch(dev, [c], [1])
        assert np.abs(dosage[0] - lazy["dosage"]).max() <= 1e-10
        check_best_haps(lists[0], lazy["best_haps"])
    finally:
        dev.set_dosage_precision(32)


# ---------------------------------------------------------------------------------------------------------------------------
# the picker fused into k_bwd64
# ---------------------------------------------------------------------------------------------------------------------------
def _reads_args(c):
    """Two chains on the case's sample: chain 0 wants dosages and lists, chain 1 lists alone."""
    return dict(samples=[c.sample], chain_sample=[0, 0], labels=[c.labels, c.labels], want_dosage=[1, 0], want_top=[1, 1])


def _reads_raw(dev, c, width):
    """qa_fullpass_reads_batch itself: top_idx, top_val (float) and the counts."""
    from quilt_amd.impute import flatten_samples
    from quilt_amd.native import check, lib, ptr
    a = _reads_args(c)
    n_chain, n_label, n_thin = 2, 2, len(c.thin_grids)
    read_off, read_ptr, u, bq, _ = flatten_samples(a["samples"], wif=False)
    H = np.concatenate([np.asarray(h, dtype=np.int32) for h in a["labels"]])
    cs, wd, wt = (np.array(a[k], dtype=np.int32) for k in ("chain_sample", "want_dosage", "want_top"))
    dosage = np.zeros((n_chain, n_label, c.panel.nSNPs))
    top = np.full((n_chain, n_label, n_thin, width), -1, dtype=np.int32)
    val = np.zeros((n_chain, n_label, n_thin, width), dtype=np.float32)
    cnt = np.zeros((n_chain, n_label, n_thin), dtype=np.int32)
    check(lib().qa_fullpass_reads_batch(dev.handle, C.c_int32(n_chain), C.c_int32(n_label), C.c_int32(1), ptr(cs), ptr(read_off),
                                        ptr(read_ptr), ptr(u), ptr(bq), ptr(H), ptr(wd), ptr(wt), ptr(c.cols), C.c_int32(c.K_top),
                                        C.c_double(MIN_GL), ptr(dosage), C.c_int32(width), ptr(top), ptr(val), ptr(cnt)))
    return dosage, top, val, cnt


@pytest.mark.parametrize("name,width", [(c.name, w) for c in GC.all_cases() for w in c.widths])   # K_top, 8 and 64, each once
def test_fused_picker(name, width, device_panel):
    from quilt_amd.driver import HipBackend
    from tests.oracle_backend import OracleBackend
    c = GC.case(name)
    dev = device_panel(c.panel)
    a = _reads_args(c)
    ref_dosage, ref_top, ref_cnt = OracleBackend(c.panel).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"],
                                                                              a["want_dosage"], a["want_top"], c.cols, c.K_top, MIN_GL,
                                                                              width)
    dosage, top, cnt = HipBackend(dev).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"], a["want_dosage"],
                                                            a["want_top"], c.cols, c.K_top, MIN_GL, width)
    assert np.array_equal(cnt, ref_cnt)
    assert np.array_equal(top, ref_top), "the ordered head of every list, order included"
    assert np.abs(dosage[0] - ref_dosage[0]).max() <= DOSAGE_ATOL
    if c.claims.get("no_reads"):   # every haplotype ties: all of them counted, the head is haplotypes 0, 1, 2 ...
        assert (cnt[:, 0, :] == c.panel.K).all() and (top[:, 0, :, :] == np.arange(width)).all()
    # the entry itself, for the values: the float rounding of the oracle's
    _, top2, val, cnt2 = _reads_raw(dev, c, width)
    assert np.array_equal(top2, ref_top) and np.array_equal(cnt2, ref_cnt)
    for label in (1, 2):
        for j, (idx, v) in enumerate(GC.oracle_ref(c, "thin", label)["best_haps"]):
            order = np.argsort(-v, kind="stable")[:width]
            for chain in (0, 1):
                np.testing.assert_allclose(val[chain, label - 1, j, :len(order)], v[order].astype(np.float32), rtol=2.4e-7, atol=0)
                assert (val[chain, label - 1, j, len(order):] == 0).all()


@pytest.mark.parametrize("name", TIE_NAMES)
def test_fused_picker_feeds_the_device_selection(name, device_panel):
    """The select= form: the fused picker's lists stay on the device and k_select draws the next small panel from them -- the
    panel the host function draws from the ORACLE's lists."""
    from quilt_amd.driver import everything_select_good_haps_dense, previously_selected
    c = GC.case(name)
    K = c.panel.K
    # sizes the few thinned grids can fill: two labels x 3 or 4 grids x K_top ranks hold 7 to 16 distinct haplotypes, so the host
    # selection COMPLETES for every case (it raises otherwise, and the test fails): nxt is compared everywhere
    Ksubset = min(10, K)
    Knew = min(4 if c.K_top > 1 else 2, max(1, Ksubset - 1))
    ref_top, which, seeds, nxt, status = _select_both(c, device_panel(c.panel), Ksubset, Knew)
    for ch in range(2):
        prev = previously_selected(which[ch], Ksubset - Knew, seeds[ch])
        sel = everything_select_good_haps_dense(Knew, c.K_top, ref_top[ch].astype(np.int64) + 1, prev, K, seeds[ch], truncated=True)
        assert len(sel) == Knew and status[ch] == 0
        assert np.array_equal(nxt[ch], np.concatenate([prev, sel]))


def _select_both(c, dev, Ksubset, Knew):
    """The oracle backend's lists, and the device selection behind the fused picker on the same reads."""
    from quilt_amd.driver import HipBackend
    from tests.oracle_backend import OracleBackend
    K, width = c.panel.K, max(c.K_top, 8)
    a = _reads_args(c)
    a["want_dosage"] = [0, 0]
    rng = np.random.default_rng(5)
    which = [np.sort(rng.choice(K, Ksubset, replace=False) + 1).astype(np.int32) for _ in range(2)]
    seeds = [int(rng.integers(0, 2 ** 63)) for _ in range(2)]
    _, ref_top, ref_cnt = OracleBackend(c.panel).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"], a["want_dosage"],
                                                                      a["want_top"], c.cols, c.K_top, MIN_GL, width)
    _, none, cnt, nxt, status = HipBackend(dev).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"], a["want_dosage"],
                                                                     a["want_top"], c.cols, c.K_top, MIN_GL, width,
                                                                     select=dict(Ksubset=Ksubset, Knew=Knew, which=which, seeds=seeds))
    assert none is None and np.array_equal(cnt, ref_cnt)
    return ref_top, which, seeds, nxt, status


def test_fused_picker_lists_too_short_for_the_selection(device_panel):
    """Knew = 20 from lists that hold 11 distinct haplotypes: the host raises, the device hands both chains back (status 1)."""
    from quilt_amd.driver import ListsTruncated, everything_select_good_haps_dense, previously_selected
    c = GC.case("tie_m6")
    ref_top, which, seeds, nxt, status = _select_both(c, device_panel(c.panel), 40, 20)
    assert len(set(ref_top[ref_top >= 0].tolist())) < 20
    for ch in range(2):
        with pytest.raises(ListsTruncated):
            everything_select_good_haps_dense(20, c.K_top, ref_top[ch].astype(np.int64) + 1, previously_selected(which[ch], 20, seeds[ch]),
                                              c.panel.K, seeds[ch], truncated=True)
        assert status[ch] == 1


# ---------------------------------------------------------------------------------------------------------------------------
# validation mode
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_validation_mode(name, device_panel):
    c = GC.case(name)
    dev = device_panel(c.panel)
    dev.set_sum_order(True)
    try:
        ref = GC.oracle_ref(c, "thin", 1, c.always_normalize)
        got = _single(dev, c, dosage=False, alpha=True, always_normalize=c.always_normalize)
        assert np.array_equal(got["c"], ref["c"])
        assert len(got["best_haps_stuff_list"]) == len(ref["best_haps"])
        for e, (oi, ov) in zip(got["best_haps_stuff_list"], ref["best_haps"]):
            assert np.array_equal(e["top_matches"], oi) and np.array_equal(e["top_matches_values"], ov)
        for g in c.thin_grids:
            assert np.array_equal(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g])
        refd = GC.oracle_ref(c, "dosage", 1, c.always_normalize)
        gotd = _single(dev, c, dosage=True, always_normalize=c.always_normalize)
        assert np.array_equal(gotd["dosage"], refd["dosage"]) and np.array_equal(gotd["c"], refd["c"])
        for e, (oi, ov) in zip(gotd["best_haps_stuff_list"], refd["best_haps"]):
            assert np.array_equal(e["top_matches"], oi) and np.array_equal(e["top_matches_values"], ov)
    finally:
        dev.set_sum_order(False)


# ---------------------------------------------------------------------------------------------------------------------------
# several cases in one qa_fullpass_batch call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64_dosage", [False, True])
@pytest.mark.parametrize("group", sorted(GC.groups()))
def test_batch_equals_one_at_a_time(group, fp64_dosage, device_panel):
    """Different passes in one call, dosage and thin mixed: the grid loop is per pass, but the flush of c and the picker's
    scratch are indexed by the pass -- every pass must come out as it does alone, bit for bit."""
    cases = GC.groups()[group]
    dev = device_panel(cases[0].panel)
    want = [int(i % 3 != 1) for i in range(len(cases))]   # dosage, thin, dosage, dosage, thin ...
    assert 0 < sum(want) < len(want)
    if fp64_dosage:
        dev.set_dosage_precision(64)
    try:
        dosage, lists = _batch(dev, cases, want)
        for i, c in enumerate(cases):
            d1, l1 = _batch(dev, [c], [want[i]])
            assert np.array_equal(dosage[i], d1[0]), c.name
            assert _lists_equal(lists[i], l1[0]), c.name
            check_best_haps(lists[i], GC.oracle_ref(c, "thin")["best_haps"])
            if want[i]:
                assert np.abs(dosage[i] - GC.oracle_ref(c, "dosage")["dosage"]).max() <= (1e-10 if fp64_dosage else DOSAGE_ATOL)
    finally:
        if fp64_dosage:
            dev.set_dosage_precision(32)
