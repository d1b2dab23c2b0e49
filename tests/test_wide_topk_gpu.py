"""K_top_matches in 9 .. 64 on the device: every constructed case of tests/wide_topk_cases.py through every kernel family, each at
the bar tests/test_grid_geometry_gpu.py holds that family to, against the fp64 CPU oracle.  Beyond kMaxTop = 8 every family's
lists come from the wide form of k_topk (csrc/fullpass.hip) -- k_topk<double, true> behind the fp64 ranking, fp64 dosage and
validation kernels, k_topk<float, true> behind the fp32-state passes of qa_panel_set_ranking_precision(32); the picker fused into
k_bwd64 keeps K_top <= 8, which the last test holds to what it was.

tests/test_wide_topk_cases_cpu.py holds every case to a separation of 1e-6 between unequal gammas among the ranks compared here,
so no comparison branches on the device's result, and nothing is skipped."""
import ctypes as C

import numpy as np
import pytest

from tests import grid_cases as GC
from tests import mode_matrix as MM
from tests import wide_topk_cases as WC
from tests.test_grid_geometry_gpu import (DOSAGE_ATOL, MIN_GL, _batch, _lists_equal, _reads_args, _reads_raw, _single,
                                          device_panel)   # noqa: F401  (device_panel: the module's fixture, one device panel per host panel)
from tests.util import check_best_haps

pytestmark = pytest.mark.gpu

NAMES = WC.case_names()
TIE_NAMES = [f"tie_m{m}_ktop{k}" for m, k in WC.TIES]
MATRIX_K_MAX = 57344   # include/quilt_amd.h: the K x nGrids outputs of the production kernels end here (validation mode: any K)


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 state (default handle): the dosage from the fp32 kernels, the lists from the fp64 ranking passes beside them
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fp32_state_passes(name, device_panel):
    c = WC.case(name)
    dev = device_panel(c.panel)
    ref = GC.oracle_ref(c, "full")
    matrices = c.panel.K <= MATRIX_K_MAX
    got = _single(dev, c, dosage=True, alpha=matrices, gamma=matrices, beta=matrices, always_normalize=True)
    assert np.abs(got["dosage"] - ref["dosage"]).max() <= DOSAGE_ATOL
    np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-4)
    if matrices:
        np.testing.assert_allclose(got["gamma_t"], ref["gamma_t"], atol=2e-5, rtol=2e-3)
        np.testing.assert_allclose(got["alphaHat_t"], ref["alphaHat_t"], atol=1e-6, rtol=2e-3)
    check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
    lazy = GC.oracle_ref(c, "dosage")
    dosage, lists = _batch(dev, [c], [1])
    assert np.abs(dosage[0] - lazy["dosage"]).max() <= DOSAGE_ATOL
    check_best_haps(lists[0], lazy["best_haps"])


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 ranking passes: k_fwd64 + k_bwd64 + k_topk<double, true>
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_ranking_passes(name, device_panel):
    c = WC.case(name)
    dev = device_panel(c.panel)
    ref = GC.oracle_ref(c, "thin")
    alpha = c.panel.K <= MATRIX_K_MAX
    got = _single(dev, c, dosage=False, alpha=alpha)
    check_best_haps(got["best_haps_stuff_list"], ref["best_haps"], exact=True)
    np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-9)
    for g in c.thin_grids if alpha else ():
        np.testing.assert_allclose(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g], rtol=1e-9, atol=1e-300)
    if "list_len" in c.claims:
        assert {len(e["top_matches"]) for e in got["best_haps_stuff_list"]} == {c.claims["list_len"]}
    _, lists = _batch(dev, [c], [0])
    check_best_haps(lists[0], ref["best_haps"], exact=True)


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 dosage passes: k_fwd64 + k_bwd64d, the lists from the ranking passes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fp64_dosage_passes(name, device_panel):
    c = WC.case(name)
    dev = device_panel(c.panel)
    dev.set_dosage_precision(64)
    try:
        ref = GC.oracle_ref(c, "dosage")
        got = _single(dev, c, dosage=True)
        assert np.abs(got["dosage"] - ref["dosage"]).max() <= 1e-10
        np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-12)
        check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
        dosage, lists = _batch(dev, [c], [1])
        assert np.abs(dosage[0] - ref["dosage"]).max() <= 1e-10
        check_best_haps(lists[0], ref["best_haps"])
    finally:
        dev.set_dosage_precision(32)


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 ranking precision: k_topk<float, true>
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fp32_ranking_precision(name, device_panel):
    c = WC.case(name)
    dev = device_panel(c.panel)
    dev.set_ranking_precision(32)
    try:
        ref = GC.oracle_ref(c, "dosage")
        got = _single(dev, c, dosage=True)
        assert np.abs(got["dosage"] - ref["dosage"]).max() <= DOSAGE_ATOL
        check_best_haps(got["best_haps_stuff_list"], ref["best_haps"], exact=False)
        _, lists = _batch(dev, [c], [0])
        check_best_haps(lists[0], GC.oracle_ref(c, "thin")["best_haps"], exact=False)
    finally:
        dev.set_ranking_precision(64)


# ---------------------------------------------------------------------------------------------------------------------------
# the reads entry: the ordered head of every list
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,width", [(c.name, w) for c in WC.all_cases() for w in sorted({c.K_top, 64})])
def test_reads_entry(name, width, device_panel):
    from quilt_amd.driver import HipBackend
    from tests.oracle_backend import OracleBackend
    c = WC.case(name)
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
    _, top2, val, cnt2 = _reads_raw(dev, c, width)
    assert np.array_equal(top2, ref_top) and np.array_equal(cnt2, ref_cnt)
    for label in (1, 2):
        for j, (idx, v) in enumerate(GC.oracle_ref(c, "thin", label)["best_haps"]):
            order = np.argsort(-v, kind="stable")[:width]
            for chain in (0, 1):
                np.testing.assert_allclose(val[chain, label - 1, j, :len(order)], v[order].astype(np.float32), rtol=2.4e-7, atol=0)
                assert (val[chain, label - 1, j, len(order):] == 0).all()


def _completes(c, ref_top, which, seeds, Ksubset, Knew, K_top):
    from quilt_amd.driver import ListsTruncated, everything_select_good_haps_dense, previously_selected
    try:
        for ch in range(2):
            everything_select_good_haps_dense(Knew, K_top, ref_top[ch].astype(np.int64) + 1,
                                              previously_selected(which[ch], Ksubset - Knew, seeds[ch]), c.panel.K, seeds[ch], truncated=True)
        return True
    except ListsTruncated:
        return False


def _selection_size(c, ref_top, which, seeds, Ksubset):
    """The largest Knew that the ORACLE's lists fill for both chains at the case's K_top and do NOT fill within eight ranks (searched
    on the host function alone; no such Knew: the case shows nothing, and the test fails)."""
    for Knew in range(Ksubset - 1, 0, -1):
        if _completes(c, ref_top, which, seeds, Ksubset, Knew, c.K_top) and not _completes(c, ref_top, which, seeds, Ksubset, Knew, GC.KMAXTOP):
            return Knew
    raise AssertionError("every Knew the lists fill is filled by ranks 1 .. 8")


@pytest.mark.parametrize("name", TIE_NAMES)
def test_wide_lists_feed_the_device_selection(name, device_panel):
    """The select= form: k_select draws the next small panel from the wide lists on the device -- the panel the host function draws
    from the ORACLE's lists, at a Knew the ranks up to 8 cannot fill."""
    from quilt_amd.driver import HipBackend, everything_select_good_haps_dense, previously_selected
    from tests.oracle_backend import OracleBackend
    c = WC.case(name)
    K, Ksubset, width = c.panel.K, 100, c.K_top
    a = dict(_reads_args(c), want_dosage=[0, 0])
    rng = np.random.default_rng(5)
    which = [np.sort(rng.choice(K, Ksubset, replace=False) + 1).astype(np.int32) for _ in range(2)]
    seeds = [int(rng.integers(0, 2 ** 63)) for _ in range(2)]
    _, ref_top, ref_cnt = OracleBackend(c.panel).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"], a["want_dosage"],
                                                                      a["want_top"], c.cols, c.K_top, MIN_GL, width)
    Knew = _selection_size(c, ref_top, which, seeds, Ksubset)
    _, none, cnt, nxt, status = HipBackend(device_panel(c.panel)).fullpass_reads_batch(
        a["samples"], a["chain_sample"], a["labels"], a["want_dosage"], a["want_top"], c.cols, c.K_top, MIN_GL, width,
        select=dict(Ksubset=Ksubset, Knew=Knew, which=which, seeds=seeds))
    assert none is None and np.array_equal(cnt, ref_cnt)
    for ch in range(2):
        prev = previously_selected(which[ch], Ksubset - Knew, seeds[ch])
        sel = everything_select_good_haps_dense(Knew, c.K_top, ref_top[ch].astype(np.int64) + 1, prev, K, seeds[ch], truncated=True)
        assert len(sel) == Knew and status[ch] == 0
        assert np.array_equal(nxt[ch], np.concatenate([prev, sel]))


# ---------------------------------------------------------------------------------------------------------------------------
# validation mode: bit-identical
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_validation_mode(name, device_panel):
    c = WC.case(name)
    dev = device_panel(c.panel)
    dev.set_sum_order(True)
    try:
        ref = GC.oracle_ref(c, "thin")
        got = _single(dev, c, dosage=False, alpha=True)
        assert np.array_equal(got["c"], ref["c"])
        assert len(got["best_haps_stuff_list"]) == len(ref["best_haps"])
        for e, (oi, ov) in zip(got["best_haps_stuff_list"], ref["best_haps"]):
            assert np.array_equal(e["top_matches"], oi) and np.array_equal(e["top_matches_values"], ov)
        for g in c.thin_grids:
            assert np.array_equal(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g])
    finally:
        dev.set_sum_order(False)


# ---------------------------------------------------------------------------------------------------------------------------
# several passes in one qa_fullpass_batch call
# ---------------------------------------------------------------------------------------------------------------------------
def test_batch_equals_one_at_a_time(device_panel):
    """Two cases of one panel and one set of columns at K_top = 16 in one call (a dosage pass and a thin pass): each as it comes out
    alone, bit for bit."""
    a = WC.case("ktop16")
    b = GC.K_top_case(16, seed=1)
    assert a.panel is b.panel and np.array_equal(a.cols, b.cols) and not np.array_equal(a.gl, b.gl)
    dev = device_panel(a.panel)
    dosage, lists = _batch(dev, [a, b], [1, 0])
    for i, (c, want) in enumerate(((a, 1), (b, 0))):
        d1, l1 = _batch(dev, [c], [want])
        assert np.array_equal(dosage[i], d1[0]) and _lists_equal(lists[i], l1[0])
        assert {len(e["top_matches"]) for e in lists[i]} >= {16}
    check_best_haps(lists[0], GC.oracle_ref(a, "thin")["best_haps"])


# ---------------------------------------------------------------------------------------------------------------------------
# the per-sample loop, both statements, on the device
# ---------------------------------------------------------------------------------------------------------------------------
from tests.test_wide_topk_cases_cpu import GUARD_ROW, WIDE_ROW   # noqa: E402  (the rows, and why there are two)


@pytest.fixture(scope="module")
def rig():
    from quilt_amd.native import DevicePanel
    panel, _, _, _ = MM.make_case(WIDE_ROW, n_samples=0)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    devs = [DevicePanel(panel) for _ in range(2)]
    for d in devs:
        d.set_device_share(2)
        d.set_dosage_precision(64)
        d.set_exclusive(True)
    yield dict(panel=panel, dev=dev, devs=devs)
    for d in devs + [dev]:
        d.close()


@pytest.mark.parametrize("K_top", [12, 64])
@pytest.mark.parametrize("row", ["wide", "guard"])
def test_both_loops_return_the_same_bytes_on_the_device(rig, row, K_top):
    from quilt_amd.driver import Driver, HipBackend
    from quilt_amd.impute import impute_samples
    panel, _, samples, P = MM.make_case(dict(dict(wide=WIDE_ROW, guard=GUARD_ROW)[row], K_top_matches=K_top), reads=300, seed0=70)
    assert np.array_equal(panel.hapMatcher, rig["panel"].hapMatcher)
    want = Driver(rig["panel"], HipBackend(rig["dev"]), P).run(samples, sample_offset=3)
    got = impute_samples(rig["devs"], samples, P, sample_offset=3, samples_per_launch_set=2)
    again = impute_samples(rig["devs"], samples, P, sample_offset=3, samples_per_launch_set=2, one_by_one=True)
    for res in (got, again):
        assert len(res) == len(want) == len(samples)
        for x, y in zip(res, want):
            assert x.nDosage == y.nDosage
            for f in ("read_labels", "dosage", "gp_t", "phasing_haps"):
                assert np.array_equal(getattr(x, f), getattr(y, f)), f


# ---------------------------------------------------------------------------------------------------------------------------
# refusals, and what stays as it was
# ---------------------------------------------------------------------------------------------------------------------------
def test_every_entry_refuses_K_top_matches_65(rig, device_panel):
    """QA_ERR_UNSUPPORTED (-3) naming 1..64 from every public entry, before anything is allocated: the range call keeps no buffer."""
    from quilt_amd.driver import Driver, HipBackend
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import QuiltAmdError, lib
    from tests.test_support_geometry_gpu import select_from_lists
    c = replace_K_top(WC.case("ktop64"), 65)
    dev = device_panel(c.panel)
    a = _reads_args(c)
    rng = np.random.default_rng(5)
    sel = dict(Ksubset=10, Knew=4, which=[np.sort(rng.choice(c.panel.K, 10, replace=False) + 1).astype(np.int32) for _ in range(2)], seeds=[1, 2])
    reads = lambda **kw: HipBackend(dev).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"], a["want_dosage"], a["want_top"],
                                                              c.cols, 65, MIN_GL, 64, **kw)
    top = np.full((2, 2, len(c.thin_grids), 64), -1, dtype=np.int32)
    calls = [lambda: _single(dev, c, dosage=False), lambda: _batch(dev, [c], [0]), lambda: _batch(dev, [c], [1]), reads,
             lambda: reads(select=sel), lambda: _reads_raw(dev, c, 64),
             lambda: select_from_lists(top, np.stack(sel["which"]), sel["seeds"], [1, 1], c.panel.K, 10, 4, 65, 64)]
    for call in calls:
        with pytest.raises(QuiltAmdError, match=r"K_top_matches = 65 .*1\.\.64") as e:
            call()
        assert e.value.status == -3
    # the range call
    L = lib()
    panel, _, samples, P = MM.make_case(dict(WIDE_ROW, K_top_matches=65), reads=300, seed0=70)
    kept = L.qa_impute_kept_buffers()
    with pytest.raises(QuiltAmdError, match=r"1\.\.64") as e:
        impute_samples(rig["devs"], samples, P, sample_offset=3, samples_per_launch_set=2)
    assert e.value.status == -3 and L.qa_impute_kept_buffers() == kept
    with pytest.raises(ValueError, match=r"1\.\.64"):
        Driver(rig["panel"], HipBackend(rig["dev"]), P).run(samples, sample_offset=3)


def replace_K_top(c, K_top):
    from dataclasses import replace
    return replace(c, K_top=K_top)


def test_K_top_8_is_still_the_fused_picker(device_panel):
    """K_top_matches = 8 at top_width = 8 on GC's `ktop8`: what test_fused_picker expects, from the kernels it ran before."""
    from quilt_amd.driver import HipBackend
    from quilt_amd.native import lib
    from tests.oracle_backend import OracleBackend
    c = GC.case("ktop8")
    dev = device_panel(c.panel)
    a = _reads_args(c)
    _, ref_top, ref_cnt = OracleBackend(c.panel).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"], a["want_dosage"],
                                                                      a["want_top"], c.cols, 8, MIN_GL, 8)
    _, top, cnt = HipBackend(dev).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"], a["want_dosage"], a["want_top"],
                                                       c.cols, 8, MIN_GL, 8)
    assert np.array_equal(cnt, ref_cnt) and np.array_equal(top, ref_top)
    # ... from the kernels that ran it before: the picker inside k_bwd64, no launch of k_topk; one rank more and k_topk picks
    for K_top, separate in ((8, False), (9, True)):
        lib().qa_profile_reset()
        HipBackend(dev).fullpass_reads_batch(a["samples"], a["chain_sample"], a["labels"], [0, 0], a["want_top"], c.cols, K_top, MIN_GL, 16)
        assert (_launches("k_topk") > 0) == separate and _launches("k_bwd64") > 0


def _launches(kernel):
    from quilt_amd.native import lib
    L = lib()
    for i in range(L.qa_profile_count()):
        if L.qa_profile_name(i).decode() == kernel:
            ms, cnt, b = C.c_double(), C.c_int64(), C.c_double()
            L.qa_profile_get(i, C.byref(ms), C.byref(cnt), C.byref(b))
            return cnt.value
    raise KeyError(kernel)


# ---------------------------------------------------------------------------------------------------------------------------
# the shim
# ---------------------------------------------------------------------------------------------------------------------------
def test_shim_full_panel_entry_at_K_top_12():
    """`.Call("_QUILT_Rcpp_haploid_dosage_versus_refs", <38 arguments>)` with K_top_matches = 12 under tests/mini_r.py:
    best_haps_stuff_list is filled as the Python mirror's call of the library fills it."""
    from quilt_amd.driver import thinned_grid_columns
    from quilt_amd.native import DevicePanel
    from quilt_amd.reference_single import Rcpp_haploid_dosage_versus_refs
    from quilt_amd.synth import make_synthetic_panel
    from tests.mini_r import R as Runtime
    from tests.test_shim_gpu import _call_by_name, _panel_args
    panel = make_synthetic_panel(K=1024, nSNPs=96 * 32, seed=21)
    K, G, T = panel.K, panel.nGrids, panel.nSNPs
    gl = np.asfortranarray(np.random.default_rng(3).random((2, T)) * 0.9 + 0.05)
    cols = thinned_grid_columns(G, 0.1)
    n_thin = int((cols >= 0).sum())
    dev = DevicePanel(panel)
    w = dict(c=np.ones(G), dosage=np.zeros(T), best_haps_stuff_list=[None] * n_thin)
    Rcpp_haploid_dosage_versus_refs(dev, gl, gammaSmall_cols_to_get=cols, K_top_matches=12, return_betaHat_t=False, return_gamma_t=False,
                                    get_best_haps_from_thinned_sites=True, **w)
    dev.close()
    R = Runtime()
    try:
        a = dict(gl=R.real(gl), arma_alphaHat_t=R.real(np.zeros((K, G))), eigen_alphaHat_t=R.real(np.zeros((1, 1))), betaHat_t=R.real(np.zeros((1, 1))),
                 c=R.real(np.ones(G)), gamma_t=R.real(np.zeros((1, 1))), gammaSmall_t=R.real(np.zeros((1, 1))),
                 best_haps_stuff_list=R.list([R.nil] * n_thin), dosage=R.real(np.zeros(T)),
                 use_eMatDH=R.logical([1]), use_eMatDH_special_symbols=R.logical([0]), gammaSmall_cols_to_get=R.integer(cols),
                 eMatDH_special_grid_which=R.integer(panel.eMatDH_special_grid_which), eMatDH_special_values_list=R.list([]),
                 K_top_matches=R.integer([12]), suppressOutput=R.integer([1]), min_emission_prob_normalization_threshold=R.real([1e-100]),
                 return_betaHat_t=R.logical([0]), return_dosage=R.logical([1]), return_gamma_t=R.logical([0]), return_gammaSmall_t=R.logical([0]),
                 get_best_haps_from_thinned_sites=R.logical([1]), is_version_2=R.logical([0]), is_version_3=R.logical([0]),
                 return_extra=R.logical([0]), always_normalize=R.logical([1]), use_eigen=R.logical([0]), normalize_emissions=R.logical([1]))
        a.update(_panel_args(R, panel))
        a["transMatRate_t"] = R.real(panel.transMatRate_t)
        assert _call_by_name(R, "_QUILT_Rcpp_haploid_dosage_versus_refs", a) is None
        assert np.array_equal(R.value(a["dosage"]), w["dosage"]) and np.array_equal(R.value(a["c"]), w["c"])
        lists = R.value(a["best_haps_stuff_list"])
        assert len(lists) == n_thin
        for got, want in zip(lists, w["best_haps_stuff_list"]):
            assert np.array_equal(got["top_matches"], want["top_matches"]) and np.array_equal(got["top_matches_values"], want["top_matches_values"])
        assert all(len(x["top_matches"]) >= 12 for x in w["best_haps_stuff_list"])
    finally:
        R.dotcall("qa_shim_release")
        R.reset()
