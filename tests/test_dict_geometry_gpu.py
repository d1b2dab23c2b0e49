"""The dictionary axis of the full-panel passes on the device: every constructed case of tests/dict_cases.py (every nMaxDH beside a
constant the row loops step by, the grid's minimum and maximum on every planted table row, a share of gamma in every code's bin,
specials by count, by grid and by position in a chunk, in both forms of use_eMatDH_special_symbols, emission edges given as gl, the
options normalize_emissions and min_emission_prob_normalization_threshold, a distinctHapsIE that is not the expansion of the words)
through every kernel family that accepts it, against the fp64 CPU oracle.

Each family is held to the bar the suite already holds it to (the header of tests/test_grid_geometry_gpu.py):

  * fp32 state (single-pass entry with alpha / beta / gamma, and qa_fullpass_batch): dosage 2e-4, c rtol 1e-4, gamma atol 2e-5
    rtol 2e-3, alpha atol 1e-6 rtol 2e-3, beta rtol 2e-3, lists identical; the oracle under always_normalize = True
  * k_fwd64 + k_bwd64 + k_topk (thin pass): lists identical with values to 1e-9, c and alpha at the thinned grids rtol 1e-9
  * k_fwd64 + k_bwd64d + k_dosage (qa_panel_set_dosage_precision(64)): dosage 1e-10, c rtol 1e-12, lists identical
  * generic fp64 (qa_panel_set_dosage_precision(64) with the K x G matrices: k_fwd / k_bwd<double> and their fold_histogram): every
    element of alpha, beta and gamma rtol 1e-9, dosage 1e-9, c rtol 1e-9 and log c summed rtol 1e-12 (tests/test_k_geometry_gpu.py)
  * the picker fused into k_bwd64 (the reads entry at top_width = K_top): `top` with its order and `cnt` identical to
    tests.oracle_backend.OracleBackend on the same reads
  * validation mode (qa_panel_set_sum_order(1)): bit-identical; qa_panel_set_sum_order_batched on launch sets of two or more:
    bit-identical too

The lazily normalised families run a case under the threshold it plants (the width cases: a renormalisation at grid 4 that any
other row for that grid's minimum would cancel); the batched entries take neither option and run under the defaults.  A code-to-bin
case whose masses cannot show at the fp32 bar (tests/test_dict_cases_cpu.py) goes through the fp64 families only.
tests/test_dict_cases_cpu.py holds every case to a separation of 1e-6 between unequal gammas among the ranks compared here, so
no comparison branches on the device's result, and nothing is skipped."""
import dataclasses

import numpy as np
import pytest

from tests import dict_cases as DC
from tests.fullpass_calls import batch, lists_equal, lists_equal_oracle, single
from tests.util import check_best_haps

pytestmark = pytest.mark.gpu

WIDTHS = DC.widths()
DOSAGE_ATOL = DC.FP32_BAR
MIN_GL = DC.MIN_GL


@pytest.fixture(scope="module")
def device_panel():
    """One device panel per host panel and form of the specials, for the whole module."""
    from quilt_amd.native import DevicePanel
    held = {}

    def get(panel, symbols=False):
        key = (id(panel), bool(symbols))
        if key not in held:
            held[key] = (panel, DevicePanel(panel, use_eMatDH_special_symbols=bool(symbols)))
        return held[key][1]
    yield get
    for _, dev in held.values():
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------------
def _fp32(dev, c, norm=True, batched=True):
    ref = DC.oracle_ref(c, "full", always_normalize=True, normalize_emissions=norm)
    got = single(dev, c, dosage=True, alpha=True, gamma=True, beta=True, always_normalize=True, normalize_emissions=norm)
    assert np.abs(got["dosage"] - ref["dosage"]).max() <= DOSAGE_ATOL, c.name
    np.testing.assert_allclose(got["gamma_t"].sum(axis=0), 1.0, atol=1e-4, err_msg=c.name)
    np.testing.assert_allclose(got["gamma_t"], ref["gamma_t"], atol=2e-5, rtol=2e-3, err_msg=c.name)
    np.testing.assert_allclose(got["alphaHat_t"], ref["alphaHat_t"], atol=1e-6, rtol=2e-3, err_msg=c.name)
    np.testing.assert_allclose(got["betaHat_t"], ref["betaHat_t"], atol=1e-30, rtol=2e-3, err_msg=c.name)
    np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-4, err_msg=c.name)
    check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
    if batched and norm:
        lazy = DC.oracle_ref(c, "dosage", threshold=1e-100)
        dosage, lists = batch(dev, [c], [1])
        assert np.abs(dosage[0] - lazy["dosage"]).max() <= DOSAGE_ATOL, c.name
        check_best_haps(lists[0], lazy["best_haps"])


def _ranking(dev, c, norm=True, batched=True):
    ref = DC.oracle_ref(c, "thin", normalize_emissions=norm)
    got = single(dev, c, dosage=False, alpha=True, normalize_emissions=norm, threshold=c.threshold)
    check_best_haps(got["best_haps_stuff_list"], ref["best_haps"], exact=True)
    np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-9, err_msg=c.name)
    for g in c.thin_grids:
        np.testing.assert_allclose(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g], rtol=1e-9, atol=1e-300, err_msg=c.name)
    if batched and norm:
        _, lists = batch(dev, [c], [0])
        check_best_haps(lists[0], DC.oracle_ref(c, "thin", threshold=1e-100)["best_haps"], exact=True)


def _dos64(dev, c, norm=True, batched=True):
    dev.set_dosage_precision(64)
    try:
        ref = DC.oracle_ref(c, "dosage", normalize_emissions=norm)
        got = single(dev, c, dosage=True, normalize_emissions=norm, threshold=c.threshold)   # no K x G output: the dosage-only call
        assert np.abs(got["dosage"] - ref["dosage"]).max() <= DC.FP64_BAR, c.name
        np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-12, err_msg=c.name)
        check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
        if batched and norm:
            lazy = DC.oracle_ref(c, "dosage", threshold=1e-100)
            dosage, lists = batch(dev, [c], [1])
            assert np.abs(dosage[0] - lazy["dosage"]).max() <= DC.FP64_BAR, c.name
            check_best_haps(lists[0], lazy["best_haps"])
    finally:
        dev.set_dosage_precision(32)


def _generic64(dev, c, norm=True):
    dev.set_dosage_precision(64)
    try:
        ref = DC.oracle_ref(c, "full", always_normalize=True, normalize_emissions=norm)
        got = single(dev, c, dosage=True, alpha=True, gamma=True, beta=True, always_normalize=True, normalize_emissions=norm)
        for name in ("alphaHat_t", "betaHat_t", "gamma_t"):
            np.testing.assert_allclose(got[name], ref[name], rtol=1e-9, atol=1e-300, err_msg=c.name + " " + name)
        assert np.abs(got["dosage"] - ref["dosage"]).max() <= 1e-9, c.name
        # (gl == 1 throughout: every c of the oracle is 1 to the rounding of its own sums and the logs sum to 0; a relative bar on
        # that sum says nothing, the elementwise bar below is the one that binds -- as in tests/test_k_geometry_gpu.py)
        if not (c.gl == 1).all():
            np.testing.assert_allclose(np.log(got["c"]).sum(), np.log(ref["c"]).sum(), rtol=1e-12, err_msg=c.name)
        np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-9, err_msg=c.name)
        check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
    finally:
        dev.set_dosage_precision(32)


def _validation(dev, c, norm=True):
    dev.set_sum_order(True)
    try:
        ref = DC.oracle_ref(c, "thin", normalize_emissions=norm)
        got = single(dev, c, dosage=False, alpha=True, normalize_emissions=norm, threshold=c.threshold)
        assert np.array_equal(got["c"], ref["c"]), c.name
        assert lists_equal_oracle(got["best_haps_stuff_list"], ref["best_haps"]), c.name
        for g in c.thin_grids:
            assert np.array_equal(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g]), c.name
        refd = DC.oracle_ref(c, "dosage", normalize_emissions=norm)
        gotd = single(dev, c, dosage=True, normalize_emissions=norm, threshold=c.threshold)
        assert np.array_equal(gotd["dosage"], refd["dosage"]) and np.array_equal(gotd["c"], refd["c"]), c.name
        assert lists_equal_oracle(gotd["best_haps_stuff_list"], refd["best_haps"]), c.name
    finally:
        dev.set_sum_order(False)


def _picker(dev, c):
    """The reads entry at top_width = K_top: two chains on the case's sample, dosages and lists of both labels."""
    from quilt_amd.driver import HipBackend
    from tests.oracle_backend import OracleBackend
    args = ([c.sample], [0, 0], [c.labels, c.labels], [1, 0], [1, 1], c.cols, c.K_top, MIN_GL, c.K_top)
    ref_dosage, ref_top, ref_cnt = OracleBackend(c.panel).fullpass_reads_batch(*args)
    dosage, top, cnt = HipBackend(dev).fullpass_reads_batch(*args)
    assert np.array_equal(cnt, ref_cnt), c.name
    assert np.array_equal(top, ref_top), c.name + ": the ordered head of every list, order included"
    assert np.abs(dosage[0] - ref_dosage[0]).max() <= DOSAGE_ATOL, c.name


def _all_families(dev, c, norm=True):
    if c.fp32:
        _fp32(dev, c, norm)
    _ranking(dev, c, norm)
    _dos64(dev, c, norm)
    _generic64(dev, c, norm)
    _validation(dev, c, norm)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. dictionary width
# ---------------------------------------------------------------------------------------------------------------------------
def _refused(panel):
    from quilt_amd.native import DevicePanel, QuiltAmdError
    with pytest.raises(QuiltAmdError) as e:
        DevicePanel(panel).close()
    return e.value.status


def test_refusals():
    """nMaxDH = 0 and 256, and an int hapMatcher that holds 256 or -1: refused before any pass could index a table with them."""
    from quilt_amd.native import QA_ERR_INVALID, QA_ERR_UNSUPPORTED
    p = DC.width_panel(8)
    assert _refused(dataclasses.replace(p, nMaxDH=0)) == QA_ERR_INVALID
    wide = dataclasses.replace(p, nMaxDH=256, distinctHapsB=np.zeros((256, p.nGrids), dtype=np.int32, order="F"), distinctHapsIE=None)
    assert _refused(wide) == QA_ERR_UNSUPPORTED
    for bad in (256, -1):
        hm = np.asfortranarray(np.asarray(p.hapMatcherR).astype(np.int32))
        hm[p.K - 1, p.nGrids - 1] = bad
        assert _refused(dataclasses.replace(p, hapMatcherR=None, hapMatcher=hm)) == QA_ERR_INVALID


def test_int_hapmatcher_equals_raw(device_panel):
    """The int hapMatcher form of qa_panel_create gives the passes what the hapMatcherR form gives them, bit for bit."""
    from quilt_amd.native import DevicePanel
    c = DC.special_case(8, "every_a")
    p = c.panel
    dev_int = DevicePanel(dataclasses.replace(p, hapMatcherR=None, hapMatcher=np.asfortranarray(np.asarray(p.hapMatcherR).astype(np.int32))))
    dev_raw = device_panel(p)
    try:
        for dev64 in (False, True):
            for dev in (dev_int, dev_raw):
                dev.set_dosage_precision(64 if dev64 else 32)
            for kw in (dict(dosage=True), dict(dosage=False, alpha=True), dict(dosage=True, alpha=True, gamma=True, beta=True)):
                a, b = single(dev_int, c, **kw), single(dev_raw, c, **kw)
                assert lists_equal(a["best_haps_stuff_list"], b["best_haps_stuff_list"])
                for k in a:
                    if k != "best_haps_stuff_list":
                        assert np.array_equal(a[k], b[k]), (k, kw)
            da, la = batch(dev_int, [c, c], [1, 0])
            db, lb = batch(dev_raw, [c, c], [1, 0])
            assert np.array_equal(da, db) and all(lists_equal(x, y) for x, y in zip(la, lb))
    finally:
        dev_raw.set_dosage_precision(32)
        dev_int.close()


@pytest.mark.parametrize("n", WIDTHS)
def test_width_fp32_state(n, device_panel):
    for c in DC.width_cases(n):
        _fp32(device_panel(c.panel), c)


@pytest.mark.parametrize("n", WIDTHS)
def test_width_ranking_passes(n, device_panel):
    for c in DC.width_cases(n):
        _ranking(device_panel(c.panel), c)


@pytest.mark.parametrize("n", WIDTHS)
def test_width_fp64_dosage_passes(n, device_panel):
    for c in DC.width_cases(n):
        _dos64(device_panel(c.panel), c)


@pytest.mark.parametrize("n", WIDTHS)
def test_width_generic_fp64_passes(n, device_panel):
    for c in DC.width_cases(n):
        _generic64(device_panel(c.panel), c)


@pytest.mark.parametrize("n", WIDTHS)
def test_width_validation_mode(n, device_panel):
    for c in DC.width_cases(n):
        _validation(device_panel(c.panel), c)


@pytest.mark.parametrize("n", WIDTHS)
def test_width_fused_picker(n, device_panel):
    for c in DC.width_cases(n):
        _picker(device_panel(c.panel), c)


@pytest.mark.parametrize("n", WIDTHS)
def test_width_without_emission_normalisation(n, device_panel):
    """normalize_emissions = 0 on the first and the last case of the width: scale, sp_scale and the minimum that drives the lazy
    schedule all change."""
    cases = DC.width_cases(n)
    for c in {cases[0].name: cases[0], cases[-1].name: cases[-1]}.values():
        _all_families(device_panel(c.panel), c, norm=False)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. code to bin
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", DC.BIN_WIDTHS)
def test_code_to_bin(n, device_panel):
    c = DC.bin_case(n)
    dev = device_panel(c.panel)
    _all_families(dev, c)
    if c.fp32:
        _picker(dev, c)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. specials
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", [c.name for c in DC.special_cases()])
def test_specials(name, norm, device_panel):
    c = DC.case(name)
    dev = device_panel(c.panel, c.symbols)
    _all_families(dev, c, norm)
    if norm and not c.symbols:
        _picker(dev, c)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. emissions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("name", [c.name for c in DC.emission_cases()])
def test_emissions(name, norm, device_panel):
    c = DC.case(name)
    _all_families(device_panel(c.panel), c, norm)


def test_planted_threshold(device_panel):
    """The schedule cases under a threshold the weak background crosses: the lazily normalised families renormalise where the
    oracle does under that threshold (tests/test_dict_cases_cpu.py: other grids than under 1e-100)."""
    for c in DC.threshold_cases():
        dev = device_panel(c.panel)
        _ranking(dev, c, batched=False)
        _dos64(dev, c, batched=False)
        _validation(dev, c)


def test_threshold_that_is_not_positive_is_the_default(device_panel):
    """0 and -1 (a zero-initialised qa_fullpass_opts_t) are read as 1e-100 by every lazily normalised family, bit for bit."""
    c0 = DC.threshold_cases()[1]
    dev = device_panel(c0.panel)
    runs = {}
    for thr in (1e-100, 0.0, -1.0):
        c = dataclasses.replace(c0, threshold=thr)
        runs[thr] = [single(dev, c, dosage=False, alpha=True, threshold=thr)]
        dev.set_dosage_precision(64)
        runs[thr].append(single(dev, c, dosage=True, threshold=thr))
        dev.set_dosage_precision(32)
        dev.set_sum_order(True)
        runs[thr].append(single(dev, c, dosage=True, threshold=thr))
        dev.set_sum_order(False)
    sigma = c0.panel.transMatRate_t[0]
    assert (runs[1e-100][0]["c"][1:-1] != 1 / sigma[:-1]).any(), "the default renormalises between the ends"
    for thr in (0.0, -1.0):
        for a, b in zip(runs[thr], runs[1e-100]):
            assert lists_equal(a["best_haps_stuff_list"], b["best_haps_stuff_list"])
            for k in a:
                if k != "best_haps_stuff_list":
                    assert np.array_equal(a[k], b[k]), (thr, k)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a free distinctHapsIE
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["other_error", "one_entry"])
def test_free_distinctHapsIE(name, device_panel):
    """The dosage follows the panel's table at every family's bar; c, alpha and the lists are those of the same panel with the
    derived table, bit for bit: k_emat does not look at IE."""
    free, derived = DC.ie_cases()[name]
    dev, dev_d = device_panel(free.panel), device_panel(derived.panel)
    _all_families(dev, free)
    _picker(dev, free)
    a = single(dev, free, dosage=False, alpha=True)
    b = single(dev_d, derived, dosage=False, alpha=True)
    assert np.array_equal(a["c"], b["c"]) and np.array_equal(a["alphaHat_t"], b["alphaHat_t"])
    assert lists_equal(a["best_haps_stuff_list"], b["best_haps_stuff_list"])
    # the batched reference-order form, a launch set of two
    ref = DC.oracle_ref(free, "dosage", threshold=1e-100)
    dev.set_sum_order(True)
    dev.set_sum_order_batched(True)
    try:
        dosage, lists = batch(dev, [free, free], [1, 1])
        for i in range(2):
            assert np.array_equal(dosage[i], ref["dosage"]) and lists_equal_oracle(lists[i], ref["best_haps"])
    finally:
        dev.set_sum_order_batched(False)
        dev.set_sum_order(False)


# ---------------------------------------------------------------------------------------------------------------------------
# several cases in one qa_fullpass_batch call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64_dosage", [False, True])
@pytest.mark.parametrize("group", sorted(DC.groups()))
def test_batch_equals_one_at_a_time(group, fp64_dosage, device_panel):
    """Dosage and thin passes of different inputs mixed in one call: every pass comes out as it does alone, bit for bit."""
    cases = DC.groups()[group]
    dev = device_panel(cases[0].panel)
    want = [int(i % 3 != 1) for i in range(len(cases))]   # dosage, thin, dosage, dosage, thin ...
    assert 0 < sum(want) < len(want)
    if fp64_dosage:
        dev.set_dosage_precision(64)
    try:
        dosage, lists = batch(dev, cases, want)
        for i, c in enumerate(cases):
            d1, l1 = batch(dev, [c], [want[i]])
            assert np.array_equal(dosage[i], d1[0]), c.name
            assert lists_equal(lists[i], l1[0]), c.name
            check_best_haps(lists[i], DC.oracle_ref(c, "thin", threshold=1e-100)["best_haps"])
            if want[i] and (fp64_dosage or c.fp32):
                ref = DC.oracle_ref(c, "dosage", threshold=1e-100)["dosage"]
                assert np.abs(dosage[i] - ref).max() <= (DC.FP64_BAR if fp64_dosage else DOSAGE_ATOL), c.name
    finally:
        if fp64_dosage:
            dev.set_dosage_precision(32)


@pytest.mark.parametrize("group", sorted(DC.groups()))
def test_batched_reference_order_equals_the_oracle(group, device_panel):
    """qa_panel_set_sum_order_batched on a launch set of two or more: the bits of validation mode, which are the oracle's."""
    cases = DC.groups()[group]
    dev = device_panel(cases[0].panel)
    dev.set_sum_order(True)
    dev.set_sum_order_batched(True)
    try:
        dosage, lists = batch(dev, cases, [1] * len(cases))
        for i, c in enumerate(cases):
            ref = DC.oracle_ref(c, "dosage", threshold=1e-100)
            assert np.array_equal(dosage[i], ref["dosage"]), c.name
            assert lists_equal_oracle(lists[i], ref["best_haps"]), c.name
    finally:
        dev.set_sum_order_batched(False)
        dev.set_sum_order(False)
