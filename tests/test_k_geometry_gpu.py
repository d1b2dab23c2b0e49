"""The K axis of the full-panel passes on the device: every K of tests/k_cases.py (the last K of every build of every kernel family
and the next, the tiny panels, all eight widths of the last chunk row in registers and in LDS, the streamed build) with its planted
panels -- the haplotypes that carry the result sit ON the edges of that K: the ends, the last chunk, both sides of every chunk
row -- through every kernel family that accepts the K, against the fp64 CPU oracle.

Each family is held to the bar the suite already holds it to:

  * fp32 state (default handle, K <= 98 304; single-pass entry with alpha / beta / gamma, and qa_fullpass_batch): the bars of
    test_dosage_pass_matches_oracle (dosage 2e-4, gamma atol 2e-5 rtol 2e-3, alpha atol 1e-6 rtol 2e-3, beta rtol 2e-3, c rtol 1e-4)
  * k_fwd64 + k_bwd64 + k_topk (thin pass): lists identical with values to 1e-9, c and alpha at the thinned grids rtol 1e-9
  * k_fwd64 + k_bwd64d (set_dosage_precision(64); dosage-only call and batch): dosage 1e-10, c rtol 1e-12, lists identical
  * generic fp64 (set_dosage_precision(64) with the K x G matrices, K <= 57 344; qa_fullpass_last_plan says that kind ran): every
    element of alpha, beta and gamma rtol 1e-9, the project's fp64 bar; dosage 1e-9 and log c summed rtol 1e-12 as
    test_dosage_pass_headline_size holds these kernels to
  * the reads entry with the fused picker (top_width = K_top = 8, and the select= form): identical to OracleBackend
  * the gamma column of an interior grid: 1e-9 absolute, as tests/test_hla_gpu.py compares it
  * validation mode, single and batched form, at one K per number of chunk rows: bit-identical
  * a batch of the K's cases equals each case alone, bit for bit

Two comparisons are written for these panels.  The sum of log c (fp32 state, rtol 1e-5) is compared wherever the label has reads;
without reads every c is 1, the logs sum to 0 and the elementwise bar on c is the one that binds.  The fp64 dosage kernels' c
(rtol 1e-12) is compared with the oracle's c after the rounding of the oracle's own K-wide sums has been divided out
(k_cases.c_without_summation_error): the background rows are exact copies, the oracle adds them one after the other, every
addition rounds the same way and its c is off by up to 2e-12 -- measured on the oracle alone, and bounded in the CPU file.

tests/test_k_cases_cpu.py proves on the oracle that the planted rows head every list in a stated order with gammas 1e-6 apart (or
exact copies), so no comparison branches on the device's result, and nothing is skipped."""

import numpy as np
import pytest

from tests import k_cases as KC
from tests.test_grid_geometry_gpu import _batch, _lists_equal, _reads_args, _select_both, _single
from tests.testhooks import last_plan
from tests.util import check_best_haps

pytestmark = pytest.mark.gpu

KS = KC.k_table()
KS_F32 = [k for k in KS if KC.geometry(k, "f32")["NT"]]
KS_FULL = [k for k in KS if KC.geometry(k, "full")["NT"]]
KS_ROWS = [k for k in KC.row_count_ks() if k <= 98304]
DOSAGE_ATOL = 2e-4
MIN_GL = 1e-10
KIND_F64_FULL = 2   # PassKind, csrc/pass_layout.hpp


@pytest.fixture(scope="module")
def device_panel():
    """The device panels of the K in hand (the tests walk the table K by K): the two latest are kept."""
    from quilt_amd.native import DevicePanel
    held = {}

    def get(panel):
        if id(panel) not in held:
            while len(held) >= 2:
                held.pop(next(iter(held)))[1].close()
            held[id(panel)] = (panel, DevicePanel(panel))
        return held[id(panel)][1]
    yield get
    for _, dev in held.values():
        dev.close()


def _singles(K):
    """The cases that go through the single-pass entry: the first promotion, the label without reads, the nMaxDH = 8 panel."""
    return [KC.first_case(K), KC.noreads_case(K), KC.dh8_case(K)]


def _batches(K):
    """The launch sets of a K: all cases of the nMaxDH = 255 panel in one call, the nMaxDH = 8 case in another."""
    return [KC.dh255_cases(K), [KC.dh8_case(K)]]


def test_the_table_reaches_every_build():
    """(the CPU file proves it; restated here so that this file fails too if the table shrinks)"""
    assert len(KC.reached("f32")) == 10 and len(KC.reached("full")) == 9 and len(KC.reached("rank")) == 8 and len(KC.reached("dos")) == 9


# ---------------------------------------------------------------------------------------------------------------------------
# fp32 state
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS_F32)
def test_fp32_state_passes(K, device_panel):
    for c in _singles(K):
        dev = device_panel(c.panel)
        ref = KC.oracle_ref(c, "full", 1, True)
        got = _single(dev, c, dosage=True, alpha=True, gamma=True, beta=True, always_normalize=True)
        assert np.abs(got["dosage"] - ref["dosage"]).max() <= DOSAGE_ATOL
        np.testing.assert_allclose(got["gamma_t"].sum(axis=0), 1.0, atol=1e-4)
        np.testing.assert_allclose(got["gamma_t"], ref["gamma_t"], atol=2e-5, rtol=2e-3)
        np.testing.assert_allclose(got["alphaHat_t"], ref["alphaHat_t"], atol=1e-6, rtol=2e-3)
        np.testing.assert_allclose(got["betaHat_t"], ref["betaHat_t"], atol=1e-30, rtol=2e-3)
        # (a label without reads: every c of the oracle is 1 to the rounding of its own sums -- test_k_cases_cpu.py -- and the logs
        # sum to 0; a relative bar on that sum says nothing, the elementwise bar below is the one that binds)
        if not c.claims["no_reads"]:
            np.testing.assert_allclose(np.log(got["c"]).sum(), np.log(ref["c"]).sum(), rtol=1e-5)
        np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-4)
        check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
    for cases in _batches(K):
        dosage, lists = _batch(device_panel(cases[0].panel), cases, [1] * len(cases))
        for i, c in enumerate(cases):
            lazy = KC.oracle_ref(c, "dosage")
            assert np.abs(dosage[i] - lazy["dosage"]).max() <= DOSAGE_ATOL, c.name
            check_best_haps(lists[i], lazy["best_haps"])


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 ranking passes: k_fwd64 + k_bwd64 + k_topk
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_ranking_passes(K, device_panel):
    for c in _singles(K):
        dev = device_panel(c.panel)
        ref = KC.oracle_ref(c, "thin")
        got = _single(dev, c, dosage=False, alpha=True)
        check_best_haps(got["best_haps_stuff_list"], ref["best_haps"], exact=True)
        assert {len(e["top_matches"]) for e in got["best_haps_stuff_list"]} == {c.claims["list_len"][1]}
        np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-9)
        for g in c.thin_grids:
            np.testing.assert_allclose(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g], rtol=1e-9, atol=1e-300)
    for cases in _batches(K):
        _, lists = _batch(device_panel(cases[0].panel), cases, [0] * len(cases))
        for i, c in enumerate(cases):
            check_best_haps(lists[i], KC.oracle_ref(c, "thin")["best_haps"], exact=True)


# ---------------------------------------------------------------------------------------------------------------------------
# fp64 dosage passes: k_fwd64 + k_bwd64d
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_fp64_dosage_passes(K, device_panel):
    for c in _singles(K):
        dev = device_panel(c.panel)
        dev.set_dosage_precision(64)
        try:
            ref = KC.oracle_ref(c, "dosage")
            got = _single(dev, c, dosage=True)   # no K x G output: the dosage-only call
            assert np.abs(got["dosage"] - ref["dosage"]).max() <= 1e-10
            # (c against the oracle's with the rounding of its one-after-the-other sums taken out: on panels whose background
            # rows are exact copies that rounding alone reaches 2e-12, tests/k_cases.py: c_without_summation_error)
            np.testing.assert_allclose(got["c"], KC.c_without_summation_error(c, ref), rtol=1e-12)
            check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
        finally:
            dev.set_dosage_precision(32)
    for cases in _batches(K):
        dev = device_panel(cases[0].panel)
        dev.set_dosage_precision(64)
        try:
            dosage, lists = _batch(dev, cases, [1] * len(cases))
            for i, c in enumerate(cases):
                lazy = KC.oracle_ref(c, "dosage")
                assert np.abs(dosage[i] - lazy["dosage"]).max() <= 1e-10, c.name
                check_best_haps(lists[i], lazy["best_haps"])
        finally:
            dev.set_dosage_precision(32)


# ---------------------------------------------------------------------------------------------------------------------------
# generic fp64: k_fwd / k_bwd<double, NCH, 256>
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS_FULL)
def test_generic_fp64_passes(K, device_panel):
    for c in (KC.first_case(K), KC.dh8_case(K)):
        dev = device_panel(c.panel)
        dev.set_dosage_precision(64)
        try:
            ref = KC.oracle_ref(c, "full", 1, True)
            got = _single(dev, c, dosage=True, alpha=True, gamma=True, beta=True, always_normalize=True)
            assert last_plan()["kind"] == KIND_F64_FULL
            for name in ("alphaHat_t", "betaHat_t", "gamma_t"):
                np.testing.assert_allclose(got[name], ref[name], rtol=1e-9, atol=1e-300, err_msg=name)
            assert np.abs(got["dosage"] - ref["dosage"]).max() <= 1e-9
            np.testing.assert_allclose(np.log(got["c"]).sum(), np.log(ref["c"]).sum(), rtol=1e-12)
            np.testing.assert_allclose(got["c"], ref["c"], rtol=1e-9)
            check_best_haps(got["best_haps_stuff_list"], ref["best_haps"])
        finally:
            dev.set_dosage_precision(32)


# ---------------------------------------------------------------------------------------------------------------------------
# the reads entry: the picker fused into k_bwd64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_reads_entry_with_the_fused_picker(K, device_panel):
    from quilt_amd.driver import HipBackend
    from tests.oracle_backend import OracleBackend
    width = KC.K_TOP   # top_width = K_top and top_width = 8 are one width here
    for c in _singles(K):
        dev = device_panel(c.panel)
        a = _reads_args(c)
        args = (a["samples"], a["chain_sample"], a["labels"], a["want_dosage"], a["want_top"], c.cols, c.K_top, MIN_GL, width)
        ref_dosage, ref_top, ref_cnt = OracleBackend(c.panel).fullpass_reads_batch(*args)
        dosage, top, cnt = HipBackend(dev).fullpass_reads_batch(*args)
        assert np.array_equal(cnt, ref_cnt)
        assert np.array_equal(top, ref_top), "the ordered head of every list, order included"
        assert np.abs(dosage[0] - ref_dosage[0]).max() <= DOSAGE_ATOL
        for label in (1, 2):
            assert (cnt[:, label - 1, :] == c.claims["list_len"][label]).all()
            promoted = c.claims["promoted"][label]
            assert (top[:, label - 1, :, :len(promoted)] == np.array(promoted)).all()
        if c.claims["no_reads"]:   # every haplotype ties: all of them counted, the head is haplotypes 0, 1, 2 ...
            assert (top[:, 0, :, :min(width, K)] == np.arange(min(width, K))).all()


@pytest.mark.parametrize("K", KS)
def test_fused_picker_feeds_the_device_selection(K, device_panel):
    """The select= form: k_select draws the next small panel from the lists that stay on the device -- the panel the host function
    draws from the ORACLE's lists (two labels x eight promoted rows: the selection completes for every K of 16 or more)."""
    from quilt_amd.driver import everything_select_good_haps_dense, previously_selected
    c = KC.first_case(K)
    Ksubset = min(10, K)
    Knew = min(4, max(1, Ksubset - 1))
    ref_top, which, seeds, nxt, status = _select_both(c, device_panel(c.panel), Ksubset, Knew)
    for ch in range(2):
        prev = previously_selected(which[ch], Ksubset - Knew, seeds[ch])
        sel = everything_select_good_haps_dense(Knew, c.K_top, ref_top[ch].astype(np.int64) + 1, prev, K, seeds[ch], truncated=True)
        assert len(sel) == Knew and status[ch] == 0
        assert np.array_equal(nxt[ch], np.concatenate([prev, sel]))


# ---------------------------------------------------------------------------------------------------------------------------
# the gamma column (k_bwd64d<..., GCOL = true>)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_gamma_column_at_an_interior_grid(K, device_panel):
    from quilt_amd.driver import HipBackend
    from tests.hla_backend import oracle_gamma_t
    grid = 3
    for c in (KC.first_case(K), KC.dh8_case(K)):
        dev = device_panel(c.panel)
        a = _reads_args(c)
        Ksubset = min(10, K)
        rng = np.random.default_rng(5)
        sel = dict(Ksubset=Ksubset, Knew=min(4, max(1, Ksubset - 1)),
                   which=[np.sort(rng.choice(K, Ksubset, replace=False) + 1).astype(np.int32) for _ in range(2)],
                   seeds=[int(rng.integers(0, 2 ** 63)) for _ in range(2)])
        ref = oracle_gamma_t(c.panel, a["samples"], a["chain_sample"], a["labels"])
        dev.set_dosage_precision(64)
        try:
            be = HipBackend(dev)
            args = (a["samples"], a["chain_sample"], a["labels"], [1, 1], a["want_top"], c.cols, c.K_top, MIN_GL, 8)
            d0, _, c0, n0, s0 = (np.copy(x) if x is not None else None for x in be.fullpass_reads_batch(*args, select=sel))
            d, _, cn, nx, st, gam = be.fullpass_reads_batch(*args, select=sel, gamma_grid=grid)
            assert np.array_equal(d, d0) and np.array_equal(cn, c0) and np.array_equal(nx, n0) and np.array_equal(st, s0)
            for ci in range(2):
                for l in range(2):
                    assert np.abs(gam[ci, l] - ref[ci][l][:, grid]).max() <= 1e-9, (c.name, ci, l)
        finally:
            dev.set_dosage_precision(32)


# ---------------------------------------------------------------------------------------------------------------------------
# validation mode: one K per number of chunk rows
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS_ROWS)
def test_validation_mode(K, device_panel):
    c = KC.first_case(K)
    dev = device_panel(c.panel)
    dev.set_sum_order(True)
    try:
        ref = KC.oracle_ref(c, "thin")
        got = _single(dev, c, dosage=False, alpha=True)
        assert np.array_equal(got["c"], ref["c"])
        for e, (oi, ov) in zip(got["best_haps_stuff_list"], ref["best_haps"]):
            assert np.array_equal(e["top_matches"], oi) and np.array_equal(e["top_matches_values"], ov)
        for g in c.thin_grids:
            assert np.array_equal(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g])
        refd = KC.oracle_ref(c, "dosage")
        gotd = _single(dev, c, dosage=True)
        assert np.array_equal(gotd["dosage"], refd["dosage"]) and np.array_equal(gotd["c"], refd["c"])
        # the batched form: one wave per pass, the same sums in the same order
        dev.set_sum_order_batched(True)
        cases = KC.dh255_cases(K)
        dosage, lists = _batch(dev, cases, [1] * len(cases))
        for i, ci in enumerate(cases):
            r = KC.oracle_ref(ci, "dosage")
            assert np.array_equal(dosage[i], r["dosage"]), ci.name
            for e, (oi, ov) in zip(lists[i], r["best_haps"]):
                assert np.array_equal(e["top_matches"], oi) and np.array_equal(e["top_matches_values"], ov)
    finally:
        dev.set_sum_order_batched(False)
        dev.set_sum_order(False)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of a K in one qa_fullpass_batch call
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp64_dosage", [False, True])
@pytest.mark.parametrize("K", KS)
def test_batch_equals_one_at_a_time(K, fp64_dosage, device_panel):
    """Dosage and thin passes of different reads mixed in one call: every pass comes out as it does alone, bit for bit."""
    cases = KC.dh255_cases(K)
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
    finally:
        if fp64_dosage:
            dev.set_dosage_precision(32)
