"""Validation mode (qa_panel_set_sum_order(panel, 1 | 2)) on panels beyond 57 344 haplotypes: the reference-order kernels
(csrc/fullpass_ref.hip, and their one-wave-per-pass form csrc/fullpass_ord.hip) take the checkpoint layout's NT and Kq at run time
and keep a pass's state in its device scratch, so pick_geometry (csrc/fullpass.hip) gives them NT = 256 and NCH = ceil(K / 4 096)
chunk rows for any K -- up to 57 344 exactly the geometry they had (the generic fp64 kernels' built variants), so nothing moves
there.  Through every entry that runs full-panel passes: the single-pass entry with its K x nGrids matrices, the launch-set hook,
the reads batch with hla_run's gamma column, and the native sample loop.

Every comparison is np.array_equal against the CPU restatement (oracle/fullpass.c): tolerance none is validation mode's
contract (fp64, the same operations on the same operands in the same order), not a measured number.

Shapes: the smallest that cross the boundary.  make_synthetic_panel(K, nSNPs=340, seed=515, nMaxDH=255) has 11 grids, a ragged
last grid of 20 SNPs and special haplotypes (code 0) at grids 2 and 9; K = 57 344 (the control: 14 chunk rows, the last built
variant), 57 345 (15 rows), 65 536 (16, exactly full) and 70 001 (18, ragged).  Before the geometry every test here but the
control failed with QA_ERR_UNSUPPORTED ("limited to K <= 57 344", "exceeds the on-chip capacity of the reference-order
validation full-pass kernels") or "K exceeds the on-chip capacity of the full-pass kernels".
"""

import numpy as np
import pytest

from tests.testhooks import last_plan, launch_set
from tests.util import label_gl, thin_cols

pytestmark = pytest.mark.gpu

KIND_F64_REF = 4   # csrc/pass_layout.hpp
K_TOP = 5


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


_PANELS = {}


def _panel(K):
    """The boundary panels: 11 grids, the last of 20 SNPs, 27-32 special haplotypes (12 or more at each of grids 2 and 9, none
    elsewhere), no two haplotypes alike.  Asserted, so that a change of the generator cannot hollow the tests out."""
    from quilt_amd.synth import make_synthetic_panel
    if K not in _PANELS:
        p = make_synthetic_panel(K=K, nSNPs=340, seed=515, nMaxDH=255)
        assert (p.K, p.nGrids, p.nSNPs - 32 * (p.nGrids - 1)) == (K, 11, 20)
        n_sp = (np.asarray(p.hapMatcherR) == 0).sum(axis=0)   # special haplotypes per grid
        assert [int(g) for g in np.nonzero(n_sp)[0]] == [2, 9] and n_sp.min(initial=99, where=n_sp > 0) >= 12, n_sp
        assert 27 <= n_sp.sum() <= 32 and [int(g) for g in np.nonzero(np.asarray(p.eMatDH_special_grid_which))[0]] == [2, 9], n_sp
        assert len(np.unique(np.asarray(p.rhb_t), axis=0)) == K
        _PANELS[K] = p
    return _PANELS[K]


def _tie_rich_panel():
    """548 distinct haplotypes among 60 000 (15 chunk rows): list membership is decided by exact ties."""
    from quilt_amd.synth import make_1000g_like_panel
    if "ties" not in _PANELS:
        p = make_1000g_like_panel(K=60000, nSNPs=340, seed=11)
        assert len(np.unique(np.asarray(p.rhb_t), axis=0)) < p.K // 50
        _PANELS["ties"] = p
    return _PANELS["ties"]


def _sample(panel):
    from quilt_amd.synth import make_synthetic_sample
    return make_synthetic_sample(panel, seed=3, n_reads=150)


def _run_gpu(dev, gl, cols, **kw):
    from quilt_amd.reference_single import Rcpp_haploid_dosage_versus_refs
    P = dev.panel
    K, G, T = P.K, P.nGrids, P.nSNPs
    n_thin = int((cols >= 0).sum())
    out = dict(alphaHat_t=np.zeros((K, G), order="F"), c=np.ones(G), dosage=np.zeros(T),
               best_haps_stuff_list=[None] * n_thin, gamma_t=np.zeros((K, G), order="F"),
               betaHat_t=np.zeros((K, G), order="F"))
    Rcpp_haploid_dosage_versus_refs(dev, gl, gammaSmall_cols_to_get=cols, **out, **kw)
    return out


def _lists_equal(got, ref):
    assert len(got) == len(ref)
    for g, (oi, ov) in zip(got, ref):
        assert np.array_equal(g["top_matches"], oi)
        assert np.array_equal(g["top_matches_values"], ov)


def _every_output(dev, panel, oracle, symbols, always_normalize, what):
    sample = _sample(panel)
    cols = thin_cols(panel.nGrids, every=3)
    for label in (1, 2):
        gl = label_gl(panel, sample, label, oracle)
        ref = oracle.haploid_dosage_versus_refs(panel, gl, cols, return_gamma_t=True, return_betaHat_t=True,
                                                always_normalize=always_normalize, get_best_haps_from_thinned_sites=True,
                                                use_eMatDH_special_symbols=symbols)
        got = _run_gpu(dev, gl, cols, return_dosage=True, return_gamma_t=True, return_betaHat_t=True,
                       get_best_haps_from_thinned_sites=True, always_normalize=always_normalize)
        for key in ("c", "alphaHat_t", "betaHat_t", "gamma_t", "dosage"):
            assert np.array_equal(got[key], ref[key]), (what, label, key)
        _lists_equal(got["best_haps_stuff_list"], ref["best_haps"])


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the single-pass entry: every output it has
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("always_normalize", [False, True])
@pytest.mark.parametrize("symbols", [False, True])
@pytest.mark.parametrize("K", [57344, 57345, 65536, 70001])
def test_every_output_equals_the_oracle_bit_for_bit(oracle, K, symbols, always_normalize):
    """c, alphaHat_t, betaHat_t, gamma_t, the dosage and the lists of both read labels; at K = 65 536 also under sum order 2 (grid
    0's sum left to right) against the oracle's matching setting."""
    from quilt_amd.native import DevicePanel
    panel = _panel(K)
    dev = DevicePanel(panel, use_eMatDH_special_symbols=symbols)
    try:
        dev.set_sum_order(1)
        _every_output(dev, panel, oracle, symbols, always_normalize, 1)
        if K == 65536:
            try:
                oracle.set_sum_order(True)
                dev.set_sum_order(2)
                _every_output(dev, panel, oracle, symbols, always_normalize, 2)
            finally:
                oracle.set_sum_order(False)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. lists only, and a label without reads
# ---------------------------------------------------------------------------------------------------------------------------
def test_thin_pass_and_label_without_reads(oracle):
    """K = 70 001.  Lists only: alpha exists at column 0 and the thinned columns (reference-single.cpp:2264-2268).  A gl of all
    ones: every grid takes the no-variant shortcut and every haplotype ties, so each list holds all 70 001 -- the non-truncating
    top-K retry at full length."""
    from quilt_amd.native import DevicePanel
    panel = _panel(70001)
    dev = DevicePanel(panel)
    try:
        dev.set_sum_order(1)
        cols = thin_cols(panel.nGrids, every=3)
        for gl in (label_gl(panel, _sample(panel), 1, oracle), np.ones((2, panel.nSNPs), order="F")):
            ref = oracle.haploid_dosage_versus_refs(panel, gl, cols, return_dosage=False, always_normalize=False,
                                                    get_best_haps_from_thinned_sites=True)
            got = _run_gpu(dev, gl, cols, return_dosage=False, return_gamma_t=False, return_betaHat_t=False,
                           get_best_haps_from_thinned_sites=True, always_normalize=False)
            _lists_equal(got["best_haps_stuff_list"], ref["best_haps"])
            assert np.array_equal(got["c"], ref["c"])
            for g in [0] + [int(g) for g in np.nonzero(cols >= 0)[0]]:
                assert np.array_equal(got["alphaHat_t"][:, g], ref["alphaHat_t"][:, g]), g
        assert all(len(b["top_matches"]) == panel.K for b in got["best_haps_stuff_list"])
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a tie-rich panel
# ---------------------------------------------------------------------------------------------------------------------------
def test_tie_rich_panel(oracle):
    """Lists of hundreds of exactly tied haplotypes at K_top_matches = 5: the membership is the oracle's, with c and the dosage."""
    from quilt_amd.native import DevicePanel
    panel = _tie_rich_panel()
    dev = DevicePanel(panel)
    try:
        dev.set_sum_order(1)
        cols = thin_cols(panel.nGrids, every=3)
        sample = _sample(panel)
        longest = 0
        for label in (1, 2):
            gl = label_gl(panel, sample, label, oracle)
            ref = oracle.haploid_dosage_versus_refs(panel, gl, cols, K_top_matches=K_TOP, always_normalize=False,
                                                    get_best_haps_from_thinned_sites=True)
            got = _run_gpu(dev, gl, cols, return_dosage=True, return_gamma_t=False, return_betaHat_t=False,
                           get_best_haps_from_thinned_sites=True, always_normalize=False, K_top_matches=K_TOP)
            _lists_equal(got["best_haps_stuff_list"], ref["best_haps"])
            assert np.array_equal(got["c"], ref["c"])
            assert np.array_equal(got["dosage"], ref["dosage"])
            longest = max(longest, max(len(oi) for oi, _ in ref["best_haps"]))
        assert longest > 100, "no long tied list on this input: the test must discriminate"
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. launch sets, both forms of the kernels
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [57345, 65536])
def test_launch_sets_in_both_forms_equal_the_oracle(oracle, K):
    """Three passes (dosage, lists only, dosage) in one launch set, always_normalize off and on: c, dosage, list pointers,
    indices and values with the batched form off and on are the same arrays, and the oracle's.  The launch set ran the
    reference-order kind and carved no more than its plan."""
    from quilt_amd.native import DevicePanel
    panel = _panel(K)
    cols = thin_cols(panel.nGrids, every=3)
    n_thin = int((cols >= 0).sum())
    sample = _sample(panel)
    gls = [label_gl(panel, sample, 1, oracle), label_gl(panel, sample, 2, oracle)]
    gls.append(gls[0] * gls[1])   # (every read of the sample on one haplotype)
    gl = np.ascontiguousarray(np.stack([g.T for g in gls]))   # [P][T][2]
    flags = np.array([1, 0, 1], dtype=np.int32)
    dev = DevicePanel(panel)
    try:
        dev.set_dosage_precision(64)
        dev.set_sum_order(1)
        for an in (0, 1):
            res = {}
            for on in (0, 1):
                dev.set_sum_order_batched(on)
                res[on] = launch_set(dev, gl, flags, cols, K_TOP, an)
                h = last_plan()
                assert h["kind"] == KIND_F64_REF and h["P"] == 3, h
                assert h["carved"] <= h["fixed"] + h["P"] * h["planned"], h
            for key in res[0]:
                assert np.array_equal(res[1][key], res[0][key]), (an, key)
            got = res[1]
            for p in range(3):
                ref = oracle.haploid_dosage_versus_refs(panel, gls[p], cols, K_top_matches=K_TOP, always_normalize=bool(an),
                                                        get_best_haps_from_thinned_sites=True)
                assert np.array_equal(got["c"][p], ref["c"]), (an, p)
                if flags[p]:
                    assert np.array_equal(got["dosage"][p], ref["dosage"]), (an, p)
                for j, (oi, ov) in enumerate(ref["best_haps"]):
                    a, b = got["list_ptr"][p * n_thin + j], got["list_ptr"][p * n_thin + j + 1]
                    assert np.array_equal(got["list_idx"][a:b], oi), (an, p, j)
                    assert np.array_equal(got["list_val"][a:b], ov), (an, p, j)
    finally:
        dev.set_sum_order_batched(0)
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the gamma column of hla_run
# ---------------------------------------------------------------------------------------------------------------------------
def test_gamma_column_is_the_oracles():
    """qa_fullpass_reads_select_gamma_batch at K = 65 536: the column at the first grids, an even interior grid, both grids with
    special haplotypes and the last grid equals the oracle's gamma_t[:, g]; the call's other outputs equal those of the same
    call without a gamma grid; with the batched form off and on."""
    from quilt_amd.driver import HipBackend
    from quilt_amd.native import DevicePanel
    from tests.hla_backend import oracle_gamma_t
    panel = _panel(65536)
    cols = thin_cols(panel.nGrids, every=3)
    samples = [_sample(panel)]
    rng = np.random.default_rng(5)
    cs = [0, 0]
    labels = [rng.integers(1, 3, size=samples[0].nReads).astype(np.int32) for _ in cs]
    which = [np.sort(rng.choice(panel.K, 64, replace=False) + 1).astype(np.int32) for _ in cs]
    sel = dict(Ksubset=64, Knew=32, which=which, seeds=[31, 32])
    ref = oracle_gamma_t(panel, samples, cs, labels)
    dev = DevicePanel(panel)
    try:
        dev.set_dosage_precision(64)
        dev.set_sum_order(1)
        be = HipBackend(dev)
        for on in (0, 1):
            dev.set_sum_order_batched(on)
            d0, _, c0, n0, s0 = (x.copy() if x is not None else None
                                 for x in be.fullpass_reads_batch(samples, cs, labels, [1, 1], [1, 1], cols, K_TOP, 1e-10, 8, select=sel))
            for g in (0, 1, 2, 6, 9, 10):
                d, _, c, nx, st, gam = be.fullpass_reads_batch(samples, cs, labels, [1, 1], [1, 1], cols, K_TOP, 1e-10, 8, select=sel,
                                                               gamma_grid=g)
                assert np.array_equal(d, d0) and np.array_equal(c, c0) and np.array_equal(nx, n0) and np.array_equal(st, s0), (on, g)
                for ci in range(len(cs)):
                    for l in range(2):
                        assert np.array_equal(gam[ci, l], ref[ci][l][:, g]), (on, g, ci, l)
    finally:
        dev.set_sum_order_batched(0)
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the pipeline
# ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_equals_the_cpu_pipeline_on_the_tie_rich_panel():
    """impute_samples on the device in validation mode against the driver over the CPU oracle, two driver seeds: read labels,
    dosage, genotype posteriors and phased haplotypes bit for bit; once more with the batched form.  (Production mode is not
    asserted here.)"""
    from quilt_amd.driver import Driver, DriverParams
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from tests.oracle_backend import OracleBackend
    panel = _tie_rich_panel()
    sample = _sample(panel)
    cpu_be = OracleBackend(panel, n_threads=8)
    dev = DevicePanel(panel)
    try:
        dev.set_dosage_precision(64)
        dev.set_sum_order(True)
        for seed in (1, 2):
            prm = DriverParams(nGibbsSamples=2, Ksubset=128, Knew=128, seed=seed)
            cpu = Driver(panel, cpu_be, prm).run([sample])[0]
            assert np.ptp(cpu.dosage) > 0
            for on in (0, 1):
                dev.set_sum_order_batched(on)
                got = impute_samples([dev], [sample], prm)[0]
                assert np.array_equal(got.read_labels, cpu.read_labels), (seed, on)
                assert np.array_equal(got.dosage, cpu.dosage), (seed, on)
                assert np.array_equal(got.gp_t, cpu.gp_t), (seed, on)
                assert np.array_equal(got.phasing_haps, cpu.phasing_haps), (seed, on)
    finally:
        dev.set_sum_order_batched(0)
        dev.close()
