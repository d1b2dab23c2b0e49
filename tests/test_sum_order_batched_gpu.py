"""The reference-order full-panel passes at batch throughput (qa_panel_set_sum_order_batched, csrc/fullpass_ord.hip): one wave per
pass instead of one 256-thread workgroup, the state in the pass's device scratch instead of LDS -- and the SAME arithmetic in the
same order as validation mode (qa_panel_set_sum_order 1 | 2, csrc/fullpass_ref.hip), which equals the CPU restatement
(oracle/fullpass.c) bit for bit.  So every comparison here is np.array_equal: switch on against switch off, and switch on against
the oracle.  No tolerance: fp64, the same operations on the same operands.

Through what a caller has: qa_fullpass_batch, qa_fullpass_reads_batch / _select_batch / _select_gamma_batch, impute_samples.  The
batched entries return dosage, lists and counts but neither c nor a choice of always_normalize, and they cut a request into
launch sets of like passes; csrc/fullpass_testhook.h's qa_fullpass_launch_set runs ONE launch set with per-pass flags, always_normalize
and c, which is how the shapes below reach the new kernels with every pass of the set in one launch.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests.testhooks import launch_set

pytestmark = pytest.mark.gpu

QA_ERR_INVALID = -2   # include/quilt_amd.h
K_TOP = 5


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def _set_batched(dev, on):
    from quilt_amd.native import lib
    return lib().qa_panel_set_sum_order_batched(dev.handle, C.c_int32(on))


_PANELS = {}


def _panel(K, G, dup=False, nMaxDH=255, seed=0):
    """T = 32 G - 5 SNPs: the last grid is short.  dup: the second half of the haplotypes repeats the first -- every haplotype
    ties with its copy at every grid.  A small nMaxDH leaves most of a grid's distinct words to the special lists."""
    from quilt_amd.synth import make_synthetic_panel
    from tests.util import panel_from_rhb
    key = (K, G, dup, nMaxDH, seed)
    if key not in _PANELS:
        T = 32 * G - 5
        p = make_synthetic_panel(K=K, nSNPs=T, seed=1000 + 7 * K + G + seed, nMaxDH=nMaxDH, stress_grids=(1, 2))
        if dup and K > 1:
            rhb = np.array(p.rhb_t, order="F")
            rhb[K - K // 2:, :] = rhb[:K // 2, :]
            q = panel_from_rhb(rhb, p.transMatRate_t, T, nMaxDH, p.ref_error)
            p = dataclasses.replace(q, L=p.L, L_grid=p.L_grid, grid=p.grid)
        _PANELS[key] = p
    return _PANELS[key]


def _gls(panel, n, seed):
    """n stacked gl matrices as the ABI wants them ([n][T][2]).  Pass 0: every SNP informative.  Pass 1: a label without reads
    (all ones: every grid takes the no-variant shortcut, every haplotype ties).  Pass 2: nothing on grid 1 (the backward pass's
    own grid-1 branch).  The rest: reads on a tenth to a half of the SNPs."""
    rng = np.random.default_rng(seed)
    T = panel.nSNPs
    gl = np.ones((n, T, 2))
    for p in range(n):
        frac = 1.0 if p == 0 else 0.0 if p == 1 else rng.uniform(0.1, 0.5)
        hit = rng.random(T) < frac
        gl[p, hit, :] = rng.uniform(0.05, 1.0, size=(int(hit.sum()), 2))
        if p == 2:
            gl[p, 32:64, :] = 1.0
    return np.ascontiguousarray(gl)


def _thin(G):
    """thinned grids that include grid 0 and the last grid"""
    cols = np.full(G, -1, dtype=np.int32)
    w = np.unique(np.r_[0, np.arange(2, G - 1, 3), G - 1])
    cols[w] = np.arange(len(w), dtype=np.int32)
    return cols


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def _mixed_flags(P):
    """dosage passes (with lists when the launch set has them) and list-only passes in one launch set"""
    return (np.arange(P) % 3 != 1).astype(np.int32)


def _both_forms(dev, gl, flags, cols, K_top, an, what):
    _set_batched(dev, 0)
    off = launch_set(dev, gl, flags, cols, K_top, an)
    assert _set_batched(dev, 1) == 0
    on = launch_set(dev, gl, flags, cols, K_top, an)
    _set_batched(dev, 0)
    _same(on, off, what)
    return on


# ---------------------------------------------------------------------------------------------------------------------------
# 1. bit-identity with validation mode
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2, 3, 9])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 300, 1000])
def test_switch_on_equals_switch_off_bit_for_bit(K, G):
    """Every K around the wave's width and beyond one 64-block, every G with its own branch (1: grid 0 alone; 2, 3: the backward
    grid-1 branch right below the last grid; 9), T = 32 G - 5; sum order 1 and 2, always_normalize 0 and 1, special symbols on
    (with a dictionary of 6 words: most haplotypes of a grid are specials) and off, P = 2, 65, 130 with dosage and list-only
    passes mixed in the launch set, lists at grid 0 and the last grid, and without lists (dosage alone).  K = 300: the second half
    of the panel duplicates the first, so every list is an exact tie."""
    from quilt_amd.native import DevicePanel
    cols = _thin(G)
    for symbols in (False, True):
        panel = _panel(K, G, dup=(K == 300), nMaxDH=6 if symbols else 255)
        dev = DevicePanel(panel, use_eMatDH_special_symbols=symbols)
        try:
            dev.set_dosage_precision(64)
            for i, P in enumerate((2, 65, 130)):
                gl = _gls(panel, P, seed=K + G + P)
                for order in (1, 2):
                    dev.set_sum_order(order)
                    for an in (0, 1):
                        what = (symbols, P, order, an)
                        got = _both_forms(dev, gl, _mixed_flags(P), cols, K_TOP, an, what + ("mixed",))
                        assert np.all(np.isfinite(got["dosage"])) and np.all(got["c"] > 0)
                        if (order + an + i) % 2 == 0:   # (dosage alone: half of the combinations, every P / order / an among them)
                            _both_forms(dev, gl, np.ones(P, dtype=np.int32), cols, 0, an, what + ("dosage",))
        finally:
            dev.close()


@pytest.mark.parametrize("rank_bits", [64, 32])
def test_public_batch_entries_with_the_switch_on_and_off(rank_bits):
    """qa_fullpass_batch (runs of dosage and of thin passes: dosage rows, full lists) and qa_fullpass_reads_batch /
    qa_fullpass_reads_select_batch (dosage, ordered list heads, true counts, the next small panels) on a panel with duplicated
    haplotypes: the same arrays with the switch on and off.  Ranking precision 64: lists from list-only passes beside the
    dosage passes; 32: one pass yields both."""
    from quilt_amd.driver import HipBackend
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_synthetic_sample
    panel = _panel(300, 9, dup=True)
    cols = _thin(panel.nGrids)
    dev = DevicePanel(panel)
    try:
        dev.set_dosage_precision(64)
        dev.set_ranking_precision(rank_bits)
        dev.set_sum_order(1)
        be = HipBackend(dev)
        gls = [np.asfortranarray(g.T) for g in _gls(panel, 7, seed=5)]
        wd = [1, 1, 1, 0, 0, 1, 1]
        samples = [make_synthetic_sample(panel, seed=900 + i, n_reads=60) for i in range(2)]
        rng = np.random.default_rng(8)
        cs = [0, 1, 0, 1]
        labels = [rng.integers(1, 3, size=samples[s].nReads).astype(np.int32) for s in cs]
        which = [np.sort(rng.choice(panel.K, 64, replace=False) + 1).astype(np.int32) for _ in cs]
        sel = dict(Ksubset=64, Knew=32, which=which, seeds=[11, 12, 13, 14])
        res = {}
        for on in (0, 1):
            assert _set_batched(dev, on) == 0
            dosage, best = be.fullpass_batch(gls, wd, cols, K_TOP)
            d2, top, cnt = be.fullpass_reads_batch(samples, cs, labels, [1, 0, 1, 1], [1, 1, 0, 1], cols, K_TOP, 1e-10, 8)
            d2 = d2.copy()
            if rank_bits == 64:   # (the device-side selection: the driver's path, fp64 ranking)
                d3, _, cnt3, nxt, status = be.fullpass_reads_batch(samples, cs, labels, [1, 1, 1, 1], [1, 1, 1, 1], cols, K_TOP, 1e-10, 8,
                                                                   select=sel)
            else:
                d3, _, cnt3 = be.fullpass_reads_batch(samples, cs, labels, [1, 1, 1, 1], [1, 1, 1, 1], cols, K_TOP, 1e-10, 8)
                nxt = status = np.zeros(0)
            res[on] = dict(dosage=np.stack(dosage), idx=np.concatenate([b["top_matches"] for p in best for b in p]),
                           val=np.concatenate([b["top_matches_values"] for p in best for b in p]),
                           n=np.array([len(b["top_matches"]) for p in best for b in p]),
                           d2=d2, top=top, cnt=cnt, d3=d3.copy(), cnt3=cnt3, nxt=nxt, status=status)
        assert res[0]["n"].max() > 1 and res[0]["cnt"].max() > 1
        _same(res[1], res[0], rank_bits)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. bit-identity with the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,G,symbols", [(65, 3, True), (300, 9, False), (300, 2, True), (1000, 9, True), (64, 1, False), (65, 2, True)])
def test_switch_on_equals_the_oracle_bit_for_bit(oracle, K, G, symbols):
    """c, dosage and the lists of every pass of a launch set on the batched kernels against oracle/fullpass.c under the matching
    qo_set_sum_order: sum order 1 (Armadillo's two accumulators at grid 0) and 2 (left to right), always_normalize 0 and 1."""
    from quilt_amd.native import DevicePanel
    panel = _panel(K, G, dup=(K == 300), nMaxDH=6 if symbols else 255)
    cols = _thin(G)
    n_thin = int((cols >= 0).sum())
    P = 5
    gl = _gls(panel, P, seed=3 * K + G)
    flags = _mixed_flags(P)
    dev = DevicePanel(panel, use_eMatDH_special_symbols=symbols)
    try:
        dev.set_dosage_precision(64)
        assert _set_batched(dev, 1) == 0
        for order, ltr in ((1, False), (2, True)):
            oracle.set_sum_order(ltr)
            dev.set_sum_order(order)
            for an in (0, 1):
                got = launch_set(dev, gl, flags, cols, K_TOP, an)
                alone = launch_set(dev, gl, np.ones(P, dtype=np.int32), cols, 0, an)   # every pass a dosage pass, the one without reads too
                for p in range(P):
                    ref = oracle.haploid_dosage_versus_refs(panel, np.asfortranarray(gl[p].T), cols, K_top_matches=K_TOP,
                                                            always_normalize=bool(an), get_best_haps_from_thinned_sites=True,
                                                            use_eMatDH_special_symbols=symbols)
                    assert np.array_equal(got["c"][p], ref["c"]), (order, an, p)
                    assert np.array_equal(alone["c"][p], ref["c"]), (order, an, p)
                    assert np.array_equal(alone["dosage"][p], ref["dosage"]), (order, an, p)
                    if flags[p]:
                        assert np.array_equal(got["dosage"][p], ref["dosage"]), (order, an, p)
                    for j, (oi, ov) in enumerate(ref["best_haps"]):
                        a, b = got["list_ptr"][p * n_thin + j], got["list_ptr"][p * n_thin + j + 1]
                        assert np.array_equal(got["list_idx"][a:b], oi), (order, an, p, j)
                        assert np.array_equal(got["list_val"][a:b], ov), (order, an, p, j)
    finally:
        oracle.set_sum_order(False)
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the gamma column of hla_run
# ---------------------------------------------------------------------------------------------------------------------------
def test_gamma_column_equals_validation_modes():
    """qa_fullpass_reads_select_gamma_batch: the column at grid 0, at an odd grid and at the last grid, and every other output of
    the call, with the switch on and off."""
    from quilt_amd.driver import HipBackend
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_synthetic_sample
    panel = _panel(300, 9, dup=True)
    cols = _thin(panel.nGrids)
    dev = DevicePanel(panel)
    try:
        dev.set_dosage_precision(64)
        dev.set_sum_order(1)
        be = HipBackend(dev)
        samples = [make_synthetic_sample(panel, seed=700 + i, n_reads=60) for i in range(2)]
        rng = np.random.default_rng(4)
        cs = [0, 1, 0]
        labels = [rng.integers(1, 3, size=samples[s].nReads).astype(np.int32) for s in cs]
        which = [np.sort(rng.choice(panel.K, 64, replace=False) + 1).astype(np.int32) for _ in cs]
        sel = dict(Ksubset=64, Knew=32, which=which, seeds=[21, 22, 23])
        for grid in (0, 5, panel.nGrids - 1):
            res = {}
            for on in (0, 1):
                assert _set_batched(dev, on) == 0
                dosage, _, cnt, nxt, status, gamma = be.fullpass_reads_batch(samples, cs, labels, [1] * 3, [1] * 3, cols, K_TOP, 1e-10, 8,
                                                                             select=sel, gamma_grid=grid)
                res[on] = dict(dosage=dosage.copy(), cnt=cnt, nxt=nxt, status=status, gamma=gamma)
            assert res[0]["gamma"].max() > 0
            _same(res[1], res[0], grid)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the scope of the switch
# ---------------------------------------------------------------------------------------------------------------------------
def test_switch_is_refused_outside_0_and_1_and_changes_nothing_else(oracle):
    """Values 2 and -1: QA_ERR_INVALID.  With sum_order = 0 the production kernels' outputs are the same arrays with the switch on
    and off; so is a single pass (P = 1: qa_Rcpp_haploid_dosage_versus_refs with its matrices) in validation mode."""
    from quilt_amd.driver import HipBackend
    from quilt_amd.native import DevicePanel
    from quilt_amd.reference_single import Rcpp_haploid_dosage_versus_refs
    panel = _panel(300, 9, dup=True)
    cols = _thin(panel.nGrids)
    K, G, T = panel.K, panel.nGrids, panel.nSNPs
    dev = DevicePanel(panel)
    try:
        for bad in (2, -1):
            assert _set_batched(dev, bad) == QA_ERR_INVALID
        dev.set_dosage_precision(64)
        gl = _gls(panel, 6, seed=12)

        def single():
            out = dict(alphaHat_t=np.zeros((K, G), order="F"), c=np.ones(G), dosage=np.zeros(T), gamma_t=np.zeros((K, G), order="F"),
                       betaHat_t=np.zeros((K, G), order="F"), best_haps_stuff_list=[None] * int((cols >= 0).sum()))
            Rcpp_haploid_dosage_versus_refs(dev, np.asfortranarray(gl[0].T), gammaSmall_cols_to_get=cols, return_dosage=True,
                                            return_gamma_t=True, return_betaHat_t=True, get_best_haps_from_thinned_sites=True, **out)
            lists = out.pop("best_haps_stuff_list")
            out["idx"] = np.concatenate([b["top_matches"] for b in lists])
            out["val"] = np.concatenate([b["top_matches_values"] for b in lists])
            return out

        for order in (0, 1):
            dev.set_sum_order(order)
            res = {}
            for on in (0, 1):
                assert _set_batched(dev, on) == 0
                res[on] = dict(single=single())
                if order == 0:   # the production kernels behind the batched entry
                    dosage, best = HipBackend(dev).fullpass_batch([np.asfortranarray(g.T) for g in gl], [1, 1, 0, 0, 1, 1], cols, K_TOP)
                    res[on]["batch"] = dict(dosage=np.stack(dosage), idx=np.concatenate([b["top_matches"] for p in best for b in p]),
                                            val=np.concatenate([b["top_matches_values"] for p in best for b in p]))
            for key in res[0]:
                _same(res[1][key], res[0][key], (order, key))
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the pipeline
# ---------------------------------------------------------------------------------------------------------------------------
def test_pipeline_ends_the_same_with_the_switch_on():
    """impute_samples for three samples of a K = 300 panel whose second half duplicates the first, 8 grids, a shortened Gibbs
    schedule, sum order 1: dosage, genotype posteriors, phasing haplotypes and read labels with the switch on equal those with
    it off, bit for bit."""
    from quilt_amd.driver import DriverParams
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_synthetic_sample
    panel = _panel(300, 8, dup=True, seed=1)
    samples = [make_synthetic_sample(panel, seed=40 + i, n_reads=60) for i in range(3)]
    prm = DriverParams(nGibbsSamples=2, n_seek_its=2, Ksubset=64, Knew=32, small_ref_panel_gibbs_iterations=5,
                       small_ref_panel_block_gibbs_iterations=(2,), seed=9)
    dev = DevicePanel(panel)
    try:
        dev.set_dosage_precision(64)
        dev.set_sum_order(1)
        res = {}
        for on in (0, 1):
            assert _set_batched(dev, on) == 0
            res[on] = impute_samples([dev], samples, prm)
        for a, b in zip(res[1], res[0]):
            assert np.array_equal(a.dosage, b.dosage)
            assert np.array_equal(a.gp_t, b.gp_t)
            assert np.array_equal(a.phasing_haps, b.phasing_haps)
            assert np.array_equal(a.read_labels, b.read_labels)
        assert np.ptp(res[0][0].dosage) > 0
    finally:
        dev.close()
