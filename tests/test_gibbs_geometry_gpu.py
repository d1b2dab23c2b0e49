"""Every Ksubset geometry of the Gibbs samplers against the fp64 CPU oracle.

The samplers are compiled once per "rows per lane" count NE = ceil(Ksubset / 64) and the launchers switch on it
(csrc/gibbs.hip: launch_gibbs; csrc/gibbs3.hip: launch_gibbs3 / launch_block3).  Per NE this file runs three sizes -- a full last
chunk (Ks = 64 NE), ONE valid row in the last chunk (Ks = 64 (NE - 1) + 1: 63 lanes of the last row masked) and one size strictly
between -- plus Ks = 1 and 2:

  diploid (k_ematread / k_gibbs / k_happrobs)      NE 1..16, both initialisations, shard passes on, state returned
  rare + common form (k_happrobs_rc's LDS sizing)  NE 1..16
  NIPT (k_gibbs3 / k_block3, block passes on)      NE 1..10, once more ending on a block pass; NE 11..16 are not built and must be
                                                   refused with QA_ERR_UNSUPPORTED before any device work

and, at one NE per width of the compact read emissions (4, 8, 12, 16 pattern bytes per lane: gibbs_dev.hpp padb_of): ONT-like reads
(every emission dense), disable_read_category_usage, and three chains of different read counts in one call.

Bar (the project's own, tests/test_gibbs_gpu.py): labels and H_class identical under the same uniforms; eMatGrid, alpha, beta, c
and hapProbs / genProbs to 1e-9 relative.  The oracle returns status 0 for every input here (asserted), so no case has a skip or
an "allowed to differ" branch.
"""
import numpy as np
import pytest

from tests.util import GIBBS_RTOL as RTOL, gibbs_compare, gibbs_setup

pytestmark = pytest.mark.gpu

NE_DIPLOID = list(range(1, 17))   # QA_KSUBSET_MAX = 1024
NE_NIPT = list(range(1, 11))      # QA_KSUBSET_MAX_NIPT = 640
NE_NIPT_REFUSED = list(range(11, 17))
QA_ERR_UNSUPPORTED = -3
# one NE per pattern width (4, 8, 12, 16 bytes per lane), chosen among the builds no other test reaches
NE_PER_WIDTH_ONT = [3, 7, 11, 15]
NE_PER_WIDTH_NOCAT = [2, 5, 9, 13]
NE_PER_WIDTH_BATCH = [4, 8, 12, 14]
NE_PER_WIDTH_BATCH_NIPT = [3, 7, 9]   # (4, 8 and 12 bytes: ten rows per lane is the largest NIPT build)


def sizes_of(ne):
    """(one valid row in the last chunk, strictly between, full last chunk); the middle size moves with NE so that the number
    of masked lanes differs from build to build."""
    lo, hi = 64 * (ne - 1) + 1, 64 * ne
    return lo, lo + 1 + (13 * ne) % 62, hi


def ks_list(nes, extra=()):
    out = sorted(set(extra) | {k for ne in nes for k in sizes_of(ne)})
    assert all(lo < mid < hi for lo, mid, hi in map(sizes_of, nes))
    return out


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def dev(medium_panel):
    from quilt_amd.native import DevicePanel
    assert medium_panel.K >= 1024
    d = DevicePanel(medium_panel)
    yield d
    d.close()


def _moved(ref, H0):
    """The sweeps did something: a sampler that returned its starting labels would not pass for one that works."""
    return (ref["H"] != H0).mean()


# ---------------------------------------------------------------------------------------------------------------------------
# diploid
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("init_iter", [False, True])
@pytest.mark.parametrize("Ks", ks_list(NE_DIPLOID, extra=(1, 2)))
def test_diploid_every_geometry(medium_panel, dev, oracle, Ks, init_iter):
    panel = medium_panel
    s, which, H0, ru, rs, fr = gibbs_setup(panel, 11, Ks, 600)
    nb = np.diff(s.read_ptr)
    assert (nb > 5).any() and (nb <= 5).any()   # both emission forms: dense columns and the compact table
    ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, rs, gibbs_initialize_iteratively=init_iter)
    assert ref["status"] == 0
    if Ks > 1:
        assert _moved(ref, H0) > 0.1
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    got = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, rs, gibbs_initialize_iteratively=init_iter, return_state=True)
    gibbs_compare(got, ref, Ks)


@pytest.mark.parametrize("ne", NE_PER_WIDTH_ONT)
def test_diploid_ont_reads_per_pattern_width(medium_panel, dev, oracle, ne):
    """Long noisy reads: every emission is a dense column of Ksp doubles (k_ematread's other output)."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    panel = medium_panel
    Ks = sizes_of(ne)[1]
    s, which, H0, ru, rs, fr = gibbs_setup(panel, 5, Ks, 40, mode="ont")
    assert (np.diff(s.read_ptr) > 5).all()
    ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, rs)
    got = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, rs, return_state=True)
    gibbs_compare(got, ref, Ks)


@pytest.mark.parametrize("ne", NE_PER_WIDTH_NOCAT)
def test_diploid_without_read_categories_per_pattern_width(medium_panel, dev, oracle, ne):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    panel = medium_panel
    Ks = sizes_of(ne)[0]
    s, which, H0, ru, rs, fr = gibbs_setup(panel, 11, Ks, 600)
    ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, rs, disable_read_category_usage=True)
    got = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, rs, disable_read_category_usage=True, return_state=True)
    gibbs_compare(got, ref, Ks)


@pytest.mark.parametrize("ne", NE_PER_WIDTH_BATCH)
def test_diploid_batch_equals_one_at_a_time(medium_panel, dev, oracle, ne):
    """Three chains of different read counts in one call: each the oracle's, and bit for bit what a call of its own returns."""
    from quilt_amd.gibbs_nipt import forwardBackwardGibbsNIPT_batch, rcpp_forwardBackwardGibbsNIPT
    panel = medium_panel
    Ks = sizes_of(ne)[1]
    setups = [gibbs_setup(panel, 200 + i, Ks, 150 + 170 * i) for i in range(3)]
    assert len({x[0].nReads for x in setups}) == 3
    got = forwardBackwardGibbsNIPT_batch(dev, [x[0] for x in setups], [x[1] for x in setups], [x[2] for x in setups],
                                         [x[3] for x in setups], [x[5] for x in setups], [x[4] for x in setups])
    for g, (s, which, H0, ru, rs, fr) in zip(got, setups):
        ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, rs)
        one = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, rs, return_state=True)
        gibbs_compare(one, ref, Ks)
        assert not g["underflow_problem"]
        for f in ("H", "H_class", "hapProbs_t", "genProbsM_t", "genProbsF_t"):
            assert np.array_equal(g[f], one[f]), f


# ---------------------------------------------------------------------------------------------------------------------------
# rare + common form (qa_gibbs_batch_rare_common)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rare(medium_panel, dev):
    from quilt_amd.native import DeviceRareCommon
    from quilt_amd.synth import make_rare_common, make_synthetic_sample_rare_common
    rc = make_rare_common(medium_panel, 23, carriers=(0, 6))
    _, s_all = make_synthetic_sample_rare_common(medium_panel, rc, 24, n_reads=600)
    drc = DeviceRareCommon(dev, rc)
    yield rc, s_all, drc
    drc.close()


@pytest.mark.parametrize("Ks", ks_list(NE_DIPLOID, extra=(1, 2)))
def test_rare_common_every_geometry(medium_panel, dev, rare, oracle, Ks):
    """The all-SNP call, with the reference's arguments for it (read categories off): k_happrobs_rc's dynamic LDS at every Ksp."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    panel = medium_panel
    rc, s_all, drc = rare
    rng = np.random.default_rng(23 + 17 + Ks)
    which = np.sort(rng.choice(panel.K, Ks, replace=False)).astype(np.int32) + 1
    H0 = rng.integers(1, 3, size=s_all.nReads).astype(np.int32)
    ru, rs = rng.random(s_all.nReads * 21), rng.random(3 * (rc.nGrids_all - 1))
    ref = oracle.forwardBackwardGibbsNIPT(panel, s_all, which, H0, ru, 0, rs, disable_read_category_usage=True, rare_common=rc)
    assert ref["status"] == 0
    if Ks > 1:
        assert _moved(ref, H0) > 0.1
    got = rcpp_forwardBackwardGibbsNIPT(dev, s_all, which, H0, ru, 0, rs, disable_read_category_usage=True, return_state=True,
                                        rare_common=drc)
    assert not got["underflow_problem"]
    assert np.array_equal(got["H"], ref["H"]), f"{(got['H'] != ref['H']).sum()} labels differ"
    assert np.array_equal(got["H_class"], ref["H_class"])
    for h in range(2):
        np.testing.assert_allclose(got[f"eMatGrid_t{h + 1}"], ref["eMatGrid_t"][h], rtol=RTOL)
        np.testing.assert_allclose(got[f"alphaHat_t{h + 1}"], ref["alphaHat_t"][h], rtol=RTOL, atol=1e-300)
        np.testing.assert_allclose(got[f"betaHat_t{h + 1}"], ref["betaHat_t"][h], rtol=RTOL, atol=1e-300)
        np.testing.assert_allclose(got[f"c{h + 1}"], ref["c"][h], rtol=RTOL)
    np.testing.assert_allclose(got["hapProbs_t"][:2], ref["hapProbs_t"][:2], rtol=RTOL, atol=1e-14)
    np.testing.assert_allclose(got["genProbsM_t"], ref["genProbsM_t"], rtol=RTOL, atol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------------
# NIPT (three labels, block Gibbs on)
# ---------------------------------------------------------------------------------------------------------------------------
def nipt_setup(panel, seed, Ks, n_reads, ff=0.2):
    from quilt_amd.synth import make_synthetic_sample
    s = make_synthetic_sample(panel, seed=seed, n_reads=n_reads, ff=ff)
    rng = np.random.default_rng(seed + 17)
    which = np.sort(rng.choice(panel.K, Ks, replace=False)).astype(np.int32) + 1
    R = s.nReads
    H0 = rng.choice([1, 2, 3], p=[0.5, 0.4, 0.1], size=R).astype(np.int32)
    ru, rb, rr = rng.random(R * 21), rng.random(3 * R), rng.random(3 * R)
    fr = int(rng.integers(0, R))
    return s, which, H0, ru, rb, rr, fr


def nipt_compare(got, ref):
    assert ref["status"] == 0 and not got["underflow_problem"]
    assert np.array_equal(got["H"], ref["H"]), f"{(got['H'] != ref['H']).sum()} labels differ"
    assert np.array_equal(got["H_class"], ref["H_class"])
    np.testing.assert_allclose(got["hapProbs_t"], ref["hapProbs_t"], rtol=RTOL, atol=1e-14)
    np.testing.assert_allclose(got["genProbsM_t"], ref["genProbsM_t"], rtol=RTOL, atol=1e-14)
    np.testing.assert_allclose(got["genProbsF_t"], ref["genProbsF_t"], rtol=RTOL, atol=1e-14)


@pytest.mark.parametrize("n_burn", [20, 9])   # 9: the call ends right after the last block pass
@pytest.mark.parametrize("Ks", ks_list(NE_NIPT, extra=(2,)))
def test_nipt_every_geometry(medium_panel, dev, oracle, Ks, n_burn):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    panel = medium_panel
    ff = 0.2
    s, which, H0, ru, rb, rr, fr = nipt_setup(panel, 11, Ks, 600, ff)
    nb = np.diff(s.read_ptr)
    assert (nb > 5).any() and (nb <= 5).any()
    ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, np.zeros(3 * panel.nGrids), ff=ff, n_gibbs_burn_in_its=n_burn,
                                          runif_block=rb, runif_resample=rr)
    assert ref["status"] == 0 and _moved(ref, H0) > 0.1
    got = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, None, ff=ff, n_gibbs_burn_in_its=n_burn, runif_block=rb,
                                        runif_resample=rr)
    nipt_compare(got, ref)


@pytest.mark.parametrize("ne", NE_PER_WIDTH_BATCH_NIPT)
def test_nipt_batch_equals_one_at_a_time(medium_panel, dev, oracle, ne):
    from quilt_amd.gibbs_nipt import forwardBackwardGibbsNIPT_batch, rcpp_forwardBackwardGibbsNIPT
    panel = medium_panel
    Ks = sizes_of(ne)[1]
    ffs = [0.2, 0.1, 0.3]
    setups = [nipt_setup(panel, 300 + i, Ks, 150 + 170 * i, ffs[i]) for i in range(3)]
    assert len({x[0].nReads for x in setups}) == 3
    got = forwardBackwardGibbsNIPT_batch(dev, [x[0] for x in setups], [x[1] for x in setups], [x[2] for x in setups],
                                         [x[3] for x in setups], [x[6] for x in setups], None, ff=ffs,
                                         runif_block=[x[4] for x in setups], runif_resample=[x[5] for x in setups])
    for g, ff, (s, which, H0, ru, rb, rr, fr) in zip(got, ffs, setups):
        ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, np.zeros(3 * panel.nGrids), ff=ff, runif_block=rb,
                                              runif_resample=rr)
        one = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, None, ff=ff, runif_block=rb, runif_resample=rr)
        nipt_compare(one, ref)
        assert not g["underflow_problem"]
        for f in ("H", "H_class", "hapProbs_t", "genProbsM_t", "genProbsF_t"):
            assert np.array_equal(g[f], one[f]), f


# ---------------------------------------------------------------------------------------------------------------------------
# what stays refused: the NIPT sampler above Ksubset = 640, either sampler above 1024
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ks", ks_list(NE_NIPT_REFUSED))
def test_nipt_sizes_that_are_not_built_are_a_documented_status(medium_panel, dev, Ks):
    """The three-label kernels hold three columns per row; ten rows per lane fill a SIMD's register file and nothing larger is
    built.  QA_ERR_UNSUPPORTED from the argument checks -- never QA_ERR_INVALID from a launcher part-way through -- with a text
    that names the sizes that run (include/quilt_amd.h: qa_gibbs_opts_t.Ks); the labels the caller passed are untouched."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.native import QuiltAmdError
    s, which, H0, ru, rb, rr, fr = nipt_setup(medium_panel, 11, Ks, 100)
    with pytest.raises(QuiltAmdError, match=r"1\.\.640") as e:
        rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, None, ff=0.2, runif_block=rb, runif_resample=rr)
    assert e.value.status == QA_ERR_UNSUPPORTED
    assert "1..1024" in str(e.value)   # (where the diploid sampler goes on)


def test_sizes_either_side_of_a_refusal_run(medium_panel, dev, oracle):
    """640 runs and 641 is refused with ff > 0; 641 runs with ff = 0; 1024 runs and 1025 is refused with ff = 0."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.native import QuiltAmdError
    panel = medium_panel
    s, which, H0, ru, rb, rr, fr = nipt_setup(panel, 12, 640, 300)
    ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, np.zeros(3 * panel.nGrids), ff=0.2, runif_block=rb, runif_resample=rr)
    nipt_compare(rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, None, ff=0.2, runif_block=rb, runif_resample=rr), ref)
    s, which, H0, ru, rb, rr, fr = nipt_setup(panel, 12, 641, 300)
    with pytest.raises(QuiltAmdError) as e:
        rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, None, ff=0.2, runif_block=rb, runif_resample=rr)
    assert e.value.status == QA_ERR_UNSUPPORTED
    for Ks in (641, 1024):
        s, which, H0, ru, rs, fr = gibbs_setup(panel, 12, Ks, 300)
        ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, rs)
        gibbs_compare(rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, rs, return_state=True), ref, Ks)
    s, which, H0, ru, rs, fr = gibbs_setup(panel, 12, 1025, 300)
    with pytest.raises(QuiltAmdError, match=r"1\.\.1024") as e:
        rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, rs)
    assert e.value.status == QA_ERR_UNSUPPORTED


def test_range_call_refuses_an_unbuilt_size_before_the_first_sample():
    """qa_impute_samples with method = "nipt" and a panel of 700 haplotypes at the default Ksubset = 600 -> 600 runs; at
    Ksubset = 1024 the reset to the panel's size leaves 700: QA_ERR_UNSUPPORTED, nothing written, the text names what runs."""
    from quilt_amd.driver import DriverParams
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel, QuiltAmdError
    from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
    panel = make_synthetic_panel(K=700, nSNPs=640, seed=5)
    samples = [make_synthetic_sample(panel, seed=80 + i, n_reads=200, ff=0.2) for i in range(2)]
    d = DevicePanel(panel)
    d.set_dosage_precision(64)
    with pytest.raises(QuiltAmdError, match=r'method = "nipt"') as e:
        impute_samples([d], samples, DriverParams(nGibbsSamples=2, Ksubset=1024, Knew=1024, seed=3, method="nipt"))
    assert e.value.status == QA_ERR_UNSUPPORTED and "1..640" in str(e.value)
    ok = impute_samples([d], samples, DriverParams(nGibbsSamples=2, Ksubset=640, Knew=640, seed=3, method="nipt"))
    assert len(ok) == 2 and all(r.nDosage == 2 for r in ok)
    d.close()


# ---------------------------------------------------------------------------------------------------------------------------
# driver level: the whole native loop at sizes that used to die in a launcher
# ---------------------------------------------------------------------------------------------------------------------------
def _native_loop_on_device_and_on_oracle(panel, samples, prm):
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from tests.native_driver_backend import impute_samples_on_oracle
    ref, _, _ = impute_samples_on_oracle(panel, samples, prm)
    d = DevicePanel(panel)
    d.set_dosage_precision(64)
    got = impute_samples([d], samples, prm)
    d.close()
    assert len(got) == len(ref) == len(samples)
    for g, r in zip(got, ref):   # tests/test_native_driver_gpu.py's bar against the CPU pipeline
        assert g.nDosage == r.nDosage == prm.nGibbsSamples
        assert np.array_equal(g.read_labels, r.read_labels)
        assert np.abs(g.dosage - r.dosage).max() <= 1e-9
        assert np.corrcoef(g.dosage, r.dosage)[0, 1] ** 2 >= 0.999999
    return got, ref


def test_driver_diploid_panel_of_700_lands_on_eleven_rows_per_lane():
    from quilt_amd.driver import DriverParams
    from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
    panel = make_synthetic_panel(K=700, nSNPs=640, seed=5)
    samples = [make_synthetic_sample(panel, seed=4300 + i, n_reads=300) for i in range(2)]
    prm = DriverParams(nGibbsSamples=2, Ksubset=1024, Knew=1024, seed=5)
    assert prm.resolved(panel.K).Ksubset == 700 and (700 + 63) // 64 == 11
    _native_loop_on_device_and_on_oracle(panel, samples, prm)


def test_driver_nipt_panel_of_420_at_default_ksubset_lands_on_seven_rows_per_lane():
    from quilt_amd.driver import DriverParams
    from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
    panel = make_synthetic_panel(K=420, nSNPs=640, seed=5)
    samples = [make_synthetic_sample(panel, seed=4400 + i, n_reads=300, ff=0.15 + 0.1 * i) for i in range(2)]
    prm = DriverParams(nGibbsSamples=2, seed=5, method="nipt")
    assert prm.Ksubset == 600 and prm.resolved(panel.K).Ksubset == 420 and (420 + 63) // 64 == 7
    got, ref = _native_loop_on_device_and_on_oracle(panel, samples, prm)
    for g, r in zip(got, ref):
        assert np.abs(g.fet_dosage - r.fet_dosage).max() <= 1e-9
