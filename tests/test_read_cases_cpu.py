"""The constructed reads of tests/read_cases.py, checked without a device: every builder's claims hold (where a read's bases lie
relative to its block of 32 reads and the 64-base chunk in flight, the informative count as prepare_chain forms it, the folded base
qualities, which rescaling outcome the oracle's column shows, no column maximum near the edge of the double range), the oracle
returns status 0 for every chain tests/test_read_geometry_gpu.py runs, and the oracle itself agrees on these reads -- Jmax clip and
carry-over across reads included -- with the independent NumPy restatement oracle/rtwin.py to 1e-12 (same arithmetic, NumPy's
order of evaluation)."""
import numpy as np
import pytest

from tests import read_cases as RC

TWIN_RTOL = 1e-12


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def _packed(panel, oracle, family, Ks, with_specials=False):
    from oracle import rtwin
    which = RC.which_for(panel, Ks, with_specials)
    cases = RC.cases_for(family, panel, which, oracle)
    assert cases
    for case in cases:
        s = case.sample
        raw, scaled = RC.check_claims(case, panel, which, oracle)
        for rescale, got in ((False, raw), (True, scaled)):
            twin = rtwin.make_eMatRead_t(panel, s, which, case.maxdiff, case.Jmax, rescale)
            np.testing.assert_allclose(got, twin, rtol=TWIN_RTOL, atol=0, err_msg=f"{case.name} rescale={rescale}")
        ru, rs, fr = RC.gibbs_inputs(case, panel)
        kw = dict(maxDifferenceBetweenReads=case.maxdiff, Jmax=case.Jmax)
        runs = [oracle.forwardBackwardGibbsNIPT(panel, s, which, case.H0, ru, fr, rs, gibbs_initialize_iteratively=it, **kw)
                for it in (False, True)]
        runs.append(oracle.forwardBackwardGibbsNIPT(panel, s, which, case.H0, ru, fr, rs, n_gibbs_burn_in_its=0, n_gibbs_sample_its=0,
                                                    perform_block_gibbs=False, **kw))
        for ref in runs:
            assert ref["status"] == 0, case.name
            np.testing.assert_array_equal(ref["eMatRead_t"], scaled)
        if case.isolating:   # a column of the oracle's eMatGrid_t after initialisation IS the read's emission column
            for r in range(s.nReads):
                assert np.array_equal(runs[2]["eMatGrid_t"][case.H0[r] - 1][:, s.wif[r]], scaled[:, r])


@pytest.mark.parametrize("family", RC.MEDIUM_FAMILIES)
def test_packed_cases_at_ks_70(medium_panel, oracle, family):
    _packed(medium_panel, oracle, family, RC.KS_SMALL)


@pytest.mark.parametrize("family", RC.LARGE_KS_FAMILIES)
def test_packed_cases_at_ks_600(medium_panel, oracle, family):
    _packed(medium_panel, oracle, family, RC.KS_LARGE)


def test_packed_cases_on_the_ragged_panel(ragged_panel, oracle):
    assert ragged_panel.nSNPs == 1003 and ragged_panel.nMaxDH == 40
    _packed(ragged_panel, oracle, "where", RC.KS_SMALL, with_specials=True)


def test_batched_chains_share_one_jmax(medium_panel, oracle):
    """The three chains the device test runs in one call (one Jmax_local for all of them)."""
    which = RC.which_for(medium_panel, RC.KS_SMALL)
    for case in (RC.chunk_offset_case(medium_panel, which, 63, 3), RC.jmax_case(medium_panel, which, 63), RC.long_read_case(medium_panel, which, 129)):
        ru, rs, fr = RC.gibbs_inputs(case, medium_panel)
        assert oracle.forwardBackwardGibbsNIPT(medium_panel, case.sample, which, case.H0, ru, fr, rs, Jmax=63)["status"] == 0


def test_a_quality_beyond_the_table_is_a_case_of_its_own(medium_panel):
    which = RC.which_for(medium_panel, RC.KS_SMALL)
    for v in (256, -256):
        case = RC.bad_quality_case(medium_panel, which, v)
        assert np.abs(case.sample.bq).max() == 256 and case.sample.bq[case.sample.read_ptr[1] + 1] == v


# ---------------------------------------------------------------------------------------------------------------------------
# dense kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
def test_dense_ont_reads_oracle_vs_twin(medium_panel, oracle, K):
    from oracle import rtwin
    full = RC.ont_sample(medium_panel)
    d = RC.dosages_near(full.truth_haps, K, 7 + K)
    for R in (1, 65):
        s = RC.prefix(full, R)
        for Jmax in RC.DENSE_JMAX:
            assert (np.diff(s.read_ptr) > Jmax + 1).all() == (Jmax == 100)
            for rescale in (False, True):
                got = oracle.calculate_eMatRead_t_vs_haplotypes(s, d, 1e10, rescale, Jmax)
                twin = rtwin.make_eMatRead_t_dense(d, s, 1e10, Jmax, rescale)
                np.testing.assert_allclose(got, twin, rtol=TWIN_RTOL, atol=0)
    raw = oracle.calculate_eMatRead_t_vs_haplotypes(full, d, 1e10, False, 1000)
    assert raw.max(axis=0).min() > 1e-250   # no column maximum near the edge of the double range


@pytest.mark.parametrize("maxdiff", RC.MAXDIFFS)
@pytest.mark.parametrize("K", [1, 2, 3])
def test_dense_rescaling_regimes(medium_panel, oracle, K, maxdiff):
    from oracle import rtwin
    s, d, claims = RC.dense_rescale_case(medium_panel.nSNPs, K, oracle, maxdiff)
    n_normal, n_sub, n_zero = claims["lengths"]
    assert 25 <= n_normal < n_sub < n_zero <= 40   # (a factor is 1.7e-10: about 31, 32-33 and 34 bases)
    raw = oracle.calculate_eMatRead_t_vs_haplotypes(s, d, maxdiff, False)
    scaled = oracle.calculate_eMatRead_t_vs_haplotypes(s, d, maxdiff, True)
    for r, want in claims["outcome"].items():
        assert RC.outcome_of(raw[:, r], scaled[:, r], maxdiff) == want, r
    for r in range(s.nReads):
        if r not in claims["edge"]:
            assert raw[:, r].max() > 1e-250 or raw[:, r].max() == 0.0
    assert s.bq[s.read_ptr[7]] == 0 and RC.fold_qualities(s, 1000)[s.read_ptr[7]] == s.bq[s.read_ptr[7] - 1]
    for rescale, got in ((False, raw), (True, scaled)):
        np.testing.assert_allclose(got, rtwin.make_eMatRead_t_dense(d, s, maxdiff, 1000, rescale), rtol=TWIN_RTOL, atol=0)


@pytest.mark.parametrize("name", RC.DENSE_CARRY_CASES)
def test_dense_carry_over_oracle_vs_twin(medium_panel, oracle, name):
    from oracle import rtwin
    case = RC.dense_carry_case(medium_panel, name)
    for K in (1, 2, 3):
        d = RC.random_dosages(medium_panel.nSNPs, K, 17 + K)
        for rescale in (False, True):
            got = oracle.calculate_eMatRead_t_vs_haplotypes(case.sample, d, 1e10, rescale, case.Jmax)
            np.testing.assert_allclose(got, rtwin.make_eMatRead_t_dense(d, case.sample, 1e10, case.Jmax, rescale), rtol=TWIN_RTOL, atol=0)
            if not rescale:
                assert got.max(axis=0).min() > 1e-250
