"""Every read geometry of the two read-emission kernels against the fp64 CPU oracle (reads from tests/read_cases.py; their
claims are checked by tests/test_read_cases_cpu.py).

k_ematread (packed panel; csrc/gibbs_dev.hpp), Ksubset = 70 on medium_panel (two rows per lane, 58 lanes of the last row masked),
one chain per call, each case twice:
  * initialisation only, state returned: eMatGrid_t1/2 equal the oracle's emission columns -- with the isolating layout (one read
    per grid and label) column by column, else their product per grid and label -- to 1e-9 relative with atol = 0; a grid without
    a read of a label is exactly 1; an all-ones column is exactly 1;
  * the default sampler run with both initialisations, by tests.util.gibbs_compare (labels and H_class identical, state and
    probabilities to 1e-9).
Families: read count against the 32-read block; base offsets against the 64-base chunk; the compact / dense threshold with the
bq == 0 carry-over (leading zeros, zeros inside and at the end of later reads, later reads that begin with one, all-zero reads);
Jmax_local in {1, 4, 5, 63, 64}; the three rescaling outcomes (divide by the maximum, floor, all ones) and the three lengths around
the smallest double; |bq| in {1, 93, 255} and 256 refused; on ragged_panel reads over several grids, the ragged last grid and
special haplotypes.  The threshold and chunk families again at Ksubset = 600 with one and two waves per chain (the compact index
layout depends on it), and three chains in one call bit for bit equal to their own calls.

k_ematread_dense (csrc/gibbs.hip) through its entry points, against oracle.calculate_eMatRead_t_vs_haplotypes to 1e-9 (all-ones
columns exactly 1): K in {1, 2, 3}, rescaling on and off, both dosage layouts, Jmax in {100, 1000} on ONT-like reads, read counts
around the 64-thread block, three chains of different size in one call, the carry-over cases, the rescaling regimes; the rare +
common entry (chains that share a sample, chains out of sample order, a sample nobody uses) must return exactly what
qa_rcpp_make_eMatRead_t_nsnps returns on the host-expanded dosages."""
import numpy as np
import pytest

from tests import read_cases as RC
from tests.util import GIBBS_RTOL as RTOL, gibbs_compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def dev(medium_panel):
    from quilt_amd.native import DevicePanel
    d = DevicePanel(medium_panel)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dev_ragged(ragged_panel):
    from quilt_amd.native import DevicePanel
    d = DevicePanel(ragged_panel)
    yield d
    d.close()


# ---------------------------------------------------------------------------------------------------------------------------
# packed-panel kernel
# ---------------------------------------------------------------------------------------------------------------------------
def check_initialisation(dev, panel, oracle, case, which):
    """Initialisation only: every read's emission column as the sampler will see it, in whichever form the kernel wrote it."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    s, H0 = case.sample, case.H0
    ru, rs, fr = RC.gibbs_inputs(case, panel)
    got = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, rs, n_gibbs_burn_in_its=0, n_gibbs_sample_its=0,
                                        perform_block_gibbs=False, return_state=True, Jmax_local=case.Jmax,
                                        maxDifferenceBetweenReads=case.maxdiff)
    assert not got["underflow_problem"] and np.array_equal(got["H"], H0)
    e = oracle.make_eMatRead_t(panel, s, which, case.maxdiff, case.Jmax)
    want = [np.ones((len(which), panel.nGrids)) for _ in range(2)]
    for r in range(s.nReads):
        want[H0[r] - 1][:, s.wif[r]] *= e[:, r]
    for h in range(2):
        eg = got[f"eMatGrid_t{h + 1}"]
        err = np.abs(eg - want[h]) / want[h]
        print(f"{case.name} label {h + 1}: max relative difference {err.max():.3e}")
        np.testing.assert_allclose(eg, want[h], rtol=RTOL, atol=0, err_msg=f"{case.name} label {h + 1}")
        empty = np.setdiff1d(np.arange(panel.nGrids), s.wif[H0 == h + 1])
        assert (eg[:, empty] == 1.0).all(), f"{case.name}: a grid without a read of label {h + 1} is not exactly 1"
        if case.isolating:
            for r in np.flatnonzero((H0 == h + 1) & (e == 1.0).all(axis=0)):
                assert (eg[:, s.wif[r]] == 1.0).all(), f"{case.name}: read {r}'s all-ones column is not exactly 1"


def check_sampler(dev, panel, oracle, case, which):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    s, H0 = case.sample, case.H0
    ru, rs, fr = RC.gibbs_inputs(case, panel)
    for init_iter in (False, True):
        kw = dict(gibbs_initialize_iteratively=init_iter, maxDifferenceBetweenReads=case.maxdiff)
        ref = oracle.forwardBackwardGibbsNIPT(panel, s, which, H0, ru, fr, rs, Jmax=case.Jmax, **kw)
        got = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ru, fr, rs, Jmax_local=case.Jmax, return_state=True, **kw)
        gibbs_compare(got, ref, len(which))


def case_ids(family):
    """The names of a family's cases, without building them (the parametrisation runs at collection)."""
    return {"count": [f"count_{R}" for R in RC.READ_COUNTS],
            "chunk": ([f"chunk_{o}_{n}" for o, n in RC.CHUNK_OFFSETS] + [f"long_{n}" for n in RC.LONG_READS] + ["block_total_64"] +
                      [f"leading_zeros_{z}" for z in RC.LEADING_ZEROS]),
            "threshold": [f"threshold_leading_{z}_{m}" for z, m in RC.THRESHOLD_LEADING] + ["zero_mid_or_end", "first_base_zero", "all_zero_reads"],
            "jmax": [f"jmax_{J}" for J in RC.JMAX_VALUES],
            "rescale": ["all_ones"] + [f"floor_{m:g}" for m in RC.MAXDIFFS] + ["edge_trio"],
            "quality": ["quality_1_93_255"], "where": ["where_bases_lie"]}[family]


_built = {}


def the_case(panel, oracle, family, name, Ks, with_specials=False):
    key = (id(panel), family, Ks)
    if key not in _built:
        which = RC.which_for(panel, Ks, with_specials)
        cases = RC.cases_for(family, panel, which, oracle)
        assert [c.name for c in cases] == case_ids(family)
        _built[key] = (which, {c.name: c for c in cases})
    which, cases = _built[key]
    return which, cases[name]


SMALL = [(f, n) for f in RC.MEDIUM_FAMILIES for n in case_ids(f)]
LARGE = [(f, n) for f in RC.LARGE_KS_FAMILIES for n in case_ids(f)]


@pytest.mark.parametrize("family,name", SMALL, ids=[n for _, n in SMALL])
def test_packed_every_read_geometry(medium_panel, dev, oracle, family, name):
    which, case = the_case(medium_panel, oracle, family, name, RC.KS_SMALL)
    assert len(which) == 70
    check_initialisation(dev, medium_panel, oracle, case, which)
    check_sampler(dev, medium_panel, oracle, case, which)


@pytest.mark.parametrize("nw", ["1", "2"])
@pytest.mark.parametrize("family,name", LARGE, ids=[n for _, n in LARGE])
def test_packed_threshold_and_chunks_per_wave_count(medium_panel, dev, oracle, family, name, nw, monkeypatch):
    """Ksubset = 600 as one and as two waves per chain: the pattern bytes of a compact read are laid out per thread of the chain."""
    monkeypatch.setenv("QA_GIBBS_NW", nw)
    which, case = the_case(medium_panel, oracle, family, name, RC.KS_LARGE)
    check_initialisation(dev, medium_panel, oracle, case, which)
    check_sampler(dev, medium_panel, oracle, case, which)


def test_packed_where_the_bases_lie(ragged_panel, dev_ragged, oracle):
    which, case = the_case(ragged_panel, oracle, "where", "where_bases_lie", RC.KS_SMALL, with_specials=True)
    assert not case.isolating and case.claims["special_grids"]
    check_initialisation(dev_ragged, ragged_panel, oracle, case, which)
    check_sampler(dev_ragged, ragged_panel, oracle, case, which)


def test_packed_three_chains_in_one_call(medium_panel, dev, oracle):
    """A chunk-family chain, a Jmax chain and a chain with a 129-base read in one call under Jmax_local = 63: each the oracle's, and
    bit for bit what a call of its own returns."""
    from quilt_amd.gibbs_nipt import forwardBackwardGibbsNIPT_batch, rcpp_forwardBackwardGibbsNIPT
    panel = medium_panel
    which = RC.which_for(panel, RC.KS_SMALL)
    cases = [RC.chunk_offset_case(panel, which, 63, 3), RC.jmax_case(panel, which, 63), RC.long_read_case(panel, which, 129)]
    assert len({c.sample.nReads for c in cases}) == 3
    ins = [RC.gibbs_inputs(c, panel) for c in cases]
    got = forwardBackwardGibbsNIPT_batch(dev, [c.sample for c in cases], [which] * 3, [c.H0 for c in cases], [x[0] for x in ins],
                                         [x[2] for x in ins], [x[1] for x in ins], Jmax_local=63)
    for g, c, (ru, rs, fr) in zip(got, cases, ins):
        ref = oracle.forwardBackwardGibbsNIPT(panel, c.sample, which, c.H0, ru, fr, rs, Jmax=63)
        one = rcpp_forwardBackwardGibbsNIPT(dev, c.sample, which, c.H0, ru, fr, rs, Jmax_local=63, return_state=True)
        gibbs_compare(one, ref, len(which))
        assert not g["underflow_problem"]
        for f in ("H", "H_class", "hapProbs_t", "genProbsM_t", "genProbsF_t"):
            assert np.array_equal(g[f], one[f]), (c.name, f)


@pytest.mark.parametrize("value", [256, -256])
def test_packed_quality_beyond_the_table_is_refused(medium_panel, dev, value):
    """|bq| = 256 has no table entry: QuiltAmdError from the host's fold, before any launch; the labels are untouched."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.native import QuiltAmdError
    which = RC.which_for(medium_panel, RC.KS_SMALL)
    case = RC.bad_quality_case(medium_panel, which, value)
    ru, rs, fr = RC.gibbs_inputs(case, medium_panel)
    with pytest.raises(QuiltAmdError, match="base quality"):
        rcpp_forwardBackwardGibbsNIPT(dev, case.sample, which, case.H0, ru, fr, rs)


# ---------------------------------------------------------------------------------------------------------------------------
# dense kernel
# ---------------------------------------------------------------------------------------------------------------------------
def dense_call(dev, samples, haps, maxdiff, rescale, Jmax, hap_major, nSNPs=None):
    """One device call for a batch of chains; haps[c] = K dosage vectors.  Both layouts go in as arrays."""
    from quilt_amd.gibbs_nipt import calculate_eMatRead_t_vs_haplotypes_batch
    e = np.stack([np.stack(h, axis=0) for h in haps])   # [chain, K, SNP]
    if not hap_major:
        e = np.ascontiguousarray(e.transpose(0, 2, 1))
    return calculate_eMatRead_t_vs_haplotypes_batch(dev, samples, e, maxdiff, rescale, Jmax, nSNPs=nSNPs, hap_major=hap_major)


def dense_compare(got, want, what):
    err = np.abs(got - want) / np.where(want == 0, 1.0, want)
    print(f"{what}: max relative difference {err.max():.3e}")
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0, err_msg=what)
    ones = (want == 1.0).all(axis=0)
    assert (got[:, ones] == 1.0).all(), f"{what}: an all-ones column is not exactly 1"


@pytest.fixture(scope="module")
def ont(medium_panel):
    return RC.ont_sample(medium_panel)


@pytest.mark.parametrize("Jmax", RC.DENSE_JMAX)
@pytest.mark.parametrize("hap_major", [False, True])
@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_dense_ont_reads_every_read_count(medium_panel, dev, oracle, ont, K, rescale, hap_major, Jmax):
    d = RC.dosages_near(ont.truth_haps, K, 7 + K)
    for R in RC.DENSE_READ_COUNTS:
        s = RC.prefix(ont, R)
        want = oracle.calculate_eMatRead_t_vs_haplotypes(s, d, 1e10, rescale, Jmax)
        got = dense_call(dev, [s], [d], 1e10, rescale, Jmax, hap_major)[0]
        assert got.shape == (K, R)
        dense_compare(got, want, f"R={R}")


@pytest.mark.parametrize("hap_major", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_dense_three_chains_of_different_size(medium_panel, dev, oracle, ont, K, hap_major):
    """The grid is sized by the largest chain (129 reads: three blocks): the surplus threads of the others write nothing."""
    sizes = (65, 1, 129)
    samples = [RC.prefix(ont, R) for R in sizes]
    haps = [RC.dosages_near(ont.truth_haps, K, 40 + i) for i in range(3)]
    for rescale in (False, True):
        got = dense_call(dev, samples, haps, 1e10, rescale, 100, hap_major)
        for c, (s, d) in enumerate(zip(samples, haps)):
            dense_compare(got[c], oracle.calculate_eMatRead_t_vs_haplotypes(s, d, 1e10, rescale, 100), f"chain {c}")
            assert np.array_equal(got[c], dense_call(dev, [s], [d], 1e10, rescale, 100, hap_major)[0])


@pytest.mark.parametrize("name", RC.DENSE_CARRY_CASES)
def test_dense_carry_over_and_clip(medium_panel, dev, oracle, name):
    """The chains of the packed kernel's carry-over and Jmax families, against dosages: quality carried into a later read, across
    all-zero reads, from a clipped read's base number Jmax; leading zeros with nothing to carry."""
    case = RC.dense_carry_case(medium_panel, name)
    for K in (1, 2, 3):
        d = RC.random_dosages(medium_panel.nSNPs, K, 17 + K)
        for rescale in (False, True):
            for hap_major in (False, True):
                want = oracle.calculate_eMatRead_t_vs_haplotypes(case.sample, d, 1e10, rescale, case.Jmax)
                dense_compare(dense_call(dev, [case.sample], [d], 1e10, rescale, case.Jmax, hap_major)[0], want, f"{name} K={K}")


@pytest.mark.parametrize("maxdiff", RC.MAXDIFFS)
@pytest.mark.parametrize("K", [1, 2, 3])
def test_dense_rescaling_regimes(medium_panel, dev, oracle, K, maxdiff):
    s, d, claims = RC.dense_rescale_case(medium_panel.nSNPs, K, oracle, maxdiff)
    raw = oracle.calculate_eMatRead_t_vs_haplotypes(s, d, maxdiff, False)
    for rescale in (False, True):
        want = oracle.calculate_eMatRead_t_vs_haplotypes(s, d, maxdiff, rescale)
        if rescale:
            for r, what in claims["outcome"].items():
                assert RC.outcome_of(raw[:, r], want[:, r], maxdiff) == what
        for hap_major in (False, True):
            dense_compare(dense_call(dev, [s], [d], maxdiff, rescale, 1000, hap_major)[0], want, f"K={K} rescale={rescale}")


def test_dense_quality_beyond_the_table_is_refused(medium_panel, dev):
    from quilt_amd.native import QuiltAmdError
    which = RC.which_for(medium_panel, RC.KS_SMALL)
    case = RC.bad_quality_case(medium_panel, which, 256)
    with pytest.raises(QuiltAmdError, match="base quality"):
        dense_call(dev, [case.sample], [RC.random_dosages(medium_panel.nSNPs, 2, 3)], 1e10, False, 1000, False)


@pytest.mark.parametrize("Jmax", [10, 1000])
@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_dense_rare_common_entry(medium_panel, dev, oracle, K, rescale, Jmax):
    """qa_rcpp_make_eMatRead_t_rare_common: dosages over the common SNPs, 0.5 at the rare ones supplied by the kernel, reads per
    sample with a chain -> sample map.  Four chains over three samples: two share sample 0, the chains are out of sample order,
    sample 1 is used by nobody.  Exactly the numbers of qa_rcpp_make_eMatRead_t_nsnps on the host-expanded dosages (the header's
    claim), and the oracle's to 1e-9."""
    from quilt_amd.gibbs_nipt import calculate_eMatRead_t_rare_common_batch
    from quilt_amd.native import DeviceRareCommon
    from quilt_amd.synth import make_rare_common, make_synthetic_sample_rare_common
    panel = medium_panel
    rc = make_rare_common(panel, 23, carriers=(0, 6))
    samples = []
    for i, n in enumerate((70, 30, 129)):
        s = make_synthetic_sample_rare_common(panel, rc, 60 + i, n_reads=n)[1]
        s.bq = s.bq.copy()
        s.bq[np.random.default_rng(i).random(len(s.bq)) < 0.1] = 0   # carry-over inside and across reads
        samples.append(s)
    assert max(np.diff(s.read_ptr).max() for s in samples) > 11   # Jmax = 10 clips
    chain_sample = [2, 0, 0, 2]
    rng = np.random.default_rng(77 + K)
    hap_common = np.stack([np.stack(RC.random_dosages(panel.nSNPs, K, int(rng.integers(1 << 30)))) for _ in chain_sample])
    expanded = np.full((len(chain_sample), K, rc.nSNPs_all), 0.5)
    expanded[:, :, np.asarray(rc.snp_is_common) == 1] = hap_common
    assert (np.asarray(rc.snp_is_common) == 0).sum() > panel.nSNPs and any((np.asarray(rc.snp_is_common)[s.u] == 0).any() for s in samples)
    drc = DeviceRareCommon(dev, rc)
    try:
        got = calculate_eMatRead_t_rare_common_batch(dev, drc, samples, chain_sample, hap_common, 1e10, rescale, Jmax)
    finally:
        drc.close()
    per_chain = [samples[i] for i in chain_sample]
    direct = dense_call(dev, per_chain, [list(expanded[c]) for c in range(len(chain_sample))], 1e10, rescale, Jmax, False,
                        nSNPs=rc.nSNPs_all)
    for c, s in enumerate(per_chain):
        assert got[c].shape == (K, s.nReads)
        assert np.array_equal(got[c], direct[c]), f"chain {c}: largest relative difference {np.abs(got[c] / direct[c] - 1).max():.3e}"
        dense_compare(got[c], oracle.calculate_eMatRead_t_vs_haplotypes(s, list(expanded[c]), 1e10, rescale, Jmax), f"chain {c}")
