"""Every all-SNP and carrier geometry of the rare + common Gibbs call (qa_gibbs_batch_rare_common) against the fp64 CPU oracle, on
the inputs of tests/rare_cases.py (their claims are proven by tests/test_rare_cases_cpu.py).

Per case, at the suite's bars:
  * initialisation only, state returned: eMatGrid_t1/2 equal the product of the oracle's rare + common emission columns per all-SNP
    grid and label to 1e-9 relative with atol = 0; a grid without a read of a label is exactly 1; in the isolating layout an
    all-ones column is exactly 1 (k_ematread's rare branch, prepare_chain's rc_any and informative count);
  * the default sampler run by tests.util.gibbs_compare (labels and H_class identical, state and probabilities to 1e-9), with read
    categories on and off.  The diploid call's genProbsF_t is the device's own definition: the reference leaves it
    unwritten, the device writes it from a third haploid dosage of 0;
  * k_happrobs_rc apart from sampler drift: hapProbs_t and genProbsM_t recomputed in long double from the alphaHat_t, betaHat_t and c
    the device itself returned (rtol 1e-9, atol 1e-14); an uncarried rare SNP is ref_error exactly.
The layout and carrier families at Ksubset 70 and 600 (full_grid and the largest pair word at 1024); the read family in the isolating
layout, its threshold and long-read cases again at Ksubset = 600 with one and two waves per chain; one sample read by two chains
whose subsets differ in exactly the carriers, as two calls, as one call, and as one call with reads_same_as over a second copy of the
reads that holds other (valid) bases: all three bit for bit equal; three labels (ff = 0.2) on two layouts; the dense rare + common
entry against qa_rcpp_make_eMatRead_t_nsnps on host-expanded dosages; every refusal of qa_rare_common_create."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests import rare_cases as RC
from tests.util import GIBBS_RTOL as RTOL, gibbs_compare, sample_from_arrays

pytestmark = pytest.mark.gpu

QA_ERR_INVALID = -2


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def dev():
    from quilt_amd.native import DevicePanel
    d = DevicePanel(RC.panel())
    yield d
    d.close()


@pytest.fixture(scope="module")
def handle_of(dev):
    """The device side of a case's RareCommon, made once per table."""
    from quilt_amd.native import DeviceRareCommon
    made = {}

    def get(rc):
        if id(rc) not in made:
            made[id(rc)] = (rc, DeviceRareCommon(dev, rc))
        return made[id(rc)][1]
    yield get
    for _, d in made.values():
        d.close()


def grid_products(case, which, e):
    s, H0 = case.sample, case.H0
    want = [np.ones((len(which), case.rc.nGrids_all)) for _ in range(2)]
    for r in range(s.nReads):
        want[H0[r] - 1][:, s.wif[r]] *= e[:, r]
    return want


def check_initialisation(dev, drc, oracle, case, which, no_categories=False):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    s, H0, ins = case.sample, case.H0, RC.gibbs_inputs(case)
    got = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ins["ru"], ins["fr"], ins["rs"], n_gibbs_burn_in_its=0, n_gibbs_sample_its=0,
                                        perform_block_gibbs=False, return_state=True, Jmax_local=case.Jmax,
                                        maxDifferenceBetweenReads=case.maxdiff, rare_common=drc, disable_read_category_usage=no_categories)
    assert not got["underflow_problem"] and np.array_equal(got["H"], H0)
    e = RC.oracle_columns(case, which, oracle)
    want = grid_products(case, which, e)
    for h in range(2):
        eg = got[f"eMatGrid_t{h + 1}"]
        print(f"{case.name} label {h + 1}: max relative difference {(np.abs(eg - want[h]) / want[h]).max():.3e}")
        np.testing.assert_allclose(eg, want[h], rtol=RTOL, atol=0, err_msg=f"{case.name} label {h + 1}")
        empty = np.setdiff1d(np.arange(case.rc.nGrids_all), s.wif[H0 == h + 1])
        assert (eg[:, empty] == 1.0).all(), f"{case.name}: a grid without a read of label {h + 1} is not exactly 1"
        if case.isolating:
            for r in np.flatnonzero((H0 == h + 1) & (e == 1.0).all(axis=0)):
                assert (eg[:, s.wif[r]] == 1.0).all(), f"{case.name}: read {r}'s all-ones column is not exactly 1"


def check_happrobs(got, case, which):
    """k_happrobs_rc on the state the device itself returned."""
    hp, gm, is_common, carried = RC.happrobs_from_state(case.rc, which, [got["alphaHat_t1"], got["alphaHat_t2"]],
                                                        [got["betaHat_t1"], got["betaHat_t2"]], [got["c1"], got["c2"]])
    dh, dm = got["hapProbs_t"][:2], got["genProbsM_t"]
    print(f"{case.name}: hapProbs from the device's state, max relative difference {(np.abs(dh - hp) / hp).max():.3e}")
    np.testing.assert_allclose(dh, hp.astype(np.float64), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(dm, gm.astype(np.float64), rtol=1e-9, atol=1e-14)
    uncarried = ~is_common & ~carried
    assert (dh[:, uncarried] == RC.panel().ref_error).all(), "an uncarried rare SNP is ref_error exactly"
    # the diploid call's third row and fetal genotypes: the device's definition (no third label: dosage 0)
    assert (got["hapProbs_t"][2] == 0).all()
    assert np.array_equal(got["genProbsF_t"], np.stack([1 - dh[0], dh[0] * (1 - 0.0) + (1 - dh[0]) * 0.0, dh[0] * 0.0]))


def check_sampler(dev, drc, oracle, case, which, categories=(False, True)):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    s, H0, ins = case.sample, case.H0, RC.gibbs_inputs(case)
    for dis in categories:
        kw = dict(disable_read_category_usage=dis, maxDifferenceBetweenReads=case.maxdiff)
        ref = oracle.forwardBackwardGibbsNIPT(RC.panel(), s, which, H0, ins["ru"], ins["fr"], ins["rs"], Jmax=case.Jmax, rare_common=case.rc, **kw)
        got = rcpp_forwardBackwardGibbsNIPT(dev, s, which, H0, ins["ru"], ins["fr"], ins["rs"], Jmax_local=case.Jmax, return_state=True,
                                            rare_common=drc, **kw)
        gibbs_compare(got, ref, len(which), fetal=False)
        check_happrobs(got, case, which)


def run_case(dev, handle_of, oracle, case):
    drc = handle_of(case.rc)
    for which in (case.which,) + (() if case.which_b is None else (case.which_b,)):
        check_initialisation(dev, drc, oracle, case, which)
        check_sampler(dev, drc, oracle, case, which)


AXIS = [i for i in RC.case_ids() if i[0] in ("layout", "carriers")]
READS = [i for i in RC.case_ids() if i[0] == "reads"]


@pytest.mark.parametrize("family,name,Ks", AXIS, ids=[RC.id_of(*i) for i in AXIS])
def test_every_all_snp_and_carrier_geometry(dev, handle_of, oracle, family, name, Ks):
    run_case(dev, handle_of, oracle, RC.case(family, name, Ks))


@pytest.mark.parametrize("family,name,Ks", READS, ids=[RC.id_of(*i) for i in READS])
def test_every_rare_read_geometry(dev, handle_of, oracle, family, name, Ks):
    case = RC.case(family, name, Ks)
    assert case.isolating
    run_case(dev, handle_of, oracle, case)
    if name == "rare_only_uncarried":   # every column is exactly 1, whether or not category 1 is in use
        check_initialisation(dev, handle_of(case.rc), oracle, case, case.which, no_categories=True)
        assert (RC.oracle_columns(case, case.which, oracle) == 1.0).all()


@pytest.mark.parametrize("nw", ["1", "2"])
@pytest.mark.parametrize("name", RC.PER_WAVE_NAMES)
def test_threshold_and_long_reads_per_wave_count(dev, handle_of, oracle, name, nw, monkeypatch):
    """Ksubset = 600 as one and as two waves per chain: the pattern bytes of a compact read are laid out per thread of the chain."""
    monkeypatch.setenv("QA_GIBBS_NW", nw)
    run_case(dev, handle_of, oracle, RC.case("reads", name, RC.KS_LARGE))


@pytest.mark.parametrize("Ks", RC.LAYOUT_KS)
def test_two_chains_read_one_sample(dev, handle_of, oracle, Ks):
    """Chain A and chain B read the same sample with subsets that differ in exactly the carriers: reads dense in A and compact in B
    and the reverse.  Two calls, one call, and one call with reads_same_as -- where chain B's own copy of the bases holds SNP 0 at
    quality 40 throughout, which must not be looked at -- agree bit for bit, and each chain is the oracle's."""
    from quilt_amd.gibbs_nipt import forwardBackwardGibbsNIPT_batch, rcpp_forwardBackwardGibbsNIPT
    case = RC.case("reads", "two_chains_one_read", Ks)
    drc, s, ins = handle_of(case.rc), case.sample, RC.gibbs_inputs(case)
    whichs = [case.which, case.which_b]
    kw = dict(rare_common=drc, disable_read_category_usage=True)
    refs = [oracle.forwardBackwardGibbsNIPT(RC.panel(), s, w, case.H0, ins["ru"], ins["fr"], ins["rs"], rare_common=case.rc,
                                            disable_read_category_usage=True) for w in whichs]
    apart = [rcpp_forwardBackwardGibbsNIPT(dev, s, w, case.H0, ins["ru"], ins["fr"], ins["rs"], return_state=True, **kw) for w in whichs]
    for got, ref, w in zip(apart, refs, whichs):
        gibbs_compare(got, ref, Ks, fetal=False)
        check_happrobs(got, case, w)
    other = sample_from_arrays(s.read_ptr, np.zeros_like(s.u), np.full_like(s.bq, 40), s.wif)
    batch = lambda samples, **more: forwardBackwardGibbsNIPT_batch(dev, samples, whichs, [case.H0] * 2, [ins["ru"]] * 2, [ins["fr"]] * 2,
                                                                   [ins["rs"]] * 2, **kw, **more)
    together = batch([s, s])
    shared = batch([s, other], reads_same_as=[0, 0])
    for c in range(2):
        for f in ("H", "H_class", "hapProbs_t", "genProbsM_t", "genProbsF_t"):
            assert np.array_equal(together[c][f], apart[c][f]), (c, f, "one call against two calls")
            assert np.array_equal(shared[c][f], apart[c][f]), (c, f, "reads_same_as against two calls")
    assert not np.array_equal(apart[0]["hapProbs_t"], apart[1]["hapProbs_t"])
    # the second copy is read when nothing says the chains share their reads: the keyword is what keeps it out
    unshared = batch([s, other])
    assert np.array_equal(unshared[0]["hapProbs_t"], apart[0]["hapProbs_t"]) and not np.array_equal(unshared[1]["hapProbs_t"], apart[1]["hapProbs_t"])


@pytest.mark.parametrize("Ks", RC.LAYOUT_KS)
@pytest.mark.parametrize("name", ["rare_grid_mid", "two_common_grids"])
def test_three_labels(dev, handle_of, oracle, name, Ks):
    """ff = 0.2: k_happrobs_rc with three gamma columns, hapProbs_t[2] and genProbsF_t included."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    case = RC.case("layout", name, Ks)
    s, rc, ins = case.sample, case.rc, RC.gibbs_inputs(case)
    ref = oracle.forwardBackwardGibbsNIPT(RC.panel(), s, case.which, ins["H3"], ins["ru"], ins["fr"], np.zeros(3 * rc.nGrids_all), ff=RC.FF,
                                          rare_common=rc, runif_block=ins["rb"], runif_resample=ins["rr"], L_grid=rc.L_grid_all)
    got = rcpp_forwardBackwardGibbsNIPT(dev, s, case.which, ins["H3"], ins["ru"], ins["fr"], None, ff=RC.FF, rare_common=handle_of(rc),
                                        runif_block=ins["rb"], runif_resample=ins["rr"])
    assert ref["status"] == 0 and not got["underflow_problem"] and (ref["H"] == 3).any()
    assert np.array_equal(got["H"], ref["H"]), f"{(got['H'] != ref['H']).sum()} labels differ"
    assert np.array_equal(got["H_class"], ref["H_class"])
    for f in ("hapProbs_t", "genProbsM_t", "genProbsF_t"):
        np.testing.assert_allclose(got[f], ref[f], rtol=RTOL, atol=1e-14, err_msg=f)
    rare_uncarried = (np.asarray(rc.snp_is_common) == 0) & ~RC.any_mask(rc, case.which)
    assert (got["hapProbs_t"][:, rare_uncarried] == RC.panel().ref_error).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the dense rare + common entry
# ---------------------------------------------------------------------------------------------------------------------------
DENSE = [("layout", "rare_grid_mid", 70), ("layout", "tail_1_rare", 70), ("layout", "tail_1_common", 70), ("reads", "rare_only_uncarried", 70),
         ("reads", "rare_only_carried", 70)]


@pytest.mark.parametrize("family,name,Ks", DENSE, ids=[n for _, n, _ in DENSE])
def test_dense_rare_common_entry_on_planted_layouts(dev, handle_of, oracle, family, name, Ks):
    """qa_rcpp_make_eMatRead_t_rare_common (dosages over the common SNPs, 0.5 at a rare one) returns exactly what
    qa_rcpp_make_eMatRead_t_nsnps returns on the host-expanded dosages, and the oracle's numbers to 1e-9."""
    from quilt_amd.gibbs_nipt import calculate_eMatRead_t_rare_common_batch, calculate_eMatRead_t_vs_haplotypes_batch
    from tests import read_cases
    case = RC.case(family, name, Ks)
    rc, s, p = case.rc, case.sample, RC.panel()
    is_common = np.asarray(rc.snp_is_common) == 1
    for K in (2, 3):
        hap_common = np.stack([np.stack(read_cases.random_dosages(p.nSNPs, K, 31 + K + c)) for c in range(2)])   # [chain, K, common SNP]
        expanded = np.full((2, K, rc.nSNPs_all), 0.5)
        expanded[:, :, is_common] = hap_common
        for rescale in (False, True):
            for Jmax in (3, 1000):
                got = calculate_eMatRead_t_rare_common_batch(dev, handle_of(rc), [s], [0, 0], hap_common, 1e10, rescale, Jmax)
                direct = calculate_eMatRead_t_vs_haplotypes_batch(dev, [s, s], np.ascontiguousarray(expanded.transpose(0, 2, 1)), 1e10, rescale,
                                                                  Jmax, nSNPs=rc.nSNPs_all)
                for c in range(2):
                    assert got[c].shape == (K, s.nReads) and np.array_equal(got[c], direct[c])
                    want = oracle.calculate_eMatRead_t_vs_haplotypes(s, list(expanded[c]), 1e10, rescale, Jmax)
                    np.testing.assert_allclose(got[c], want, rtol=1e-9, atol=0)
                    assert (got[c][:, (want == 1.0).all(axis=0)] == 1.0).all()


# ---------------------------------------------------------------------------------------------------------------------------
# qa_rare_common_create: every refusal, and the empty table
# ---------------------------------------------------------------------------------------------------------------------------
def create(dev, nSNPs_all, is_common, rare_ptr, rare_snp, tm):
    from quilt_amd.native import lib, ptr
    h = C.c_void_p()
    keep = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((is_common, np.uint8), (rare_ptr, np.int64),
                                                                                   (rare_snp, np.int32), (tm, np.float64))]
    st = lib().qa_rare_common_create(dev.handle, C.c_int32(nSNPs_all), *[ptr(a) for a in keep], C.byref(h))
    msg = lib().qa_last_error().decode() if st < 0 else ""
    if st >= 0:
        lib().qa_rare_common_destroy(h)
    return st, msg


def good_table():
    """Common SNPs at 2 .. 161 of 164; haplotype 3 carries all-SNPs 0 and 163, haplotype 5 all-SNP 1 (1-based in rare_snp)."""
    rc = RC.planted_rc(RC.panel(), RC.R(2) + RC.C(160) + RC.R(2), {0: [3], 163: [3], 1: [5]})
    return dict(nSNPs_all=rc.nSNPs_all, is_common=rc.snp_is_common.copy(), rare_ptr=rc.rare_ptr.copy(), rare_snp=rc.rare_snp.copy(),
                tm=np.asfortranarray(rc.transMatRate_t_all).ravel(order="F"))


def _bad(**change):
    t = good_table()
    for k, f in change.items():
        t[k] = f(t[k])
    return t


def _set(i, v):
    def f(a):
        a = a.copy()
        a[i] = v
        return a
    return f


def _ptr_above_its_end(p):
    """Haplotype 3's row ends at entry 3 while the table's last pointer says it holds 2 (with entries that are valid and ascend:
    nothing else is wrong with the row that runs past the end)."""
    p = p.copy()
    p[4], p[5:] = 3, 2
    return p


REFUSALS = {
    "fewer_snps_than_the_panel": (dict(nSNPs_all=lambda n: RC.T_COMMON - 1), "fewer SNPs than the panel"),
    "common_count_differs": (dict(is_common=_set(0, 1)), "sum\\(snp_is_common\\) differs"),
    "rare_ptr_does_not_start_at_0": (dict(rare_ptr=_set(0, 1)), "bad rare_per_hap_info CSR"),
    "rare_ptr_decreases": (dict(rare_ptr=lambda p: np.r_[0, 2, 1, p[3:]]), "bad rare_per_hap_info CSR"),
    "rare_ptr_above_its_last_entry": (dict(rare_ptr=_ptr_above_its_end, rare_snp=lambda s: np.array([1, 2, 164], dtype=np.int32)),
                                      "a row ends beyond the last entry"),
    "entry_names_a_common_snp": (dict(rare_snp=_set(0, 3)), "names a SNP that is not rare"),
    "entry_below_range": (dict(rare_snp=_set(0, 0)), "names a SNP that is not rare"),
    "entry_above_range": (dict(rare_snp=_set(1, 165)), "names a SNP that is not rare"),
    "entries_descend": (dict(rare_snp=lambda s: np.r_[s[1], s[0], s[2:]]), "must ascend within a haplotype"),
    "entry_twice": (dict(rare_snp=_set(1, 1)), "must ascend within a haplotype"),
}


def test_the_table_the_refusals_start_from_is_accepted(dev):
    t = good_table()
    assert t["rare_snp"].tolist() == [1, 164, 2] and t["rare_ptr"][3:7].tolist() == [0, 2, 2, 3]
    assert create(dev, **t) == (0, "")


@pytest.mark.parametrize("what", list(REFUSALS))
def test_rare_common_create_refuses(dev, what):
    change, message = REFUSALS[what]
    t = _bad(**change)
    if what == "rare_ptr_above_its_last_entry":
        assert t["rare_ptr"][-1] == 2 < t["rare_ptr"][4] == 3 and len(t["rare_snp"]) == 3 and (np.diff(t["rare_ptr"][:5]) >= 0).all()
    st, msg = create(dev, **t)
    assert st == QA_ERR_INVALID
    import re
    assert re.search(message, msg), msg


def test_rare_common_create_accepts_no_rare_entries_and_a_null_list(dev, oracle):
    """n_rare = 0 with rare_snp NULL: accepted, and the call on it is the oracle's (every rare SNP is ref_error)."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.native import DeviceRareCommon
    t = good_table()
    t["rare_ptr"], t["rare_snp"] = np.zeros_like(t["rare_ptr"]), None
    assert create(dev, **t) == (0, "")
    case = RC.case("carriers", "nobody", RC.KS_SMALL)
    assert len(case.rc.rare_snp) == 0
    null_list = dataclasses.replace(case.rc, rare_snp=np.zeros(0, dtype=np.int32))
    drc = DeviceRareCommon(dev, null_list)
    try:
        ins = RC.gibbs_inputs(case)
        got = rcpp_forwardBackwardGibbsNIPT(dev, case.sample, case.which, case.H0, ins["ru"], ins["fr"], ins["rs"], rare_common=drc,
                                            return_state=True)
        ref = oracle.forwardBackwardGibbsNIPT(RC.panel(), case.sample, case.which, case.H0, ins["ru"], ins["fr"], ins["rs"], rare_common=case.rc)
        gibbs_compare(got, ref, RC.KS_SMALL, fetal=False)
    finally:
        drc.close()
