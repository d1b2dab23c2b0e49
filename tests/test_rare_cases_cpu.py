"""The claims of tests/rare_cases.py, proven without a device: numpy restatements of the host code (prepare_chain's rc_any and
informative count with the fold, upload_rare_pairs' words, k_happrobs_rc's view of an all-SNP grid) and the oracle's emission columns
must say of every constructed input what its builder says.  A case whose claim fails here is a broken builder, and
tests/test_rare_geometry_gpu.py would pin nothing with it.  No case is skipped or filtered; the coverage table is derived from the same
facts, never from a case's name, and fails when a constant listed at the top of rare_cases.py is hit by no case."""
import numpy as np
import pytest

from tests import rare_cases as RC
from tests import read_cases

IDS = RC.case_ids()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def all_facts(oracle):
    return {i: RC.facts(RC.case(*i), oracle) for i in IDS}


def test_the_panel_and_the_subsets():
    p = RC.panel()
    assert (p.K, p.nSNPs, p.nGrids) == (RC.K, RC.T_COMMON, 5)
    assert (np.asarray(p.hapMatcherR)[:, 2] == 0).any(), "grid 2 holds special haplotypes"
    w70, w600, w1024 = (RC.which_of(k) for k in (RC.KS_SMALL, RC.KS_LARGE, RC.KS_MAX))
    for w, n in ((w70, 70), (w600, 600), (w1024, 1024)):
        assert len(w) == n and (np.diff(w) > 0).all() and w[0] == 1 and w[-1] == RC.K
    assert set(w70) < set(w600) < set(w1024)
    assert not set(RC.never_selected() + 1) & set(w1024) and set(RC.always_selected() + 1) <= set(w70)
    for Ks in RC.LAYOUT_KS:
        a, b, only_a, only_b = RC.two_chain_subsets(Ks)
        assert len(a) == len(b) == Ks and set(a) - set(b) == set(only_a + 1) and set(b) - set(a) == set(only_b + 1)
        assert not set(RC.never_selected()) & (set(only_a) | set(only_b))


def test_planted_rc_refuses_what_does_not_fit():
    p = RC.panel()
    with pytest.raises(AssertionError):
        RC.planted_rc(p, RC.C(159) + RC.R(3), {})
    with pytest.raises(AssertionError):
        RC.planted_rc(p, RC.C(160) + RC.R(1), {0: [1]})
    with pytest.raises(AssertionError):
        RC.planted_rc(p, RC.C(1) + RC.R(int(p.L[1] - p.L[0])) + RC.C(159), {})
    rc = RC.planted_rc(p, RC.R(2) + RC.C(160) + RC.R(2), {0: [5, 3], 163: [3]})
    assert rc.rare_snp.tolist() == [1, 164, 1] and rc.rare_ptr[3] == 0 and rc.rare_ptr[4] == 2 and rc.rare_ptr[6] == rc.rare_ptr[-1] == 3
    assert rc.transMatRate_t_all.shape == (2, rc.nGrids_all - 1) and len(rc.L_grid_all) == rc.nGrids_all == 6


@pytest.mark.parametrize("family,name,Ks", IDS, ids=[RC.id_of(*i) for i in IDS])
def test_case_is_what_it_claims(family, name, Ks, all_facts, oracle):
    c, f = RC.case(family, name, Ks), all_facts[(family, name, Ks)]
    s, rc, cl, p = c.sample, c.rc, c.claims, RC.panel()
    T, G = rc.nSNPs_all, rc.nGrids_all
    # the inputs are well formed
    assert len(c.which) == Ks and (T + 31) // 32 == G and 150 < T <= 700 and 1 <= s.nReads <= 200
    assert int(np.asarray(rc.snp_is_common).sum()) == p.nSNPs and rc.rare_ptr[0] == 0 and (np.diff(rc.rare_ptr) >= 0).all()
    for k in range(p.K):
        lst = rc.rare_snp[rc.rare_ptr[k]:rc.rare_ptr[k + 1]] - 1
        assert (np.diff(lst) > 0).all() and (len(lst) == 0 or (lst[0] >= 0 and lst[-1] < T and not rc.snp_is_common[lst].any()))
    assert (np.diff(s.read_ptr) >= 1).all() and s.read_ptr[0] == 0 and s.read_ptr[-1] == len(s.u) == len(s.bq)
    assert (np.diff(s.wif) >= 0).all() and s.wif.max() < G and s.u.min() >= 0 and s.u.max() < T and np.abs(s.bq).max() <= 93
    assert set(c.H0.tolist()) <= {1, 2} and len(c.H0) == s.nReads
    for r in range(s.nReads):
        assert (np.diff(s.u[s.read_ptr[r]:s.read_ptr[r + 1]]) > 0).all()
    if c.isolating:
        counts = np.zeros((G, 2), dtype=np.int64)
        np.add.at(counts, (s.wif, c.H0 - 1), 1)
        assert counts.max() == 1
    # no column maximum near the edge of the double range; the sampler runs on the oracle
    assert f["raw"].max(axis=0).min() > 1e-250
    ins = RC.gibbs_inputs(c)
    for which in (c.which,) + (() if c.which_b is None else (c.which_b,)):
        ref = oracle.forwardBackwardGibbsNIPT(p, s, which, c.H0, ins["ru"], ins["fr"], ins["rs"], rare_common=rc, Jmax=c.Jmax,
                                              maxDifferenceBetweenReads=c.maxdiff)
        assert ref["status"] == 0
    lay, rows, n_inf = f["layout"], f["rows"], f["n_inf"]
    # layout claims
    if "no_common" in cl:
        assert tuple(g for g in range(G) if lay[g]["n_common"] == 0) == cl["no_common"]
        assert all(lay[g]["cg"] == -1 and lay[g]["first_b"] == -1 for g in cl["no_common"])
    if "two_cg" in cl:
        assert tuple(g for g in range(G) if len(lay[g]["cgs"]) == 2) == cl["two_cg"]
    for g, b in cl.get("first_b", {}).items():
        assert lay[g]["first_b"] == b
    for g, n in cl.get("n_common", {}).items():
        assert lay[g]["n_common"] == n
    if "guarded" in cl:
        assert tuple(g for g in range(G) if lay[g]["second_word_guarded"]) == cl["guarded"]
        assert all(lay[g]["cgs"] == (p.nGrids - 2, p.nGrids - 1) for g in cl["reaches_last_cg"])
    if "tail" in cl:
        assert lay[-1]["nLocal"] == cl["tail"] and T % 32 == cl["tail"] % 32
        if cl["last"] == "rare":
            assert not rc.snp_is_common[T - 1] and T - 1 in rows and (s.u[s.bq != 0] == T - 1).any()
        else:
            assert rc.snp_is_common[T - 1] and lay[-1]["n_common"] == 1 and lay[-1]["cg"] == p.nGrids - 1
    for t in cl.get("carried", ()):
        assert t in rows and (s.u[s.bq != 0] == t).any()
    for t in cl.get("uncarried", ()):
        assert not rc.snp_is_common[t] and t not in f["named"]
    # carrier claims
    if "pairs_total" in cl:
        assert f["pairs"].sum() == cl["pairs_total"]
    if cl.get("csr_empty"):
        assert rc.rare_ptr[-1] == 0 and len(rc.rare_snp) == 0
    for t in cl.get("named_not_carried", ()):
        assert t in f["named"] and t not in rows and (s.u[s.bq != 0] == t).any()
    for t, want in cl.get("rows", {}).items():
        assert tuple(rows[t]) == tuple(want)
    for g, n in cl.get("pairs", {}).items():
        assert f["pairs"][g] == n
    if "parts" in cl:
        assert tuple(sorted(r[0] % RC.PARTS for r in rows.values())) == cl["parts"] and all(len(r) == 1 for r in rows.values())
    for t in cl.get("everyone", ()):
        assert rows[t] == list(range(Ks))
    if "csr_row" in cl:
        k = cl["csr_row"]
        assert rc.rare_ptr[k + 1] - rc.rare_ptr[k] == 3 and rc.rare_ptr[-1] == 3 and k in (0, p.K - 1)
    if "list_len" in cl:
        k = RC.hap_of(c.which, cl["list_row"])
        lst = (rc.rare_snp[rc.rare_ptr[k]:rc.rare_ptr[k + 1]] - 1).tolist()
        assert len(lst) == cl["list_len"] and cl["present"] == (lst[0], lst[len(lst) // 2], lst[-1])
        below, between, above = cl["absent"]
        assert below < lst[0] and lst[0] < between < lst[-1] and above > lst[-1] and not set(cl["absent"]) & set(lst)
        for t in cl["present"] + cl["absent"]:   # k_ematread searches every row's list for it: carried by someone, read with a quality
            assert t in rows and (s.u[s.bq != 0] == t).any()
        assert set(cl["list_lens"]) <= {int(rc.rare_ptr[k] - rc.rare_ptr[k - 1]) for k in c.which}
    if "max_word" in cl:
        assert f["max_word"] == cl["max_word"] == ((RC.SNPS_PER_GRID - 1) << 10 | RC.ROW_MASK) == 0x7FFF
    # read claims
    for r, n in cl.get("n_inf", {}).items():
        assert n_inf[r] == n, (name, "n_inf", r, n_inf[r], n)
    for r, n in cl.get("n_inf_b", {}).items():
        assert f["n_inf_b"][r] == n, (name, "n_inf_b", r, f["n_inf_b"][r], n)
    for r, d in cl.get("dense", {}).items():
        assert (n_inf[r] > RC.MAX_PATTERN_BITS) == d
    eff = read_cases.fold_qualities(s, c.Jmax)
    for r, idx in cl.get("zeros", {}).items():
        at = s.read_ptr[r] + np.asarray(idx)
        assert (s.bq[at] == 0).all() and (eff[at] != 0).all() and (eff[at] == eff[at - 1]).all()
    for j, v in cl.get("folded", {}).items():
        assert s.bq[j] == 0 and v != 0 and eff[j] == v
    for r, n in cl.get("n_bases", {}).items():
        assert s.read_ptr[r + 1] - s.read_ptr[r] == n
    cs = RC.common_index(rc)
    for key, pred in (("rare_at_block_offsets", lambda t: cs[t] < 0), ("carried_at_block_offsets", lambda t: int(t) in rows)):
        for r, offs in cl.get(key, {}).items():
            off = RC.block_offsets(s, r)
            for o in offs:
                assert pred(s.u[s.read_ptr[r] + int(np.flatnonzero(off == o)[0])]), (key, o)
    for r, js in cl.get("carried_at_base", {}).items():
        assert all(int(s.u[s.read_ptr[r] + j]) in rows for j in js) and s.read_ptr[r + 1] - s.read_ptr[r] - 1 > c.Jmax == js[0]
    for r in cl.get("clip_visible", ()):   # a clip one base early or late gives another column
        for other in (c.Jmax - 1, c.Jmax + 1):
            col = RC.oracle_columns(c, c.which, oracle, Jmax=other)[:, r]
            assert np.abs(col / f["cols"][:, r] - 1).max() > 1e-3, (name, "clip is invisible", other)
    for r in cl.get("equal", ()):
        col = f["cols"][:, r]
        assert f["raw"][:, r].min() == f["raw"][:, r].max() < 1 and col.min() == col.max() >= 1 - 1e-12 and n_inf[r] > 0
    for r in cl.get("floor", ()):
        col = f["cols"][:, r]
        assert (col == 1 / c.maxdiff).any() and col.max() >= 1 - 1e-12 and c.maxdiff == 1e3
    if cl.get("chain_starts_at_zero_on_carried"):
        assert s.bq[0] == 0 and eff[0] == 0 and int(s.u[0]) in rows
    for r in cl.get("all_ones", ()):
        assert (f["cols"][:, r] == 1.0).all()
    for r in cl.get("rare_only", ()):
        assert (cs[s.u[s.read_ptr[r]:s.read_ptr[r + 1]]] < 0).all()
    for r in cl.get("then_common_in_block", ()):
        assert cs[s.u[s.read_ptr[r + 1]]] >= 0 and (r + 1) // RC.READS_PER_WAVE == r // RC.READS_PER_WAVE
        assert (cs[s.u[s.read_ptr[r - r % RC.READS_PER_WAVE]:s.read_ptr[r + 1]]] < 0).all() or r % RC.READS_PER_WAVE == 0
    # conditions that are not measurements
    if name.startswith("threshold_"):
        forms = {bool(n_inf[r] > RC.MAX_PATTERN_BITS) for r in cl["n_inf"]}
        assert forms == {False, True}, "a threshold case holds a compact and a dense read"
    if name == "two_chains_one_read":
        da, db = n_inf > RC.MAX_PATTERN_BITS, f["n_inf_b"] > RC.MAX_PATTERN_BITS
        assert tuple(np.flatnonzero(da & ~db)) == cl["dense_a_compact_b"] and tuple(np.flatnonzero(~da & db)) == cl["compact_a_dense_b"]
        assert len(cl["dense_a_compact_b"]) >= 1 and len(cl["compact_a_dense_b"]) >= 1
        ra, rb = RC.carried_rows(rc, c.which), RC.carried_rows(rc, c.which_b)
        assert ra and rb and not set(ra) & set(rb), "what one chain's haplotypes carry, no haplotype of the other does"
        assert (f["cols_b"][:, 5] == 1.0).all() and not (f["cols"][:, 5] == 1.0).all()


def test_the_single_row_cases_tell_rows_apart(oracle):
    """row_63 against row_64 (and every single-row case): the oracle's posterior at the rare SNP's grid differs between the carrying
    row and its neighbours, so a sum that takes the neighbour's row gives another dosage."""
    p = RC.panel()
    for family, name, Ks in IDS:
        if not name.startswith("row_") and name != "ks1024_row1023_b31":
            continue
        c = RC.case(family, name, Ks)
        ins = RC.gibbs_inputs(c)
        ref = oracle.forwardBackwardGibbsNIPT(p, c.sample, c.which, c.H0, ins["ru"], ins["fr"], ins["rs"], rare_common=c.rc)
        for t, (row,) in c.claims["rows"].items():
            g = t // 32
            for h in range(2):
                gam = ref["alphaHat_t"][h][:, g] * ref["betaHat_t"][h][:, g] / ref["c"][h][g]
                for other in (row - 1, row + 1):
                    if 0 <= other < Ks:
                        assert abs(gam[row] - gam[other]) > 1e-6 * gam[row], (name, Ks, t, h, other)


@pytest.mark.parametrize("name,Ks", [("two_common_grids_at_end", 70), ("long_list", 600), ("tail_1_rare", 70)])
def test_happrobs_restatement_agrees_with_the_oracle(oracle, name, Ks):
    """The long-double restatement the device test holds k_happrobs_rc against, on the oracle's own final state; and the three-label
    call runs on the oracle with the all-SNP grid's positions."""
    p = RC.panel()
    c = RC.case("carriers" if name == "long_list" else "layout", name, Ks)
    ins = RC.gibbs_inputs(c)
    ref = oracle.forwardBackwardGibbsNIPT(p, c.sample, c.which, c.H0, ins["ru"], ins["fr"], ins["rs"], rare_common=c.rc)
    hp, gm, is_common, carried = RC.happrobs_from_state(c.rc, c.which, ref["alphaHat_t"][:2], ref["betaHat_t"][:2], ref["c"][:2])
    np.testing.assert_allclose(ref["hapProbs_t"][:2], hp.astype(np.float64), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ref["genProbsM_t"], gm.astype(np.float64), rtol=1e-9, atol=1e-14)   # ((1 - g) cancels: the device test's bar)
    assert (ref["hapProbs_t"][:2][:, ~is_common & ~carried] == p.ref_error).all() and (~is_common & ~carried).any() and carried.any()
    assert (ref["genProbsF_t"] == 0).all(), "the diploid all-SNP call leaves genProbsF_t as it was (gibbs-small.cpp:858)"
    ref3 = oracle.forwardBackwardGibbsNIPT(p, c.sample, c.which, ins["H3"], ins["ru"], ins["fr"], np.zeros(3 * c.rc.nGrids_all), ff=RC.FF,
                                           rare_common=c.rc, runif_block=ins["rb"], runif_resample=ins["rr"], L_grid=c.rc.L_grid_all)
    assert ref3["status"] == 0 and (ref3["hapProbs_t"][2] > 0).all() and (ref3["genProbsF_t"] != 0).any()


def test_coverage_table(all_facts):
    """Every edge the suite is there for is hit by at least one case, and so is every constant."""
    table = {}
    for i, f in all_facts.items():
        for e in RC.edges_of(RC.case(*i), f):
            table.setdefault(e, []).append(RC.id_of(*i))
    for constant in RC.CONSTANTS:
        missing = RC.REQUIRED[constant] - set(table)
        assert not missing, (constant, sorted(missing))
    for e in sorted(table):
        print(f"{e}: {len(table[e])} cases, e.g. {table[e][0]}")
    assert len(IDS) == len(set(IDS))
