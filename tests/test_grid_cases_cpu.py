"""The claims of tests/grid_cases.py, checked without a device: the oracle alone must say of every constructed input what its
builder says -- where alpha is renormalised, which grids have no variant, which hold special haplotypes, how long the lists are --
and its gammas must be separate enough that the device's lists can be compared with no "allowed to differ" branch.  A case whose
claim fails here is a broken builder, and tests/test_grid_geometry_gpu.py would pin nothing with it.  No case is skipped or
filtered; the coverage table is the union of what these same checks derive."""
import numpy as np
import pytest

from tests import grid_cases as GC

NAMES = GC.case_names()


@pytest.fixture(scope="module")
def all_facts():
    return {c.name: GC.facts(c) for c in GC.all_cases()}


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_it_claims(name, all_facts):
    c, f, cl = GC.case(name), all_facts[name], GC.case(name).claims
    G, T = c.panel.nGrids, c.panel.nSNPs
    assert (T + 31) // 32 == G and len(c.cols) == G and len(c.labels) == c.sample.nReads and set(c.labels.tolist()) <= {1, 2}
    assert c.panel.transMatRate_t.shape == (2, G - 1), "one grid: the transition matrix is the empty one, as the header states it"
    assert np.all(np.diff(c.sample.wif) >= 0), "reads ordered by grid"
    assert np.array_equal(c.cols[c.cols >= 0], np.arange(len(c.thin_grids))), "columns numbered ascending"
    # the oracle ran (status 0: oracle_ref raises otherwise) and everything it returns is finite
    for kind, always in (("thin", c.always_normalize), ("dosage", False), ("full", False)):
        r = GC.oracle_ref(c, kind, 1, always)
        assert np.isfinite(r["c"]).all() and (r["c"] > 0).all()
        if kind != "thin":
            assert np.isfinite(r["dosage"]).all() and r["dosage"].min() >= 0 and r["dosage"].max() <= 1 + 1e-12
        assert len(r["best_haps"]) == len(c.thin_grids)
        for idx, val in r["best_haps"]:
            assert len(idx) >= min(c.K_top, c.panel.K) and np.isfinite(val).all() and (val > 0).all() and np.all(np.diff(idx) > 0)
    for label in (1, 2):   # both labels ride through the reads entries
        assert np.isfinite(GC.oracle_ref(c, "dosage", label)["gamma_t"]).all()
    # the claims
    if "G" in cl:
        assert (f["G"], f["T"], f["last_grid_snps"]) == (cl["G"], cl["T"], cl["last_grid_snps"]) and cl["last_grid_snps"] in (1, 32)
        assert c.panel.K == GC.K_BASE
    if "renorm" in cl:
        assert f["renorm"] == cl["renorm"], "alpha is renormalised at exactly the interior grids the case names"
        lazy = GC.renormalised(c, GC.oracle_ref(c, "thin")["c"])
        assert lazy == (() if c.always_normalize else cl["renorm"])
        assert f["novar"] == ()
    if "novar" in cl:
        assert f["novar"] == tuple(cl["novar"]), "gl == 1 throughout exactly the grids the case names"
    if cl.get("nMaxDH") == 8:
        assert c.panel.nMaxDH == 8
        if f["last_grid_snps"] == 32:
            assert {0, G - 1} <= set(f["specials"]), "specials in the first and in the last grid"
        if "novar" in cl:
            assert set(cl["novar"]) <= set(f["specials"]), "the no-variant grids hold specials"
    elif "nMaxDH" in cl:
        assert f["specials"] == ()
    if "thin" in cl:
        assert f["thin"] == tuple(cl["thin"])
    if "list_len" in cl:
        assert set(f["lens"]) == {cl["list_len"]}, "every list has the stated length"
        assert set(GC.list_lengths(c, 1)) == set(len(i) for i, _ in GC.oracle_ref(c, "dosage")["best_haps"])
    if "tie" in cl:
        rhb = np.asarray(c.panel.rhb_t)
        copies = list(cl["copies"])
        assert len(copies) == cl["tie"] and (rhb[copies] == rhb[17]).all()
        assert (rhb != rhb[17]).any(axis=1).sum() == c.panel.K - cl["tie"], "no other row equals the copied one"
        for idx, val in GC.oracle_ref(c, "thin")["best_haps"]:
            order = np.argsort(-val, kind="stable")
            assert idx[order][:cl["tie"]].tolist() == copies[:len(idx)], "the copies lead every list, in haplotype order"
            assert len(set(val[np.isin(idx, copies)].tolist())) == 1
    if cl.get("no_reads"):
        assert (c.gl == 1).all() and (c.labels == 2).all() and c.sample.nReads > 0
        for idx, val in GC.oracle_ref(c, "thin")["best_haps"]:
            assert np.array_equal(idx, np.arange(c.panel.K)) and len(set(val.tolist())) == 1
    # separation: any two gammas among the first 65 ranks of a thinned grid are equal or apart, for both labels
    assert f["separation"] > GC.SEP_RTOL


def test_schedule_inputs(all_facts):
    """The strong grids do what the builder computes: one of them alone takes the running product of minimum emissions below
    1e-100, and the weak background never does over the whole region."""
    p = GC.schedule_panel()
    assert p.K == GC.K_BASE and p.nGrids == GC.G_BIG and p.ref_error == GC.SCHED_REF_ERROR
    assert (np.asarray(p.rhb_t)[0] == 0).all() and (np.asarray(p.rhb_t)[1] == -1).all()
    assert (GC.SCHED_REF_ERROR * 1.01) ** GC.STRONG_SNPS < 1e-100 < (GC.SCHED_REF_ERROR * 1.01) ** (GC.STRONG_SNPS - 2)
    c = GC.case("renorm_block_edge")
    gl = c.gl
    for g in GC.SCHEDULES["block_edge"]:
        strong = gl[:, 32 * g:32 * g + GC.STRONG_SNPS]
        assert (strong[0] == GC.MIN_GL).all() and (strong[1] == 1).all()
    assert all_facts["renorm_none"]["renorm"] == () and all_facts["renorm_every_grid"]["renorm"] == tuple(range(1, GC.G_BIG - 1))
    assert np.array_equal(GC.case("renorm_none").gl, GC.case("renorm_every_grid").gl)


def test_groups():
    """The cases that share a qa_fullpass_batch call share panel, columns and K_top."""
    groups = GC.groups()
    assert {"schedule", "novar", "novar_dh8"} <= set(groups)
    for cs in groups.values():
        assert all(c.panel is cs[0].panel and np.array_equal(c.cols, cs[0].cols) and c.K_top == cs[0].K_top for c in cs)


def test_coverage_table(all_facts):
    """Every edge the suite is there for is hit by at least one case -- derived from the oracle's facts, not from names."""
    table = {}
    for name, f in all_facts.items():
        for e in GC.edges_of(f):
            table.setdefault(e, []).append(name)
    missing = GC.required_edges() - set(table)
    assert not missing, sorted(missing)
    assert len(NAMES) == len(set(NAMES)) == len(GC.builders())
