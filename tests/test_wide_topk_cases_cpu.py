"""The claims of tests/wide_topk_cases.py, checked without a device, under the rules of tests/test_grid_cases_cpu.py: the oracle
alone says of every constructed input what its builder says, and its gammas are separate enough (GC.SEP_RTOL among the first 65
ranks, both labels) that the device's lists are compared with no "allowed to differ" branch.  Then what the host side of the
feature does without a device: both statements of the per-sample loop refuse K_top_matches = 65 before the first sample, and agree
byte for byte at K_top_matches = 12 and 64 on the oracle backend."""
import numpy as np
import pytest

from tests import grid_cases as GC
from tests import mode_matrix as MM
from tests import wide_topk_cases as WC
from tests.oracle_backend import OracleBackend

NAMES = WC.case_names()


@pytest.fixture(scope="module")
def all_facts():
    return {c.name: WC.facts(c) for c in WC.all_cases()}


def check_case(c, f):
    """What a case must be for tests/test_wide_topk_gpu.py to pin anything with it."""
    cl = c.claims
    G, T, K = c.panel.nGrids, c.panel.nSNPs, c.panel.K
    assert GC.KMAXTOP < c.K_top <= WC.K_TOP_MAX
    assert (T + 31) // 32 == G and len(c.cols) == G and len(c.labels) == c.sample.nReads and set(c.labels.tolist()) <= {1, 2}
    assert np.all(np.diff(c.sample.wif) >= 0), "reads ordered by grid"
    for kind in ("thin", "dosage", "full"):
        r = GC.oracle_ref(c, kind, 1)
        assert np.isfinite(r["c"]).all() and (r["c"] > 0).all() and len(r["best_haps"]) == len(c.thin_grids)
        for idx, val in r["best_haps"]:
            assert len(idx) >= min(c.K_top, K) and np.isfinite(val).all() and (val > 0).all() and np.all(np.diff(idx) > 0)
    if "K_top" in cl:
        assert K == GC.K_BASE and set(f["lens"]) == {c.K_top}, "lists of exactly K_top"
    if "list_len" in cl:
        assert set(f["lens"]) == {cl["list_len"]}, "every list has the stated length"
    if "tie" in cl:
        rhb = np.asarray(c.panel.rhb_t)
        copies = list(cl["copies"])
        assert cl["list_len"] == max(c.K_top, cl["tie"])
        src = cl.get("source", 17)
        assert len(copies) == cl["tie"] and (rhb[copies] == rhb[src]).all()
        assert (rhb != rhb[src]).any(axis=1).sum() == K - cl["tie"], "no other row equals the copied one"
        for idx, val in GC.oracle_ref(c, "thin")["best_haps"]:
            order = np.argsort(-val, kind="stable")
            assert idx[order][:cl["tie"]].tolist() == copies[:len(idx)], "the copies lead every list, in haplotype order"
            assert len(set(val[np.isin(idx, copies)].tolist())) == 1
    if cl.get("one_lane"):
        for epv in (2, 4):
            assert len(set(WC.picker_lane(np.array(cl["copies"]), epv).tolist())) == 1, "one thread of the picker reads every copy"
        assert all(c.K_top <= n <= WC.WIDE_LIST for n in f["above_first_bound"]), "the first bound falls short; the gather holds what is above"
    if cl.get("overflow"):
        assert all(n > WC.WIDE_LIST for n in f["above_first_bound"])
    if cl.get("no_reads"):
        assert (c.gl == 1).all() and K > c.K_top
        for idx, val in GC.oracle_ref(c, "thin")["best_haps"]:
            assert np.array_equal(idx, np.arange(K)) and len(set(val.tolist())) == 1
    if "rows" in cl:
        assert K > WC.ROW and cl["rows"] == (K + WC.ROW - 1) // WC.ROW and K % WC.ROW, "several chunk rows, the last one partial"
        assert all(n >= c.K_top for n in f["distinct_head"]), ">= K_top distinct values among the first K_top ranks"
        assert len(f["rows_listed"]) > 1, "the listed haplotypes span more than one chunk row"
        assert cl["rows"] - 1 in f["rows_listed"], "... and reach the last, partial one (K = 57 600: the row that is streamed)"
    assert f["separation"] > GC.SEP_RTOL


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_it_claims(name, all_facts):
    check_case(WC.case(name), all_facts[name])


def test_label_2_outgrows_the_first_capacity(all_facts):
    """The reads entries run both labels: label 2 (two bases per grid) ties widely, and some of its lists pass 64 entries."""
    lens2 = [n for k in WC.K_TOPS for n in all_facts[f"ktop{k}"]["lens2"]]
    assert min(lens2) > GC.KMAXTOP and max(lens2) > GC.LIST_CAP


def test_coverage_table(all_facts):
    table = {}
    for name, f in all_facts.items():
        for e in WC.edges_of(f):
            table.setdefault(e, []).append(name)
    missing = WC.required_edges() - set(table)
    assert not missing, sorted(missing)
    assert len(NAMES) == len(set(NAMES)) == len(WC.all_cases())
    assert set(WC.SEEDS) <= set(NAMES)


# ---------------------------------------------------------------------------------------------------------------------------
# the per-sample loop, both statements, on the oracle backend
# ---------------------------------------------------------------------------------------------------------------------------
WIDE_ROW = dict(MM.BASE, method="diploid", Ksubset=64, Knew=40, heuristic_match_thin=0.5)
# On WIDE_ROW (10 thinned grids x 2 labels = 20 lists) the first three ranks already yield Knew = 40 new haplotypes: the oracle's
# result is the same for every K_top_matches >= 3, so it cannot show that ranks 9 .. 12 are read.  With three thinned grids (6 lists)
# eight ranks hold at most 48 entries and do not fill Knew = 40 -- the loop falls back to the complete lists -- while twelve ranks
# do: the row the guard below is made on.
GUARD_ROW = dict(WIDE_ROW, heuristic_match_thin=0.15)


def test_both_loops_refuse_K_top_matches_65_before_the_first_sample():
    from quilt_amd.driver import Driver
    from tests.native_driver_backend import impute_samples_on_oracle
    panel, rc, samples, P = MM.make_case(dict(WIDE_ROW, K_top_matches=WC.K_TOP_MAX + 1))
    with pytest.raises(ValueError, match=r"1\.\.64"):
        Driver(panel, OracleBackend(panel), P).run(samples, sample_offset=3)
    asked = []
    with pytest.raises(RuntimeError, match=r"status -3: .*1\.\.64") as e:   # QA_ERR_UNSUPPORTED
        impute_samples_on_oracle(panel, samples, P, sample_offset=3, samples_per_launch_set=2, source=dict(order_log=asked))
    assert "K_top_matches = 65" in str(e.value)
    assert asked == [], "sample_source->acquire was never called"


def _run_both(row, K_top):
    from quilt_amd.driver import Driver
    from tests.native_driver_backend import impute_samples_on_oracle
    panel, rc, samples, P = MM.make_case(dict(row, K_top_matches=K_top))
    want = Driver(panel, OracleBackend(panel), P).run(samples, sample_offset=3)
    got, stats, tab = impute_samples_on_oracle(panel, samples, P, sample_offset=3, samples_per_launch_set=2, n_threads=2)
    assert tab.calls["select"] > 0
    assert len(got) == len(want) == 3
    for a, b in zip(got, want):
        assert a.nDosage == b.nDosage
        for f in ("read_labels", "dosage", "gp_t", "phasing_haps"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
    return want, stats


@pytest.mark.parametrize("K_top", [12, 64])
@pytest.mark.parametrize("row", ["wide", "guard"])
def test_both_loops_return_the_same_bytes(row, K_top):
    _run_both(dict(wide=WIDE_ROW, guard=GUARD_ROW)[row], K_top)


def test_ranks_9_to_12_are_used():
    """The guard: on GUARD_ROW the selection at K_top_matches = 12 completes from the ranks alone, at 8 it needs the complete lists,
    and the two results differ -- ranks 9 .. 12 decide what is imputed from."""
    at8, stats8 = _run_both(GUARD_ROW, 8)
    at12, stats12 = _run_both(GUARD_ROW, 12)
    assert stats8["full_list_refetches"] > 0 and stats12["full_list_refetches"] == 0
    assert any(not np.array_equal(a.dosage, b.dosage) for a, b in zip(at12, at8))
