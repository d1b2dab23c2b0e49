"""Every claim of tests/chain_cases.py, proved on the arrays and the CPU oracle alone (no device).

The GPU suite (tests/test_chain_geometry_gpu.py) compares the samplers with the oracle on these chains; it says something about the
stream refills only if each chain sits where its builder says, if the sweeps and passes do something there, and if the oracle
itself survives the input.  So: status 0 for every case; labels that move; every stated run, read-less range, category-1 read and
emission form recomputed from the arrays and the oracle's own read categories; every planted block table what
qo_make_gibbs_considers returns, and the same under a 1e-9 relative perturbation of the rates; passes that change labels on both
sides of read 64; and every edge the suite names hit by at least one case.  No case is skipped or allowed to differ: a case
that misses a claim gets another seed in chain_cases.SEEDS.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import chain_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = cc.all_cases()
BY_FAMILY = lambda *f: [c for c in ALL if c.spec.family in f]
ids = lambda cs: [c.name for c in cs]


@pytest.mark.parametrize("c", ALL + cc.big_build_cases(), ids=ids(ALL + cc.big_build_cases()))
def test_oracle_status_and_movement(c):
    ref = cc.oracle_ref(c)
    assert ref["status"] == 0
    assert ref["H"].min(initial=1) >= 1 and ref["H"].max(initial=1) <= (3 if c.mode == "nipt" else 2)
    if c.R >= 20:
        assert (ref["H"] != c.H0).mean() >= 0.1


def test_sizes():
    for c in ALL:
        s = c.sample
        n = np.diff(s.read_ptr)
        assert c.Ks in (cc.KS, cc.KS_BIG) and c.G <= 130 and c.R <= 260
        assert c.R == 0 or (n.min() >= 1 and n.max() <= 7)
        assert (s.u // 32 == np.repeat(s.wif, n)).all()   # every read inside its own grid
        q = np.abs(s.bq)
        crowded = np.repeat(np.bincount(s.wif, minlength=c.G)[s.wif] > cc.CROWDED, n)
        assert ((q[crowded] >= 1) & (q[crowded] <= 6)).all() and ((q[~crowded] >= 20) & (q[~crowded] <= 30)).all()
        for k in ("G", "T", "R"):
            if k in c.claims:
                assert c.claims[k] == dict(G=c.G, T=c.panel.nSNPs, R=c.R)[k], c.name
        if "last_grid_snps" in c.claims:
            assert c.panel.nSNPs - 32 * (c.G - 1) == c.claims["last_grid_snps"]


@pytest.mark.parametrize("c", BY_FAMILY("runs"), ids=ids(BY_FAMILY("runs")))
def test_runs_and_readless_ranges(c):
    runs = cc.runs_of(c.sample.wif)
    for run in c.claims.get("runs", ()):
        assert tuple(run) in runs, (run, runs)
    quiet = [g for a, b in cc.readless_runs(c.sample.wif, c.G) for g in range(a, b + 1)]
    if "readless" in c.claims:
        assert set(c.claims["readless"]) <= set(quiet)
        if len(c.claims["readless"]) == 4:   # the run across the refill is exactly 62 .. 65
            assert (62, 65) in cc.readless_runs(c.sample.wif, c.G)
    if c.claims.get("one_per_grid"):
        assert np.array_equal(c.sample.wif, np.arange(c.G))


@pytest.mark.parametrize("c", BY_FAMILY("skipped"), ids=ids(BY_FAMILY("skipped")))
def test_category_one_reads(c):
    """The oracle's read categories (gibbs-nipt.cpp:338-382) say which reads the sweeps skip: exactly the planted ones, none with
    the categories switched off; and no entry of a planted read's emission column lies below 1 - 1e-12."""
    ref = cc.oracle_ref(c)
    planted = np.array(c.claims["cat1"])
    if c.claims["nocat"]:
        assert (ref["read_category"] == 0).all()
        on = cc.oracle_ref(c, disable_read_category_usage=False)
        assert np.array_equal(np.flatnonzero(on["read_category"] == 1), planted)
    else:
        assert np.array_equal(np.flatnonzero(ref["read_category"] == 1), planted)
    assert (ref["eMatRead_t"][:, planted] >= 1 - 1e-12).all()
    others = np.setdiff1d(np.arange(c.R), planted)
    assert (ref["eMatRead_t"][:, others].min(axis=0) < 1 - 1e-12).all()


@pytest.mark.parametrize("c", BY_FAMILY("forms"), ids=ids(BY_FAMILY("forms")))
def test_emission_forms_across_the_refill(c):
    n = np.diff(c.sample.read_ptr)   # every base has a quality: all of them are informative
    assert (c.sample.bq != 0).all()
    for r, form in c.claims["forms"].items():
        assert (n[r] > cc.MAX_PATTERN_BITS) == (form == "dense")
    assert (n[63] > cc.MAX_PATTERN_BITS) != (n[64] > cc.MAX_PATTERN_BITS)
    assert c.sample.wif[63] != c.sample.wif[64]   # and read 64 opens a grid's run


@pytest.mark.parametrize("c", BY_FAMILY("blocks"), ids=ids(BY_FAMILY("blocks")))
def test_planted_block_tables(c):
    t = cc.first_pass_table(c)
    assert tuple(int(x) for x in t["consider_grid_end_0_based"]) == c.claims["ends"]
    assert t["n_blocks"] == len(c.claims["ends"])
    rs, re = t["consider_reads_start_0_based"], t["consider_reads_end_0_based"]
    assert rs[0] == 0 and re[-1] == c.R - 1 and (rs[1:] == re[:-1] + 1).all()
    if "reads" in c.claims:
        assert [tuple(x) for x in zip(rs.tolist(), re.tolist())] == list(c.claims["reads"])
    planted = np.array(c.claims["planted"], dtype=np.int64)
    natural = np.delete(t["rate2"], planted)
    assert natural.max() < 1 and (len(planted) == 0 or t["rate2"][planted].min() > 2)
    rng = np.random.default_rng(5)
    for _ in range(4):
        t2 = cc.first_pass_table(c, perturb=1 + 1e-9 * rng.uniform(-1, 1, size=c.G - 1))
        for k in ("consider_grid_start_0_based", "consider_grid_end_0_based", "consider_reads_start_0_based", "consider_reads_end_0_based",
                  "consider_grid_where_0_based"):
            assert np.array_equal(t[k], t2[k]), k


NIPT_WITH_READS = [c for c in ALL if c.mode == "nipt" and c.R > 0]


@pytest.mark.parametrize("c", NIPT_WITH_READS, ids=ids(NIPT_WITH_READS))
def test_first_pass_table_is_the_one_inside_the_call(c):
    """chain_cases.first_pass_table forms the rates in NumPy from a call cut short at the first block iteration; the blocked grids
    it arrives at are those qo_define_blocked_grids returned INSIDE the whole call at its first pass (the oracle's capture aid),
    and the second and third pass took place."""
    full = cc.oracle_ref(c, return_blocked_grids=True)
    assert full["status"] == 0 and np.array_equal(full["H"], cc.oracle_ref(c)["H"])
    assert np.array_equal(full["blocked_grids"][0], cc.first_pass_table(c)["blocked_grid"])
    assert (full["blocked_grids"] >= 0).all()


def _passes_matter(c):
    on, off = cc.oracle_ref(c), cc.oracle_ref(c, perform_block_gibbs=False)
    d = np.flatnonzero(on["H"] != off["H"])
    return (d < cc.STREAM).any() and (d >= cc.STREAM).any()


# The shard pass flips what lies to the right of a decision, so reads on grid 0 are never touched by it, and a chain of at most
# 64 reads has no read on the far side of the refill: every other run case is held to the claim.
SHARD_CASES = [c for c in BY_FAMILY("runs") if c.mode != "nipt" and c.R > cc.STREAM and c.sample.wif.max() > 0]


@pytest.mark.parametrize("c", SHARD_CASES, ids=ids(SHARD_CASES))
def test_shard_passes_matter_on_both_sides_of_read_64(c):
    assert _passes_matter(c)


def test_shard_claim_leaves_out_only_what_cannot_hold():
    left_out = {c.spec.name for c in BY_FAMILY("runs") if c.mode != "nipt"} - {c.spec.name for c in SHARD_CASES}
    assert left_out == {"runs_all_on_g0", "runs_G129_five_on_last"}


@pytest.mark.parametrize("c", BY_FAMILY("blocks"), ids=ids(BY_FAMILY("blocks")))
def test_block_passes_matter_on_both_sides_of_read_64(c):
    assert _passes_matter(c)


def test_every_named_edge_is_hit():
    have = set()
    for c in ALL:
        have |= cc.edges_of(c)
    assert not cc.required_edges() - have, sorted(cc.required_edges() - have)


def test_groups_share_what_a_batch_call_shares():
    for cs in list(cc.groups(ALL).values()) + list(cc.groups(cc.big_build_cases()).values()):
        assert len({(id(c.panel), c.Ks, c.mode, str(sorted((k, str(v)) for k, v in c.kwargs().items()))) for c in cs}) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# what the oracle used to die on: a single read, and a single grid, with block passes (NIPT)
# ---------------------------------------------------------------------------------------------------------------------------
DIED = ("reads_R1:nipt", "one_read_G2:nipt", "grids_G1_T32:nipt", "grids_G1_T1:nipt")


@pytest.mark.parametrize("name", DIED)
def test_oracle_survives_one_read_and_one_grid_in_a_child_process(name):
    """In a process of its own, so that a heap corruption or a fault fails this test and nothing else."""
    code = ("import numpy as np\nfrom tests import chain_cases as cc\n"
            f"c = cc.case({name!r})\nr = cc.oracle_ref(c)\nassert r['status'] == 0\n"
            "off = cc.oracle_ref(c, perform_block_gibbs=False)\nassert off['status'] == 0\nprint('survived', c.G, c.R)\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, MALLOC_CHECK_="3", MALLOC_PERTURB_="165"))
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    c = cc.case(name)
    assert run.stdout.split("\n")[-2] == f"survived {c.G} {c.R}"
    assert c.R == 1 or c.G == 1


def test_a_block_never_recorded_is_a_block_without_reads():
    """One read: no block's reads are recorded and the removal is skipped because every block would go; the table then says
    start 0, end -1 for every block (an empty loop), never -1 / -1 (an index before the chain's reads)."""
    from oracle import oracle as O
    for blocked, wif in (([0, 0, 1, 1, 2], [3]), ([0, 0, 0], [1]), ([0, 1], [0]), ([0], [0]), ([0, 0, 1], [])):
        t = O.make_gibbs_considers(blocked, wif)
        assert t["n_blocks"] == blocked[-1] + 1
        assert (t["consider_reads_start_0_based"] == 0).all() and (t["consider_reads_end_0_based"] == -1).all()
    t = O.make_gibbs_considers([0, 0, 1, 1, 2], [0, 3])   # two reads: the last read's block takes both, the others are merged away
    assert t["n_blocks"] == 1 and t["consider_reads_start_0_based"][0] == 0 and t["consider_reads_end_0_based"][0] == 1
    assert np.array_equal(O.define_blocked_grids(np.zeros(0), [1000]), [0])   # one grid: one block, no rate looked at


# ---------------------------------------------------------------------------------------------------------------------------
# oracle and host header side by side under AddressSanitizer + UBSan, as a stand-alone program (tests/c/gibbs_blocks_san.cpp)
# ---------------------------------------------------------------------------------------------------------------------------
def _record(f, a, dtype=None):
    b = b"" if a is None else (np.asarray(a, dtype=dtype) if dtype is not None else np.asarray(a)).tobytes(order="A")
    f.write(np.int64(len(b)).tobytes() + b)


def _write_call(f, c):
    from oracle.oracle import grid_has_read_of
    p, s = c.panel, c.sample
    sptr, svals = p.special_csr()
    kw = c.kwargs()
    _record(f, [p.K, p.nGrids, p.nSNPs, p.nMaxDH, p.eMatDH_special_matrix.shape[0], int(p.rhb_t is None), c.Ks, c.R, c.first_read,
                kw.get("shuffle_bin_radius", 5000), 20, 1], np.int32)
    _record(f, [p.ref_error, cc.FF, kw.get("block_gibbs_quantile_prob", 0.95)], np.float64)
    for a, dt in ((p.rhb_t, np.int32), (p.hapMatcher, np.int32), (p.hapMatcherR, np.uint8), (p.distinctHapsB, np.int32),
                  (p.distinctHapsIE, np.float64), (p.eMatDH_special_grid_which, np.int32), (sptr, np.int32), (svals, np.int32),
                  (p.eMatDH_special_matrix_helper, np.int32), (p.eMatDH_special_matrix, np.int32), (p.transMatRate_t, np.float64),
                  (c.which, np.int32), (s.read_ptr, np.int32), (s.u, np.int32), (s.bq, np.int32), (s.wif, np.int32),
                  (grid_has_read_of(s, c.G), np.uint8), (c.runif_reads, np.float64), (c.runif_block, np.float64),
                  (c.runif_resample, np.float64), (p.L_grid if kw.get("L_grid") is None else kw["L_grid"], np.int32), (c.H0, np.int32),
                  (cc.BLOCK_ITS, np.int32)):
        assert a is None or np.asarray(a).dtype == dt or dt == np.int32 and np.asarray(a).dtype.kind == "i", (dt, np.asarray(a).dtype)
        _record(f, a, None if a is None or np.asarray(a).dtype == dt else dt)


def test_block_tables_agree_and_are_clean_under_the_sanitizers(tmp_path):
    """qo_define_blocked_grids / qo_make_gibbs_considers (oracle/gibbs.c) and qa::define_blocked_grids / qa::make_gibbs_considers
    (csrc/gibbs_blocks.hpp) on the rates and reads of every block-table case, of the one-read and one-grid cases, and of R in
    (0, 1, 2) x G in (1, 2, 3): equal tables, every read range inside the chain or empty; then the oracle's whole sampler on the
    one-read and one-grid NIPT inputs.  Built with -fsanitize=address,undefined; a clean exit, no report."""
    objs = []
    for src in ("gibbs.c", "fullpass.c"):
        o = tmp_path / (src + ".o")
        b = subprocess.run(["gcc", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g1", "-O0",
                            "-std=c11", "-D_GNU_SOURCE", "-c", os.path.join(ROOT, "oracle", src), "-o", str(o)], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        objs.append(str(o))
    exe = tmp_path / "gibbs_blocks_san"
    b = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g1", "-O0",
                        "-std=c++17", "-I", ROOT, os.path.join(ROOT, "tests", "c", "gibbs_blocks_san.cpp"), *objs, "-lm", "-o", str(exe)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    tables = BY_FAMILY("blocks") + [cc.case(n) for n in DIED]
    calls = [cc.case(n) for n in DIED]
    expect = []
    with open(tmp_path / "input.bin", "wb") as f:
        _record(f, [len(tables), len(calls)], np.int32)
        for c in tables:
            t = cc.first_pass_table(c)
            kw = c.kwargs()
            _record(f, [c.G, c.R, kw.get("shuffle_bin_radius", 5000)], np.int32)
            _record(f, [kw.get("block_gibbs_quantile_prob", 0.95)], np.float64)
            _record(f, t["rate2"], np.float64)
            _record(f, c.panel.L_grid if kw.get("L_grid") is None else kw["L_grid"], np.int32)
            _record(f, c.sample.wif, np.int32)
            expect.append(" ".join(f"[{a}-{b}|{r0}-{r1}]" for a, b, r0, r1 in zip(
                t["consider_grid_start_0_based"], t["consider_grid_end_0_based"], t["consider_reads_start_0_based"], t["consider_reads_end_0_based"])))
        for c in calls:
            _write_call(f, c)
    run = subprocess.run([str(exe), str(tmp_path / "input.bin")], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1"))
    for mark in ("AddressSanitizer", "runtime error:"):
        assert mark not in run.stderr, run.stderr[-6000:]
    assert run.returncode == 0, (run.returncode, run.stdout[-3000:], run.stderr[-3000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "gibbs blocks: ok" and "DIFFERENT" not in run.stdout
    for i, want in enumerate(expect):   # the program saw the tables this file's other tests are about
        assert lines[i].startswith(f"table {i}: ") and lines[i].endswith(want), (lines[i], want)
    for i, c in enumerate(calls):       # ... and its sampler returns what the oracle library returns
        H = cc.oracle_ref(c)["H"]
        assert f"call {i}: G={c.G} R={c.R} status=0 H={''.join(str(h) for h in H[:8])}" in lines
