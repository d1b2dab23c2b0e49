"""output_read_label_prob (per read: name, confidence of its label, final label) and hla_run from BAM paths, without a device:
the loader's names against a plain-Python statement of the rule of include/quilt_amd_io.h; the one confidence helper against a
literal restatement of the reference's R; the native loop over the CPU oracle against quilt_amd/driver.py over the same oracle;
the range call's extensible entry (test hook: qa_impute_bam_range_backend_ex); the loader with names as a stand-alone program
under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Seeds of the loop-against-loop tests, found on the CPU oracle for the two conditions _check_loop asserts.  Nearly every seed gives
# confidences on both sides of 0.95; few make a sample's consensus labels differ from its last Gibbs sample's, and none can with
# two Gibbs samples (determine_best_read_label_so_far flips the canonical sample only when MORE than half of the samples moved), so these
# tests run three.
DIPLOID_SAMPLE_SEED, DIPLOID_SEED = 300, 11
NIPT_SAMPLE_SEED, NIPT_SEED = 900, 14
RARE_SAMPLE_SEED, RARE_SEED = 50, 1


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the loader's names
# ---------------------------------------------------------------------------------------------------------------------------
def names_model(alns, use_bx, limit, cap, seed=1, bqFilter=17):
    """The rule for a read's name, in plain Python over the alignments in file order -> (names, reads [(u, bq)], facts).
    A read's name is the query name of the first alignment, in file order, of the fragment that holds the read's slot; mates merge
    by name into the first mate's fragment; a BX molecule lives in the slot of the first of its fragments in file order; names
    follow the reads through the coverage cap and the stable ordering by grid."""
    from tests.test_bx_loader_cpu import GRID, _pileup, _stream_key, _tag
    frags, open_pair = [], {}
    merged = 0
    for a in alns:   # every alignment of the file passes the flag / mapping-quality / insert-size filters and carries a site
        calls, lo, hi = _pileup(a, bqFilter)
        assert calls
        if a["flag"] & 1:
            if a["name"] in open_pair:
                f = frags[open_pair.pop(a["name"])]
                f["alns"].append(calls)
                f["lo"], f["hi"] = min(f["lo"], lo), max(f["hi"], hi)
                merged += 1
                continue
            open_pair[a["name"]] = len(frags)
        frags.append(dict(name=a["name"], alns=[calls], lo=lo, hi=hi, tag=_tag(a) if use_bx else None))
    molecules, open_of, splits = [], {}, 0
    for i in sorted(range(len(frags)), key=lambda i: (frags[i]["lo"], i)):
        f = frags[i]
        m = open_of.get(f["tag"]) if f["tag"] is not None else None
        if m is not None and f["lo"] - m["end"] <= limit:
            m["frags"].append(i)
            m["end"] = max(m["end"], f["hi"])
            continue
        splits += m is not None
        m = dict(frags=[i], end=f["hi"])
        if f["tag"] is not None:
            open_of[f["tag"]] = m
        molecules.append(m["frags"])
    slots = {}
    for m in molecules:
        by_site = {}
        for i in sorted(m):
            for calls in frags[i]["alns"]:
                for t, q in calls:
                    by_site.setdefault(t, []).append(q)
        read = [(t, max(qs, key=abs)) for t, qs in sorted(by_site.items()) if len({q < 0 for q in qs}) == 1]
        if read:
            slots[min(m)] = read   # the slot -- and so the name -- of the first of its fragments in file order
    removed = 0
    if cap > 0:
        depth = {}
        for r in slots.values():
            for t, _ in r:
                depth[t] = depth.get(t, 0) + 1
        for t in sorted(depth):
            for _, s in sorted((_stream_key(seed, s), s) for s, r in slots.items() if any(tt == t for tt, _ in r)):
                if depth[t] <= cap:
                    break
                for tt, _ in slots.pop(s):
                    depth[tt] -= 1
                removed += 1
    central_grid = lambda s: GRID[slots[s][(len(slots[s]) - 1) // 2][0]]
    order = sorted(sorted(slots), key=central_grid)   # (sorted() is stable)
    facts = dict(merged=merged, removed=removed, splits=splits, largest_molecule=max(len(m) for m in molecules),
                 permuted=order != sorted(slots))
    return [frags[s]["name"] for s in order], [([t for t, _ in slots[s]], [q for _, q in slots[s]]) for s in order], facts


def _write_names_file(tmp_path):
    from tests import bamaux
    from tests.rlp_files import names_file_alignments
    from tests.test_bx_loader_cpu import REFS
    alns = names_file_alignments()
    path = str(tmp_path / "names.bam")
    bamaux.write_bam(path, REFS, alns, sorted_header=False)
    return path, alns


def test_loader_names_follow_the_rule(tmp_path):
    from quilt_amd.io import loadBamAndConvert
    from tests.rlp_files import NAMES_CAP, NAMES_LIMIT
    from tests.test_bx_loader_cpu import ALT, GRID, L, REF
    path, alns = _write_names_file(tmp_path)
    for use_bx, cap in ((True, NAMES_CAP), (True, 0), (False, NAMES_CAP), (False, 0)):
        kw = dict(use_bx_tag=use_bx, bxTagUpperLimit=NAMES_LIMIT, downsampleToCov=cap)
        s, st, bx, names = loadBamAndConvert(path, "1", L, REF, ALT, GRID, return_stats=True, return_bx_stats=True, return_names=True, **kw)
        want_names, want_reads, facts = names_model(alns, use_bx, NAMES_LIMIT, cap)
        reads = [(s.u[a:b].tolist(), s.bq[a:b].tolist()) for a, b in zip(s.read_ptr[:-1], s.read_ptr[1:])]
        assert reads == want_reads and names == want_names, (use_bx, cap, names, want_names)
        assert len(names) == s.nReads
        # the file holds what it was made to hold -- by the loader's own counters and by the model's
        assert st["mates_merged"] == facts["merged"] == 1 and facts["permuted"]
        assert st["removed_by_coverage_cap"] == facts["removed"] and (facts["removed"] == 3 if cap else facts["removed"] == 0)
        if use_bx:
            assert facts["largest_molecule"] == 3 and bx["fragments_absorbed"] == 2 and bx["molecules_of_several_fragments"] == 1
            assert bx["split_by_limit"] == facts["splits"] == 1
            assert "mol_c" in names and "mol_a" not in names and "mol_b" not in names   # the slot of the fragment written first
            assert "spl_far" in names and "spl_near" in names
        else:
            assert {"mol_a", "mol_b", "mol_c"} <= set(names)
        assert names.count("pair") == 1
        # byte-identical read arrays with and without the request; no names without it
        plain, st2 = loadBamAndConvert(path, "1", L, REF, ALT, GRID, return_stats=True, **kw)
        for name in ("read_ptr", "u", "bq", "wif"):
            assert getattr(plain, name).tobytes() == getattr(s, name).tobytes(), name
        assert st2 == st


def test_loader_with_names_is_clean_under_the_sanitizers(tmp_path):
    """csrc/hostio.cpp alone behind tests/c/read_names_san.cpp, built here with g++ -fsanitize=address,undefined: the file above
    loaded with names requested, the names exported into exactly-sized buffers.  A clean exit, no report, the names of the rule."""
    from tests.rlp_files import NAMES_CAP, NAMES_LIMIT
    from tests.test_bx_loader_cpu import ALT, GRID, L, REF
    exe = tmp_path / "read_names_san"
    build = subprocess.run(["g++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g1", "-O0",
                            "-std=c++17", os.path.join(ROOT, "quilt_amd", "csrc", "hostio.cpp"), os.path.join(ROOT, "tests", "c", "read_names_san.cpp"),
                            os.path.join(ROOT, "tests", "c", "bx_loader_stubs.cpp"), "-lz", "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    path, alns = _write_names_file(tmp_path)
    with open(tmp_path / "sites.bin", "wb") as f:
        f.write(np.int32(len(L)).tobytes() + L.tobytes() + "".join(REF).encode() + "".join(ALT).encode() + GRID.tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "sites.bin"), path, str(NAMES_LIMIT), str(NAMES_CAP)], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:exitcode=67", UBSAN_OPTIONS="print_stacktrace=1"))
    for mark in ("AddressSanitizer", "runtime error:"):
        assert mark not in run.stderr, run.stderr[-6000:]
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    lines = run.stdout.split("\n")
    assert lines[-2] == "read names: ok"
    assert lines[:-2] == names_model(alns, True, NAMES_LIMIT, NAMES_CAP)[0]


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the helper against the reference's R
# ---------------------------------------------------------------------------------------------------------------------------
def r_mp(p, method):
    """functions.R:1635-1658, line by line (R's is.na() is true for NaN; a comparison with NaN selects nothing)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        if method == "diploid":
            p1 = p[0, :]
            p2 = p[1, :]
            mp = p1 / (p1 + p2)
            mp[np.isnan(mp)] = 0.5
            mp[mp < 0.5] = 1 - mp[mp < 0.5]
        else:
            d = p[0, :] + p[1, :] + p[2, :]   # colSums(p)
            p1 = p[0, :] / d
            p2 = p[1, :] / d
            p3 = p[2, :] / d
            mp = p1.copy()
            mp[p2 > p1] = p2[p2 > p1]
            mp[p3 > mp] = p3[p3 > mp]
            mp[np.isnan(mp)] = 1 / 3
    return mp


def test_confidence_helper_equals_the_reference_expression():
    from quilt_amd.driver import assess_ability_of_reads_to_be_confident, read_label_confidence as twin
    from quilt_amd.io import consensus_read_labels, read_label_confidence
    rng = np.random.default_rng(3)
    # direct inputs first: both likelihoods 0; a ratio below 0.5; exactly 0.5; 0.95 either side; one likelihood 0; tiny values
    p2 = np.array([[0.0, 0.2, 0.5, 0.95, 0.9500001, 0.0, 3.0, 1e-300, 4e-320],
                   [0.0, 0.8, 0.5, 0.05, 0.0499999, 1e-200, 0.0, 3e-300, 1e-320]])
    p2 = np.concatenate([p2, 10.0 ** rng.uniform(-300, 0, size=(2, 500))], axis=1)
    got = read_label_confidence(p2)
    assert np.array_equal(got, r_mp(p2.copy(), "diploid")) and np.array_equal(got, twin(p2))
    assert got[0] == 0.5 and got[1] == 0.8 and got[2] == 0.5 and got[5] == 1.0 and got[6] == 1.0
    # NIPT: all three 0; a three-way tie; a two-way tie on top; the third largest; one 0
    p3 = np.array([[0.0, 0.25, 0.4, 0.1, 0.0, 1e-310],
                   [0.0, 0.25, 0.4, 0.2, 0.5, 1e-310],
                   [0.0, 0.25, 0.2, 0.7, 0.5, 1e-310]])
    p3 = np.concatenate([p3, 10.0 ** rng.uniform(-300, 0, size=(3, 500))], axis=1)
    got3 = read_label_confidence(p3)
    assert np.array_equal(got3, r_mp(p3.copy(), "nipt")) and np.array_equal(got3, twin(p3))
    assert got3[0] == 1 / 3 and got3[1] == 1 / 3 and got3[2] == 0.4 and got3[3] == 0.7 and got3[4] == 0.5 and got3[5] == 1 / 3
    # and qa_consensus_read_labels thresholds this very value: with one Gibbs sample its confidence filter is mp > minrp
    for p in (p2, p3):
        assert np.array_equal(assess_ability_of_reads_to_be_confident(p), read_label_confidence(p) > 0.95)
        lab = rng.integers(1, 3, size=(1, p.shape[1])).astype(np.int32)
        assert np.array_equal(consensus_read_labels(lab, p[None], can_hap=1), lab[0])
    with pytest.raises(ValueError):
        read_label_confidence(np.zeros((4, 3)))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. loop against loop
# ---------------------------------------------------------------------------------------------------------------------------
def _python_loop(panel, samples, P, sample_offset, monkeypatch, rare_common=None):
    """quilt_amd/driver.py over the oracle -> (results, per sample: (last chain's labels, consensus labels))"""
    import quilt_amd.io as qio
    from quilt_amd.driver import Driver
    from tests.oracle_backend import OracleBackend
    seen = []
    real = qio.consensus_read_labels

    def recording(labels, p, can_hap, minrp=0.95):
        out = real(labels, p, can_hap, minrp)
        seen.append((np.asarray(labels)[can_hap - 1].copy(), out.copy()))
        return out

    monkeypatch.setattr(qio, "consensus_read_labels", recording)
    kw = {} if rare_common is None else dict(rare_common=rare_common)
    want = Driver(panel, OracleBackend(panel, rare_common), P, **kw).run(samples, sample_offset=sample_offset)
    monkeypatch.setattr(qio, "consensus_read_labels", real)
    assert len(seen) == len(samples)
    return want, seen


def _same_but_prob(a, b):
    assert a.nDosage == b.nDosage
    for f in ("read_labels", "dosage", "gp_t", "phasing_haps", "fet_dosage", "fet_gp_t"):
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None) == (y is None) and (x is None or np.asarray(x).tobytes() == np.asarray(y).tobytes()), f


def _check_loop(panel, samples, P, sample_offset, monkeypatch, lo, rare_common=None, **kw):
    from tests.native_driver_backend import impute_samples_on_oracle
    from tests.rlp_files import impute_samples_reads_on_oracle
    want, seen = _python_loop(panel, samples, P, sample_offset, monkeypatch, rare_common)
    got = impute_samples_reads_on_oracle(panel, samples, P, sample_offset=sample_offset, rare_common=rare_common, **kw)
    plain, _, _ = impute_samples_on_oracle(panel, samples, P, sample_offset=sample_offset, rare_common=rare_common, **kw)
    off = impute_samples_reads_on_oracle(panel, samples, P, sample_offset=sample_offset, rare_common=rare_common, output_read_label_prob=False, **kw)
    for a, b, c, d, s in zip(got, want, plain, off, samples):
        assert a.read_label_prob.shape == (s.nReads,) and np.array_equal(a.read_label_prob, b.read_label_prob)
        _same_but_prob(a, b)
        _same_but_prob(a, c)   # asking for the output changes no other output bit
        _same_but_prob(d, c)
        assert c.read_label_prob is None and d.read_label_prob is None
        mp = a.read_label_prob
        # the seeds were chosen so that the comparison means something: confidences on both sides of 0.95, and some that are
        # neither of the expression's fixed points
        assert (mp > 0.95).any() and (mp < 0.95).any() and ((mp > lo) & (mp < 1)).any() and mp.min() >= lo and mp.max() <= 1
    # ... and so that the labels returned with the confidences are not simply the last Gibbs sample's
    assert any(not np.array_equal(last, cons) for last, cons in seen)
    for (_, cons), a in zip(seen, got):
        assert np.array_equal(cons, a.read_labels)


def test_read_label_prob_native_loop_equals_python_loop_diploid(monkeypatch):
    from quilt_amd.driver import DriverParams
    from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
    panel = make_synthetic_panel(K=400, nSNPs=3200, seed=77, ref_error=1e-3)
    samples = [make_synthetic_sample(panel, seed=DIPLOID_SAMPLE_SEED + i, n_reads=260) for i in range(3)]
    P = DriverParams(nGibbsSamples=3, n_seek_its=3, Ksubset=64, Knew=24, small_ref_panel_gibbs_iterations=6,
                     small_ref_panel_block_gibbs_iterations=(1, 3), seed=DIPLOID_SEED)
    _check_loop(panel, samples, P, 5, monkeypatch, 0.5, samples_per_launch_set=2, n_threads=2)


def test_read_label_prob_native_loop_equals_python_loop_nipt(monkeypatch):
    from quilt_amd.driver import DriverParams
    from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
    panel = make_synthetic_panel(K=400, nSNPs=3200, seed=77, ref_error=1e-3)
    samples = [make_synthetic_sample(panel, seed=NIPT_SAMPLE_SEED + i, n_reads=220, ff=0.1 + 0.05 * i) for i in range(3)]
    P = DriverParams(nGibbsSamples=3, n_seek_its=2, Ksubset=64, Knew=64, seed=NIPT_SEED, method="nipt", small_ref_panel_gibbs_iterations=5,
                     small_ref_panel_block_gibbs_iterations=(2,))
    _check_loop(panel, samples, P, 2, monkeypatch, 1 / 3, samples_per_launch_set=2, n_threads=2)


def test_read_label_prob_native_loop_equals_python_loop_rare_common(monkeypatch):
    from quilt_amd.driver import DriverParams
    from quilt_amd.synth import make_rare_common, make_synthetic_panel, make_synthetic_sample_rare_common
    panel = make_synthetic_panel(K=300, nSNPs=640, seed=5)
    rc = make_rare_common(panel, 3)
    samples = [make_synthetic_sample_rare_common(panel, rc, RARE_SAMPLE_SEED + i, n_reads=150)[0] for i in range(4)]
    P = DriverParams(nGibbsSamples=3, Ksubset=64, Knew=64, seed=RARE_SEED, impute_rare_common=True, small_ref_panel_gibbs_iterations=5,
                     small_ref_panel_block_gibbs_iterations=(2,))
    _check_loop(panel, samples, P, 3, monkeypatch, 0.5, rare_common=rc, samples_per_launch_set=2, n_threads=2)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the range call's extensible entry over the oracle
# ---------------------------------------------------------------------------------------------------------------------------
CHR, INDEX, KEPT = "chr20", [0, 99, 1, 2], (0, 2, 3)


@pytest.fixture(scope="module")
def bx_range(tmp_path_factory, small_panel):
    """four files (the second without reads), and the call without extras on them"""
    from quilt_amd.driver import DriverParams
    from tests.bx_files import impute_bam_range_bx_on_oracle, write_tagged_files
    paths, ref, alt, limit = write_tagged_files(tmp_path_factory.mktemp("rlp"), small_panel)
    prm = DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64, seed=9)
    kw = dict(sample_index=INDEX, n_io_threads=3, samples_per_launch_set=2, use_bx_tag=True, bxTagUpperLimit=limit)
    base = impute_bam_range_bx_on_oracle(small_panel, paths, CHR, ref, alt, prm, **kw)   # qa_impute_bam_range_backend_bx
    return dict(paths=paths, ref=ref, alt=alt, limit=limit, prm=prm, kw=kw, base=base)


def _same_text_and_counts(got, base):
    from tests.bx_files import assert_same_range
    assert got["imputed"] == base["imputed"] == [True, False, True, True] and got["n_reads"] == base["n_reads"]
    assert got["load_stats"] == base["load_stats"] and got["bx_stats"] == base["bx_stats"]
    assert_same_range(got, base, KEPT)
    for i in KEPT:
        assert got["results"][i].nDosage == base["results"][i].nDosage
        for f in ("dosage", "phasing_haps"):
            assert np.array_equal(getattr(got["results"][i], f), getattr(base["results"][i], f)), f
    assert got["columns"][1] is None and 1 not in got["results"]


def test_backend_ex_read_label_prob(small_panel, bx_range):
    from quilt_amd.io import impute_bams_to_vcf, loadBamAndConvert
    from tests.oracle_backend import OracleBackend
    from tests.rlp_files import impute_bam_range_ex_on_oracle
    F, panel = bx_range, small_panel
    got = impute_bam_range_ex_on_oracle(panel, F["paths"], CHR, F["ref"], F["alt"], F["prm"], output_read_label_prob=True, **F["kw"])
    _same_text_and_counts(got, F["base"])
    frlp = got["final_read_labels_prob"]
    assert sorted(frlp) == list(KEPT)   # nothing for the dropped file
    for i in KEPT:
        names, prob, labels = frlp[i]
        n = got["n_reads"][i]
        assert len(names) == len(prob) == len(labels) == n
        s, want_names = loadBamAndConvert(F["paths"][i], CHR, panel.L, F["ref"], F["alt"], panel.grid, use_bx_tag=True,
                                          bxTagUpperLimit=F["limit"], return_names=True)
        assert names == want_names and s.nReads == n
        assert np.array_equal(labels, F["base"]["results"][i].read_labels)
        assert (prob >= 0.5).all() and (prob <= 1).all() and ((prob > 0.5) & (prob < 1)).any()
    # the Python path carries the option too, and says the same
    rec = impute_bams_to_vcf(panel, OracleBackend(panel), F["paths"], [f"NA{i}" for i in range(4)], CHR, F["ref"], F["alt"],
                             os.path.join(os.path.dirname(F["paths"][0]), "py.vcf.gz"), params=F["prm"], use_bx_tag=True,
                             bxTagUpperLimit=F["limit"], output_read_label_prob=True)
    assert sorted(rec["final_read_labels_prob"]) == list(KEPT)
    for i in KEPT:
        for a, b in zip(frlp[i], rec["final_read_labels_prob"][i]):
            assert np.array_equal(np.asarray(a), np.asarray(b))
    # discard_sample_arrays does not discard the new arrays
    lean = impute_bam_range_ex_on_oracle(panel, F["paths"], CHR, F["ref"], F["alt"], F["prm"], output_read_label_prob=True,
                                         discard_sample_arrays=True, **F["kw"])
    for i in KEPT:
        assert lean["results"][i].dosage is None
        for a, b in zip(frlp[i], lean["final_read_labels_prob"][i]):
            assert np.array_equal(np.asarray(a), np.asarray(b))


def test_backend_ex_hla(small_panel, bx_range):
    from quilt_amd.driver import HlaDriverParams
    from quilt_amd.io import loadBamAndConvert
    from tests.hla_backend import impute_samples_hla_on_oracle
    from tests.rlp_files import impute_bam_range_ex_on_oracle
    F, panel = bx_range, small_panel
    grid = panel.nGrids // 2
    got = impute_bam_range_ex_on_oracle(panel, F["paths"], CHR, F["ref"], F["alt"], F["prm"], hla_grid=grid, output_read_label_prob=True,
                                        discard_sample_arrays=True, **F["kw"])
    full = impute_bam_range_ex_on_oracle(panel, F["paths"], CHR, F["ref"], F["alt"], F["prm"], hla_grid=grid, **F["kw"])
    _same_text_and_counts(full, F["base"])
    assert "final_read_labels_prob" not in full
    # qa_impute_samples_backend_hla on the same loaded reads (the kept files' global indices are 0, 1, 2)
    samples = [loadBamAndConvert(F["paths"][i], CHR, panel.L, F["ref"], F["alt"], panel.grid, use_bx_tag=True, bxTagUpperLimit=F["limit"])
               for i in KEPT]
    P = HlaDriverParams(**F["prm"].__dict__, hla_grid=grid)
    want, _, _ = impute_samples_hla_on_oracle(panel, samples, P, grid, sample_offset=0, samples_per_launch_set=2)
    for i, w in zip(KEPT, want):
        for r in (got["results"][i], full["results"][i]):
            assert r.gamma1.shape == (panel.K,) and r.list_of_gammas.shape == (P.nGibbsSamples, 2, panel.K)
            for f in ("gamma1", "gamma2", "gamma_total", "list_of_gammas"):
                assert np.asarray(getattr(r, f)).tobytes() == np.ascontiguousarray(getattr(w, f)).tobytes(), (i, f)
        assert np.array_equal(full["results"][i].read_labels, w.read_labels)
    for r in F["base"]["results"].values():
        assert r.gamma1 is None and r.read_label_prob is None


def test_backend_ex_refuses_before_a_file_is_opened(tmp_path, small_panel, bx_range):
    """hla_grid with what qa_impute_samples_hla refuses: the refusal arrives, not the error of the file that does not exist."""
    from quilt_amd.driver import DriverParams
    from quilt_amd.synth import make_rare_common
    from tests.rlp_files import impute_bam_range_ex_on_oracle
    F, panel = bx_range, small_panel
    missing = [str(tmp_path / "does_not_exist.bam")]
    base = dict(nGibbsSamples=2, Ksubset=64, Knew=64, seed=9)
    run = lambda prm, **kw: impute_bam_range_ex_on_oracle(panel, missing, CHR, F["ref"], F["alt"], prm, **kw)
    with pytest.raises(RuntimeError, match="does_not_exist.bam"):   # (the path is reached when nothing is refused)
        run(DriverParams(**base), hla_grid=1)
    with pytest.raises(RuntimeError, match="status -2.*use_mspbwt"):
        run(DriverParams(**base, use_mspbwt=True, mspbwt_nindices=2), hla_grid=1)
    with pytest.raises(RuntimeError, match="status -2.*nipt"):
        run(DriverParams(**base, method="nipt"), hla_grid=1, ff=[0.2])
    rc = make_rare_common(panel, 3)
    rng = np.random.default_rng(1)
    ref_all, alt_all = list(rng.choice(list("AC"), rc.nSNPs_all)), list(rng.choice(list("GT"), rc.nSNPs_all))
    with pytest.raises(RuntimeError, match="status -2.*impute_rare_common"):
        run(DriverParams(**base, impute_rare_common=True), hla_grid=1, rare_common=rc,
            all_sites=(rc.L_all, ref_all, alt_all, (np.arange(rc.nSNPs_all) // 32).astype(np.int32)))
    for g in (panel.nGrids, panel.nGrids + 7):
        with pytest.raises(RuntimeError, match="status -2.*grid outside"):
            run(DriverParams(**base), hla_grid=g)
    with pytest.raises(RuntimeError, match="status -2.*not a dosage pass"):
        run(DriverParams(**base, n_seek_its=2, n_burn_in_seek_its=2), hla_grid=1)
    with pytest.raises(RuntimeError, match="status -2.*bxTagUpperLimit"):
        run(DriverParams(**base), output_read_label_prob=True, use_bx_tag=True, bxTagUpperLimit=-1)


def test_new_symbols_and_struct_mirrors():
    import ctypes as C
    from quilt_amd import native
    from quilt_amd.impute import BamRangeExtras, ImputeReadsOut
    L = native.lib()
    for name in ("qa_bam_load_sample_reads_named", "qa_sample_reads_names_bytes", "qa_sample_reads_export_names", "qa_read_label_confidence",
                 "qa_impute_samples_reads", "qa_impute_samples_backend_reads", "qa_impute_bam_range_ex", "qa_impute_bam_range_backend_ex",
                 "qa_bam_range_read_label_prob", "qa_bam_range_hla"):
        assert hasattr(L, name), name
    from tests.test_struct_layout_cpu import _header_text, _members
    text = _header_text()
    assert [f[0] for f in ImputeReadsOut._fields_] == _members("qa_impute_reads_out_t", text)
    assert C.sizeof(BamRangeExtras) == 16 and [f[0] for f in BamRangeExtras._fields_] == ["use_bx_tag", "bxTagUpperLimit",
                                                                                        "output_read_label_prob", "hla_grid"]
