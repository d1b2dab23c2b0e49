"""Test infrastructure for the linked-read (BX tag) range tests: tagged BAM files of a synthetic panel, and the range call with the
tag over the CPU oracle's entry points (the private test hook, csrc/impute_testhook.h).  Nothing in the product imports this."""
import ctypes as C

import numpy as np

from tests import bamaux, bamutil


def tagged_alignments(sample, panel, ref, alt, rng, n_barcodes=6, frac=0.4):
    """bamutil.sample_to_alignments(sample) with BX:Z tags, and a bxTagUpperLimit to load them with, such that
      * the barcode CHAIN joins one alignment from each of three consecutive grids (every gap at most the limit),
      * the barcode SPLIT sits on the first and the last alignment of the file, further apart than the limit,
      * `frac` of the other alignments carry one of `n_barcodes` random barcodes (some join, some are split),
    with other auxiliary fields in front of some of the tags."""
    L = np.asarray(panel.L)
    grid = np.asarray(panel.grid if panel.grid is not None else np.arange(panel.nSNPs) // 32)
    alns = bamutil.sample_to_alignments(sample, L, ref, alt, rng)
    end = lambda a: a["pos"] + len(a["seq"]) - 1
    g_of = [int(grid[min(int(np.searchsorted(L, a["pos"])), len(L) - 1)]) for a in alns]
    g0 = max(g_of) // 2
    chain = [g_of.index(g) for g in (g0, g0 + 1, g0 + 2)]   # (alns is sorted by position: ascending indices)
    assert chain == sorted(chain) and chain[0] > 0 and chain[-1] < len(alns) - 1
    limit, far = 1, end(alns[chain[0]])
    for i in chain[1:]:
        limit = max(limit, alns[i]["pos"] - far)
        far = max(far, end(alns[i]))
    assert alns[-1]["pos"] - end(alns[0]) > limit, "the panel is too short for a split at this limit"
    for i, a in enumerate(alns):
        tag = "CHAIN" if i in chain else "SPLIT" if i in (0, len(alns) - 1) else \
            ("BC%02d" % rng.integers(0, n_barcodes)) if rng.random() < frac else None
        a["aux"] = [("NM", "C", 1), ("XB", "B", ("s", [1, -2, 3]))] if i % 3 == 0 else []
        if tag is not None:
            a["aux"].append(("BX", "Z", tag))
    return alns, int(limit)


def write_tagged_files(tmp_path, panel, n_files=3, n_reads=300, seed=21, untagged=False):
    """-> (bam paths with an empty file second, ref, alt, the limit that suits them all)"""
    from quilt_amd.synth import make_synthetic_sample
    rng = np.random.default_rng(seed)
    alleles = [tuple(rng.choice(list("ACGT"), size=2, replace=False)) for _ in range(panel.nSNPs)]
    ref, alt = [a for a, _ in alleles], [b for _, b in alleles]
    refs = [("chr20", int(panel.L[-1]) + 1000)]
    made = []
    for i in range(n_files):
        s = make_synthetic_sample(panel, seed=300 + i, n_reads=n_reads)
        made.append(tagged_alignments(s, panel, ref, alt, rng))
    limit = max(l for _, l in made)
    paths = []
    for i, (alns, _) in enumerate(made):
        if untagged:
            for a in alns:
                a["aux"] = [f for f in a["aux"] if f[0] != "BX"]
        assert untagged or alns[-1]["pos"] - (alns[0]["pos"] + len(alns[0]["seq"]) - 1) > limit
        paths.append(str(tmp_path / f"bx{i}.bam"))
        bamaux.write_bam(paths[-1], refs, alns)
    paths.insert(1, str(tmp_path / "bx_empty.bam"))
    bamaux.write_bam(paths[1], refs, [])
    return paths, ref, alt, limit


def impute_bam_range_bx_on_oracle(panel, bam_files, chr, ref, alt, params, n_threads=1, **kw):
    """qa_impute_bam_range_backend_bx over the oracle table: tests/native_driver_backend.impute_bam_range_on_oracle with the loader's
    pair of tag arguments."""
    from quilt_amd.native import ptr
    from tests.native_driver_backend import OracleTable, bam_range_on_table

    def call(fn, tab, handles, n_threads, q, io, n, paths, sidx, ffv, h, use_bx_tag=0, bxTagUpperLimit=0):
        return fn(C.byref(tab.table), handles, n_threads, panel.K, panel.nGrids, C.byref(q), C.byref(io), use_bx_tag, bxTagUpperLimit, n,
                  paths, ptr(sidx), ptr(ffv), C.byref(h))
    return bam_range_on_table(OracleTable(panel), "qa_impute_bam_range_backend_bx", call, bam_files, chr, ref, alt, params, n_threads, **kw)


def assert_same_range(got, rec, kept):
    """the range call's result against impute_bams_to_vcf's record: column text, read labels, posteriors, the four count arrays"""
    for i in kept:
        assert got["columns"][i].tolist() == rec["columns"][i].tolist(), i
        assert np.array_equal(got["results"][i].read_labels, rec["results"][i].read_labels), i
        if got["results"][i].gp_t is not None:
            assert np.array_equal(got["results"][i].gp_t, rec["results"][i].gp_t), i
    for name in ("infoCount", "afCount", "hweCount", "alleleCount"):
        assert np.array_equal(getattr(got["counts"], name), getattr(rec["counts"], name)), name
