"""The range call with the BX tag (qa_impute_bam_range_bx, csrc/bamrange.cpp) over the CPU oracle's entry points, in the manner of
test_native_driver_cpu.py::test_bam_range_call_equals_the_python_bam_to_vcf_path: three tagged files and one file without reads
against the Python path (loader with the tag -> driver -> column writers -> SummaryCounts) on the same entry points, bit for bit;
and on untagged files the call with the tag on against the call without it."""
import numpy as np
import pytest

from tests.bx_files import assert_same_range, impute_bam_range_bx_on_oracle, write_tagged_files


def _sum_bx(paths, chr, panel, ref, alt, limit):
    from quilt_amd.io import loadBamAndConvert
    tot, spans = np.zeros(4, dtype=np.int64), []
    for p in paths:
        s, bx = loadBamAndConvert(p, chr, panel.L, ref, alt, panel.grid, use_bx_tag=True, bxTagUpperLimit=limit, return_bx_stats=True)
        tot += np.array(list(bx.values()))
        grid = panel.grid if panel.grid is not None else np.arange(panel.nSNPs) // 32
        spans.append(max([len(set(grid[s.u[a:b]].tolist())) for a, b in zip(s.read_ptr[:-1], s.read_ptr[1:])] or [0]))
    return tot.tolist(), spans


def test_bx_range_call_equals_the_python_path(tmp_path, small_panel):
    from quilt_amd.driver import DriverParams
    from quilt_amd.io import impute_bams_to_vcf
    from tests.oracle_backend import OracleBackend
    panel = small_panel
    prm = DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64, seed=9)
    paths, ref, alt, limit = write_tagged_files(tmp_path, panel)
    names = [f"NA{i}" for i in range(4)]
    rec = impute_bams_to_vcf(panel, OracleBackend(panel), paths, names, "chr20", ref, alt, str(tmp_path / "bx.vcf.gz"), params=prm,
                             use_bx_tag=True, bxTagUpperLimit=limit)
    got = impute_bam_range_bx_on_oracle(panel, paths, "chr20", ref, alt, prm, sample_index=[0, 99, 1, 2], n_io_threads=3,
                                        samples_per_launch_set=2, use_bx_tag=True, bxTagUpperLimit=limit)
    assert got["imputed"] == [True, False, True, True] and got["columns"][1] is None
    assert_same_range(got, rec, (0, 2, 3))
    # the files do what they were made for: per file a molecule over three grids and a tag split by the limit; the range's counters
    # are the files' sums
    bx, spans = _sum_bx(paths, "chr20", panel, ref, alt, limit)
    assert got["bx_stats"] == bx and bx[1] >= 3 and bx[2] >= 6 and bx[3] >= 3
    assert all(s >= 3 for s in (spans[0], spans[2], spans[3]))
    # the tag changes the reads: without it the same files give more of them
    off = impute_bam_range_bx_on_oracle(panel, paths, "chr20", ref, alt, prm, sample_index=[0, 99, 1, 2], n_io_threads=3,
                                        samples_per_launch_set=2)
    assert off["bx_stats"] == [0, 0, 0, 0]
    assert sum(off["n_reads"]) > sum(got["n_reads"])
    with pytest.raises(RuntimeError, match="status -2.*bxTagUpperLimit"):
        impute_bam_range_bx_on_oracle(panel, paths, "chr20", ref, alt, prm, use_bx_tag=True, bxTagUpperLimit=-1)


def test_bx_range_call_on_untagged_files_equals_the_call_without_the_tag(tmp_path, small_panel):
    from quilt_amd.driver import DriverParams
    from tests.native_driver_backend import impute_bam_range_on_oracle
    panel = small_panel
    prm = DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64, seed=9)
    paths, ref, alt, limit = write_tagged_files(tmp_path, panel, untagged=True)
    kw = dict(sample_index=[0, 99, 1, 2], n_io_threads=2, samples_per_launch_set=2)
    want = impute_bam_range_on_oracle(panel, paths, "chr20", ref, alt, prm, **kw)       # qa_impute_bam_range_backend
    got = impute_bam_range_bx_on_oracle(panel, paths, "chr20", ref, alt, prm, use_bx_tag=True, bxTagUpperLimit=limit, **kw)
    assert got["imputed"] == want["imputed"] and got["n_reads"] == want["n_reads"] and got["bx_stats"] == [0, 0, 0, 0]
    assert got["load_stats"] == want["load_stats"]
    assert_same_range(got, want, (0, 2, 3))
    for i in (0, 2, 3):
        for name in ("dosage", "phasing_haps"):
            assert np.array_equal(getattr(got["results"][i], name), getattr(want["results"][i], name))
