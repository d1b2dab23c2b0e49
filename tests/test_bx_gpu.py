"""Linked reads (BX tag) through the range call ON THE DEVICE: a molecule is a longer, sparser read of the kind the samplers and
k_ematread already take -- no kernel is new; these tests show that this holds on the device.  Panel of 20 grids, three files of a
few hundred alignments (per file one barcode joins alignments of three consecutive grids, one is split by the limit, some random
ones do either) plus one file without reads."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHR = "chr20"
INDEX = [0, 99, 1, 2]   # (impute_bams_to_vcf numbers the samples it keeps 0, 1, 2: the kept files' global indices)
KEPT = (0, 2, 3)


@pytest.fixture(scope="module")
def panel():
    from quilt_amd.synth import make_synthetic_panel
    return make_synthetic_panel(K=1000, nSNPs=640, seed=4916)


@pytest.fixture(scope="module")
def files(tmp_path_factory, panel):
    from tests.bx_files import write_tagged_files
    paths, ref, alt, limit = write_tagged_files(tmp_path_factory.mktemp("bx"), panel, n_reads=300)
    return dict(paths=paths, ref=ref, alt=alt, limit=limit, names=[f"NA{i}" for i in range(4)])


def _prm(method):
    from quilt_amd.driver import DriverParams
    return DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64, seed=9, method=method)


@pytest.fixture(scope="module")
def python_path(tmp_path_factory, panel, files):
    """impute_bams_to_vcf(..., use_bx_tag=True) per method: on the device, and on the CPU oracle (computed once, shared)"""
    from quilt_amd.driver import HipBackend
    from quilt_amd.io import impute_bams_to_vcf
    from quilt_amd.native import DevicePanel
    from tests.oracle_backend import OracleBackend
    tmp = tmp_path_factory.mktemp("bx_vcf")
    out = {}
    for method in ("diploid", "nipt"):
        ff = [0.2] * 4 if method == "nipt" else None
        kw = dict(params=_prm(method), ff=ff, use_bx_tag=True, bxTagUpperLimit=files["limit"])
        dev = DevicePanel(panel)
        dev.set_dosage_precision(64)
        out[method, "gpu"] = impute_bams_to_vcf(panel, HipBackend(dev), files["paths"], files["names"], CHR, files["ref"], files["alt"],
                                                str(tmp / f"{method}_gpu.vcf.gz"), **kw)
        dev.close()
        out[method, "cpu"] = impute_bams_to_vcf(panel, OracleBackend(panel), files["paths"], files["names"], CHR, files["ref"], files["alt"],
                                                str(tmp / f"{method}_cpu.vcf.gz"), **kw)
    return out


def _files_do_what_they_were_made_for(panel, files, bx_stats):
    from quilt_amd.io import loadBamAndConvert
    tot = np.zeros(4, dtype=np.int64)
    for p in files["paths"]:
        s, bx = loadBamAndConvert(p, CHR, panel.L, files["ref"], files["alt"], panel.grid, use_bx_tag=True, bxTagUpperLimit=files["limit"],
                                  return_bx_stats=True)
        tot += np.array(list(bx.values()))
        if s.nReads:   # a molecule of three or more alignments over three or more grids, a tag split by the limit
            grid = panel.grid if panel.grid is not None else np.arange(panel.nSNPs) // 32
            assert max(len(set(np.asarray(grid)[s.u[a:b]].tolist())) for a, b in zip(s.read_ptr[:-1], s.read_ptr[1:])) >= 3
            assert bx["fragments_absorbed"] >= 2 and bx["split_by_limit"] >= 1
    assert list(bx_stats) == tot.tolist()


@pytest.mark.parametrize("method", ["diploid", "nipt"])
def test_bx_range_call_on_the_device(panel, files, python_path, method):
    """Production mode: qa_impute_bam_range_bx on the device == impute_bams_to_vcf(..., use_bx_tag=True) on the same device in text,
    read labels and counts, bit for bit.  Validation mode (sum_order = 1): the text of the Python path over the CPU oracle."""
    from quilt_amd.impute import impute_bam_range
    from quilt_amd.native import DevicePanel
    from tests.bx_files import assert_same_range
    ff = [0.2] * 4 if method == "nipt" else None
    kw = dict(sample_index=INDEX, ff=ff, n_io_threads=3, samples_per_launch_set=2, use_bx_tag=True, bxTagUpperLimit=files["limit"])
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    got = impute_bam_range([dev], files["paths"], CHR, files["ref"], files["alt"], _prm(method), **kw)
    dev.set_sum_order(1)
    val = impute_bam_range([dev], files["paths"], CHR, files["ref"], files["alt"], _prm(method), **kw)
    dev.close()
    assert got["imputed"] == [True, False, True, True] and got["columns"][1] is None
    assert_same_range(got, python_path[method, "gpu"], KEPT)
    _files_do_what_they_were_made_for(panel, files, got["bx_stats"])
    cpu = python_path[method, "cpu"]
    for i in KEPT:
        assert val["columns"][i].tolist() == cpu["columns"][i].tolist(), i
        assert np.array_equal(val["results"][i].read_labels, cpu["results"][i].read_labels)


def test_bx_through_the_shim(panel, files, python_path):
    """`.Call("qa_impute_bam_range", ...)` under tests/c/mini_r.c with sites$use_bx_tag = TRUE: the columns of the Python path on the
    device and a bx_stats equal to the C call's; without the two entries, what the call returns without the tag; a negative limit
    is an R error."""
    from quilt_amd.impute import impute_bam_range
    from quilt_amd.native import DevicePanel
    from tests.mini_r import R as Runtime, RError
    from tests.test_shim_gpu import _params
    prm = _prm("diploid")
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    common = dict(sample_index=INDEX, n_io_threads=3, samples_per_launch_set=2)
    c_on = impute_bam_range([dev], files["paths"], CHR, files["ref"], files["alt"], prm, use_bx_tag=True, bxTagUpperLimit=files["limit"], **common)
    c_off = impute_bam_range([dev], files["paths"], CHR, files["ref"], files["alt"], prm, **common)
    dev.close()
    R = Runtime()
    try:
        sites = dict(chr=R.string(CHR), L=R.integer(panel.L), ref=R.strings(files["ref"]), alt=R.strings(files["alt"]),
                     grid=R.integer(np.arange(panel.nSNPs) // 32), minimum_number_of_sample_reads=R.integer([2]),
                     output_gt_phased_genotypes=R.logical([1]), n_io_threads=R.integer([3]))
        call = lambda s: R.dotcall("qa_impute_bam_range", R.strings(files["paths"]), R.named(s), R.panel_objects(panel), _params(R, prm),
                                   R.real([float(i) for i in INDEX]), R.integer([1]))   # (one handle: what the C calls above use)
        assert R.arity("qa_impute_bam_range") == 6
        on = call(dict(sites, use_bx_tag=R.logical([1]), bxTagUpperLimit=R.real([float(files["limit"])])))
        off = call(sites)
        rec = python_path["diploid", "gpu"]
        for out, want, py in ((on, c_on, rec), (off, c_off, None)):
            assert out["sample_was_imputed"].tolist() == [1, 0, 1, 1] and out["n_reads"].tolist() == want["n_reads"]
            for i in KEPT:
                assert out["per_sample_vcf_col"][i] == want["columns"][i].tolist()
                assert np.array_equal(out["read_labels"][i], want["results"][i].read_labels)
                if py is not None:
                    assert out["per_sample_vcf_col"][i] == py["columns"][i].tolist()
            for name in ("infoCount", "afCount", "hweCount", "alleleCount"):
                assert np.array_equal(out[name], getattr(want["counts"], name)), name
            assert [int(x) for x in out["bx_stats"]] == want["bx_stats"]
        assert c_on["bx_stats"][2] >= 6 and c_off["bx_stats"] == [0, 0, 0, 0]
        assert sum(c_off["n_reads"]) > sum(c_on["n_reads"])
        for bad in (R.real([-1.0]), R.real([0.5]), R.integer([-3])):
            with pytest.raises(RError, match="bxTagUpperLimit"):
                call(dict(sites, use_bx_tag=R.logical([1]), bxTagUpperLimit=bad))
    finally:
        R.dotcall("qa_shim_release")
        R.reset()
