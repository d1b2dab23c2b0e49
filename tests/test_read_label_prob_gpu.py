"""output_read_label_prob and hla_run through the range call from BAM paths (qa_impute_bam_range_ex) ON THE DEVICE.  No kernel is
new: the confidence comes from k_ematread_dense output the loop already downloads, the gamma columns from
qa_fullpass_reads_select_gamma_batch -- these tests show that this holds on the device.  Panel of 20 grids, the four files of
tests/bx_files.py (one without reads, in the middle), two samples per launch set so that the range spans launch sets."""
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
    paths, ref, alt, limit = write_tagged_files(tmp_path_factory.mktemp("rlp"), panel, n_reads=300)
    return dict(paths=paths, ref=ref, alt=alt, limit=limit, names=[f"NA{i}" for i in range(4)])


def _prm(method="diploid"):
    from quilt_amd.driver import DriverParams
    return DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64, seed=9, method=method)


def _kw(files, method="diploid"):
    return dict(sample_index=INDEX, ff=[0.2] * 4 if method == "nipt" else None, n_io_threads=3, samples_per_launch_set=2, use_bx_tag=True,
                bxTagUpperLimit=files["limit"])


def _device(panel):
    from quilt_amd.native import DevicePanel
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    dev.set_ranking_precision(64)
    return dev


@pytest.fixture(scope="module")
def python_path(tmp_path_factory, panel, files):
    """impute_bams_to_vcf(..., output_read_label_prob=True) per method: on the device, and on the CPU oracle (computed once)"""
    from quilt_amd.driver import HipBackend
    from quilt_amd.io import impute_bams_to_vcf
    from tests.oracle_backend import OracleBackend
    tmp = tmp_path_factory.mktemp("rlp_vcf")
    out = {}
    for method in ("diploid", "nipt"):
        kw = dict(params=_prm(method), ff=[0.2] * 4 if method == "nipt" else None, use_bx_tag=True, bxTagUpperLimit=files["limit"],
                  output_read_label_prob=True)
        dev = _device(panel)
        out[method, "gpu"] = impute_bams_to_vcf(panel, HipBackend(dev), files["paths"], files["names"], CHR, files["ref"], files["alt"],
                                                str(tmp / f"{method}_gpu.vcf.gz"), **kw)
        dev.close()
        out[method, "cpu"] = impute_bams_to_vcf(panel, OracleBackend(panel), files["paths"], files["names"], CHR, files["ref"], files["alt"],
                                                str(tmp / f"{method}_cpu.vcf.gz"), **kw)
    return out


@pytest.fixture(scope="module")
def native(panel, files):
    """the C calls on the device, per method: with the option, without it, and with it in validation mode (computed once)"""
    from quilt_amd.impute import impute_bam_range
    out = {}
    for method in ("diploid", "nipt"):
        dev = _device(panel)
        run = lambda **more: impute_bam_range([dev], files["paths"], CHR, files["ref"], files["alt"], _prm(method), **_kw(files, method), **more)
        out[method, "on"] = run(output_read_label_prob=True)
        out[method, "off"] = run()
        dev.set_sum_order(1)
        out[method, "val"] = run(output_read_label_prob=True)
        dev.close()
    return out


@pytest.mark.parametrize("method", ["diploid", "nipt"])
def test_read_label_prob_on_the_device_equals_the_python_path(panel, files, python_path, native, method):
    """Production mode: names, read_label_prob and labels of qa_impute_bam_range_ex == impute_bams_to_vcf on the same device, bit for
    bit; text, counts and labels == the call without the option, bit for bit."""
    from tests.bx_files import assert_same_range
    got, off, rec = native[method, "on"], native[method, "off"], python_path[method, "gpu"]
    assert got["imputed"] == off["imputed"] == [True, False, True, True] and got["columns"][1] is None
    assert sorted(got["final_read_labels_prob"]) == list(KEPT) and "final_read_labels_prob" not in off
    lo = 1 / 3 if method == "nipt" else 0.5
    for i in KEPT:
        names, prob, labels = got["final_read_labels_prob"][i]
        want_names, want_prob, want_labels = rec["final_read_labels_prob"][i]
        assert names == want_names and len(names) == got["n_reads"][i]
        assert np.array_equal(prob, want_prob) and np.array_equal(labels, want_labels)
        assert prob.min() >= lo and prob.max() <= 1 and (prob > 0.95).any() and (prob < 0.95).any()
        assert off["results"][i].read_label_prob is None
    assert_same_range(got, rec, KEPT)
    assert_same_range(got, off, KEPT)
    assert got["n_reads"] == off["n_reads"] and got["bx_stats"] == off["bx_stats"] and got["load_stats"] == off["load_stats"]
    for i in KEPT:
        for f in ("dosage", "phasing_haps", "fet_dosage", "fet_gp_t"):
            a, b = getattr(got["results"][i], f), getattr(off["results"][i], f)
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b)), f


@pytest.mark.parametrize("method", ["diploid", "nipt"])
def test_read_label_prob_in_validation_mode_against_the_oracle(python_path, native, method):
    """sum_order = 1 against the Python path over the CPU oracle: labels equal; read_label_prob within the fp64 tolerance of DESIGN
    3.4 (1e-9) -- the on-device dense emissions deviate by up to 1 ulp from the oracle's, so equality is not asked."""
    val, cpu = native[method, "val"], python_path[method, "cpu"]
    for i in KEPT:
        names, prob, labels = val["final_read_labels_prob"][i]
        want_names, want_prob, want_labels = cpu["final_read_labels_prob"][i]
        assert names == want_names and np.array_equal(labels, want_labels)
        err = float(np.abs(prob - want_prob).max())
        print(f"{method} file {i}: max |read_label_prob - oracle| = {err:.3e}")
        assert err <= 1e-9


def test_hla_from_bam_paths_on_the_device(panel, files):
    """hla_grid = nGrids // 2 on a handle with fp64 dosage and ranking: gamma1, gamma2, gamma_total and list_of_gammas of the range
    call == impute_samples(..., hla) on the reads loadBamAndConvert returns, bit for bit; nothing else of the call changes."""
    from quilt_amd.driver import HlaDriverParams
    from quilt_amd.impute import impute_bam_range, impute_samples
    from quilt_amd.io import loadBamAndConvert
    from tests.bx_files import assert_same_range
    grid = panel.nGrids // 2
    prm = _prm()
    dev = _device(panel)
    got = impute_bam_range([dev], files["paths"], CHR, files["ref"], files["alt"], prm, hla_grid=grid, **_kw(files))
    off = impute_bam_range([dev], files["paths"], CHR, files["ref"], files["alt"], prm, **_kw(files))
    samples = [loadBamAndConvert(files["paths"][i], CHR, panel.L, files["ref"], files["alt"], panel.grid, use_bx_tag=True,
                                 bxTagUpperLimit=files["limit"]) for i in KEPT]
    want = impute_samples([dev], samples, HlaDriverParams(**prm.__dict__, hla_grid=grid), sample_offset=0, samples_per_launch_set=2)
    dev.close()
    assert got["imputed"] == [True, False, True, True] and 1 not in got["results"]
    for i, w in zip(KEPT, want):
        r = got["results"][i]
        assert r.gamma1.shape == (panel.K,) and r.list_of_gammas.shape == (prm.nGibbsSamples, 2, panel.K)
        for f in ("gamma1", "gamma2", "gamma_total", "list_of_gammas"):
            assert np.array_equal(getattr(r, f), getattr(w, f)), (i, f)
        assert abs(r.gamma1.sum() - 1) < 1e-9 and abs(r.gamma2.sum() - 1) < 1e-9   # a gamma column sums to 1 over the panel
        assert np.array_equal(r.read_labels, w.read_labels) and np.array_equal(r.dosage, w.dosage)
        assert off["results"][i].gamma1 is None
    assert_same_range(got, off, KEPT)


def test_both_options_through_the_shim(panel, files, native):
    """`.Call("qa_impute_bam_range", ...)` under tests/c/mini_r.c with sites$output_read_label_prob and with params$hla_grid: the C
    call's values; without the new entries, what the call returned before; and `.Call("qa_impute_sample_range", ...)` with
    params$output_read_label_prob: the same probabilities for the same reads."""
    from quilt_amd.impute import impute_bam_range
    from quilt_amd.io import loadBamAndConvert
    from tests.mini_r import R as Runtime
    from tests.test_shim_gpu import _params
    prm, grid = _prm(), panel.nGrids // 2
    c_on, c_off = native["diploid", "on"], native["diploid", "off"]
    dev = _device(panel)
    c_hla = impute_bam_range([dev], files["paths"], CHR, files["ref"], files["alt"], prm, hla_grid=grid, **_kw(files))
    dev.close()
    samples = [loadBamAndConvert(files["paths"][i], CHR, panel.L, files["ref"], files["alt"], panel.grid, use_bx_tag=True,
                                 bxTagUpperLimit=files["limit"]) for i in KEPT]
    R = Runtime()
    try:
        sites = dict(chr=R.string(CHR), L=R.integer(panel.L), ref=R.strings(files["ref"]), alt=R.strings(files["alt"]),
                     grid=R.integer(np.arange(panel.nSNPs) // 32), minimum_number_of_sample_reads=R.integer([2]),
                     output_gt_phased_genotypes=R.logical([1]), n_io_threads=R.integer([3]), use_bx_tag=R.logical([1]),
                     bxTagUpperLimit=R.real([float(files["limit"])]))
        call = lambda s, **p: R.dotcall("qa_impute_bam_range", R.strings(files["paths"]), R.named(s), R.panel_objects(panel), _params(R, prm, **p),
                                        R.real([float(i) for i in INDEX]), R.integer([1]))   # (one handle: what the C calls use)
        assert R.arity("qa_impute_bam_range") == 6 and R.arity("qa_impute_sample_range") == 6
        on = call(dict(sites, output_read_label_prob=R.logical([1])))
        off = call(sites)
        both = call(dict(sites, output_read_label_prob=R.logical([1])), hla_grid=R.integer([grid]))
        before = ["sample_was_imputed", "n_reads", "per_sample_vcf_col", "read_labels", "infoCount", "afCount", "hweCount", "alleleCount",
                  "seconds", "stats", "bx_stats"]
        assert list(off) == before and list(on) == before + ["final_read_labels_prob"]
        assert list(both) == before + ["final_read_labels_prob", "gamma1", "gamma2", "gamma_total", "list_of_gammas"]
        for out, want in ((on, c_on), (off, c_off), (both, c_hla)):
            assert out["sample_was_imputed"].tolist() == [1, 0, 1, 1] and out["n_reads"].tolist() == want["n_reads"]
            for i in KEPT:
                assert out["per_sample_vcf_col"][i] == want["columns"][i].tolist()
                assert np.array_equal(out["read_labels"][i], want["results"][i].read_labels)
            assert out["per_sample_vcf_col"][1] is None
            for name in ("infoCount", "afCount", "hweCount", "alleleCount"):
                assert np.array_equal(out[name], getattr(want["counts"], name)), name
            assert [int(x) for x in out["bx_stats"]] == want["bx_stats"]
        for out in (on, both):
            assert out["final_read_labels_prob"][1] is None
            for i in KEPT:
                names, prob, labels = out["final_read_labels_prob"][i]
                w_names, w_prob, w_labels = c_on["final_read_labels_prob"][i]
                assert names == w_names and np.array_equal(prob, w_prob) and np.array_equal(labels, w_labels)
        K, nG = panel.K, prm.nGibbsSamples
        assert both["gamma1"].shape == (K, 4) and both["list_of_gammas"].shape == (K * 2 * nG, 4)
        for f in ("gamma1", "gamma2", "gamma_total", "list_of_gammas"):
            assert np.isnan(both[f][:, 1]).all()   # the file that was not imputed
            for i in KEPT:
                assert np.array_equal(both[f][:, i], np.asarray(getattr(c_hla["results"][i], f)).ravel()), (f, i)
        # the sample-range call on the same reads (the kept files' global indices)
        rng = R.dotcall("qa_impute_sample_range", R.list([R.sample_reads(s) for s in samples]), R.panel_objects(panel),
                        _params(R, prm, output_read_label_prob=R.logical([1])), R.real([0.0, 1.0, 2.0]), R.integer([1]), R.nil)
        plain = R.dotcall("qa_impute_sample_range", R.list([R.sample_reads(s) for s in samples]), R.panel_objects(panel), _params(R, prm),
                          R.real([0.0, 1.0, 2.0]), R.integer([1]), R.nil)
        assert list(plain) == ["dosage", "gp_t", "phasing_haps", "read_labels", "nDosage", "stats"] and list(rng) == list(plain) + ["read_label_prob"]
        for j, i in enumerate(KEPT):
            assert np.array_equal(rng["read_label_prob"][j], c_on["final_read_labels_prob"][i][1])
            assert np.array_equal(rng["read_labels"][j], c_on["results"][i].read_labels)
            assert np.array_equal(rng["dosage"][:, j], plain["dosage"][:, j]) and np.array_equal(rng["read_labels"][j], plain["read_labels"][j])
        with pytest.raises(Exception, match="output_read_label_prob"):
            call(dict(sites, output_read_label_prob=R.integer([1])))
        with pytest.raises(Exception, match="hla_grid"):
            call(sites, hla_grid=R.integer([panel.nGrids]))
    finally:
        R.dotcall("qa_shim_release")
        R.reset()
