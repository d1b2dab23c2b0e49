"""hla_run on the device: the gamma column of one grid kept by the fp64 dosage passes (k_bwd64d<..., GCOL = true>, streamed rows
included) and by the validation kernels (k_bwd_ro<true>), through qa_fullpass_reads_select_gamma_batch, against the oracle's
gamma_t[, grid] (reference-single.cpp:2045-2050, :2170-2172); the same call's other outputs against
qa_fullpass_reads_select_batch's; qa_impute_samples_hla against qa_impute_samples and against the native loop on the oracle; and
`.Call("qa_impute_sample_range", ...)` with params$hla_grid under the test runtime of R's C API."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _inputs(panel, n_samples=2, n_chains=3, Ksubset=64, seed=5):
    from quilt_amd.driver import thinned_grid_columns
    from quilt_amd.synth import make_synthetic_sample
    rng = np.random.default_rng(seed)
    samples = [make_synthetic_sample(panel, seed=800 + i, n_reads=220) for i in range(n_samples)]
    cs = [c % n_samples for c in range(n_chains)]
    labels = [rng.integers(1, 3, size=samples[s].nReads).astype(np.int32) for s in cs]
    want_top = [1] * n_chains
    want_top[1] = 0
    cols = thinned_grid_columns(panel.nGrids, 0.1)
    which = [np.sort(rng.choice(panel.K, Ksubset, replace=False) + 1).astype(np.int32) for _ in range(n_chains)]
    seeds = [int(rng.integers(0, 2 ** 63)) for _ in range(n_chains)]
    return samples, cs, labels, want_top, cols, dict(Ksubset=Ksubset, Knew=Ksubset // 2, which=which, seeds=seeds)


def _grids(panel):
    """0, 1, an odd and an even interior grid, G - 1 and the first two grids holding special haplotypes (code 0)."""
    G = panel.nGrids
    sp = [int(g) for g in np.nonzero(np.asarray(panel.eMatDH_special_grid_which))[0]]
    odd = next(g for g in range(3, G - 1) if g % 2 == 1)
    even = next(g for g in range(G // 2, G - 1) if g % 2 == 0)
    return sorted({0, 1, odd, even, G - 1, *sp[:2]})


def _run(panel, sum_order=0, grids=None):
    from quilt_amd.driver import HipBackend
    from quilt_amd.native import DevicePanel
    from tests.hla_backend import oracle_gamma_t
    samples, cs, labels, wt, cols, sel = _inputs(panel)
    n = len(cs)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    if sum_order:
        dev.set_sum_order(sum_order)
    be = HipBackend(dev)
    d0, _, c0, n0, s0 = be.fullpass_reads_batch(samples, cs, labels, [1] * n, wt, cols, 5, 1e-10, 8, select=sel)
    d0, c0, n0, s0 = d0.copy(), c0.copy(), n0.copy(), s0.copy()
    ref = oracle_gamma_t(panel, samples, cs, labels)
    worst = 0.0
    for g in (grids or _grids(panel)):
        d, _, c, nx, st, gam = be.fullpass_reads_batch(samples, cs, labels, [1] * n, wt, cols, 5, 1e-10, 8, select=sel, gamma_grid=g)
        # the same call's other outputs: bit-identical to qa_fullpass_reads_select_batch's
        assert np.array_equal(d, d0) and np.array_equal(c, c0) and np.array_equal(nx, n0) and np.array_equal(st, s0), g
        for ci in range(n):
            for l in range(2):
                want = ref[ci][l][:, g]
                if sum_order:
                    assert np.array_equal(gam[ci, l], want), (g, ci, l)
                else:
                    d_max = float(np.abs(gam[ci, l] - want).max())
                    worst = max(worst, d_max)
                    assert d_max <= 1e-9, (g, ci, l, d_max)
    dev.close()
    print("K = %d, grids %s: max |gamma - oracle| = %.2e" % (panel.K, grids or _grids(panel), worst))
    return worst


def test_gamma_column_1000g_like_panel():
    from quilt_amd.synth import make_1000g_like_panel
    _run(make_1000g_like_panel(K=5008, nSNPs=640))


@pytest.mark.parametrize("K", [50000, 65536])
def test_gamma_column_large_panels(K):
    """K = 50 000: chunk rows in registers and LDS; K = 65 536: rows past the seventh streamed through HBM (the SP kernels);
    grids 2 and 9 hold special haplotypes."""
    from quilt_amd.synth import make_synthetic_panel
    panel = make_synthetic_panel(K=K, nSNPs=640, seed=515, nMaxDH=255)
    assert set(_grids(panel)) >= {2, 9}
    _run(panel)


def test_gamma_column_in_validation_mode_is_the_oracles(small_panel):
    from quilt_amd.synth import make_1000g_like_panel
    _run(small_panel, sum_order=1)
    _run(make_1000g_like_panel(K=5008, nSNPs=640), sum_order=1, grids=[0, 9, 19])


def test_fp32_dosage_passes_are_refused(small_panel):
    from quilt_amd.native import DevicePanel, lib, ptr
    samples, cs, labels, wt, cols, sel = _inputs(small_panel)
    dev = DevicePanel(small_panel)
    dev.set_dosage_precision(32)
    L = lib()
    n = len(cs)
    read_off = np.array([0, samples[0].nReads, samples[0].nReads + samples[1].nReads], dtype=np.int32)
    read_ptr = np.concatenate([np.asarray(s.read_ptr, dtype=np.int32) for s in samples])
    u = np.concatenate([np.asarray(s.u, dtype=np.int32) for s in samples])
    bq = np.concatenate([np.asarray(s.bq, dtype=np.int32) for s in samples])
    H = np.concatenate(labels)
    csa, wd, wta = (np.asarray(x, dtype=np.int32) for x in (cs, [1] * n, wt))
    which = np.ascontiguousarray(np.stack(sel["which"]))
    seeds = np.asarray(sel["seeds"], dtype=np.uint64)
    dosage, cnt = np.zeros((n, 2, small_panel.nSNPs)), np.zeros(n * 2 * int((cols >= 0).sum()), dtype=np.int32)
    nxt, status, gam = np.zeros_like(which), np.zeros(n, dtype=np.int32), np.zeros((n, 2, small_panel.K))
    st = L.qa_fullpass_reads_select_gamma_batch(dev.handle, C.c_int32(n), C.c_int32(2), C.c_int32(2), ptr(csa), ptr(read_off),
                                                ptr(read_ptr), ptr(u), ptr(bq), ptr(H), ptr(wd), ptr(wta), ptr(cols), C.c_int32(5),
                                                C.c_double(1e-10), ptr(dosage), C.c_int32(8), None, None, ptr(cnt),
                                                C.c_int32(sel["Ksubset"]), C.c_int32(sel["Knew"]), ptr(which), ptr(seeds), ptr(nxt),
                                                ptr(status), C.c_int32(3), ptr(gam))
    dev.close()
    assert st == -3 and b"qa_panel_set_dosage_precision(64)" in L.qa_last_error()


def _same(a, b):
    assert a.nDosage == b.nDosage
    assert np.array_equal(a.read_labels, b.read_labels)
    assert np.array_equal(a.dosage, b.dosage)
    assert np.array_equal(a.gp_t, b.gp_t)
    assert np.array_equal(a.phasing_haps, b.phasing_haps)


@pytest.mark.parametrize("n_threads", [1, 2])
def test_impute_samples_hla_on_the_device(n_threads):
    """qa_impute_samples_hla: every existing output bit-identical to qa_impute_samples'; gamma_total the reference's sum of
    list_of_gammas; every gamma column sums to 1."""
    from quilt_amd.driver import DriverParams, HlaDriverParams, hla_gamma_total
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_1000g_like_panel, make_synthetic_sample
    panel = make_1000g_like_panel(K=5008, nSNPs=1600)
    samples = [make_synthetic_sample(panel, seed=4300 + i, n_reads=400) for i in range(5)]
    common = dict(nGibbsSamples=3, Ksubset=200, Knew=200, seed=21)
    devs = [DevicePanel(panel) for _ in range(n_threads)]
    for d in devs:
        d.set_dosage_precision(64)
        d.set_device_share(n_threads)
        if n_threads > 1:
            d.set_exclusive(True)
    grid = int(np.round(panel.nGrids / 2)) - 1
    plain = impute_samples(devs, samples, DriverParams(**common), sample_offset=7, samples_per_launch_set=2)
    hla = impute_samples(devs, samples, HlaDriverParams(**common, hla_grid=grid), sample_offset=7, samples_per_launch_set=2)
    for d in devs:
        d.close()
    for a, b in zip(hla, plain):
        _same(a, b)
        assert a.list_of_gammas.shape == (3, 2, panel.K)
        assert np.array_equal(a.gamma_total, hla_gamma_total(a.list_of_gammas))
        assert abs(a.gamma1.sum() - 1) < 1e-9 and abs(a.gamma2.sum() - 1) < 1e-9
        assert np.all(np.abs(a.list_of_gammas.sum(axis=2) - 1) < 1e-9)


def test_impute_samples_hla_validation_mode_equals_the_native_loop_on_the_oracle():
    from quilt_amd.driver import DriverParams, HlaDriverParams
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
    from tests.hla_backend import impute_samples_hla_on_oracle
    panel = make_synthetic_panel(K=400, nSNPs=3200, seed=77, ref_error=1e-3)
    samples = [make_synthetic_sample(panel, seed=960 + i, n_reads=200) for i in range(3)]
    grid = 49
    P = HlaDriverParams(nGibbsSamples=2, n_seek_its=2, Ksubset=48, Knew=48, small_ref_panel_gibbs_iterations=4,
                        small_ref_panel_block_gibbs_iterations=(2,), seed=5, hla_grid=grid)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    dev.set_sum_order(1)
    got = impute_samples([dev], samples, P, samples_per_launch_set=2)
    dev.close()
    want, _, _ = impute_samples_hla_on_oracle(panel, samples, P, grid, samples_per_launch_set=2)
    for a, b in zip(got, want):
        assert np.array_equal(a.read_labels, b.read_labels)
        for f in ("gamma1", "gamma2", "gamma_total", "list_of_gammas"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f


def test_sample_range_call_with_hla_grid():
    """`.Call("qa_impute_sample_range", ...)` with params$hla_grid: gamma1 / gamma2 / gamma_total K x n and list_of_gammas
    (K x 2 x nGibbsSamples) x n, equal to the direct C call's (quilt_amd.impute over the same device); the other outputs unchanged;
    a grid outside [0, nGrids) an R error."""
    from quilt_amd.driver import DriverParams, HlaDriverParams
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
    from tests.mini_r import R as Runtime
    panel = make_synthetic_panel(K=1024, nSNPs=96 * 32, seed=21)
    samples = [make_synthetic_sample(panel, seed=830 + i, n_reads=300) for i in range(3)]
    grid = 47
    prm = HlaDriverParams(nGibbsSamples=2, Ksubset=128, Knew=128, seed=77, hla_grid=grid)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    want = impute_samples([dev], samples, prm, sample_offset=4, samples_per_launch_set=2)
    dev.close()
    R = Runtime()
    try:
        params = dict(nGibbsSamples=R.integer([2]), Ksubset=R.integer([128]), Knew=R.integer([128]), seed=R.real([77.0]),
                      samples_per_launch_set=R.integer([2]), hla_grid=R.integer([grid]))
        out = R.dotcall("qa_impute_sample_range", R.list([R.sample_reads(s) for s in samples]), R.panel_objects(panel), R.named(params),
                        R.real([4.0]), R.integer([1]), R.nil)
        K, n = panel.K, len(samples)
        assert out["gamma1"].shape == (K, n) and out["gamma2"].shape == (K, n) and out["gamma_total"].shape == (K, n)
        assert out["list_of_gammas"].shape == (K * 2 * 2, n)
        for i, w in enumerate(want):
            assert np.array_equal(out["dosage"][:, i], w.dosage)
            assert np.array_equal(out["read_labels"][i], w.read_labels)
            assert np.array_equal(out["gamma1"][:, i], w.gamma1) and np.array_equal(out["gamma2"][:, i], w.gamma2)
            assert np.array_equal(out["gamma_total"][:, i], w.gamma_total)
            assert np.array_equal(out["list_of_gammas"][:, i].reshape(2, 2, K), w.list_of_gammas)
        with pytest.raises(Exception, match="hla_grid"):
            R.dotcall("qa_impute_sample_range", R.list([R.sample_reads(samples[0])]), R.panel_objects(panel),
                      R.named(dict(params, hla_grid=R.integer([panel.nGrids]))), R.real([4.0]), R.integer([1]), R.nil)
    finally:
        R.dotcall("qa_shim_release")
        R.reset()
