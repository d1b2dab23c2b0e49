"""The Gibbs sampler's fp32 state mode (qa_panel_set_gibbs_state_bits(panel, 32)) on the device against the fp64 reference, on the cases of
tests/state32_cases.py -- whose uniforms lie further than DELTA from every threshold (tests/test_state32_cases_cpu.py), so the
labels must be the reference's.  Bars, with E the storage error of a column (5.96e-8):
    H, H_class                 identical
    eMatGrid_t, c              rtol 1e-6
    alphaHat_t, betaHat_t      rtol 4 E (the sweeps recompute from stored columns, which E's emulation of the initial recursions
                               does not cover), atol 2^-126 (indifferent to whether fp32 denormals flush)
    hapProbs_t, genProbsM_t    2e-6 absolute, the bar of the fp32-state dosage passes
"""
import ctypes as C

import numpy as np
import pytest

from tests import state32_cases as S
from tests.util import r2

pytestmark = pytest.mark.gpu

ATOL_STATE = 2.0 ** -126
_DEV, _RC, _GOT = {}, {}, {}


def _device(c):
    from quilt_amd.native import DevicePanel
    if id(c.panel) not in _DEV:
        _DEV[id(c.panel)] = DevicePanel(c.panel)
    return _DEV[id(c.panel)]


def _rare(c):
    from quilt_amd.native import DeviceRareCommon
    if c.rc is None:
        return {}
    if c.name not in _RC:
        _RC[c.name] = DeviceRareCommon(_device(c), c.rc)
    return dict(rare_common=_RC[c.name])


def _run(c, bits, **kw):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    return rcpp_forwardBackwardGibbsNIPT(_device(c), c.sample, c.which, c.H0, c.runif_reads, c.first_read, c.runif_shard,
                                         state_bits=bits, return_state=True, **{**c.device_kwargs(), **_rare(c), **kw})


def _mode(c, bits):
    """the case in one mode, default build choice (run once per process; shared: do not write into it)"""
    if (c.name, bits) not in _GOT:
        _GOT[c.name, bits] = _run(c, bits)
    return _GOT[c.name, bits]


def _holds_the_bars(c, got):
    ref = S.reference(c)
    rtol_ab = 4 * S.E()
    assert not got["underflow_problem"]
    for h in range(2):   # (printed before anything is asserted: what the mode does to the state)
        for n in ("alphaHat_t", "betaHat_t", "eMatGrid_t"):
            x, y = got[f"{n}{h + 1}"], np.asarray(ref[n][h])
            big = np.abs(y) >= ATOL_STATE
            print(f"{c.name} {n}{h + 1}: max rel {np.max(np.abs(x[big] - y[big]) / np.abs(y[big])) if big.any() else 0.0:.3e}")
    lab = min(2, np.asarray(ref["hapProbs_t"]).shape[0])
    print(f"{c.name} hapProbs_t: max abs {np.abs(got['hapProbs_t'][:lab] - np.asarray(ref['hapProbs_t'])[:lab]).max():.3e}")
    assert np.array_equal(got["H"], ref["H"]), f"{(got['H'] != ref['H']).sum()} labels differ"
    assert np.array_equal(got["H_class"], ref["H_class"])
    for h in range(2):
        np.testing.assert_allclose(got[f"eMatGrid_t{h + 1}"], ref["eMatGrid_t"][h], rtol=1e-6)
        np.testing.assert_allclose(got[f"c{h + 1}"], ref["c"][h], rtol=1e-6)
        np.testing.assert_allclose(got[f"alphaHat_t{h + 1}"], ref["alphaHat_t"][h], rtol=rtol_ab, atol=ATOL_STATE)
        np.testing.assert_allclose(got[f"betaHat_t{h + 1}"], ref["betaHat_t"][h], rtol=rtol_ab, atol=ATOL_STATE)
    np.testing.assert_allclose(got["hapProbs_t"][:lab], np.asarray(ref["hapProbs_t"])[:lab], rtol=0, atol=2e-6)
    if "genProbsM_t" in ref and ref["genProbsM_t"] is not None:
        np.testing.assert_allclose(got["genProbsM_t"], ref["genProbsM_t"], rtol=0, atol=2e-6)


@pytest.mark.parametrize("name", S.NAMES)
def test_case_holds_the_bars_in_fp32_state(name):
    c = S.case(name)
    _holds_the_bars(c, _mode(c, 32))


@pytest.mark.parametrize("name,hook,value", [("g129_ks600", "QA_GIBBS_LEAN", "1"), ("g129_ks600", "QA_GIBBS_NW", "2"),
                                             ("g129_ks600", "QA_GIBBS_NW", "5"), ("g129_ks600", "QA_GIBBS_NW", "10"),
                                             ("g130_ks600_blocks", "QA_GIBBS_LEAN", "1")])
def test_every_build_of_the_production_geometry(name, hook, value, monkeypatch):
    """Ks = 600 as the 256-register build and as 2, 5 and 10 waves per chain; the segmented sweeps and k_shard_blocks of the
    256-register build: the fp32 builds of each against the same bars."""
    monkeypatch.setenv(hook, value)
    c = S.case(name)
    _holds_the_bars(c, _run(c, 32))


def test_the_mode_is_really_narrow():
    """What comes back as alpha and beta went through fp32 storage, and is not what the fp64 mode returns; eMatGrid_t did not."""
    c = S.case("g129_ks600")
    narrow, wide = _mode(c, 32), _mode(c, 64)
    differs = 0
    for n in ("alphaHat_t1", "alphaHat_t2", "betaHat_t1", "betaHat_t2"):
        x = narrow[n]
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64)), f"{n} holds values fp32 cannot"
        differs += int((x != wide[n]).sum())
        assert not np.array_equal(wide[n], wide[n].astype(np.float32).astype(np.float64)), f"{n} of the fp64 mode is fp32 already"
    assert differs > 0
    for n in ("eMatGrid_t1", "eMatGrid_t2"):
        np.testing.assert_allclose(narrow[n], wide[n], rtol=1e-6)


@pytest.mark.parametrize("name", ["g129_ks600", "rc_small"])
def test_default_is_untouched(name):
    """state_bits = 0 and 64 are the same call -- and the reference's at the fp64 bars the suite holds everywhere else."""
    c = S.case(name)
    a, b = _mode(c, 0), _mode(c, 64)
    for n in a:
        if isinstance(a[n], np.ndarray):
            assert np.array_equal(a[n], b[n]), n
    ref = S.reference(c)
    assert np.array_equal(a["H"], ref["H"])
    for h in range(2):
        np.testing.assert_allclose(a[f"alphaHat_t{h + 1}"], ref["alphaHat_t"][h], rtol=1e-8, atol=1e-300)
        np.testing.assert_allclose(a[f"betaHat_t{h + 1}"], ref["betaHat_t"][h], rtol=1e-8, atol=1e-300)


def test_chains_of_one_call_equal_their_own_calls():
    """Four chains of g65_ks65 with different subsets in one call, the last of them reading its sample through reads_same_as:
    each equals its own call bit for bit in the fp32 mode."""
    from quilt_amd.gibbs_nipt import forwardBackwardGibbsNIPT_batch
    c = S.case("g65_ks65")
    dev = _device(c)
    rng = np.random.default_rng(65)
    n = 4
    whichs = [c.which] + [np.sort(rng.choice(c.panel.K, c.Ks, replace=False)).astype(np.int32) + 1 for _ in range(n - 1)]
    H0s = [c.H0] + [rng.integers(1, 3, size=c.sample.nReads).astype(np.int32) for _ in range(n - 1)]
    rus = [c.runif_reads] + [rng.random(len(c.runif_reads)) for _ in range(n - 1)]
    rss = [c.runif_shard] + [rng.random(len(c.runif_shard)) for _ in range(n - 1)]
    frs = [c.first_read] * n
    kw = dict(state_bits=32, **c.device_kwargs())
    # chains 0 .. 2 carry their own copy of the reads; chain 3 names chain 2 and its own bases are left out (zeros)
    hollow = S.sample_from_arrays(c.sample.read_ptr, np.zeros_like(c.sample.u), np.zeros_like(c.sample.bq), c.sample.wif)
    together = forwardBackwardGibbsNIPT_batch(dev, [c.sample] * 3 + [hollow], whichs, H0s, rus, frs, rss, reads_same_as=[0, 1, 2, 2], **kw)
    for i in range(n):
        alone = forwardBackwardGibbsNIPT_batch(dev, [c.sample], [whichs[i]], [H0s[i]], [rus[i]], [frs[i]], [rss[i]], **kw)[0]
        for k in ("H", "H_class", "hapProbs_t", "genProbsM_t", "genProbsF_t"):
            assert np.array_equal(together[i][k], alone[k]), (i, k)
    assert not np.array_equal(together[0]["H"], together[1]["H"])
    assert np.array_equal(together[0]["H"], _mode(c, 32)["H"])


def test_refusals(small_panel):
    from quilt_amd.driver import DriverParams
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.impute import prepare_range, run_prepared
    from quilt_amd.native import DevicePanel, QuiltAmdError, lib
    from quilt_amd.synth import make_synthetic_sample
    c = S.case("g65_ks63")
    dev = _device(c)
    H = c.H0.copy()
    R = c.sample.nReads
    rb, rr = np.full(3 * R, 0.5), np.full(3 * R, 0.5)
    assert dev.gibbs_state_bits() == 64
    with pytest.raises(QuiltAmdError, match=r"fp32 .*ff = 0.* 0 or 64") as e:
        rcpp_forwardBackwardGibbsNIPT(dev, c.sample, c.which, H, c.runif_reads, c.first_read, None, ff=0.2, runif_block=rb,
                                      runif_resample=rr, state_bits=32, return_state=True)
    assert e.value.status == -3 and np.array_equal(H, c.H0) and dev.gibbs_state_bits() == 64   # (the call's width is not left behind)
    with pytest.raises(QuiltAmdError, match=r"bits = 16.*64.*32") as e:
        rcpp_forwardBackwardGibbsNIPT(dev, c.sample, c.which, H, c.runif_reads, c.first_read, c.runif_shard, state_bits=16)
    assert e.value.status == -2 and np.array_equal(H, c.H0) and dev.gibbs_state_bits() == 64
    # a refused width leaves the handle where it was, also at 32; 0 means 64
    dev.set_gibbs_state_bits(32)
    with pytest.raises(QuiltAmdError):
        dev.set_gibbs_state_bits(48)
    assert dev.gibbs_state_bits() == 32
    dev.set_gibbs_state_bits(0)
    assert dev.gibbs_state_bits() == 64
    # the range call with method = "nipt" on a handle at 32: refused before the first sample
    L = lib()
    pdev = DevicePanel(small_panel)
    samples = [make_synthetic_sample(small_panel, seed=3200 + i, n_reads=80, ff=0.2) for i in range(2)]
    prep = prepare_range([pdev], samples, DriverParams(nGibbsSamples=1, Ksubset=64, Knew=64, method="nipt"))
    kept = L.qa_impute_kept_buffers()
    pdev.set_gibbs_state_bits(32)
    with pytest.raises(QuiltAmdError, match="qa_panel_set_gibbs_state_bits = 32") as e:
        run_prepared(prep)
    assert e.value.status == -3 and L.qa_impute_kept_buffers() == kept
    pdev.close()


def test_native_loop_in_fp32_state(small_panel):
    """qa_impute_samples on a handle at qa_panel_set_gibbs_state_bits(32) runs to QA_OK, and every sample's dosage r2 against the synthetic truth is no
    lower than the lowest the CPU oracle loop reaches on the same samples over 8 driver seeds, minus the spread of those 8 (the
    seed-to-seed bar tests/test_pipeline_gpu.py holds runs that part to).  Labels are not compared: over a whole pipeline a
    uniform does come close to a threshold sooner or later."""
    import dataclasses
    from quilt_amd.driver import Driver, DriverParams, HipBackend
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_synthetic_sample
    from tests.oracle_backend import OracleBackend
    panel = small_panel
    samples = [make_synthetic_sample(panel, seed=3300 + i, n_reads=150) for i in range(4)]
    prm = DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64, seed=3)
    dev = DevicePanel(panel)
    dev.set_gibbs_state_bits(32)
    got, stats = impute_samples([dev], samples, prm, return_stats=True)   # (check() raises on anything but QA_OK)
    # the Python statement of the loop on the same handle: the same Gibbs calls at the same width, so the same labels
    py = Driver(panel, HipBackend(dev), prm).run(samples)
    dev.set_gibbs_state_bits(64)
    wide = impute_samples([dev], samples, prm)
    dev.close()
    for a, b in zip(got, py):
        assert np.array_equal(a.read_labels, b.read_labels)
    assert stats["gibbs_chain_calls"] > 0
    cpu = [Driver(panel, OracleBackend(panel, n_threads=4), dataclasses.replace(prm, seed=100 + k)).run(samples)
           for k in range(8)]
    for i, s in enumerate(samples):
        truth = s.truth_haps.sum(axis=0)
        r = np.array([r2(run[i].dosage, truth) for run in cpu])
        bar = r.min() - (r.max() - r.min())
        print(f"sample {i}: r2 vs truth fp32 state {r2(got[i].dosage, truth):.4f}, fp64 state {r2(wide[i].dosage, truth):.4f}; "
              f"CPU loop over 8 seeds {r.min():.4f} .. {r.max():.4f}, bar {bar:.4f}")
        assert got[i].nDosage == 2 and np.isfinite(got[i].dosage).all()
        assert r2(got[i].dosage, truth) >= bar
