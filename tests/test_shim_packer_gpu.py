"""The one sampleReads -> CSR packer of shim/quilt_amd_shim.c at its edges, through the three `.Call` entries that share it: a sample
whose FIRST and LAST reads have exactly one base (a packer that is off by one at either end of read_ptr moves every base of the
sample, or reads past the last one), as a range of one sample (the list-of-lists form, with the central grids), through the
63-argument entry and through the 15-argument entry (the one-list form, without them).  Each equals the Python mirror's call of
the same library bit for bit.  K = 64, 10 grids, Ksubset = 64, 40 reads."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from tests.shim_calls import call_by_name, ematread_args, gibbs_args, params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from tests.mini_r import R as Runtime
    r = Runtime()
    yield r
    r.dotcall("qa_shim_release")
    r.reset()


@pytest.fixture(scope="module")
def panel():
    from quilt_amd.synth import make_synthetic_panel
    return make_synthetic_panel(K=64, nSNPs=320, seed=2)


@pytest.fixture(scope="module")
def sample(panel):
    """40 reads; the first keeps only its first base, the last only its last base (the central grids stay non-decreasing)."""
    from quilt_amd.synth import make_synthetic_sample
    s = make_synthetic_sample(panel, seed=3, n_reads=40)
    ptr = np.asarray(s.read_ptr)
    assert ptr[1] - ptr[0] > 1 and ptr[-1] - ptr[-2] > 1   # (there is something to cut)
    keep = np.ones(ptr[-1], dtype=bool)
    keep[ptr[0] + 1:ptr[1]] = False
    keep[ptr[-2]:ptr[-1] - 1] = False
    n = np.diff(ptr)
    n[0] = n[-1] = 1
    u, wif = np.asarray(s.u)[keep], np.asarray(s.wif).copy()
    new_ptr = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
    wif[0], wif[-1] = u[0] // 32, u[-1] // 32
    assert (np.diff(wif) >= 0).all() and new_ptr[1] == 1 and new_ptr[-1] - new_ptr[-2] == 1
    return dataclasses.replace(s, read_ptr=new_ptr, u=u, bq=np.asarray(s.bq)[keep], wif=wif.astype(np.int32))


def _range_of_one_sample(R, panel, sample):
    from quilt_amd.driver import DriverParams
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    prm = DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64, seed=5)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    want = impute_samples([dev], [sample], prm, sample_offset=3, samples_per_launch_set=2)[0]
    dev.close()
    out = R.dotcall("qa_impute_sample_range", R.list([R.sample_reads(sample)]), R.panel_objects(panel), params(R, prm), R.real([3.0]),
                    R.integer([1]), R.nil)
    T = panel.nSNPs
    assert np.array_equal(out["dosage"][:, 0], want.dosage) and np.array_equal(out["gp_t"][:, 0].reshape(3, T), want.gp_t)
    assert np.array_equal(out["phasing_haps"][:, 0].reshape(2, T).T, want.phasing_haps)
    assert np.array_equal(out["read_labels"][0], want.read_labels) and len(want.read_labels) == 40
    assert out["nDosage"][0] == want.nDosage and want.dosage.std() > 0


def _gibbs_entry(R, panel, sample):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.native import DevicePanel
    s, G, Rn, Ks, n_burn, n_samp = sample, panel.nGrids, sample.nReads, 64, 4, 1
    blocks = np.array([2], dtype=np.int32)
    n_its, per_block = n_burn + n_samp, 8 * Rn + G - 1
    rng = np.random.default_rng(11)
    which = np.arange(1, Ks + 1, dtype=np.int32)
    start = rng.integers(1, 3, size=Rn).astype(np.int32)
    U = rng.random(Rn * n_its + 1 + per_block)
    base = Rn * n_its + 1
    dev = DevicePanel(panel)
    want = rcpp_forwardBackwardGibbsNIPT(dev, s, which, start, U[:Rn * n_its], min(int(U[Rn * n_its] * Rn), Rn - 1), U[base + 8 * Rn:], ff=0.0,
                                         n_gibbs_burn_in_its=n_burn, n_gibbs_sample_its=n_samp, block_gibbs_iterations=blocks, return_state=True)
    dev.close()
    assert not want["underflow_problem"]
    R.load_unif(U)
    a = gibbs_args(R, panel, s, which, start, n_burn, n_samp, blocks=blocks, param_list=dict(do_shard_block_gibbs=R.logical([1])))
    out = call_by_name(R, "_QUILT_rcpp_forwardBackwardGibbsNIPT", a)
    assert R.L.mini_r_unif_drawn() == U.size and R.L.mini_r_rng_violations() == 0
    assert out["underflow_problem"][0] == 0
    assert np.array_equal(out["H"], want["H"]) and np.array_equal(out["H_class"], want["H_class"])
    assert np.array_equal(out["hapProbs_t"], want["hapProbs_t"])
    assert np.array_equal(out["genProbsM_t"], want["genProbsM_t"]) and np.array_equal(out["genProbsF_t"], want["genProbsF_t"])
    for name in ("alphaHat_t1", "alphaHat_t2", "betaHat_t1", "betaHat_t2", "eMatGrid_t1", "eMatGrid_t2"):
        assert np.array_equal(R.value(a[name]), want[name]), name
    assert len(set(out["H"].tolist())) == 2


def _read_likelihood_entry(R, panel, sample):
    from quilt_amd.native import DevicePanel, check, lib, ptr
    s, T = sample, panel.nSNPs
    eh = np.random.default_rng(4).random((2, T, 2))   # K x nSNPs x S
    dev = DevicePanel(panel)
    want = np.zeros((s.nReads, 2))
    sl = np.ascontiguousarray(eh[:, :, 1].T)   # [SNP][K]: R's K x nSNPs slice, column-major
    read_off = np.array([0, s.nReads], dtype=np.int32)
    check(lib().qa_rcpp_make_eMatRead_t_nsnps(dev.handle, C.c_int32(T), C.c_int32(1), C.c_int32(2), ptr(sl), ptr(read_off),
                                              ptr(np.asarray(s.read_ptr, dtype=np.int32)), ptr(np.asarray(s.u, dtype=np.int32)),
                                              ptr(np.asarray(s.bq, dtype=np.int32)), C.c_double(1000.0), C.c_int32(1000), C.c_int32(0), ptr(want)))
    dev.close()
    em = R.real(np.zeros((2, s.nReads)))
    assert R.dotcall("_QUILT_rcpp_make_eMatRead_t", *ematread_args(R, s, em, eh, 1)) is None
    assert np.array_equal(R.value(em).T, want) and want.std() > 0


def test_one_base_reads_at_both_ends_through_the_three_entries(R, panel, sample):
    _range_of_one_sample(R, panel, sample)
    _gibbs_entry(R, panel, sample)             # (uploads and caches the panel ...
    _read_likelihood_entry(R, panel, sample)   # ... that this entry needs)
