"""The shim's 63-argument Gibbs entry with shard_check_every_pair = FALSE, executed under tests/c/mini_r.c (tests/mini_r.py): the
same call as the Python mirror's bit for bit, and R's generator consumed in the reference's order and number -- after the reads'
own uniforms and the first read, per block iteration 8 x nReads unused draws (gibbs-nipt.cpp:3013-3018) and then the
n_blocks - 1 of the pass's own table (gibbs-nipt-block.cpp:2054)."""
import numpy as np
import pytest

from tests import shard_block_cases as SB
from tests.test_shim_gpu import _call_by_name, _panel_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from tests.mini_r import R as Runtime
    r = Runtime()
    yield r
    r.dotcall("qa_shim_release")
    r.reset()


@pytest.mark.parametrize("name", ["g40_readless", "g40_ks600_one_block"])
def test_gibbs_entry_63_arguments_block_wise(R, name):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.native import DevicePanel
    case = SB.cases()[name]
    panel, s = case.panel, case.sample
    G, Rn, Ks = case.G, s.nReads, len(case.which)
    n_its, nb = SB.N_BURN + SB.N_SAMPLE, len(SB.BLOCK_ITS)
    n_blocks = [t["n_blocks"] for t in case.reference()["trace"]]
    # R's stream: the sweeps' uniforms, the first read, then per pass 8 x nReads unused and the pass's n_blocks - 1
    rng = np.random.default_rng(12)
    n_expected = Rn * n_its + 1 + sum(8 * Rn + n - 1 for n in n_blocks)
    U = rng.random(n_expected + 50)
    U[:Rn * n_its] = case.runif_reads
    U[Rn * n_its] = (case.first_read + 0.5) / Rn
    shard = np.full(nb * (G - 1), np.nan)
    at = Rn * n_its + 1
    for j, n in enumerate(n_blocks):
        at += 8 * Rn
        U[at:at + n - 1] = case.runif_shard[j * (G - 1):j * (G - 1) + n - 1]
        shard[j * (G - 1):j * (G - 1) + n - 1] = U[at:at + n - 1]
        at += n - 1
    assert at == n_expected
    dev = DevicePanel(panel)
    want = rcpp_forwardBackwardGibbsNIPT(dev, s, case.which, case.H0, case.runif_reads, case.first_read, shard,
                                         shard_check_every_pair=False, return_state=True, **case.kwargs())
    dev.close()
    R.load_unif(U)
    z = lambda: R.real(np.zeros((Ks, G)))
    pl = dict(perform_block_gibbs=R.logical([1]), do_shard_block_gibbs=R.logical([1]), return_hapProbs=R.logical([1]),
              return_genProbs=R.logical([1]), use_starting_read_labels=R.logical([1]), shard_check_every_pair=R.logical([0]),
              gibbs_initialize_iteratively=R.logical([0]), sample_is_diploid=R.logical([1]), rescale_eMatRead_t=R.logical([1]))
    a = dict(sampleReads=R.sample_reads(s), transMatRate_tc_H=R.real(np.asarray(panel.transMatRate_t).reshape(2, G - 1, 1, order="F")),
             ff=R.real([0.0]), alphaHat_t1=z(), betaHat_t1=z(), alphaHat_t2=z(), betaHat_t2=z(), eMatGrid_t1=z(), eMatGrid_t2=z(),
             which_haps_to_use=R.integer(case.which), wif0=R.integer(s.wif), L_grid=R.integer(case.L_grid), param_list=R.named(pl),
             Jmax_local=R.integer([10000]), maxDifferenceBetweenReads=R.real([1e10]), generate_fb_snp_offsets=R.logical([0]),
             n_gibbs_starts=R.integer([1]), n_gibbs_sample_its=R.integer([SB.N_SAMPLE]), n_gibbs_burn_in_its=R.integer([SB.N_BURN]),
             double_list_of_starting_read_labels=R.list([R.list([R.integer(case.H0)])]), class_sum_cutoff=R.real([0.06]),
             shuffle_bin_radius=R.integer([case.radius]), block_gibbs_iterations=R.integer(np.array(SB.BLOCK_ITS, dtype=np.int32)),
             block_gibbs_quantile_prob=R.real([case.q]))
    a.update(_panel_args(R, panel))
    out = _call_by_name(R, "_QUILT_rcpp_forwardBackwardGibbsNIPT", a)
    assert R.L.mini_r_unif_drawn() == n_expected and R.L.mini_r_rng_violations() == 0
    assert out["underflow_problem"][0] == 0
    assert np.array_equal(out["H"], want["H"]) and np.array_equal(out["H_class"], want["H_class"])
    assert np.array_equal(out["hapProbs_t"], want["hapProbs_t"])
    assert np.array_equal(out["genProbsM_t"], want["genProbsM_t"]) and np.array_equal(out["genProbsF_t"], want["genProbsF_t"])
    for nm in ("alphaHat_t1", "alphaHat_t2", "betaHat_t1", "betaHat_t2", "eMatGrid_t1", "eMatGrid_t2"):
        assert np.array_equal(R.value(a[nm]), want[nm]), nm


def test_sample_range_call_block_wise(R):
    """`.Call("qa_impute_sample_range", ...)` with params$shard_check_every_pair = FALSE and panel_objects$L_grid == the Python
    caller's qa_impute_samples with the shard_blocks struct, bit for bit; absent from params, the flag is TRUE."""
    from quilt_amd.driver import DriverParams, ShardBlocks
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
    from tests.test_shim_gpu import _check, _params
    panel = make_synthetic_panel(K=1024, nSNPs=96 * 32, seed=21)
    samples = [make_synthetic_sample(panel, seed=870 + i, n_reads=300) for i in range(3)]
    prm = DriverParams(nGibbsSamples=2, Ksubset=128, Knew=128, seed=81)
    sb = ShardBlocks(L_grid=panel.L_grid, shuffle_bin_radius=prm.shuffle_bin_radius, block_gibbs_quantile_prob=0.8)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    want = impute_samples([dev], samples, prm, samples_per_launch_set=2, shard_blocks=sb)
    plain = impute_samples([dev], samples, prm, samples_per_launch_set=2)
    dev.close()
    assert any(not np.array_equal(a.dosage, b.dosage) for a, b in zip(want, plain))
    reads = R.list([R.sample_reads(s) for s in samples])
    out = R.dotcall("qa_impute_sample_range", reads, R.panel_objects(panel, L_grid=R.integer(panel.L_grid)),
                    _params(R, prm, shard_check_every_pair=R.logical([0]), shuffle_bin_radius=R.integer([prm.shuffle_bin_radius]),
                            block_gibbs_quantile_prob=R.real([0.8])),
                    R.real([0.0]), R.integer([1]), R.nil)
    _check(out, want)
    out = R.dotcall("qa_impute_sample_range", reads, R.panel_objects(panel, L_grid=R.integer(panel.L_grid)), _params(R, prm),
                    R.real([0.0]), R.integer([1]), R.nil)
    _check(out, plain)
