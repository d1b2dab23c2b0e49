"""`.Call("qa_impute_sample_range", ...)` with params$gibbs_state_bits = 32L under the test runtime of R's C API (tests/c/mini_r.c):
the shim sets the width on the range's panel handles, and the columns are those of the native loop called directly on a handle
at that width."""
import numpy as np
import pytest

from tests.shim_calls import params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from tests.mini_r import R as Runtime
    r = Runtime()
    yield r
    r.dotcall("qa_shim_release")
    r.reset()


def test_range_entry_passes_the_state_width_on(R, small_panel):
    from quilt_amd.driver import DriverParams
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel
    from quilt_amd.synth import make_synthetic_sample
    from tests.mini_r import RError
    panel = small_panel
    samples = [make_synthetic_sample(panel, seed=3400 + i, n_reads=120) for i in range(2)]
    prm = DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64, seed=5)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    dev.set_gibbs_state_bits(32)
    want = impute_samples([dev], samples, prm, sample_offset=3, samples_per_launch_set=2)
    dev.close()
    reads = R.list([R.sample_reads(s) for s in samples])
    out = R.dotcall("qa_impute_sample_range", reads, R.panel_objects(panel), params(R, prm, gibbs_state_bits=R.integer([32])),
                    R.real([3.0]), R.integer([1]), R.nil)
    T = panel.nSNPs
    for i, w in enumerate(want):
        assert np.array_equal(out["dosage"][:, i], w.dosage) and np.array_equal(out["gp_t"][:, i].reshape(3, T), w.gp_t)
        assert np.array_equal(out["phasing_haps"][:, i].reshape(2, T).T, w.phasing_haps)
        assert np.array_equal(out["read_labels"][i], w.read_labels)
        assert out["nDosage"][i] == w.nDosage and w.dosage.std() > 0
    # a width the library does not run is its refusal, raised as an R error before any sample
    with pytest.raises(RError, match="gibbs_state_bits"):
        R.dotcall("qa_impute_sample_range", reads, R.panel_objects(panel), params(R, prm, gibbs_state_bits=R.integer([16])),
                  R.real([3.0]), R.integer([1]), R.nil)
