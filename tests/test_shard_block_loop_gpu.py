"""shard_check_every_pair = FALSE in the per-sample loop: qa_impute_params_t.shard_blocks through qa_impute_samples (csrc/impute.cpp)
and quilt_amd.driver.ShardBlocks through the Python statement of the loop, on rows of tests/mode_matrix.py -- the same bytes from
both; without the struct the calls are what they were; with impute_rare_common both refuse before the first sample."""
import numpy as np
import pytest

from tests import mode_matrix as MM

pytestmark = pytest.mark.gpu

ROWS = [("diploid", dict(MM.BASE, method="diploid")), ("diploid+mspbwt", dict(MM.BASE, method="diploid", use_mspbwt=True))]
FIELDS = ("read_labels", "dosage", "gp_t", "phasing_haps")


@pytest.fixture(scope="module")
def rig():
    from quilt_amd.native import DevicePanel
    panel, _, _, _ = MM.make_case(dict(MM.BASE), n_samples=0)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    devs = [DevicePanel(panel) for _ in range(2)]
    for d in devs:
        d.set_device_share(2)
        d.set_dosage_precision(64)
        d.set_exclusive(True)
    yield dict(panel=panel, dev=dev, devs=devs)
    for d in devs + [dev]:
        d.close()


def _same(res, want, name):
    assert len(res) == len(want)
    for a, b in zip(res, want):
        assert a.nDosage == b.nDosage
        for f in FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f"{name}: {f}"


@pytest.mark.parametrize("name,kw", ROWS, ids=[n for n, _ in ROWS])
def test_both_loops_return_the_same_bytes_block_by_block(rig, name, kw):
    from quilt_amd.driver import Driver, HipBackend, ShardBlocks
    from quilt_amd.impute import impute_samples
    panel, _, samples, P = MM.make_case(kw, reads=300, seed0=70)
    sb = ShardBlocks(L_grid=rig["panel"].L_grid, shuffle_bin_radius=P.shuffle_bin_radius, block_gibbs_quantile_prob=0.8)
    want = Driver(rig["panel"], HipBackend(rig["dev"]), P, shard_blocks=sb).run(samples, sample_offset=3)
    got = impute_samples(rig["devs"], samples, P, sample_offset=3, samples_per_launch_set=2, shard_blocks=sb)
    _same(got, want, name)
    # without the struct: the call form there was before, both loops, and another result than block by block
    plain = impute_samples(rig["devs"], samples, P, sample_offset=3, samples_per_launch_set=2)
    _same(plain, Driver(rig["panel"], HipBackend(rig["dev"]), P).run(samples, sample_offset=3), name)
    assert any(not np.array_equal(a.dosage, b.dosage) for a, b in zip(plain, got)), "the mode changed nothing on this row"


def test_both_loops_refuse_it_with_rare_common():
    from quilt_amd.driver import Driver, HipBackend, ShardBlocks
    from quilt_amd.impute import impute_samples
    from quilt_amd.native import DevicePanel, DeviceRareCommon, QuiltAmdError
    panel, rc, samples, P = MM.make_case(dict(MM.BASE, impute_rare_common=True), reads=300, seed0=70)
    sb = ShardBlocks(L_grid=panel.L_grid)
    dev = DevicePanel(panel)
    drc = DeviceRareCommon(dev, rc)
    with pytest.raises(ValueError, match="impute_rare_common"):
        Driver(panel, HipBackend(dev, drc), P, rare_common=rc, shard_blocks=sb)
    with pytest.raises(QuiltAmdError, match="impute_rare_common") as e:
        impute_samples([dev], samples, P, sample_offset=3, samples_per_launch_set=2, drcs=[drc], shard_blocks=sb)
    assert e.value.status == -3
    drc.close()
    dev.close()
