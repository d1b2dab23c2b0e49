"""The constructed chains of tests/chain_cases.py on the device: every grid count and read-stream geometry of the Gibbs samplers.

k_gibbs, its every-pair shard pass, k_gibbs3, k_block_rate3, k_block3 and k_resample3 hold their per-grid and per-read scalars in
lane-held streams of 64 (csrc/gibbs_dev.hpp).  The chains put the grid count, the read count, a grid's run of reads, read-less
runs, skipped reads, the two emission forms and the block pass's table ON the indices where a stream is refilled or stored;
tests/test_chain_cases_cpu.py proves that they sit there and that the sweeps and passes act there.

Bar (the project's own, tests/util.py): labels and H_class identical to the fp64 CPU oracle under the same uniforms; eMatGrid, alpha,
beta, c and hapProbs / genProbs to GIBBS_RTOL = 1e-9 (return_state = True: the two-label call of one chain offers it); the
three-label outputs as tests/test_gibbs_geometry_gpu.py compares them.  Every group of cases runs as ONE batch call, and every chain
once more in a call of its own that must return the same bits.  The grid-count and run groups run again at Ksubset = 600 under every
build of the samplers (1, 2, 5, 10 waves per chain; the 256-register builds, which exist for one wave), and one group with the counter-based uniform streams.
"""
import numpy as np
import pytest

from tests import chain_cases as cc
from tests.util import GIBBS_RTOL as RTOL, gibbs_compare

pytestmark = pytest.mark.gpu

GROUPS = cc.groups(cc.all_cases())
OUT_FIELDS = ("H", "H_class", "hapProbs_t", "genProbsM_t", "genProbsF_t")


@pytest.fixture(scope="module")
def devs():
    """DevicePanel of a case's panel, made once per panel"""
    from quilt_amd.native import DevicePanel
    made = {}

    def get(panel):
        if id(panel) not in made:
            made[id(panel)] = DevicePanel(panel)
        return made[id(panel)]
    yield get
    for d in made.values():
        d.close()


def launches(kernel):
    """launches the library has counted for a kernel's profile slot since qa_profile_reset"""
    import ctypes as C
    from quilt_amd.native import lib
    L = lib()
    for i in range(L.qa_profile_count()):
        if L.qa_profile_name(i).decode() == kernel:
            ms, cnt, b = C.c_double(), C.c_int64(), C.c_double()
            L.qa_profile_get(i, C.byref(ms), C.byref(cnt), C.byref(b))
            return cnt.value
    raise KeyError(kernel)


def call_kwargs(c):
    kw = c.kwargs()
    if c.mode == "nipt":
        kw.pop("ff")
    return kw


def batch_call(dev, cs, **more):
    from quilt_amd.gibbs_nipt import forwardBackwardGibbsNIPT_batch
    c0 = cs[0]
    kw = dict(call_kwargs(c0), **more)
    if c0.mode == "nipt":
        kw.update(ff=[cc.FF] * len(cs))
        if "seed_reads" not in more:
            kw.update(runif_block=[c.runif_block for c in cs], runif_resample=[c.runif_resample for c in cs])
    seeded = "seed_reads" in more
    return forwardBackwardGibbsNIPT_batch(dev, [c.sample for c in cs], [c.which for c in cs], [c.H0 for c in cs],
                                          None if seeded else [c.runif_reads for c in cs], [c.first_read for c in cs],
                                          None if seeded or c0.mode == "nipt" else [c.runif_shard for c in cs], **kw)


def single_call(dev, c):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    if c.mode == "nipt":
        return rcpp_forwardBackwardGibbsNIPT(dev, c.sample, c.which, c.H0, c.runif_reads, c.first_read, None, ff=cc.FF,
                                             runif_block=c.runif_block, runif_resample=c.runif_resample, **call_kwargs(c))
    return rcpp_forwardBackwardGibbsNIPT(dev, c.sample, c.which, c.H0, c.runif_reads, c.first_read, c.runif_shard, return_state=True,
                                         **call_kwargs(c))


def compare_outputs(got, ref, name):
    """What every call returns: labels and classes identical, probabilities to 1e-9."""
    assert ref["status"] == 0 and not got["underflow_problem"], name
    assert np.array_equal(got["H"], ref["H"]), f"{name}: labels differ at reads {np.flatnonzero(got['H'] != ref['H'])[:10]}"
    assert np.array_equal(got["H_class"], ref["H_class"]), f"{name}: classes differ at reads {np.flatnonzero(got['H_class'] != ref['H_class'])[:10]}"
    for f in ("hapProbs_t", "genProbsM_t", "genProbsF_t"):
        np.testing.assert_allclose(got[f], ref[f], rtol=RTOL, atol=1e-14, err_msg=f"{name}: {f}")


def compare_alone(got, c):
    ref = cc.oracle_ref(c)
    if c.mode == "nipt":
        compare_outputs(got, ref, c.name)
    else:
        gibbs_compare(got, ref, c.Ks)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_group_in_one_call_and_chain_by_chain(devs, group):
    cs = GROUPS[group]
    dev = devs(cs[0].panel)
    got = batch_call(dev, cs)
    for g, c in zip(got, cs):
        compare_outputs(g, cc.oracle_ref(c), c.name)
        one = single_call(dev, c)
        compare_alone(one, c)
        for f in OUT_FIELDS:
            assert np.array_equal(g[f], one[f]), (c.name, f)


# ---------------------------------------------------------------------------------------------------------------------------
# the builds of the samplers at Ksubset = 600: several waves per chain (wave 0 stores H / H_class, the others re-read them at the
# refill), and the 256-register builds (eMatGrid in LDS, columns fetched late)
# ---------------------------------------------------------------------------------------------------------------------------
BIG = cc.big_build_cases()
# (one chain at Ksubset = 600 runs two waves by default, and the 256-register builds exist for one wave only: gibbs.hip
# choose_gibbs_waves / launch_gibbs_sweeps, gibbs3.hip gibbs3_waves -- so the lean rows force one wave, and the one-wave rows
# without them are the kernels that launches of 896 chains run)
DIPLOID_BUILDS = [{"QA_GIBBS_NW": "1", "QA_GIBBS_LEAN": "0"}, {"QA_GIBBS_NW": "2"}, {"QA_GIBBS_NW": "5"}, {"QA_GIBBS_NW": "10"},
                  {"QA_GIBBS_NW": "1", "QA_GIBBS_LEAN": "1"}]
NIPT_BUILDS = [{"QA_GIBBS_NW": "1", "QA_GIBBS3_LEAN": "0"}, {"QA_GIBBS_NW": "2"}, {"QA_GIBBS_NW": "1", "QA_GIBBS3_LEAN": "1"}]
LEAN_KERNEL, PLAIN_KERNEL = "k_gibbs<10, 1, true>", "k_gibbs"   # the profile slots of the two-label sweeps (csrc/panel.hip)
build_id = lambda env: ",".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.parametrize("family", ["grids", "runs"])
@pytest.mark.parametrize("env", DIPLOID_BUILDS, ids=build_id)
def test_diploid_builds_at_ks600(devs, monkeypatch, env, family):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cs = [c for c in BIG if c.spec.family == family and c.mode != "nipt"]
    assert len(cs) >= 20 and all(c.Ks == cc.KS_BIG for c in cs)
    from quilt_amd.native import lib
    lib().qa_profile_reset()
    for c in cs:
        compare_alone(single_call(devs(c.panel), c), c)
    # the hook took: every sweep launch went to the 256-register build, or none did
    lean = env.get("QA_GIBBS_LEAN") == "1"
    assert (launches(LEAN_KERNEL) > 0) == lean and (launches(PLAIN_KERNEL) > 0) == (not lean)


@pytest.mark.parametrize("family", ["grids", "runs"])
@pytest.mark.parametrize("env", NIPT_BUILDS, ids=build_id)
def test_nipt_builds_at_ks600(devs, monkeypatch, env, family):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cs = [c for c in BIG if c.spec.family == family and c.mode == "nipt"]
    assert len(cs) >= 10 and all(c.Ks == cc.KS_BIG for c in cs)
    for group in cc.groups(cs).values():
        for g, c in zip(batch_call(devs(group[0].panel), group), group):
            compare_outputs(g, cc.oracle_ref(c), c.name)


# ---------------------------------------------------------------------------------------------------------------------------
# counter-based uniforms: the read stream draws 64 at a time at its refill
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dip", "dip_iter", "nipt"])
def test_run_group_with_seeded_streams(devs, mode):
    """seed_reads / seed_shard: the device's streams are quilt_amd.rng.stream_uniform, fed to the oracle as arrays."""
    from oracle import oracle as O
    from quilt_amd.rng import stream_uniform
    cs = [c for c in cc.all_cases() if c.spec.family == "runs" and c.mode == mode and c.G == cc.G_RUNS]
    assert len(cs) >= 9 and len({c.group for c in cs}) == 1
    rng = np.random.default_rng(77)
    sr = [int(x) for x in rng.integers(0, 2 ** 62, size=len(cs))]
    ss = [int(x) for x in rng.integers(0, 2 ** 62, size=len(cs))]
    got = batch_call(devs(cs[0].panel), cs, seed_reads=sr, seed_shard=ss)
    n_pass = len(cc.BLOCK_ITS)
    for g, c, a, b in zip(got, cs, sr, ss):
        ru = stream_uniform(a, c.R * cc.N_ITS)
        if mode == "nipt":
            blk = stream_uniform(b, n_pass * 2 * c.R).reshape(n_pass, 2, c.R)
            ref = O.forwardBackwardGibbsNIPT(c.panel, c.sample, c.which, c.H0, ru, c.first_read, np.zeros(n_pass * c.G),
                                             runif_block=blk[:, 0, :].copy(), runif_resample=blk[:, 1, :].copy(), **c.kwargs())
        else:
            ref = O.forwardBackwardGibbsNIPT(c.panel, c.sample, c.which, c.H0, ru, c.first_read, stream_uniform(b, n_pass * (c.G - 1)),
                                             **c.kwargs())
        compare_outputs(g, ref, c.name)
        assert (ref["H"] != cc.oracle_ref(c)["H"]).any() or c.R < 10   # (other uniforms than the explicit ones: another chain)
