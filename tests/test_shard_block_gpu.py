"""The block-wise shard pass (QUILT(shard_check_every_pair = FALSE), diploid) on the device against the CPU reference of
tests/shard_block_cases.py: labels and classes identical, the state at the bars of tests/test_rtwin_gpu.py.  The conditions that
make the comparison of decisions exact are checked on the CPU (tests/test_shard_block_cases_cpu.py).  Then what the mode adds to
the call: entries of runif_shard that must not be read, the three sources of the passes' uniforms, several chains in one call,
and the refusals."""
import dataclasses

import numpy as np
import pytest

from tests import shard_block_cases as SB

pytestmark = pytest.mark.gpu

NAMES = ["g40_readless", "g130_ks600_end63", "g130_ks40_end64", "g40_ks600_one_block"]
_DEV, _GOT = {}, {}


def _device(case):
    from quilt_amd.native import DevicePanel
    if case.name not in _DEV:
        _DEV[case.name] = DevicePanel(case.panel)
    return _DEV[case.name]


def _run(case, runif_shard, **kw):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    return rcpp_forwardBackwardGibbsNIPT(_device(case), case.sample, case.which, case.H0, case.runif_reads, case.first_read,
                                         runif_shard, shard_check_every_pair=False, return_state=True, **{**case.kwargs(), **kw})


def _explicit(case):
    """the case with its explicit uniforms (run once per process)"""
    if case.name not in _GOT:
        _GOT[case.name] = _run(case, case.runif_shard)
    return _GOT[case.name]


STATE = ("alphaHat_t1", "alphaHat_t2", "betaHat_t1", "betaHat_t2", "eMatGrid_t1", "eMatGrid_t2", "c1", "c2", "hapProbs_t",
         "genProbsM_t", "genProbsF_t")


def _same_call(a, b):
    assert np.array_equal(a["H"], b["H"]) and np.array_equal(a["H_class"], b["H_class"])
    for n in STATE:
        if n in a or n in b:
            assert np.array_equal(a[n], b[n]), n


def _matches_reference(case, got):
    ref = case.reference()
    assert not got["underflow_problem"]
    assert np.array_equal(got["H"], ref["H"]), f"{(got['H'] != ref['H']).sum()} labels differ"
    assert np.array_equal(got["H_class"], ref["H_class"])
    for h in range(2):
        np.testing.assert_allclose(got[f"alphaHat_t{h + 1}"], ref["alphaHat_t"][h], rtol=1e-8, atol=1e-300)
        np.testing.assert_allclose(got[f"betaHat_t{h + 1}"], ref["betaHat_t"][h], rtol=1e-8, atol=1e-300)
        np.testing.assert_allclose(got[f"c{h + 1}"], ref["c"][h], rtol=1e-8)
        np.testing.assert_allclose(got[f"eMatGrid_t{h + 1}"], ref["eMatGrid_t"][h], rtol=1e-8)
    np.testing.assert_allclose(got["hapProbs_t"][:2], ref["hapProbs_t"][:2], rtol=1e-8, atol=1e-14)


@pytest.mark.parametrize("name", NAMES)
def test_case_matches_the_reference(name):
    case = SB.cases()[name]
    _matches_reference(case, _explicit(case))


@pytest.mark.parametrize("hook,value", [("QA_GIBBS_LEAN", "1"), ("QA_GIBBS_NW", "2"), ("QA_GIBBS_NW", "5"), ("QA_GIBBS_NW", "10")])
def test_every_build_of_the_production_geometry_matches_the_reference(hook, value, monkeypatch):
    """Ks = 600 runs as the 256-register build when a launch carries more than 1 024 chains (QA_GIBBS_LEAN = 1 forces it for one
    chain: eMatGrid's columns in LDS, late loads, and the segments resumed past the initialisation) and as 2, 5 or 10 waves per
    chain (QA_GIBBS_NW): the segmented sweeps and k_shard_blocks of each build against the reference."""
    monkeypatch.setenv(hook, value)
    case = SB.cases()["g130_ks600_end63"]
    _matches_reference(case, _run(case, case.runif_shard))


def test_the_mode_differs_from_every_pair():
    """(the cases would show nothing if deciding at every grid gave the same call)"""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    case = SB.cases()["g130_ks40_end64"]
    every = rcpp_forwardBackwardGibbsNIPT(_device(case), case.sample, case.which, case.H0, case.runif_reads, case.first_read,
                                          case.runif_shard, **case.kwargs())
    assert not np.array_equal(every["H"], _explicit(case)["H"])


@pytest.mark.parametrize("name", NAMES)
def test_entries_beyond_the_blocks_are_not_read(name):
    case = SB.cases()[name]
    rs = SB.nan_beyond_blocks(case)
    assert np.isnan(rs).any()
    _same_call(_run(case, rs), _explicit(case))


@pytest.mark.parametrize("name", ["g130_ks600_end63", "g40_readless", "g40_ks600_one_block"])
def test_callback_is_asked_for_the_blocks_uniforms(name):
    """qa_gibbs_opts_t.draw_uniforms, what = 2: n_blocks - 1 values before each pass, never 0, and the same call."""
    case = SB.cases()[name]
    G, asked = case.G, []

    def draw(chain, pass_, what, n):
        asked.append((chain, pass_, what, n))
        return case.runif_shard[pass_ * (G - 1):pass_ * (G - 1) + n]

    got = _run(case, None, draw_uniforms=draw)
    want = [(0, j, 2, t["n_blocks"] - 1) for j, t in enumerate(case.reference()["trace"]) if t["n_blocks"] > 1]
    assert asked == want and all(a[3] > 0 for a in asked)
    _same_call(got, _explicit(case))


def test_a_failing_callback_fails_the_call():
    case = SB.cases()["g40_readless"]
    with pytest.raises(ValueError, match="returned 0 values"):
        _run(case, None, draw_uniforms=lambda chain, pass_, what, n: [])

    def boom(chain, pass_, what, n):
        raise KeyError("boom")
    with pytest.raises(KeyError):
        _run(case, None, draw_uniforms=boom)


def test_seeds_give_the_call_of_their_expanded_streams():
    """seed_reads / seed_shard: block b of pass j takes element j * (G - 1) + b of the shard stream."""
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.rng import stream_uniform
    case = SB.cases()["g130_ks40_end64"]
    G, R, n_its = case.G, case.sample.nReads, SB.N_BURN + SB.N_SAMPLE
    sr, ss = 0x1234567, 0x89abcde
    ru = stream_uniform(sr, R * n_its)
    rs = stream_uniform(ss, len(SB.BLOCK_ITS) * (G - 1))
    dev = _device(case)
    common = dict(shard_check_every_pair=False, return_state=True, **case.kwargs())
    seeded = rcpp_forwardBackwardGibbsNIPT(dev, case.sample, case.which, case.H0, None, case.first_read, None,
                                           seed_reads=[sr], seed_shard=[ss], **common)
    explicit = rcpp_forwardBackwardGibbsNIPT(dev, case.sample, case.which, case.H0, ru, case.first_read, rs, **common)
    _same_call(seeded, explicit)


def test_chains_of_one_call_equal_their_own_calls():
    """Four chains in one call: three with different block tables, one of them with a single read, and one without reads (one
    block over every grid: its pass is the forward and backward recomputation, and it is asked for no uniform)."""
    from quilt_amd.gibbs_nipt import forwardBackwardGibbsNIPT_batch
    case = SB.cases()["g130_ks40_end64"]
    samples = SB.multi_chain_samples(case)
    assert samples[2].nReads == 1 and samples[3].nReads == 0
    rng = np.random.default_rng(9)
    n_its, G = SB.N_BURN + SB.N_SAMPLE, case.G
    whichs = [np.sort(rng.choice(case.panel.K, len(case.which), replace=False)).astype(np.int32) + 1 for _ in samples]
    H0s = [rng.integers(1, 3, size=s.nReads).astype(np.int32) for s in samples]
    rus = [rng.random(s.nReads * n_its) for s in samples]
    rss = [rng.random(len(SB.BLOCK_ITS) * (G - 1)) for _ in samples]
    frs = [0 for _ in samples]
    n_asked = {}

    def draw(chain, pass_, what, n):
        n_asked[(pass_, chain)] = n
        return rss[chain][pass_ * (G - 1):pass_ * (G - 1) + n]

    dev = _device(case)
    kw = dict(shard_check_every_pair=False, **case.kwargs())
    together = forwardBackwardGibbsNIPT_batch(dev, samples, whichs, H0s, rus, frs, rss, **kw)
    alone = [forwardBackwardGibbsNIPT_batch(dev, [samples[c]], [whichs[c]], [H0s[c]], [rus[c]], [frs[c]], [rss[c]], **kw)[0]
             for c in range(3)]
    for a, b in zip(together, alone):
        _same_call(a, b)
    # (a launch needs a read somewhere: the chain without reads in another call, beside another chain)
    sel = [3, 2]
    other = forwardBackwardGibbsNIPT_batch(dev, *[[x[c] for c in sel] for x in (samples, whichs, H0s, rus, frs, rss)], **kw)
    _same_call(other[0], together[3])
    _same_call(other[1], together[2])
    # (the callback form of the same call tells the chains' numbers of blocks: they differ)
    asked = forwardBackwardGibbsNIPT_batch(dev, samples, whichs, H0s, rus, frs, [None] * len(samples), draw_uniforms=draw, **kw)
    for a, b in zip(asked, together):
        _same_call(a, b)
    assert list(n_asked) == sorted(n_asked), "pass by pass, chain by chain within a pass"
    per_chain = [tuple(n_asked.get((j, c), 0) for j in range(len(SB.BLOCK_ITS))) for c in range(3)]
    assert len(set(per_chain)) == 3, per_chain
    assert not any(c == 3 for _, c in n_asked), "the chain without reads has nothing to decide"


def test_null_L_grid_is_refused():
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.native import DevicePanel, QuiltAmdError
    case = SB.cases()["g40_readless"]
    dev = DevicePanel(dataclasses.replace(case.panel, L_grid=None))
    kw = {**case.kwargs(), "L_grid": None}
    with pytest.raises(QuiltAmdError) as e:
        rcpp_forwardBackwardGibbsNIPT(dev, case.sample, case.which, case.H0, case.runif_reads, case.first_read, case.runif_shard,
                                      shard_check_every_pair=False, **kw)
    assert e.value.status == -2 and "L_grid" in str(e.value)
    # (and the same call with every pair decided needs none)
    rcpp_forwardBackwardGibbsNIPT(dev, case.sample, case.which, case.H0, case.runif_reads, case.first_read, case.runif_shard, **kw)
    dev.close()


def test_rare_common_call_refuses_the_flag(small_panel):
    from quilt_amd.gibbs_nipt import rcpp_forwardBackwardGibbsNIPT
    from quilt_amd.native import DevicePanel, DeviceRareCommon, QuiltAmdError
    from quilt_amd.synth import make_rare_common, make_synthetic_sample_rare_common
    rc = make_rare_common(small_panel, 23)
    _, s_all = make_synthetic_sample_rare_common(small_panel, rc, 24, n_reads=60)
    rng = np.random.default_rng(1)
    which = np.sort(rng.choice(small_panel.K, 64, replace=False)).astype(np.int32) + 1
    H0 = rng.integers(1, 3, size=s_all.nReads).astype(np.int32)
    ru, rs = rng.random(s_all.nReads * 21), rng.random(3 * (rc.nGrids_all - 1))
    dev = DevicePanel(small_panel)
    drc = DeviceRareCommon(dev, rc)
    H_before = H0.copy()
    with pytest.raises(QuiltAmdError) as e:
        rcpp_forwardBackwardGibbsNIPT(dev, s_all, which, H0, ru, 0, rs, rare_common=drc, shard_check_every_pair=False)
    assert e.value.status == -3 and "shard_by_blocks" in str(e.value)
    assert np.array_equal(H0, H_before)
    drc.close()
    dev.close()
