"""Cases for the Gibbs sampler's fp32 state mode (qa_panel_set_gibbs_state_bits(panel, 32); helper, no test; imports no device code).

The mode stores alphaHat_t and betaHat_t as fp32 and computes in fp64, so a read visit's probabilities move by a small relative
amount and a label can differ from the fp64 reference's only where a uniform lies that close to a threshold.  The cases are
chosen so that none does, and that choice is proven on the CPU with the reference alone (tests/test_state32_cases_cpu.py):

  E      the storage error of a column: the initial forward and backward recursions of every case (oracle/rtwin.py's
         _forward_haploid / _backward_haploid, which carry a column in fp64 from grid to grid as the kernels' registers do) with
         alpha and beta rounded to np.float32 at each store, against their fp64 output -- the largest relative deviation over the
         entries of normal fp32 range (below 2^-126 fp32 has no full mantissa, or flushes: the device bar's atol covers those).
  DELTA  max(1e-5, 20 E).  A case is admitted only if the reference returns identical H, H_class and state (rtol 1e-12) with
         runif_reads, runif_reads - DELTA and runif_reads + DELTA (clipped into (0, 1)), and likewise for runif_shard.

The seed of a case's reads, labels and uniforms is the first of 0 .. 63 that is admitted (search_seed), fixed in SEEDS.
The reference is the C oracle (qo_gibbs); for the block-wise shard pass, which it does not have, oracle/rtwin.py with
tests/shard_block_cases.py's pass in it.  Builders of tests/chain_cases.py, tests/rare_cases.py and tests/shard_block_cases.py
are used by import.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from oracle import rtwin
from tests import chain_cases as CC
from tests.util import sample_from_arrays

N_BURN, N_SAMPLE = 20, 1
N_ITS = N_BURN + N_SAMPLE
BLOCK_ITS = (3, 6, 9)
F32_MIN_NORMAL = 2.0 ** -126
NAMES = ("g1", "g2_ks1", "g65_ks63", "g65_ks65", "g129_ks600", "g129_ks640", "g40_ks1024", "g130_ks600_blocks", "rc_small",
         "readless_run")
# name -> (G, Ks, reads, panel haplotypes); rc_small and the block case take theirs from the builders they import
GEOMETRY = {"g1": (1, 40, 3, 300), "g2_ks1": (2, 1, 4, 300), "g65_ks63": (65, 63, 40, 300), "g65_ks65": (65, 65, 40, 300),
            "g129_ks600": (129, 600, 60, 700), "g129_ks640": (129, 640, 60, 700), "g40_ks1024": (40, 1024, 30, 1100),
            "readless_run": (70, 600, 24, 700)}
# the admitted seed of every case (search_seed; tests/test_state32_cases_cpu.py asserts the admission condition for it)
SEEDS = {"g1": 0, "g2_ks1": 0, "g65_ks63": 0, "g65_ks65": 0, "g129_ks600": 0, "g129_ks640": 0, "g40_ks1024": 0,
         "g130_ks600_blocks": 0, "rc_small": 0, "readless_run": 0}
MAX_SEEDS = 64


@dataclass
class Case:
    name: str
    seed: int
    panel: object
    sample: object
    which: np.ndarray
    H0: np.ndarray
    runif_reads: np.ndarray
    runif_shard: np.ndarray
    first_read: int = 0
    rc: object = None            # rc_small: the all-SNP side (quilt_amd.panel.RareCommon); sample then holds the all-SNP reads
    blocks: object = None        # g130_ks600_blocks: the tests.shard_block_cases.Case the planted table comes from
    Jmax: int = 10000
    _ref: dict = field(default_factory=dict, repr=False)

    @property
    def G(self):
        return self.rc.nGrids_all if self.rc is not None else self.panel.nGrids

    @property
    def Ks(self):
        return len(self.which)

    @property
    def tm(self):
        return np.asarray(self.rc.transMatRate_t_all if self.rc is not None else self.panel.transMatRate_t)

    def device_kwargs(self):
        """keywords of quilt_amd.gibbs_nipt's call beyond rare_common (a device handle: the test's)"""
        kw = dict(n_gibbs_burn_in_its=N_BURN, n_gibbs_sample_its=N_SAMPLE, block_gibbs_iterations=BLOCK_ITS, Jmax_local=self.Jmax)
        if self.blocks is not None:
            b = self.blocks
            kw.update(shard_check_every_pair=False, L_grid=b.L_grid, shuffle_bin_radius=b.radius, block_gibbs_quantile_prob=b.q)
        return kw


# ---------------------------------------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------------------------------------
def _uniforms(name, seed, R, G):
    rng = np.random.default_rng([seed, CC.zlib.crc32(name.encode()), 32])
    return (rng.integers(1, 3, size=R).astype(np.int32), rng.random(R * N_ITS), rng.random(len(BLOCK_ITS) * max(G - 1, 0)),
            int(rng.integers(0, max(R, 1))))


def _grids_of(name, G, R):
    if name == "g1":
        return np.zeros(R, dtype=np.int64)
    if name == "g2_ks1":
        return np.array([0, 0, 1, 1])
    if name == "readless_run":   # reads in grids 0 .. 3 and 66 .. 69 only: 62 read-less grids across the refill at grid 64
        return np.repeat(np.r_[0:4, 66:70], R // 8)
    return (np.arange(R) * G) // R


def _one_row_sample(panel, which, grids, rng):
    """Ks = 1 (tests.chain_cases.build_sample draws three haplotypes): reads of 1 .. 4 SNPs copied from the one haplotype."""
    bits = CC.read_cases.hap_bits(panel, which)[0]
    ptr, u, bq = [0], [], []
    for g in grids:
        lo, hi = 32 * int(g), min(32 * int(g) + 32, panel.nSNPs)
        t = np.sort(rng.choice(np.arange(lo, hi), size=int(rng.integers(1, 5)), replace=False))
        q = rng.integers(20, 31, size=len(t))
        ptr.append(ptr[-1] + len(t)); u.append(t); bq.append(np.where(bits[t] == 1, q, -q))
    return sample_from_arrays(ptr, np.concatenate(u), np.concatenate(bq), grids)


def _plain(name, seed):
    G, Ks, R, K = GEOMETRY[name]
    panel = CC.panel_of(CC._panel(G, K=K))
    which = CC.which_of(panel, Ks)
    grids = _grids_of(name, G, R)
    if Ks < 3:
        sample = _one_row_sample(panel, which, grids, np.random.default_rng([seed, 1, Ks]))
    else:
        sample = CC.build_sample(f"state32_{name}_{seed}", panel, which, grids)
    H0, ru, rs, fr = _uniforms(name, seed, sample.nReads, G)
    return Case(name, seed, panel, sample, which, H0, ru, rs, fr)


def _blocks(name, seed):
    """The planted table of tests/shard_block_cases.py's g130_ks600_end63 (boundaries 20, 63 and 100 keep a haplotype with
    probability 1e-3, each in a gap wider than the smoothing window) under 60 reads and this file's 21 sweeps."""
    from tests import shard_block_cases as SB
    b = SB._make(name, 702 + 10 * seed, G=130, K=700, Ks=600, n_reads=60, planted=(20, 63, 100), q=0.95, radius=5000, spacing=3000,
                 gap=50000, plant_uniforms=False)
    H0, ru, rs, fr = _uniforms(name, seed, b.sample.nReads, b.G)
    return Case(name, seed, b.panel, b.sample, b.which, H0, ru, rs, fr, blocks=b)


def _rare(name, seed):
    """tests/rare_cases.py's isolating layout on the all-SNP grid (one read per all-SNP grid and label) at Ks = 64."""
    from tests import rare_cases as RC
    c = RC.read_case("long_compact", 64)
    assert c.isolating and len(c.which) == 64
    _, ru, rs, fr = _uniforms(name, seed, c.sample.nReads, c.rc.nGrids_all)
    return Case(name, seed, RC.panel(), c.sample, c.which, c.H0.copy(), ru, rs, fr, rc=c.rc, Jmax=c.Jmax)


def build(name, seed):
    return {"g130_ks600_blocks": _blocks, "rc_small": _rare}.get(name, _plain)(name, seed)


@lru_cache(maxsize=None)
def case(name):
    return build(name, SEEDS[name])


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def _run_reference(c, ru, rs):
    if c.blocks is not None:
        from tests import shard_block_cases as SB
        b = c.blocks
        saved = rtwin.R_shard_block_gibbs_resampler
        rtwin.R_shard_block_gibbs_resampler = SB.blockwise_resampler(b.L_grid, b.radius, b.q, c.panel.nSNPs)
        try:
            out = rtwin.forwardBackwardGibbsNIPT(c.panel, c.sample, c.which, c.H0, ru, c.first_read, n_gibbs_burn_in_its=N_BURN,
                                                 n_gibbs_sample_its=N_SAMPLE, block_gibbs_iterations=BLOCK_ITS, runif_shard=rs)
        finally:
            rtwin.R_shard_block_gibbs_resampler = saved
        out.setdefault("status", 0)
        return out
    from oracle import oracle as O
    kw = dict(rare_common=c.rc) if c.rc is not None else {}
    return O.forwardBackwardGibbsNIPT(c.panel, c.sample, c.which, c.H0, ru, c.first_read, rs, n_gibbs_burn_in_its=N_BURN,
                                      n_gibbs_sample_its=N_SAMPLE, block_gibbs_iterations=BLOCK_ITS, Jmax=c.Jmax, **kw)


def reference(c):
    """The whole call in fp64 on the CPU (once per case; shared between tests: do not write into it)."""
    if "base" not in c._ref:
        c._ref["base"] = _run_reference(c, c.runif_reads, c.runif_shard)
    return c._ref["base"]


STATE = ("alphaHat_t", "betaHat_t", "eMatGrid_t", "c")


def same_result(a, b, rtol=1e-12):
    """identical labels and classes, the state of the two labels within rtol; what differs first, or None"""
    if a.get("status", 0) != 0 or b.get("status", 0) != 0:
        return "status"
    for n in ("H", "H_class"):
        if not np.array_equal(a[n], b[n]):
            return n
    for n in STATE:
        for h in range(2):
            if not np.allclose(np.asarray(a[n][h]), np.asarray(b[n][h]), rtol=rtol, atol=0.0):
                return f"{n}[{h}]"
    return None


def _shift(u, d):
    return np.clip(u + d, 2.0 ** -60, 1 - 2.0 ** -53)


def admission(c, delta):
    """None when the case is admitted at ``delta``, else which perturbed run parted from the base run and where."""
    base = reference(c)
    if base.get("status", 0) != 0:
        return "the reference underflows"
    for what, d in (("runif_reads", -delta), ("runif_reads", delta), ("runif_shard", -delta), ("runif_shard", delta)):
        ru = _shift(c.runif_reads, d) if what == "runif_reads" else c.runif_reads
        rs = _shift(c.runif_shard, d) if what == "runif_shard" else c.runif_shard
        if what == "runif_shard" and len(rs) == 0:
            continue
        bad = same_result(base, _run_reference(c, ru, rs))
        if bad is not None:
            return f"{what} {d:+.1e}: {bad}"
    return None


def search_seed(name, delta):
    """The first seed of 0 .. MAX_SEEDS - 1 whose case is admitted (what SEEDS records), or None: a finding to report."""
    for seed in range(MAX_SEEDS):
        if admission(build(name, seed), delta) is None:
            return seed
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# E: the storage error of a column
# ---------------------------------------------------------------------------------------------------------------------------
def stored32(x):
    """what a column holds after an fp32 store and the widening load: rounded to nearest-even"""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def initial_recursions(c, store=lambda x: x):
    """alpha and beta of both labels after the call's initialisation (rcpp_make_eMatGrid_t, then rtwin's forward and backward
    recursions), every column passed through ``store`` as it is written.  The recursions carry the column they just formed in
    fp64 -- the kernels' registers -- so only what is stored is rounded."""
    ref = reference(c)
    eMatRead_t = np.asarray(ref["eMatRead_t"]) if "eMatRead_t" in ref else rtwin.make_eMatRead_t(c.panel, c.sample, c.which)
    K, G = c.Ks, c.G
    out = []
    for h in range(2):
        e = np.ones((K, G))
        for r in range(c.sample.nReads):
            if c.H0[r] == h + 1:
                e[:, c.sample.wif[r]] *= eMatRead_t[:, r]
        a, cc = rtwin._forward_haploid(e, c.tm, K)
        b = np.zeros((K, G))
        b[:, G - 1] = cc[G - 1]
        b = rtwin._backward_haploid(b, cc, e, c.tm, K)
        out.append((store(a), store(b)))
    return out


def storage_error(c):
    """largest relative deviation of the fp32-stored initial alpha / beta from the fp64 ones, over entries of normal fp32 range"""
    worst = 0.0
    for (a64, b64), (a32, b32) in zip(initial_recursions(c), initial_recursions(c, stored32)):
        for x64, x32 in ((a64, a32), (b64, b32)):
            ok = np.abs(x64) >= F32_MIN_NORMAL
            if ok.any():
                worst = max(worst, float(np.max(np.abs(x32[ok] - x64[ok]) / np.abs(x64[ok]))))
    return worst


@lru_cache(maxsize=None)
def E():
    return max(storage_error(case(n)) for n in NAMES)


def DELTA():
    return max(1e-5, 20 * E())
