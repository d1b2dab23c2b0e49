"""Constructed chains for the Gibbs samplers' own chunk constants (helper, no test; imports no device code).

k_gibbs / k_gibbs3 / k_block3 keep every per-grid and per-read scalar in lane-held streams of 64 (csrc/gibbs_dev.hpp: GridStreams,
GridStreams3, ReadStreams): one vector load per 64 grids or reads, a refill at (g & 63) == 0 going right and at (g & 63) == 63 going
left, a store of the labels by wave 0 before the read stream is refilled, a prefetch of the next read's emission whose entry count
comes from the lane unless the read opens a stream block.  Random samples put nothing ON such an index; the builders here do: the
number of grids and reads either side of 64 and 128, a grid's run of reads that ends, starts or lies across a refill, read-less
runs across it, skipped (category 1) reads at stream positions 63, 0 and 64, dense next to compact emissions across it, and for
the NIPT block pass planted block tables whose blocks end at grids 62 .. 65.

A ``ChainCase`` is one chain of one call: panel, reads, the haplotype subset, starting labels, every uniform the call takes, the
keywords, and ``claims`` -- what the builder says about its input.  tests/test_chain_cases_cpu.py proves every claim from the
arrays and the oracle alone; tests/test_chain_geometry_gpu.py runs the cases on the device.  A *spec* is the geometry (panel and
reads); every spec gives a diploid case with each initialisation (shard passes on) and a NIPT case (ff = 0.2, block passes after
sweeps 3, 6 and 9), except the block-table specs, which are NIPT only.
"""
from __future__ import annotations

import copy
import zlib
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from tests import grid_cases, read_cases
from tests.util import sample_from_arrays

STREAM = 64                 # gibbs_dev.hpp: elements per lane-held stream
MAX_PATTERN_BITS = read_cases.MAX_PATTERN_BITS   # a read with more informative SNPs has a dense emission column
KS = 70                     # two rows per lane, 58 lanes of the last row masked
KS_BIG, K_BIG = 600, 700    # the production geometry (ten rows per lane; several waves per chain exist only there)
FF = 0.2
BLOCK_ITS = (3, 6, 9)
N_ITS = 21                  # 20 burn-in sweeps and one sampling sweep: the calls' defaults
CROWDED = 30                # a grid with more reads than this gets weak reads: strong ones would underflow its emission product
G_COUNTS = (1, 2, 3, 63, 64, 65, 128, 129)
R_COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129)
G_RUNS = 65
FIRST_READS_ITER = (0, 63, 64, 128)   # at R = 129: R - 1 = 128
MODES = ("dip", "dip_iter", "nipt")
PLANTED_SIGMA = 1e-3        # tests/shard_block_cases.py: a planted boundary keeps a haplotype with this probability
BLOCK_G = 130
BLOCK_RADIUS, BLOCK_SPACING, BLOCK_GAP = 1000, 3000, 50000   # the smoothing window never leaves a boundary's own segment

# The seed of a case's reads and uniforms where it is not 0: the first of 0, 1, 2 ... for which the ORACLE satisfies what
# tests/test_chain_cases_cpu.py asks of the case (status 0, labels that move, passes that matter on both sides of read 64, natural switch rates below 1 at the first block pass).
# A spec's name seeds its reads, a case's name ("spec:mode") its starting labels and uniforms.
SEEDS = {"runs_one_per_grid": 2, "runs_one_per_grid:dip_iter": 1, "runs_end63_start64:dip": 1, "runs_crowd70_g30:dip": 1,
         "runs_crowd70_g63_g64:dip_iter": 2, "runs_all_on_last:dip": 11, "runs_all_on_last:dip_iter": 2, "runs_only_lt64:dip": 3,
         "runs_readless_62_65:dip_iter": 2, "blocks_end63_end65:nipt": 1, "blocks_readless_runs:nipt": 2, "blocks_last_read_quirk:nipt": 1}


@dataclass
class Spec:
    """The geometry of a chain.  Listing the specs costs nothing: the panel, the haplotype subset and the reads are made when a
    test first asks for them, so that collecting these files does not build 240 chains for a run that deselects them."""
    name: str
    family: str               # grids | reads | runs | skipped | forms | blocks | first_read
    panel_key: tuple          # what panel_of builds: ("base", G, T, K) or ("block", planted boundaries)
    Ks: int
    grids: np.ndarray         # the grid of every read
    kinds: dict = field(default_factory=dict)   # read -> "cat1" | "dense" | "compact"
    claims: dict = field(default_factory=dict)
    kw: dict = field(default_factory=dict)      # keywords of both calls (L_grid, radius, quantile, read categories off)
    modes: tuple = MODES
    first_read: int = None    # fixed (the first-read cases); otherwise drawn
    _sample: object = field(default=None, repr=False)

    @property
    def G(self):
        return BLOCK_G if self.panel_key[0] == "block" else self.panel_key[1]

    @property
    def T(self):
        return 32 * BLOCK_G if self.panel_key[0] == "block" else self.panel_key[2]

    @property
    def panel(self):
        return panel_of(self.panel_key)

    @property
    def which(self):
        return which_of(self.panel, self.Ks)

    @property
    def sample(self):         # quilt_amd.synth.SampleReads
        if self._sample is None:
            self._sample = build_sample(self.name, self.panel, self.which, self.grids, self.kinds)
        return self._sample


@dataclass
class ChainCase:
    name: str
    spec: Spec
    mode: str
    H0: np.ndarray
    runif_reads: np.ndarray
    runif_shard: np.ndarray   # diploid: 3 x (G - 1)
    runif_block: np.ndarray   # NIPT: 3 x R
    runif_resample: np.ndarray
    first_read: int
    group: str                # cases of one group share panel, Ks and keywords: one forwardBackwardGibbsNIPT_batch call

    @property
    def panel(self):
        return self.spec.panel

    @property
    def sample(self):
        return self.spec.sample

    @property
    def which(self):
        return self.spec.which

    @property
    def claims(self):
        return self.spec.claims

    @property
    def ff(self):
        return FF if self.mode == "nipt" else 0.0

    @property
    def R(self):
        return len(self.spec.grids)

    @property
    def G(self):
        return self.spec.G

    @property
    def Ks(self):
        return self.spec.Ks

    def kwargs(self):
        """keywords both the oracle's and the device's call take"""
        kw = dict(self.spec.kw)
        kw["gibbs_initialize_iteratively"] = self.mode == "dip_iter"
        if self.mode == "nipt":
            kw["ff"] = FF
        return kw


# ---------------------------------------------------------------------------------------------------------------------------
# reads
# ---------------------------------------------------------------------------------------------------------------------------
def _rng(name, salt=0):
    return np.random.default_rng([SEEDS.get(name, 0), zlib.crc32(name.encode()), salt])


_which = {}


def which_of(panel, Ks):
    if (id(panel), Ks) not in _which:
        _which[id(panel), Ks] = read_cases.which_for(panel, Ks)
    return _which[id(panel), Ks]


def monomorphic(panel, which):
    """bool [T]: every chosen haplotype carries the same allele (a read over such SNPs alone is category 1)."""
    b = read_cases.hap_bits(panel, which)
    return (b == b[0]).all(axis=0)


def build_sample(name, panel, which, grids, kinds=None):
    """One read per entry of ``grids`` (non-decreasing), each of 1 .. 7 SNPs inside its grid, copied from one of three chosen
    haplotypes.  ``kinds[r]``: "cat1" -- SNPs on which the chosen haplotypes agree; "dense" / "compact" -- 6 or 7 against 1 .. 5
    SNPs; every other read holds at least one SNP on which they differ (where its grid has one), so that it is not category 1 by
    accident.  Base qualities 20 .. 30, and 1 .. 6 on a grid that holds more than CROWDED reads."""
    kinds = kinds or {}
    grids = np.asarray(grids, dtype=np.int64)
    assert (np.diff(grids) >= 0).all() and (len(grids) == 0 or (grids[0] >= 0 and grids[-1] < panel.nGrids))
    rng = _rng(name, 1)
    bits = read_cases.hap_bits(panel, which)
    mono = monomorphic(panel, which)
    truth = bits[rng.choice(len(which), 3, replace=False)]
    per_grid = np.bincount(grids, minlength=panel.nGrids)
    ptr, u, bq = [0], [], []
    for r, g in enumerate(grids):
        lo, hi = 32 * int(g), min(32 * int(g) + 32, panel.nSNPs)
        snps = np.arange(lo, hi)
        poly, same = snps[~mono[lo:hi]], snps[mono[lo:hi]]
        kind = kinds.get(r, "any")
        if kind == "cat1":
            assert len(same), (name, r, int(g))
            t = rng.choice(same, size=min(len(same), int(rng.integers(1, 4))), replace=False)
        else:
            n = {"dense": int(rng.integers(MAX_PATTERN_BITS + 1, 8)), "compact": int(rng.integers(1, MAX_PATTERN_BITS + 1))}.get(
                kind, int(rng.integers(1, 8)))
            n = min(n, len(snps))
            assert kind != "dense" or n > MAX_PATTERN_BITS, (name, r)
            t = rng.choice(snps, size=n, replace=False)
            if len(poly) and mono[t].all():
                t[0] = rng.choice(poly)
        t = np.sort(t)
        q = rng.integers(1, 7, size=len(t)) if per_grid[g] > CROWDED else rng.integers(20, 31, size=len(t))
        label = rng.choice(3, p=[0.5, 0.4, 0.1])
        ptr.append(ptr[-1] + len(t))
        u.append(t)
        bq.append(np.where(truth[label][t] == 1, q, -q))
    cat = lambda x: np.concatenate(x) if x else np.zeros(0, dtype=np.int64)
    s = sample_from_arrays(ptr, cat(u), cat(bq), grids)
    # (the ABI's grid of a read is that of its central SNP: every SNP of a read lies in one grid here)
    assert all(int(s.u[(s.read_ptr[r] + s.read_ptr[r + 1] - 1) // 2]) // 32 == s.wif[r] for r in range(s.nReads))
    return s


def per_grid_counts(counts):
    """grids of the reads from {grid: count} (ascending)"""
    return np.repeat(sorted(counts), [counts[g] for g in sorted(counts)])


# ---------------------------------------------------------------------------------------------------------------------------
# specs
# ---------------------------------------------------------------------------------------------------------------------------
def _panel(G, T=None, K=grid_cases.K_BASE):
    """the key of a plain panel (panel_of builds it)"""
    return ("base", G, 32 * G if T is None else T, K)


@lru_cache(maxsize=None)
def panel_of(key):
    if key[0] == "block":
        return _block_panel(key[1])
    return grid_cases.base_panel(key[1], key[2], K=key[3], seed=8100)


def _spec(name, family, panel_key, grids, Ks=KS, kinds=None, claims=None, **kw):
    return Spec(name, family, panel_key, Ks, np.asarray(grids, dtype=np.int64), dict(kinds or {}), dict(claims or {}), **kw)


def grid_count_specs(Ks=KS):
    """G grids over 32 G SNPs, or over 32 (G - 1) + 1 so that the last grid holds one SNP; two reads on every grid."""
    out = []
    sfx = "" if Ks == KS else f"_ks{Ks}"
    for G in G_COUNTS:
        for T in (32 * G, 32 * (G - 1) + 1):
            p = _panel(G, T, K=grid_cases.K_BASE if Ks == KS else K_BIG)
            out.append(_spec(f"grids_G{G}_T{T}{sfx}", "grids", p, np.repeat(np.arange(G), 2), Ks,
                             claims=dict(G=G, T=T, last_grid_snps=T - 32 * (G - 1), R=2 * G)))
    return out


def read_count_specs():
    p = _panel(G_RUNS)
    return [_spec(f"reads_R{R}", "reads", p, (np.arange(R) * G_RUNS) // R, claims=dict(R=R, G=G_RUNS)) for R in R_COUNTS]


def run_layouts():
    """name -> (G, {grid: reads}, claims): where a grid's run of reads meets a stream refill.  ``runs``: (grid, first read, last
    read) of the runs the case is about; ``readless``: grids without reads that it is about."""
    G = G_RUNS
    one = lambda grids: {g: 1 for g in grids}
    out = {}
    out["end63_start64"] = (G, {**one(range(54)), 54: 10, 55: 5, **one(range(56, G))}, dict(runs=((54, 54, 63), (55, 64, 68))))
    out["straddle64"] = (G, {**one(range(59)), 59: 10, **one(range(60, G))}, dict(runs=((59, 59, 68),)))
    out["crowd70_g30"] = (G, {**{g: 2 for g in range(30)}, 30: 70, **one(range(31, G))}, dict(runs=((30, 60, 129),)))
    out["crowd70_g63_g64"] = (G, {**one(range(60)), 63: 70, 64: 40}, dict(runs=((63, 60, 129), (64, 130, 169)), readless=(60, 61, 62)))
    out["all_on_g0"] = (G, {0: 70}, dict(runs=((0, 0, 69),), readless=tuple(range(1, G))))
    out["all_on_last"] = (G, {G - 1: 70}, dict(runs=((G - 1, 0, 69),), readless=tuple(range(G - 1))))
    # grids >= 64 of 65 are grid 64 alone; unlike all_on_last the run also lies across read 128
    out["only_ge64"] = (G, {G - 1: 130}, dict(runs=((G - 1, 0, 129),), readless=tuple(range(64))))
    out["only_lt64"] = (G, {g: 2 for g in range(64)}, dict(readless=(64,)))
    # (a run over grids 62 .. 65 needs grids beyond 65: on the 129-grid panel, where it lies across the refill at grid 64)
    out["readless_62_65"] = (129, {g: 1 for g in range(129) if not 62 <= g <= 65}, dict(readless=(62, 63, 64, 65)))
    out["one_per_grid"] = (G, one(range(G)), dict(one_per_grid=True))
    out["G129_five_on_last"] = (129, {128: 5}, dict(runs=((128, 0, 4),), readless=tuple(range(128))))
    return out


def run_specs(Ks=KS):
    sfx = "" if Ks == KS else f"_ks{Ks}"
    out = []
    for name, (G, counts, claims) in run_layouts().items():
        p = _panel(G, K=grid_cases.K_BASE if Ks == KS else K_BIG)
        out.append(_spec(f"runs_{name}{sfx}", "runs", p, per_grid_counts(counts), Ks, claims=dict(claims, G=G)))
    return out


SKIPPED = dict(at0=(0,), at63=(63,), at64=(64,), last=(129,), both_63_64=(63, 64))


def skipped_specs():
    """G = 65, two reads per grid (R = 130): category-1 reads at the named positions -- 0 and 64 open a grid's run (and a stream
    block), 63 closes a block, 129 is the chain's last read.  Once more with disable_read_category_usage."""
    p = _panel(G_RUNS)
    grids = np.repeat(np.arange(G_RUNS), 2)
    out = []
    for name, pos in SKIPPED.items():
        for nocat in (False, True):
            out.append(_spec(f"skipped_{name}" + ("_nocat" if nocat else ""), "skipped", p, grids, kinds={r: "cat1" for r in pos},
                             claims=dict(cat1=tuple(pos), nocat=nocat, G=G_RUNS),
                             kw=dict(disable_read_category_usage=True) if nocat else {}))
    return out


def form_specs():
    """Reads 63 and 64 of the chain in opposite emission forms, both ways round."""
    p = _panel(G_RUNS)
    grids = np.repeat(np.arange(G_RUNS), 2)
    return [_spec(f"forms_63{a}_64{b}", "forms", p, grids, kinds={63: a, 64: b}, claims=dict(forms={63: a, 64: b}, G=G_RUNS))
            for a, b in (("dense", "compact"), ("compact", "dense"))]


def first_read_specs():
    """R = 129 on G = 65: the iterative initialisation from reads 0, 63, 64 and R - 1."""
    p = _panel(G_RUNS)
    return [_spec(f"first_read_{fr}", "first_read", p, (np.arange(129) * G_RUNS) // 129, claims=dict(R=129, first_read=fr, G=G_RUNS),
                  modes=("dip_iter",), first_read=fr) for fr in FIRST_READS_ITER]


def big_specs():
    """One case per mode at G = 129 with K = 700 / Ks = 600."""
    p = _panel(129, K=K_BIG)
    return [_spec("big_G129_ks600", "grids", p, np.repeat(np.arange(129), 2), KS_BIG, claims=dict(G=129, T=32 * 129, last_grid_snps=32, R=258))]


def one_read_specs():
    """A single read, at the grid counts the oracle died on with block passes (2 and 65 before the fix; 65 is reads_R1)."""
    return [_spec("one_read_G2", "reads", _panel(2), [1], claims=dict(R=1, G=2))]


# ---- planted block tables (NIPT) -------------------------------------------------------------------------------------------
BLOCK_LAYOUTS = dict(
    end62_end64=dict(planted=(62, 64), ends=(62, 64, 129)),
    end63_end65=dict(planted=(63, 65), ends=(63, 65, 129)),
    one_block=dict(planted=(), ends=(129,)),
    reads_straddle64=dict(planted=(30, 99), ends=(30, 99, 129)),
    # blocks 51-55 and 56-60 are without reads and shared out at the midpoint of 51 .. 60, likewise 71-75 and 76-80
    readless_runs=dict(planted=(50, 55, 60, 70, 75, 80), no_reads=((51, 60), (71, 80)), ends=(55, 75, 129)),
    # reads 0 .. 201 on grids 0 .. 100 and read 202 alone beyond the cut at 100: block 41-100 is never recorded, its reads
    # 82 .. 201 go to the last block and its grids are shared out at the midpoint (gibbs-nipt-block.cpp:1398-1400)
    last_read_quirk=dict(planted=(40, 100), reads_to=100, last_read_on=120, ends=(70, 129), reads=((0, 81), (82, 202))),
)


def block_panel(planted):
    return ("block", tuple(planted))


def _block_panel(planted):
    """The 130-grid panel with the transition across every planted boundary keeping a haplotype with probability 1e-3."""
    p = copy.copy(panel_of(_panel(BLOCK_G)))
    tm = np.array(p.transMatRate_t, order="F")
    for g in planted:
        tm[0, g], tm[1, g] = PLANTED_SIGMA, 1 - PLANTED_SIGMA
    p.transMatRate_t = tm
    return p


def block_specs():
    from tests.shard_block_cases import positions
    out = []
    G = BLOCK_G
    for name, lay in BLOCK_LAYOUTS.items():
        planted = tuple(lay["planted"])
        p = block_panel(planted)
        grids = np.repeat(np.arange(G), 2)
        for lo, hi in lay.get("no_reads", ()):
            grids = grids[(grids < lo) | (grids > hi)]
        if "reads_to" in lay:
            grids = np.r_[grids[grids <= lay["reads_to"]], lay["last_read_on"]]
        n = G - 1
        # the quantile's index lands on the smallest planted rate (about 3), the threshold is capped at 1 and every natural
        # rate lies below it; without a planted boundary the quantile is the largest rate and nothing is above it
        q = (n - len(planted) + 0.5) / n if planted else 0.999
        kw = dict(L_grid=positions(G, BLOCK_SPACING, planted, BLOCK_GAP), shuffle_bin_radius=BLOCK_RADIUS, block_gibbs_quantile_prob=q)
        out.append(_spec(f"blocks_{name}", "blocks", p, grids, claims=dict(planted=planted, G=G, ends=tuple(lay["ends"]), **({"reads": lay["reads"]} if "reads" in lay else {})),
                         kw=kw, modes=("nipt",)))
    return out


@lru_cache(maxsize=None)
def all_specs():
    out = (grid_count_specs() + read_count_specs() + run_specs() + skipped_specs() + form_specs() + first_read_specs() +
           one_read_specs() + big_specs() + block_specs())
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return tuple(out)


@lru_cache(maxsize=None)
def big_build_specs():
    """The grid-count and run specs at Ks = 600 (the build matrix: several waves per chain, the 256-register builds)."""
    return tuple(grid_count_specs(KS_BIG) + run_specs(KS_BIG))


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
def make_case(spec, mode):
    name = f"{spec.name}:{mode}"
    rng = _rng(name, 2)
    R, G = len(spec.grids), spec.G
    nipt = mode == "nipt"
    H0 = (rng.choice([1, 2, 3], p=[0.5, 0.4, 0.1], size=R) if nipt else rng.integers(1, 3, size=R)).astype(np.int32)
    ru, rs = rng.random(R * N_ITS), rng.random(len(BLOCK_ITS) * (G - 1))
    rb, rr = rng.random(len(BLOCK_ITS) * R), rng.random(len(BLOCK_ITS) * R)
    fr = int(rng.integers(0, max(R, 1))) if spec.first_read is None else spec.first_read
    group = f"{mode}|G{G}|T{spec.T}|Ks{spec.Ks}|{spec.claims.get('planted', '')}|{','.join(sorted(spec.kw))}"
    return ChainCase(name, spec, mode, H0, ru, rs, rb, rr, fr, group)


def _cases_of(specs):
    return tuple(make_case(s, m) for s in specs for m in s.modes)


@lru_cache(maxsize=None)
def all_cases():
    return _cases_of(all_specs())


@lru_cache(maxsize=None)
def big_build_cases():
    return _cases_of(big_build_specs())


def case(name):
    return {c.name: c for c in all_cases() + big_build_cases()}[name]


def groups(cases):
    out = {}
    for c in cases:
        out.setdefault(c.group, []).append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle on a case (computed once per case and variant; shared between tests: do not write into the results)
# ---------------------------------------------------------------------------------------------------------------------------
_ref = {}


def oracle_ref(c, **override):
    """The whole call on the CPU.  ``override``: keywords that replace the case's (perform_block_gibbs = False, a shorter call)."""
    from oracle import oracle as O
    key = (c.name, tuple(sorted((k, str(v)) for k, v in override.items())))
    if key not in _ref:
        kw = dict(c.kwargs(), **override)
        if c.mode == "nipt":
            kw.update(runif_block=c.runif_block, runif_resample=c.runif_resample)
            shard = np.zeros(len(BLOCK_ITS) * c.G)
        else:
            shard = c.runif_shard
        _ref[key] = O.forwardBackwardGibbsNIPT(c.panel, c.sample, c.which, c.H0, c.runif_reads, c.first_read, shard, **kw)
    return _ref[key]


def first_pass_table(c, perturb=None):
    """The block table of a NIPT case's first block pass, from the oracle's pieces: the state after sweep BLOCK_ITS[0] (the same
    call cut short, no pass), rate2 of it (gibbs-nipt-block.cpp:347-363), qo_define_blocked_grids, qo_make_gibbs_considers.
    ``perturb``: a relative perturbation of the rates (a vector of factors)."""
    from oracle import oracle as O
    assert c.mode == "nipt"
    st = oracle_ref(c, n_gibbs_burn_in_its=BLOCK_ITS[0], n_gibbs_sample_its=1, perform_block_gibbs=False)
    assert st["status"] == 0
    G, tm = c.G, c.panel.transMatRate_t
    rate2 = np.zeros(max(G - 1, 0))
    for h in range(3):
        a, b, e = st["alphaHat_t"][h], st["betaHat_t"][h], st["eMatGrid_t"][h]
        for g in range(G - 2):
            rate2[g] += 1 - tm[0, g] * float(np.sum(a[:, g] * b[:, g + 1] * e[:, g + 1]))
    if perturb is not None:
        rate2 = rate2 * perturb
    kw = c.kwargs()
    L = c.panel.L_grid if kw.get("L_grid") is None else kw["L_grid"]
    blocked = O.define_blocked_grids(rate2, L, kw.get("shuffle_bin_radius", 5000), kw.get("block_gibbs_quantile_prob", 0.95))
    tab = O.make_gibbs_considers(blocked, c.sample.wif)
    tab["rate2"], tab["blocked_grid"] = rate2, blocked
    return tab


# ---------------------------------------------------------------------------------------------------------------------------
# what the arrays and the oracle say about a case; the edges the suite must sit on
# ---------------------------------------------------------------------------------------------------------------------------
def runs_of(wif):
    """(grid, first read, last read) of every grid that holds reads"""
    wif = np.asarray(wif)
    out = []
    for g in np.unique(wif):
        r = np.flatnonzero(wif == g)
        assert r[-1] - r[0] + 1 == len(r)
        out.append((int(g), int(r[0]), int(r[-1])))
    return out


def readless_runs(wif, G):
    """maximal runs (first grid, last grid) of grids without reads"""
    has = np.zeros(G, dtype=bool)
    has[np.asarray(wif, dtype=np.int64)] = True
    out, g = [], 0
    while g < G:
        if has[g]:
            g += 1
            continue
        e = g
        while e + 1 < G and not has[e + 1]:
            e += 1
        out.append((g, e))
        g = e + 1
    return out


def edges_of(c):
    """The named edges a case sits on, from its arrays, the oracle's read categories and (NIPT block cases) the oracle's table."""
    s, G, R = c.sample, c.G, c.R
    T = c.panel.nSNPs
    m = "NIPT" if c.mode == "nipt" else "diploid"
    e = {f"{m}: G={G}", f"{m}: R={R}", f"{m}: G={G}, last grid of {T - 32 * (G - 1)} SNP(s)"}
    if c.mode == "dip_iter" and R == 129:
        e.add(f"iterative initialisation from read {c.first_read} of 129")
    if c.Ks == KS_BIG and G == 129:
        e.add(f"{m}: G=129 at Ks=600")
    runs = runs_of(s.wif)
    for g, a, b in runs:
        for edge in (STREAM, 2 * STREAM):
            if b == edge - 1 and any(a2 == edge for _, a2, _ in runs):
                e.add(f"{m}: a run ends at read {edge - 1} and the next starts at read {edge}")
            if a < edge - 1 and b > edge and b - a + 1 <= 10:
                e.add(f"{m}: a run of at most 10 straddles read {edge}")
        if b - a + 1 == 70 and a == 60:
            e.add(f"{m}: 70 reads from read 60 on grid {g}" + (", a crowded grid after it" if any(
                g2 == g + 1 and b2 - a2 + 1 > CROWDED for g2, a2, b2 in runs) else ""))
        if len(runs) == 1 and R >= 65:
            e.add(f"{m}: every read on grid " + ("0" if g == 0 else "G - 1" if g == G - 1 else str(g)))
        if len(runs) == 1 and R == 5 and G == 129 and g == 128:
            e.add(f"{m}: G=129, five reads on grid 128")
    if R and G == G_RUNS:
        if s.wif.min() >= 64:
            e.add(f"{m}: reads only in grids >= 64")
        if s.wif.max() < 64 and len(runs) == 64:
            e.add(f"{m}: reads only in grids < 64")
    if len(runs) == G and R == G:
        e.add(f"{m}: exactly one read per grid")
    if (62, 65) in readless_runs(s.wif, G):
        e.add(f"{m}: a read-less run over grids 62 .. 65")
    ref = oracle_ref(c)
    cat1 = set(np.flatnonzero(ref["read_category"] == 1).tolist())
    tag = f"{m}, categories " + ("off" if c.kwargs().get("disable_read_category_usage") else "on")
    planted = set(np.flatnonzero(oracle_ref(c, disable_read_category_usage=False)["read_category"] == 1).tolist()) if R else set()
    if planted and len(planted) <= 2:
        first_of_grid = {a for _, a, _ in runs}
        for r in planted:
            if r in (0, STREAM - 1, STREAM):
                e.add(f"{tag}: a category-1 read at stream position {r}")
            if r in first_of_grid:
                e.add(f"{tag}: a category-1 read opens a grid's run")
            if r == R - 1:
                e.add(f"{tag}: the chain's last read is category 1")
        if {63, 64} <= planted:
            e.add(f"{tag}: two category-1 reads in a row across the refill")
        if c.kwargs().get("disable_read_category_usage"):
            assert not cat1
    if R > 64:
        n = np.diff(s.read_ptr)
        d63, d64 = n[63] > MAX_PATTERN_BITS, n[64] > MAX_PATTERN_BITS
        if d63 != d64:
            e.add(f"{m}: read 63 {'dense' if d63 else 'compact'}, read 64 {'dense' if d64 else 'compact'}")
    if c.spec.family == "blocks":
        t = first_pass_table(c)
        ends = set(int(x) for x in t["consider_grid_end_0_based"][:-1])
        for g in (62, 63, 64, 65):
            if g in ends:
                e.add(f"block table: a block ends at grid {g}")
        if t["n_blocks"] == 1:
            e.add("block table: one block only")
        for a, b in zip(t["consider_reads_start_0_based"], t["consider_reads_end_0_based"]):
            if a < 63 and b > 64 and t["n_blocks"] > 1:
                e.add("block table: a block's reads straddle read 64")
        blocked = t["blocked_grid"]
        empty = sorted(set(range(int(blocked[-1]) + 1)) - set(int(b) for b in blocked[s.wif]))
        if t["n_blocks"] == int(blocked[-1]) + 1 - len(empty):
            hi_of = lambda b: int(np.flatnonzero(blocked == b)[-1])
            lo_of = lambda b: int(np.flatnonzero(blocked == b)[0])
            if any(hi_of(b) < 64 for b in empty) and any(lo_of(b) > 64 for b in empty):
                e.add("block table: read-less blocks merged away on each side of grid 64")
        if R >= 2 and blocked[s.wif[-1]] != blocked[s.wif[-2]] and int(t["consider_reads_start_0_based"][-1]) < R - 1:
            e.add("block table: the last read alone opens a block and takes the unrecorded block's reads")
    return e


def required_edges():
    e = set()
    for m in ("diploid", "NIPT"):
        e |= {f"{m}: G={g}" for g in G_COUNTS} | {f"{m}: R={r}" for r in R_COUNTS}
        e |= {f"{m}: G={g}, last grid of {n} SNP(s)" for g in G_COUNTS for n in (32, 1)}
        e |= {f"{m}: G=129 at Ks=600"}
        e |= {f"{m}: a run ends at read 63 and the next starts at read 64", f"{m}: a run of at most 10 straddles read 64",
              f"{m}: 70 reads from read 60 on grid 30", f"{m}: 70 reads from read 60 on grid 63, a crowded grid after it",
              f"{m}: every read on grid 0", f"{m}: every read on grid G - 1", f"{m}: reads only in grids >= 64",
              f"{m}: reads only in grids < 64", f"{m}: a read-less run over grids 62 .. 65", f"{m}: exactly one read per grid",
              f"{m}: G=129, five reads on grid 128"}
        for tag in (f"{m}, categories on", f"{m}, categories off"):
            e |= {f"{tag}: a category-1 read at stream position {r}" for r in (0, 63, 64)}
            e |= {f"{tag}: a category-1 read opens a grid's run", f"{tag}: the chain's last read is category 1",
                  f"{tag}: two category-1 reads in a row across the refill"}
        e |= {f"{m}: read 63 dense, read 64 compact", f"{m}: read 63 compact, read 64 dense"}
    e |= {f"iterative initialisation from read {r} of 129" for r in FIRST_READS_ITER}
    e |= {f"block table: a block ends at grid {g}" for g in (62, 63, 64, 65)}
    e |= {"block table: one block only", "block table: a block's reads straddle read 64",
          "block table: read-less blocks merged away on each side of grid 64",
          "block table: the last read alone opens a block and takes the unrecorded block's reads"}
    return e
