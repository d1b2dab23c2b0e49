"""Constructed inputs for the rare + common ("all-SNP") Gibbs call (helper, no test; imports no device code).

qa_gibbs_batch_rare_common runs two pieces of device code nothing else runs -- the rare branch of k_ematread (csrc/gibbs_dev.hpp) and
k_happrobs_rc (csrc/gibbs.hip) -- and host code that has to agree with them bit for bit: prepare_chain's bitmap of the rare SNPs a
selected haplotype carries (rc_any) with its count of informative bases, upload_rare_pairs' (SNP, row) words, and the launch planner's
second statement of the same count.  quilt_amd.synth.make_rare_common scatters rare SNPs and carriers at random and meets the constants
of that code by accident; the builders here place SNPs, carriers and reads ON them.

Three families on one panel of K = 1100 haplotypes and 160 common SNPs (five common grids; grid 2 holds special haplotypes):
  layout    where the common SNPs lie on the all-SNP axis (a grid without one, a grid that spans two common grids, the first common
            SNP at bit 0 / 31, the ragged last grid);
  carriers  who carries a rare SNP (nobody, only unselected haplotypes, one given row, every row, a full grid of 32 * Ks pairs, the
            largest pair word);
  reads     the rare branch of k_ematread in the isolating layout of tests/read_cases.py (one read per all-SNP grid and label):
            rare-only reads, the compact / dense threshold made of common and carried rare SNPs, Jmax, rescaling outcomes, and one
            sample read by two chains whose haplotype subsets differ in exactly the carriers.
Every builder returns a RareCase whose ``claims`` say what it planted; tests/test_rare_cases_cpu.py proves every claim with numpy and
the oracle alone and derives the coverage table from the same facts; tests/test_rare_geometry_gpu.py runs the cases.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from tests import read_cases
from tests.util import sample_from_arrays

# The constants the cases are placed on, with where the code states them.
SNPS_PER_GRID = 32      # gibbs.hip k_happrobs_rc: s = 32 * g, b = threadIdx.x & 31; rc_any word t >> 5, bit t & 31 (prepare_chain)
READS_PER_WAVE = 32     # gibbs_dev.hpp: kReadsPerWave (g_prev and the panel words live for one block of reads)
CHUNK = 64              # gibbs_dev.hpp k_ematread: `if (s + j >= chunk0 + 64) load_chunk(s + j)`
MAX_PATTERN_BITS = 5    # gibbs_dev.hpp: kMaxPatternBits; gibbs.hip prepare_chain: n_inf > kMaxPatternBits -> dense
ROW_MASK = 1023         # gibbs.hip k_happrobs_rc: k = e & 1023u, b = e >> 10; upload_rare_pairs packs ((snp & 31) << 10) | row
PARTS = 8               # gibbs.hip k_happrobs_rc: part = threadIdx.x >> 5, a pair is summed by the thread with (k & 7) == part
CONSTANTS = ("SNPS_PER_GRID", "READS_PER_WAVE", "CHUNK", "MAX_PATTERN_BITS", "ROW_MASK", "PARTS")

K, T_COMMON = 1100, 160
KS_SMALL, KS_LARGE, KS_MAX = 70, 600, 1024
FF = 0.2


@dataclass
class RareCase:
    name: str
    family: str               # layout | carriers | reads
    Ks: int
    rc: object                # quilt_amd.panel.RareCommon
    which: np.ndarray         # 1-based sorted panel haplotypes
    sample: object            # all-SNP reads
    H0: np.ndarray
    Jmax: int = 10000
    maxdiff: float = 1e10
    isolating: bool = False   # one read per (all-SNP grid, label)
    claims: dict = field(default_factory=dict)
    which_b: np.ndarray = None   # two_chains_one_read: the second chain's subset


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


# ---------------------------------------------------------------------------------------------------------------------------
# the panel and the haplotype subsets
# ---------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def panel():
    """Made when a test first asks: 160 common SNPs over 5 Mb leave room for 32 and more rare SNPs between two neighbours."""
    from quilt_amd.synth import make_synthetic_panel
    return make_synthetic_panel(K=K, nSNPs=T_COMMON, seed=2024, ref_error=1e-3, nGen=10, expRate=1.0, region_bp=5_000_000,
                                stress_grids=(2,))


@lru_cache(maxsize=None)
def _order():
    """Haplotypes 0 and K - 1 first (the first and the last CSR row are selected by every subset), the others shuffled."""
    return np.r_[0, K - 1, 1 + np.random.default_rng(41).permutation(K - 2)].astype(np.int64)


def which_of(Ks):
    """Nested subsets: which_of(70) < which_of(600) < which_of(1024).  Row 0 is haplotype 0, row Ks - 1 is haplotype K - 1."""
    return (np.sort(_order()[:Ks]) + 1).astype(np.int32)


def always_selected():
    return _order()[2:KS_SMALL]


def never_selected():
    return _order()[KS_MAX + 8:]


def hap_of(which, row):
    return int(which[row]) - 1


# ---------------------------------------------------------------------------------------------------------------------------
# the all-SNP side from an explicit pattern
# ---------------------------------------------------------------------------------------------------------------------------
def planted_rc(pnl, is_common, carriers):
    """A RareCommon from ``is_common`` (0 / 1 per all-SNP index, panel.nSNPs ones) and ``carriers`` {rare all-SNP index: panel
    haplotypes (0-based) that carry its alt allele}.  Positions: the common SNPs keep the panel's, a run of rare SNPs is spread
    evenly over the gap it sits in; L_grid_all and transMatRate_t_all follow as in quilt_amd.synth.make_rare_common."""
    from quilt_amd.panel import RareCommon
    from quilt_amd.synth import _sigma_from_positions
    is_common = np.asarray(is_common, dtype=np.uint8)
    T_all = len(is_common)
    cidx = np.flatnonzero(is_common == 1)
    assert len(cidx) == pnl.nSNPs
    L = np.asarray(pnl.L, dtype=np.int64)
    L_all = np.zeros(T_all, dtype=np.int64)
    L_all[cidx] = L
    n = int(cidx[0])
    assert L[0] - n >= 1, "no room before the first common SNP"
    L_all[:n] = L[0] - n + np.arange(n)
    for i in range(len(cidx) - 1):
        n, gap = int(cidx[i + 1] - cidx[i] - 1), int(L[i + 1] - L[i])
        assert gap > n, f"{n} rare SNPs do not fit between common SNPs {i} and {i + 1}"
        L_all[cidx[i] + 1:cidx[i + 1]] = L[i] + (np.arange(1, n + 1) * gap) // (n + 1)
    n = T_all - 1 - int(cidx[-1])
    L_all[cidx[-1] + 1:] = L[-1] + 1000 * np.arange(1, n + 1)
    assert (np.diff(L_all) > 0).all()
    common_snp_index = np.zeros(T_all, dtype=np.int32)
    common_snp_index[cidx] = np.arange(1, pnl.nSNPs + 1, dtype=np.int32)
    starts = np.arange(0, T_all, 32)
    L_grid_all = (np.add.reduceat(L_all, starts) // np.diff(np.r_[starts, T_all])).astype(np.int64)
    ex = pnl.extra
    sigma = _sigma_from_positions(L_grid_all, ex.get("nGen", 100.0), ex.get("expRate", 1.0))
    per_hap = [[] for _ in range(pnl.K)]
    for t, haps in carriers.items():
        assert 0 <= t < T_all and is_common[t] == 0, f"SNP {t} is not rare"
        haps = sorted(int(h) for h in haps)
        assert len(set(haps)) == len(haps) and (not haps or (0 <= haps[0] and haps[-1] < pnl.K))
        for h in haps:
            per_hap[h].append(int(t) + 1)
    rare_ptr = np.r_[0, np.cumsum([len(x) for x in per_hap])].astype(np.int64)
    rare_snp = np.array([t for x in per_hap for t in sorted(x)], dtype=np.int32)
    return RareCommon(nSNPs_all=T_all, nGrids_all=(T_all + 31) // 32, snp_is_common=is_common, common_snp_index=common_snp_index,
                      rare_ptr=rare_ptr, rare_snp=rare_snp, transMatRate_t_all=np.asfortranarray(np.stack([sigma, 1.0 - sigma])),
                      L_all=L_all, L_grid_all=L_grid_all)


def all_bits(rc, which):
    """Alleles [Ks, T_all] of the selected haplotypes over all SNPs."""
    out = np.zeros((len(which), rc.nSNPs_all), dtype=np.int64)
    out[:, np.asarray(rc.snp_is_common) == 1] = read_cases.hap_bits(panel(), which)
    for row, k in enumerate(np.asarray(which) - 1):
        out[row, rc.rare_snp[rc.rare_ptr[k]:rc.rare_ptr[k + 1]] - 1] = 1
    return out


def gibbs_inputs(case, ff=0.0):
    """The uniforms of a whole sampler run on a case, and the read the iterative initialisation starts from."""
    rng = np.random.default_rng(_seed("gibbs", case.name, case.Ks))
    R, G = case.sample.nReads, case.rc.nGrids_all
    return dict(ru=rng.random(R * 21), rs=rng.random(3 * (G - 1)), fr=int(rng.integers(0, R)), rb=rng.random(3 * R), rr=rng.random(3 * R),
                H3=rng.choice([1, 2, 3], p=[0.5, 0.4, 0.1], size=R).astype(np.int32))


# ---------------------------------------------------------------------------------------------------------------------------
# what the host and the kernels do, restated for the claims
# ---------------------------------------------------------------------------------------------------------------------------
def common_index(rc):
    """All-SNP index -> index among the common SNPs, -1 for a rare SNP (qa_rare_common_create: h_common_index)."""
    return np.asarray(rc.common_snp_index, dtype=np.int64) - 1


def layout_facts(rc, Gc):
    """Per all-SNP grid what k_happrobs_rc meets: the SNPs in it, its common SNPs, the bit of the first one, the common grid s_cg
    takes from it, and the common grids its common SNPs lie in."""
    cs = common_index(rc)
    out = []
    for g in range(rc.nGrids_all):
        loc = cs[32 * g:32 * g + 32]
        com = loc[loc >= 0]
        first = int(np.argmax(loc >= 0)) if len(com) else -1
        cgs = tuple(sorted(set((com >> 5).tolist())))
        assert len(cgs) <= 2 and (len(cgs) < 2 or cgs[1] == cgs[0] + 1), "32 all-SNPs span at most two neighbouring common grids"
        out.append(dict(nLocal=len(loc), n_common=len(com), first_b=first, cg=int(com[0] >> 5) if len(com) else -1, cgs=cgs,
                        second_word_guarded=bool(len(com)) and int(com[0] >> 5) + 1 == Gc))
    return out


def carried_rows(rc, which):
    """{rare all-SNP index: rows of ``which`` whose haplotype carries it, ascending}."""
    out = {}
    for row, k in enumerate(np.asarray(which) - 1):
        for t in rc.rare_snp[rc.rare_ptr[k]:rc.rare_ptr[k + 1]] - 1:
            out.setdefault(int(t), []).append(row)
    return out


def named_in_csr(rc):
    return set((np.asarray(rc.rare_snp, dtype=np.int64) - 1).tolist())


def pair_facts(rc, which):
    """upload_rare_pairs restated: per all-SNP grid the number of (SNP, row) pairs, and the largest packed word."""
    rows = carried_rows(rc, which)
    per_grid = np.zeros(rc.nGrids_all, dtype=np.int64)
    words = [0]
    for t, rs in rows.items():
        per_grid[t >> 5] += len(rs)
        words += [((t & 31) << 10) | r for r in rs]
        assert max(rs) <= ROW_MASK
    assert max(words) <= 0xFFFF
    return per_grid, max(words)


def any_mask(rc, which):
    """prepare_chain's rc_any as a boolean per all-SNP index."""
    m = np.zeros(rc.nSNPs_all, dtype=bool)
    m[list(carried_rows(rc, which))] = True
    return m


def informative_counts(case, which):
    """prepare_chain's count per read: visited bases whose folded quality is not 0 and whose SNP is common or a rare SNP some
    selected haplotype carries.  The fold (fold_zero_base_qualities) runs over every visited base, rare and uncarried ones too."""
    s = case.sample
    eff = read_cases.fold_qualities(s, case.Jmax)
    inf_snp = (common_index(case.rc) >= 0) | any_mask(case.rc, which)
    out = np.zeros(s.nReads, dtype=np.int64)
    for r in range(s.nReads):
        a, e = int(s.read_ptr[r]), int(s.read_ptr[r + 1])
        v = slice(a, a + min(e - a - 1, case.Jmax) + 1)
        out[r] = int(((eff[v] != 0) & inf_snp[s.u[v]]).sum())
    return out


def block_offsets(sample, r):
    """Offsets of read r's bases from the first base of its block of READS_PER_WAVE reads (the first chunk starts there)."""
    r0 = r - r % READS_PER_WAVE
    return np.arange(sample.read_ptr[r], sample.read_ptr[r + 1]) - sample.read_ptr[r0]


def oracle_columns(case, which, oracle, Jmax=None, rescale=True):
    return oracle.make_eMatRead_t_rare_common(panel(), case.rc, case.sample, which, case.maxdiff, case.Jmax if Jmax is None else Jmax,
                                              rescale_eMatRead_t=rescale)


def happrobs_from_state(rc, which, alpha, beta, c):
    """rcpp_calculate_genProbs_and_hapProbs_final_rare_common from a returned state, in long double: gamma = alpha * beta / c per
    all-SNP grid; a common SNP sums gamma over the rows with the alt allele (t - o of the total t weigh ref_error), a carried rare
    SNP is t * eps + o * (1 - 2 eps), an uncarried one is eps.  ``alpha``, ``beta``: [Ks, G] per label; ``c``: [G] per label.
    Returns (hapProbs [n_label, T], genProbsM [3, T], is_common, carried) -- carried: the rare SNPs some selected row carries."""
    ld = np.longdouble
    eps = ld(panel().ref_error)
    T = rc.nSNPs_all
    bits = all_bits(rc, which).astype(ld)
    is_common = np.asarray(rc.snp_is_common) == 1
    carried = any_mask(rc, which)
    grid = np.arange(T) // SNPS_PER_GRID
    hp = np.zeros((len(alpha), T), dtype=ld)
    for h in range(len(alpha)):
        gam = (np.asarray(alpha[h], dtype=ld) * np.asarray(beta[h], dtype=ld) / np.asarray(c[h], dtype=ld)[None, :])[:, grid]
        on, tot = (gam * bits).sum(axis=0), gam.sum(axis=0)
        hp[h] = np.where(is_common, on * (1 - eps) + (tot - on) * eps, np.where(carried, tot * eps + on * (1 - 2 * eps), eps))
    g0, g1 = hp[0], hp[1]
    gm = np.stack([(1 - g0) * (1 - g1), g0 * (1 - g1) + (1 - g0) * g1, g0 * g1])
    return hp, gm, is_common, carried


# ---------------------------------------------------------------------------------------------------------------------------
# layout and carrier families: reads that cover the axis
# ---------------------------------------------------------------------------------------------------------------------------
def C(n):
    return [1] * n


def R(n):
    return [0] * n


def _read_from(bits, row, u, rng, err=0.05, q=(20, 40)):
    u = np.asarray(u, dtype=np.int64)
    allele = bits[row, u] ^ (rng.random(len(u)) < err)
    phred = rng.integers(q[0], q[1] + 1, len(u))
    return u.astype(np.int32), np.where(allele == 1, phred, -phred).astype(np.int32)


def cover_reads(rc, which, seed, must_cover=()):
    """Three reads of 1-8 consecutive all-SNPs per grid from three of the selected haplotypes (the posterior is far from flat: a row
    that is summed in the wrong place shows), and one read of quality 40 showing the alt allele at every SNP of ``must_cover``."""
    rng = np.random.default_rng(seed)
    bits = all_bits(rc, which)
    T = rc.nSNPs_all
    truth = rng.choice(len(which), 3, replace=False)
    reads = []
    for g in range(rc.nGrids_all):
        for _ in range(3):
            start = int(rng.integers(32 * g, min(32 * g + 32, T)))
            reads.append(_read_from(bits, int(rng.choice(truth)), np.arange(start, min(start + int(rng.integers(1, 9)), T)), rng))
    for t in must_cover:
        u = np.arange(max(t - 1, 0), min(t + 2, T))
        rows = np.flatnonzero(bits[:, t])
        x, b = _read_from(bits, int(rows[0]) if len(rows) else int(truth[0]), u, rng, err=0.0, q=(40, 40))
        b[x == t] = 40
        reads.append((x, b))
    cen = np.array([int(x[(len(x) - 1) // 2]) for x, _ in reads])
    o = np.argsort(cen, kind="stable")
    reads = [reads[i] for i in o]
    ptr = np.r_[0, np.cumsum([len(x) for x, _ in reads])]
    s = sample_from_arrays(ptr, np.concatenate([x for x, _ in reads]), np.concatenate([b for _, b in reads]), cen[o] // 32)
    assert s.nReads <= 200
    return s, rng.integers(1, 3, size=s.nReads).astype(np.int32)


def scattered_carriers(is_common, seed):
    """Background carriers of a layout case: of every ten rare SNPs four have none, three have 1-3 haplotypes every subset selects,
    two have haplotypes no subset selects, one has both."""
    rng = np.random.default_rng(seed)
    sel, uns = always_selected(), never_selected()
    out = {}
    for t in np.flatnonzero(np.asarray(is_common) == 0):
        x = rng.random()
        if x < 0.4:
            continue
        haps = []
        if x < 0.7 or x >= 0.9:
            haps += rng.choice(sel, int(rng.integers(1, 4)), replace=False).tolist()
        if x >= 0.7:
            haps += rng.choice(uns, int(rng.integers(1, 3)), replace=False).tolist()
        out[int(t)] = haps
    return out


def _tail(n, last):
    return (C(1) + R(1)) * 160 + R(n) if last == "rare" else (C(1) + R(1)) * 159 + R(n + 1) + C(1)


# name -> (pattern, claims about the all-SNP grids)
LAYOUTS = {
    "interleaved": lambda: ((C(1) + R(2)) * 160, dict(no_common=(), two_cg=())),
    "rare_grid_first": lambda: (R(32) + (C(1) + R(1)) * 160, dict(no_common=(0,), two_cg=())),
    "rare_grid_mid": lambda: ((C(1) + R(1)) * 48 + R(32) + (C(1) + R(1)) * 112, dict(no_common=(3,), two_cg=())),
    "rare_grid_last": lambda: ((C(1) + R(1)) * 160 + R(32), dict(no_common=(10,), two_cg=())),
    "two_common_grids": lambda: (C(30) + R(2) + C(4) + R(28) + (C(1) + R(1)) * 126, dict(no_common=(), two_cg=(1, 3, 5, 7), first_b={1: 0})),
    "two_common_grids_at_end": lambda: (C(126) + R(2) + C(4) + R(28) + (R(1) + C(1)) * 15 + R(2) + (C(1) + R(1)) * 15 + R(2),
                                        dict(no_common=(), two_cg=(4,), guarded=(4 + 1, 4 + 2), reaches_last_cg=(4,))),
    "first_common_b0": lambda: ((C(1) + R(1)) * 160, dict(no_common=(), two_cg=(), first_b={g: 0 for g in range(10)})),
    "first_common_b31": lambda: ((R(31) + C(1)) * 3 + C(157), dict(no_common=(), two_cg=(3, 4, 5, 6), first_b={0: 31, 1: 31, 2: 31},
                                                                  n_common={0: 1, 1: 1, 2: 1})),
    "single_common": lambda: ((R(10) + C(1) + R(21)) * 2 + C(158), dict(no_common=(), two_cg=(2, 3, 4, 5), first_b={0: 10, 1: 10},
                                                                       n_common={0: 1, 1: 1})),
    "word_edges": lambda: (C(30) + R(4) + C(28) + R(4) + C(102) + R(3), dict(no_common=(), carried=(31, 32, 63, 64, 170),
                                                                              uncarried=(30, 33, 62, 65, 168, 169))),
}
for _n in (1, 31, 32):
    for _last in ("rare", "common"):
        LAYOUTS[f"tail_{_n}_{_last}"] = (lambda n=_n, last=_last: (_tail(n, last), dict(tail=n, last=last)))
LAYOUT_KS = (KS_SMALL, KS_LARGE)


def layout_case(name, Ks):
    pattern, claims = LAYOUTS[name]()
    which = which_of(Ks)
    car = scattered_carriers(pattern, _seed("carriers", name))
    T_all = len(pattern)
    must = []
    if name == "word_edges":
        for t in claims["uncarried"]:
            car.pop(t, None)
        for i, t in enumerate(claims["carried"]):
            car[t] = [int(always_selected()[3 * i]), int(always_selected()[3 * i + 1])]
        must = list(claims["carried"])
    if claims.get("last") == "rare":   # the last SNP of all is rare and a selected haplotype carries it
        car[T_all - 1] = [int(always_selected()[0]), int(always_selected()[7])]
        must = [T_all - 1]
    rc = planted_rc(panel(), pattern, car)
    if not must:   # a few of the carried rare SNPs are read with their alt allele
        must = sorted(any_rare for any_rare in carried_rows(rc, which))[::7][:20]
    s, H0 = cover_reads(rc, which, _seed("reads", name, Ks), must)
    return RareCase(name, "layout", Ks, rc, which, s, H0, claims=claims)


# ---------------------------------------------------------------------------------------------------------------------------
# carrier family (on the rare_grid_mid layout: grid 3 = all-SNPs 96 .. 127 is rare throughout)
# ---------------------------------------------------------------------------------------------------------------------------
LONG_LIST = tuple(range(96, 128, 2)) + tuple(range(129, 177, 2))   # 40 rare SNPs of one haplotype
CARRIER_KS = {"ks1024_row1023_b31": (KS_MAX,), "full_grid": (KS_LARGE, KS_MAX)}
CARRIER_NAMES = ("nobody", "unselected_only", "row_0", "row_63", "row_64", "row_last", "each_part", "everyone", "hap_0", "hap_Km1",
                 "long_list", "full_grid", "ks1024_row1023_b31")


def carrier_case(name, Ks):
    pattern, _ = LAYOUTS["rare_grid_mid"]()
    which = which_of(Ks)
    uns = never_selected()
    hap = lambda row: hap_of(which, row)
    everyone = [int(k) - 1 for k in which]
    claims, must = {}, None
    if name == "nobody":
        car, claims = {}, dict(pairs_total=0, csr_empty=True)
    elif name == "unselected_only":
        car = {97: uns[:3].tolist(), 101: uns[3:5].tolist(), 33: uns[:1].tolist()}
        claims, must = dict(pairs_total=0, named_not_carried=(33, 97, 101)), [33, 97, 101]
    elif name.startswith("row_"):
        row = Ks - 1 if name == "row_last" else int(name[4:])
        car = {100: [hap(row)], 1: [hap(row)]}
        claims = dict(rows={100: (row,), 1: (row,)}, pairs={3: 1, 0: 1})
    elif name == "each_part":
        car = {96 + i: [hap(9 * i)] for i in range(PARTS)}
        claims = dict(rows={96 + i: (9 * i,) for i in range(PARTS)}, parts=tuple(range(PARTS)))
    elif name == "everyone":
        car = {100: everyone, 5: everyone}
        claims = dict(everyone=(5, 100), pairs={3: Ks, 0: Ks})
    elif name in ("hap_0", "hap_Km1"):
        h = 0 if name == "hap_0" else K - 1
        car = {3: [h], 100: [h], 131: [h]}
        claims = dict(csr_row=h, rows={t: (0 if h == 0 else Ks - 1,) for t in (3, 100, 131)})
    elif name == "long_list":
        # row 5's haplotype carries LONG_LIST; row 7's carries the three SNPs that are absent from it (below, between, above) and
        # row 9's a list of one: k_ematread probes every row's list (0, 1, 3 and 40 entries) for every carried SNP a read covers
        car = {t: [hap(5)] for t in LONG_LIST}
        absent = (95, 97, 177)
        for t in absent:
            car[t] = [hap(7)]
        car[97].append(hap(9))
        present = (LONG_LIST[0], LONG_LIST[20], LONG_LIST[-1])
        claims = dict(list_row=5, list_len=40, present=present, absent=absent, list_lens=(0, 1, 3, 40))
        must = sorted(present + absent)
    elif name == "full_grid":
        car = {96 + b: everyone for b in range(32)}
        claims, must = dict(pairs={3: 32 * Ks}, everyone=tuple(range(96, 128))), [96, 111, 127]
    elif name == "ks1024_row1023_b31":
        assert Ks == KS_MAX and hap(1023) == K - 1
        car = {127: [K - 1]}
        claims = dict(rows={127: (1023,)}, max_word=0x7FFF)
    else:
        raise KeyError(name)
    rc = planted_rc(panel(), pattern, car)
    if must is None:
        must = sorted(carried_rows(rc, which))[:40]
    s, H0 = cover_reads(rc, which, _seed("reads", name, Ks), must)
    return RareCase(name, "carriers", Ks, rc, which, s, H0, claims=claims)


# ---------------------------------------------------------------------------------------------------------------------------
# read family: the rare branch of k_ematread, isolating layout on the all-SNP grid
# ---------------------------------------------------------------------------------------------------------------------------
READ_PATTERN = (C(1) + R(3)) * 160   # 640 all-SNPs, 20 all-SNP grids; the kind of an all-SNP index follows from index % 8
_KINDS = {"read": ("c", "car", "all", "unsel", "c", "unc", "unc", "unc"),      # car: a third of the rows; all: every selected row
          "two": ("c", "ca", "cb", "unc", "c", "unc", "unc", "unc")}           # ca: only chain A's haplotypes; cb: only chain B's


def kinds_of(style):
    return np.array([_KINDS[style][t % 8] for t in range(len(READ_PATTERN))])


@lru_cache(maxsize=None)
def read_rc(Ks):
    which = which_of(Ks)
    rng = np.random.default_rng(_seed("read_rc", Ks))
    kinds = kinds_of("read")
    car = {}
    for t in range(len(READ_PATTERN)):
        if kinds[t] == "car":
            car[t] = (which[rng.random(Ks) < 1 / 3] - 1).tolist()
            assert 5 <= len(car[t]) <= Ks - 5
        elif kinds[t] == "all":
            car[t] = (which - 1).tolist()
        elif kinds[t] == "unsel":
            car[t] = never_selected()[:3].tolist()
    return planted_rc(panel(), READ_PATTERN, car)


def two_chain_subsets(Ks):
    o = _order()
    a = (np.sort(o[:Ks]) + 1).astype(np.int32)
    b = (np.sort(np.r_[o[:Ks - 5], o[Ks:Ks + 5]]) + 1).astype(np.int32)
    return a, b, o[Ks - 5:Ks], o[Ks:Ks + 5]


@lru_cache(maxsize=None)
def two_chain_rc(Ks):
    _, _, only_a, only_b = two_chain_subsets(Ks)
    rng = np.random.default_rng(_seed("two_rc", Ks))
    kinds = kinds_of("two")
    car = {}
    for t in range(len(READ_PATTERN)):
        if kinds[t] in ("ca", "cb"):
            car[t] = rng.choice(only_a if kinds[t] == "ca" else only_b, int(rng.integers(2, 4)), replace=False).tolist()
    return planted_rc(panel(), READ_PATTERN, car)


class _Reads:
    """Assembles a chain of the read family: reads as sequences of SNP kinds, alleles from one selected row."""

    def __init__(self, name, Ks, style="read"):
        self.name, self.Ks = name, Ks
        self.rc = read_rc(Ks) if style == "read" else two_chain_rc(Ks)
        self.which = which_of(Ks) if style == "read" else two_chain_subsets(Ks)[0]
        self.kinds = kinds_of(style)
        self.bits = all_bits(self.rc, self.which)
        self.rng = np.random.default_rng(_seed("reads", name, Ks))
        self.T = self.rc.nSNPs_all

    def seq(self, start, *segs):
        """All-SNP indices, ascending from ``start``: per segment (kind, n) the next n SNPs of that kind behind the last one taken."""
        cur, out = start - 1, []
        for kind, n in segs:
            cand = np.flatnonzero((self.kinds == kind) & (np.arange(self.T) > cur))[:n]
            assert len(cand) == n, (self.name, kind, n)
            out += cand.tolist()
            cur = int(cand[-1])
        return np.array(out, dtype=np.int64)

    def read(self, start, *segs, row=None, **kw):
        row = int(self.rng.integers(self.Ks)) if row is None else row
        return _read_from(self.bits, row, self.seq(start, *segs), self.rng, **kw)

    def short(self):
        """A plain read of three bases: common, carried, common."""
        kind = "car" if "car" in self.kinds else "ca"
        return self.read(int(self.rng.integers(0, 500)), ("c", 1), (kind, 1), ("c", 1))

    def finish(self, reads, Jmax=10000, maxdiff=1e10, **claims):
        n = len(reads)
        assert all(len(u) == len(b) >= 1 and (np.diff(u) > 0).all() for u, b in reads)
        ptr = np.r_[0, np.cumsum([len(u) for u, _ in reads])]
        wif = np.arange(n) // 2
        assert wif.max() < self.rc.nGrids_all
        s = sample_from_arrays(ptr, np.concatenate([u for u, _ in reads]), np.concatenate([b for _, b in reads]), wif)
        return RareCase(self.name, "reads", self.Ks, self.rc, self.which, s, (1 + np.arange(n) % 2).astype(np.int32), Jmax, maxdiff, True,
                        claims)


def _zero(read, idx):
    u, b = read
    b = b.copy()
    b[idx] = 0
    return u, b


# read A has five informative bases (compact), read B six (dense)
THRESHOLDS = {
    "common_unc0": ([("c", 5)], [("c", 6)]),
    "common_unc7": ([("c", 2), ("unc", 3), ("c", 3), ("unc", 4)], [("c", 3), ("unc", 3), ("c", 3), ("unc", 4)]),
    "common_unc20": ([("c", 1), ("unc", 10), ("c", 4), ("unc", 10)], [("c", 2), ("unc", 10), ("c", 4), ("unc", 10)]),
    "carried_among": ([("c", 2), ("unc", 2), ("car", 1), ("c", 2), ("unc", 4)], [("c", 5), ("car", 1)]),   # B: the sixth is a carried rare SNP
    "carried_only": ([("car", 5)], [("car", 6)]),
}
THRESHOLD_NAMES = tuple(f"threshold_{k}{z}" for k in THRESHOLDS for z in ("", "_z"))


def threshold_case(name, Ks):
    key, zeros = (name[len("threshold_"):-2], True) if name.endswith("_z") else (name[len("threshold_"):], False)
    b = _Reads(name, Ks)
    sa, sb = THRESHOLDS[key]
    A, B = b.read(40, *sa), b.read(200, *sb)
    claims = {}
    if zeros:   # bases without a quality inside the reads: they take the base before them, sign included, whatever SNP that was on
        za = sorted({1, len(A[0]) - 1})
        zb = [2] if len(B[0]) > 2 else [1]
        A, B = _zero(A, za), _zero(B, zb)
        claims["zeros"] = {1: tuple(za), 3: tuple(zb)}
    return b.finish([b.short(), A, b.short(), B, b.short()], n_inf={1: 5, 3: 6}, dense={1: False, 3: True}, **claims)


def long_compact_case(Ks):
    """A read of 100 bases, four of them informative; its bases at block offsets 62 .. 65 are rare SNPs (the two in the middle carried)."""
    b = _Reads("long_compact", Ks)
    lead = b.read(0, ("c", 1), ("car", 1), ("c", 1))
    long_ = b.read(8, ("c", 1), ("unc", 58), ("unc", 1), ("car", 1), ("car", 1), ("unc", 1), ("c", 1), ("unc", 36))
    assert len(long_[0]) == 100
    return b.finish([lead, long_, b.short(), b.short()], n_inf={1: 4}, dense={1: False}, n_bases={1: 100}, rare_at_block_offsets={1: (62, 63, 64, 65)},
                    carried_at_block_offsets={1: (63, 64)})


def jmax_case(Jmax, Ks):
    """Base number Jmax of read 1 is a carried rare SNP and counts; base Jmax + 1 is one too and does not.  Read 2 begins without a
    quality and takes base Jmax's."""
    b = _Reads(f"jmax_{Jmax}", Ks)
    X = b.read(30, ("c", Jmax), ("car", 1), ("car", 1), ("c", 2))
    X[1][Jmax + 1] = -X[1][Jmax]   # what a wrong carry-over would take differs in sign
    nxt = _zero(b.short(), 0)
    n = Jmax + 1
    c = b.finish([b.short(), X, nxt, b.short()], Jmax=Jmax, n_inf={1: n}, dense={1: n > MAX_PATTERN_BITS}, clip_visible=(1,),
                 carried_at_base={1: (Jmax, Jmax + 1)})
    c.claims["folded"] = {int(c.sample.read_ptr[2]): int(X[1][Jmax])}
    return c


def all_equal_case(Ks):
    b = _Reads("all_equal", Ks)
    E = b.read(100, ("all", 3), ("unc", 4), ("all", 1))
    return b.finish([b.short(), E, b.short()], n_inf={1: 4}, dense={1: False}, equal=(1,))


def floor_case(Ks):
    b = _Reads("floor", Ks)
    F = b.read(60, ("car", 6), err=0.0, q=(40, 40))
    return b.finish([b.short(), F, b.short()], maxdiff=1e3, n_inf={1: 6}, dense={1: True}, floor=(1,))


def leading_zero_rare_case(Ks):
    b = _Reads("leading_zero_rare", Ks)
    Z = _zero(b.read(20, ("car", 1), ("c", 2), ("car", 1)), 0)
    return b.finish([Z, _zero(b.short(), 0), b.short()], n_inf={0: 3, 1: 3}, dense={0: False}, chain_starts_at_zero_on_carried=True)


def rare_only_uncarried_case(Ks):
    b = _Reads("rare_only_uncarried", Ks)
    shapes = [[("unc", 1)], [("unc", 2), ("unsel", 1)], [("unc", 40), ("unsel", 10), ("unc", 20)], [("unsel", 2)], [("unc", 5)], [("unc", 8)]]
    reads = [b.read(10 + 30 * i, *sh) for i, sh in enumerate(shapes)]
    return b.finish(reads, n_inf={r: 0 for r in range(6)}, dense={r: False for r in range(6)}, all_ones=tuple(range(6)), rare_only=tuple(range(6)))


def rare_only_carried_case(Ks):
    b = _Reads("rare_only_carried", Ks)
    reads = [b.read(10, ("car", 3)), b.read(50, ("c", 2), ("car", 1)), b.read(90, ("car", 2), ("all", 1)), b.read(130, ("car", 6)), b.short()]
    return b.finish(reads, n_inf={0: 3, 2: 3, 3: 6}, dense={0: False, 3: True}, rare_only=(0, 2, 3), then_common_in_block=(0,))


def rare_only_block2_case(Ks):
    """The second block of 32 reads begins with a rare-only read; the read behind it begins with a common SNP."""
    b = _Reads("rare_only_block2", Ks)
    reads = [b.short() for _ in range(READS_PER_WAVE)] + [b.read(300, ("car", 4)), b.read(340, ("c", 1), ("car", 2)), b.short()]
    return b.finish(reads, n_inf={32: 4}, rare_only=(32,), then_common_in_block=(32,))


def two_chains_case(Ks):
    """One sample, two chains: the subsets differ in five haplotypes each, which are exactly the carriers of the "ca" resp. "cb" SNPs."""
    b = _Reads("two_chains_one_read", Ks, style="two")
    wa, wb, _, _ = two_chain_subsets(Ks)
    reads = [b.short(), b.read(20, ("c", 3), ("ca", 3)), b.read(80, ("c", 3), ("cb", 3)), b.read(140, ("c", 2), ("ca", 2), ("cb", 2)),
             b.read(200, ("c", 6)), b.read(260, ("ca", 6)), b.read(320, ("c", 2), ("unc", 3), ("cb", 4)), b.short()]
    c = b.finish(reads, n_inf={1: 6, 2: 3, 3: 4, 4: 6, 5: 6, 6: 2}, n_inf_b={1: 3, 2: 6, 3: 4, 4: 6, 5: 0, 6: 6},
                 dense_a_compact_b=(1, 5), compact_a_dense_b=(2, 6))
    c.which_b = wb
    assert np.array_equal(c.which, wa)
    return c


READ_NAMES = (("rare_only_uncarried", "rare_only_carried", "rare_only_block2") + THRESHOLD_NAMES +
              ("long_compact", "jmax_1", "jmax_5", "all_equal", "floor", "leading_zero_rare", "two_chains_one_read"))
PER_WAVE_NAMES = THRESHOLD_NAMES + ("long_compact",)    # again at Ks = 600 with one and two waves per chain


def read_case(name, Ks):
    if name.startswith("threshold_"):
        return threshold_case(name, Ks)
    if name.startswith("jmax_"):
        return jmax_case(int(name[5:]), Ks)
    return {"rare_only_uncarried": rare_only_uncarried_case, "rare_only_carried": rare_only_carried_case,
            "rare_only_block2": rare_only_block2_case, "long_compact": long_compact_case, "all_equal": all_equal_case, "floor": floor_case,
            "leading_zero_rare": leading_zero_rare_case, "two_chains_one_read": two_chains_case}[name](Ks)


# ---------------------------------------------------------------------------------------------------------------------------
# the registry
# ---------------------------------------------------------------------------------------------------------------------------
def case_ids():
    """(family, name, Ks) of every case, without building any."""
    out = [("layout", n, Ks) for n in LAYOUTS for Ks in LAYOUT_KS]
    out += [("carriers", n, Ks) for n in CARRIER_NAMES for Ks in CARRIER_KS.get(n, LAYOUT_KS)]
    out += [("reads", n, Ks) for n in READ_NAMES for Ks in LAYOUT_KS]
    return out


@lru_cache(maxsize=None)
def case(family, name, Ks):
    c = {"layout": layout_case, "carriers": carrier_case, "reads": read_case}[family](name, Ks)
    assert (c.family, c.name, c.Ks) == (family, name, Ks)
    return c


def id_of(family, name, Ks):
    return f"{name}-{Ks}"


# ---------------------------------------------------------------------------------------------------------------------------
# facts and edges (CPU): what a case hits, derived from its arrays and the oracle -- never from its name
# ---------------------------------------------------------------------------------------------------------------------------
def facts(c, oracle):
    pnl = panel()
    per_grid, max_word = pair_facts(c.rc, c.which)
    f = dict(layout=layout_facts(c.rc, pnl.nGrids), rows=carried_rows(c.rc, c.which), pairs=per_grid, max_word=max_word,
             named=named_in_csr(c.rc), n_inf=informative_counts(c, c.which), cols=oracle_columns(c, c.which, oracle),
             raw=oracle_columns(c, c.which, oracle, rescale=False), T_all=c.rc.nSNPs_all)
    if c.which_b is not None:
        f["n_inf_b"] = informative_counts(c, c.which_b)
        f["cols_b"] = oracle_columns(c, c.which_b, oracle)
    return f


def edges_of(c, f):
    s, rc = c.sample, c.rc
    cs = common_index(rc)
    e = set()
    for g, lay in enumerate(f["layout"]):
        if lay["n_common"] == 0:
            e.add("grid_without_common_snp")
        if len(lay["cgs"]) == 2:
            e.add("grid_over_two_common_grids")
            if lay["cgs"][1] == panel().nGrids - 1:
                e.add("second_word_is_last_common_grid")
        if lay["second_word_guarded"]:
            e.add("second_word_guarded_by_Gc")
        if lay["first_b"] in (0, SNPS_PER_GRID - 1):
            e.add(f"first_common_b{lay['first_b']}")
        if lay["n_common"] == 1:
            e.add("single_common_snp")
        if f["pairs"][g] == SNPS_PER_GRID * c.Ks:
            e.add("grid_of_32Ks_pairs")
        if f["pairs"][g] == 1:
            e.add("grid_of_one_pair")
        if f["pairs"][g] == 0:
            e.add("grid_without_pairs")
    last = f["layout"][-1]
    e.add(f"last_grid_{last['nLocal']}_snps")
    T = f["T_all"]
    e.add("last_snp_common" if cs[T - 1] >= 0 else ("last_snp_rare_carried" if T - 1 in f["rows"] else "last_snp_rare_uncarried"))
    if f["named"] - set(f["rows"]):
        e.add("named_in_csr_but_no_selected_carrier")
    if not f["named"]:
        e.add("empty_csr")
    for t, rows in f["rows"].items():
        if len(rows) == 1:
            e.add(f"part_{rows[0] % PARTS}")
            if rows[0] in (0, 63, 64, c.Ks - 1):
                e.add("single_row_" + ("last" if rows[0] == c.Ks - 1 else str(rows[0])))
        if len(rows) == c.Ks:
            e.add("carried_by_every_row")
        if max(rows) > 511:
            e.add("row_above_511")
        if t % SNPS_PER_GRID in (0, SNPS_PER_GRID - 1):
            e.add(f"carried_at_bit_{t % SNPS_PER_GRID}")
    if f["max_word"] == 0x7FFF:
        e.add("pair_word_0x7FFF")
    for k in (0, K - 1):
        if rc.rare_ptr[k + 1] > rc.rare_ptr[k]:
            e.add(f"csr_row_{'first' if k == 0 else 'last'}_nonempty")
    lens = {int(rc.rare_ptr[k] - rc.rare_ptr[k - 1]) for k in c.which}
    covered = {int(t) for t, q in zip(s.u, s.bq) if q != 0 and t in f["rows"]}
    if covered:
        for n in lens:
            e.add("bisect_list_of_" + ("0" if n == 0 else "1" if n == 1 else "about_40" if 35 <= n <= 45 else "some"))
    for k in c.which:
        lst = rc.rare_snp[rc.rare_ptr[k - 1]:rc.rare_ptr[k]] - 1
        if 35 <= len(lst) <= 45:
            for t in covered:
                if t == lst[0]:
                    e.add("probe_first")
                elif t == lst[-1]:
                    e.add("probe_last")
                elif t in lst:
                    e.add("probe_inside")
                elif t < lst[0]:
                    e.add("probe_absent_below")
                elif t > lst[-1]:
                    e.add("probe_absent_above")
                else:
                    e.add("probe_absent_between")
    rare_base = cs[s.u] < 0
    for r in range(s.nReads):
        a, b = int(s.read_ptr[r]), int(s.read_ptr[r + 1])
        v = slice(a, a + min(b - a - 1, c.Jmax) + 1)
        carried = np.array([int(t) in f["rows"] for t in s.u[v]])
        if rare_base[v].all():
            e.add("rare_only_read")
            nxt_same_block = r + 1 < s.nReads and (r + 1) // READS_PER_WAVE == r // READS_PER_WAVE
            first_in_block_so_far = all(rare_base[s.read_ptr[q]:s.read_ptr[q + 1]].all() for q in range(r - r % READS_PER_WAVE, r))
            if carried.any() and nxt_same_block and first_in_block_so_far and not rare_base[s.read_ptr[r + 1]]:
                e.add("rare_only_then_common_in_block" + ("_2" if r >= READS_PER_WAVE else "_1"))
            if (f["cols"][:, r] == 1.0).all() and not carried.any():
                e.add("rare_only_all_ones")
        n = f["n_inf"][r]
        if n in (MAX_PATTERN_BITS, MAX_PATTERN_BITS + 1) and (carried & (s.bq[v] != 0)).any():
            e.add(f"n_inf_{n}_with_carried_rare")
            inf_idx = np.flatnonzero((read_cases.fold_qualities(s, c.Jmax)[v] != 0) & ((cs[s.u[v]] >= 0) | carried))
            if n == MAX_PATTERN_BITS + 1 and carried[inf_idx[-1]] and (cs[s.u[v]][inf_idx[:-1]] >= 0).all():
                e.add("sixth_informative_is_carried_rare")
            if not (cs[s.u[v]] >= 0).any():
                e.add(f"n_inf_{n}_carried_only")
        if b - a >= 100 and n <= MAX_PATTERN_BITS:
            e.add("compact_read_of_100_bases")
        off = block_offsets(s, r)[:v.stop - v.start]
        if {CHUNK - 2, CHUNK - 1, CHUNK, CHUNK + 1} <= set(off[rare_base[v]].tolist()):
            e.add("rare_bases_at_chunk_offsets_62_65")
        if {CHUNK - 1, CHUNK} <= set(off[carried].tolist()):
            e.add("carried_bases_either_side_of_chunk")
        if b - a - 1 > c.Jmax and carried[-1] and int(s.u[v.stop]) in f["rows"]:
            e.add("jmax_between_two_carried_rare")
        col, raw = f["cols"][:, r], f["raw"][:, r]
        if (col == 1 / c.maxdiff).any():
            e.add("floor_on_carried_rare" if carried.any() else "floor")
        if carried.any() and raw.min() == raw.max() and n > 0:
            e.add("informative_but_all_rows_equal")
        if r == 0 and s.bq[a] == 0 and carried[0]:
            e.add("chain_starts_without_quality_on_carried_rare")
        if (s.bq[v] == 0).any() and r > 0:
            e.add("folded_base_inside_rare_common_read")
        if "n_inf_b" in f:
            da, db = n > MAX_PATTERN_BITS, f["n_inf_b"][r] > MAX_PATTERN_BITS
            if da != db:
                e.add("dense_in_a_compact_in_b" if da else "compact_in_a_dense_in_b")
    return e


REQUIRED = {
    "SNPS_PER_GRID": {"grid_without_common_snp", "grid_over_two_common_grids", "second_word_is_last_common_grid", "second_word_guarded_by_Gc",
                      "first_common_b0", "first_common_b31", "single_common_snp", "last_grid_1_snps", "last_grid_31_snps", "last_grid_32_snps",
                      "last_snp_common", "last_snp_rare_carried", "carried_at_bit_31", "carried_at_bit_0", "grid_of_32Ks_pairs",
                      "grid_of_one_pair", "grid_without_pairs", "named_in_csr_but_no_selected_carrier", "empty_csr", "carried_by_every_row",
                      "csr_row_first_nonempty", "csr_row_last_nonempty", "bisect_list_of_0", "bisect_list_of_1", "bisect_list_of_about_40",
                      "probe_first", "probe_last", "probe_inside", "probe_absent_below", "probe_absent_between", "probe_absent_above"},
    "READS_PER_WAVE": {"rare_only_read", "rare_only_all_ones", "rare_only_then_common_in_block_1", "rare_only_then_common_in_block_2"},
    "CHUNK": {"rare_bases_at_chunk_offsets_62_65", "carried_bases_either_side_of_chunk", "compact_read_of_100_bases"},
    "MAX_PATTERN_BITS": {"n_inf_5_with_carried_rare", "n_inf_6_with_carried_rare", "sixth_informative_is_carried_rare", "n_inf_5_carried_only",
                         "n_inf_6_carried_only", "dense_in_a_compact_in_b", "compact_in_a_dense_in_b", "jmax_between_two_carried_rare",
                         "floor_on_carried_rare", "informative_but_all_rows_equal", "chain_starts_without_quality_on_carried_rare",
                         "folded_base_inside_rare_common_read"},
    "ROW_MASK": {"pair_word_0x7FFF", "row_above_511", "single_row_0", "single_row_63", "single_row_64", "single_row_last"},
    "PARTS": {f"part_{i}" for i in range(PARTS)},
}
assert tuple(REQUIRED) == CONSTANTS
