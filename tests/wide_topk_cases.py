"""Constructed inputs for K_top_matches in 9 .. 64 (helper, no test; imports no device code).

Up to kMaxTop = 8 the fp64 ranking kernels pick the lists themselves; beyond it every family hands the column to the wide form of
k_topk (csrc/fullpass.hip): per-lane lists of 8, a lower bound of the threshold from them, a gather of what lies above the bound
when a lane may have dropped such a value.  The cases are tests/grid_cases.py's builders at the new values -- lists of exactly
K_top, ties that reach across the threshold, lists beyond the 64-entry first capacity, a panel smaller than K_top, a label whose
gammas all tie -- and panels of several chunk rows of 8 192 haplotypes, where the listed haplotypes lie in a second row, in the
partial last one and in a row the ranking kernels stream through HBM.  tests/test_wide_topk_cases_cpu.py checks every claim
against the oracle alone; tests/test_wide_topk_gpu.py runs the cases on the device.
"""
from __future__ import annotations

from dataclasses import replace
from functools import lru_cache

import numpy as np

from tests import grid_cases as GC

K_TOP_MAX = 64          # include/quilt_amd.h: QA_K_TOP_MATCHES_MAX
K_TOPS = (9, 16, 33, 63, 64)
TIES = ((8, 9), (9, 9), (10, 9), (40, 33), (64, 64), (65, 64), (2, 64))   # (m copies, K_top): lists of max(K_top, m)
ROW = 8192              # fullpass64.hip: haplotypes of a chunk row
ROWS_ON_CHIP = 7        # ... and the rows a pass keeps on chip; the rows beyond stream through HBM
BIG_K = (8500, 33000, 57600)
BIG_G = 16
BIG_COLS = (0, 8, 15)
LANE_TIES = ((20, 33), (40, 33), (64, 64))   # (m copies in ONE lane of the picker, K_top)
LANE_K = 33000
WIDE_LIST = 2048        # fullpass.hip: constexpr int kWideList (values above the lower bound that the wide picker gathers in LDS)
OVERFLOW_K, OVERFLOW_LANES = 80000, 7

# The seed of each case's reads: the first of 0, 1, 2 ... (the panels of several rows: of 100, 101, ...) for which the oracle's
# gammas are separate (GC.SEP_RTOL) among the 65 first ranks of every thinned grid, for both labels, and for which label 1's lists
# have the lengths the case states (the panels of several rows: K_top distinct values among the first K_top ranks).  Found with
# the checks of tests/test_wide_topk_cases_cpu.py, which holds every case to them.
SEEDS = {"tie_m8_ktop9": 6, "tie_m9_ktop9": 6, "tie_m40_ktop33": 3, "tie_m2_ktop64": 9,
         "rows_K8500": 100, "rows_K33000": 100, "rows_K57600": 102}


def _named(c, name, **kw):
    return replace(c, name=name, group=name, _gl=None, **kw)


def rows_case(K, seed=None):
    """K haplotypes over G = 16 grids, lists of K_top = 64 at grids 0, 8 and 15: 2, 5 and 8 chunk rows, the last one partial."""
    name = f"rows_K{K}"
    p = GC.base_panel(BIG_G, 32 * BIG_G, K=K, seed=7800)
    s, H = GC.sample_of(GC.background(p, SEEDS[name] if seed is None else seed, **GC.TIE_READS), BIG_G)
    return GC.GridCase(name, p, s, H, GC.cols_of(BIG_G, BIG_COLS), K_top=K_TOP_MAX, claims=dict(K=K, rows=(K + ROW - 1) // ROW),
                       group=name)


def picker_lane(k, epv):
    """The thread of k_topk (256 of them) that reads haplotype k: columns are stored lane-interleaved, 16 haplotypes per (chunk,
    thread of the pass) as 16-byte vectors of ``epv`` elements (2: fp64 state, 4: fp32 state); thread t of the picker takes the
    vectors t, t + 256, ...  Whatever the pass geometry, that is vector (k & 15) // epv, modulo 4, of chunk (k >> 4) & 63."""
    k = np.asarray(k)
    return (((k & 15) // epv) & 3) * 64 + ((k >> 4) & 63)


def _planted_copies(like, where, random_row=None):
    """The row of haplotype ``where[0]`` at every haplotype of ``where`` (as GC.tie_case plants its copies); ``random_row``: a seed,
    for a row of fresh random words instead (few grids: a natural row has many equals in a large panel)."""
    rhb = np.array(like.rhb_t, order="F")
    if random_row is not None:
        rhb[where[0], :] = np.random.default_rng(random_row).integers(-2 ** 31, 2 ** 31, size=like.nGrids).astype(np.int32)
    rhb[where, :] = rhb[where[0], :]
    return GC.planted_panel(rhb, like)


def lane_tie_case(m, K_top, seed=None):
    """K = 33 000: m copies of one row at haplotypes 1024 a + 80 and 1024 a + 81 -- one thread of the picker in both element types
    reads them all, keeps eight, and its lower bound of the threshold falls short: the values above it are gathered.  m < K_top: the
    threshold lies among the other haplotypes; m >= K_top: it is the copies' value."""
    name = f"lane_m{m}_ktop{K_top}"
    like = GC.base_panel(BIG_G, 32 * BIG_G, K=LANE_K, seed=7800)
    where = np.sort(np.concatenate([1024 * np.arange(LANE_K // 1024) + 80 + e for e in (0, 1)]))[:m]
    p = _planted_copies(like, where)
    seed = SEEDS.get(name, 0) if seed is None else seed
    s, H = GC.sample_of(GC.weak_reads(p, seed, 1, along=int(where[0]), **GC.TIE_READS) + GC.weak_reads(p, seed + 1000, 2), BIG_G)
    return GC.GridCase(name, p, s, H, GC.cols_of(BIG_G, BIG_COLS), K_top=K_top,
                       claims=dict(tie=m, source=int(where[0]), copies=tuple(where.tolist()), list_len=max(K_top, m), one_lane=True), group=name)


def overflow_case(seed=None):
    """K = 80 000, K_top = 64: every haplotype that seven threads of the fp64 picker read is a copy of one row, 7 x 316 = 2 212 equal
    gammas at the head of every list.  The per-lane lists hold 56 of them, the lower bound is the eighth best of the others, and
    more values lie above it than the 2 048 the LDS list holds: the bound is raised from what was caught and the gather repeats."""
    name = f"overflow_K{OVERFLOW_K}"
    like = GC.base_panel(4, 128, K=OVERFLOW_K, seed=7800)
    k = np.arange(OVERFLOW_K)
    where = k[picker_lane(k, 2) < OVERFLOW_LANES]
    p = _planted_copies(like, where, random_row=7601)
    seed = SEEDS.get(name, 0) if seed is None else seed
    s, H = GC.sample_of(GC.weak_reads(p, seed, 1, along=int(where[0]), **GC.TIE_READS) + GC.weak_reads(p, seed + 1000, 2), 4)
    return GC.GridCase(name, p, s, H, GC.cols_of(4, (0, 3)), K_top=K_TOP_MAX,
                       claims=dict(tie=len(where), source=int(where[0]), copies=tuple(where.tolist()), list_len=len(where), overflow=True),
                       group=name)


def builders():
    """Every case as (name, builder of the case from a seed)."""
    out = [(f"ktop{k}", lambda seed, k=k: GC.K_top_case(k, seed=seed)) for k in K_TOPS]
    out += [(f"tie_m{m}_ktop{k}", lambda seed, m=m, k=k: GC.tie_case(m, k, seed=seed)) for m, k in TIES]
    out.append(("small_K20_ktop33", lambda seed: _named(GC.small_K_case(20, seed=seed), "small_K20_ktop33", K_top=33)))
    # (the seed of GC's own all_tie_K1025: the case as tests/grid_cases.py has it, at the widest K_top)
    out.append(("all_tie_K1025_ktop64", lambda seed: _named(GC.all_tie_case(1025), "all_tie_K1025_ktop64", K_top=K_TOP_MAX)))
    out += [(f"rows_K{K}", lambda seed, K=K: rows_case(K, seed=seed)) for K in BIG_K]
    out += [(f"lane_m{m}_ktop{k}", lambda seed, m=m, k=k: lane_tie_case(m, k, seed=seed)) for m, k in LANE_TIES]
    out.append((f"overflow_K{OVERFLOW_K}", lambda seed: overflow_case(seed=seed)))
    return out


@lru_cache(maxsize=None)
def all_cases():
    out = []
    for name, f in builders():
        c = f(SEEDS.get(name, 0))
        assert c.name == name
        out.append(c)
    assert not set(c.name for c in out) & set(GC.case_names()), "GC.oracle_ref shares results by name"
    return tuple(out)


def case_names():
    return [n for n, _ in builders()]


def small_case_names():
    return [n for n in case_names() if not n.startswith("rows_")]


def case(name):
    return {c.name: c for c in all_cases()}[name]


# ---------------------------------------------------------------------------------------------------------------------------
# coverage, derived from what the ORACLE says about a case (as GC.edges_of does), never from its name
# ---------------------------------------------------------------------------------------------------------------------------
def facts(c):
    f = GC.facts(c)
    lists = [GC.oracle_ref(c, "thin", label)["best_haps"] for label in (1, 2)]
    f["lens2"] = tuple(len(i) for i, _ in lists[1])
    f["rows_listed"] = tuple(sorted({int(k) // ROW for i, _ in lists[0] for k in i}))
    f["distinct_head"] = tuple(len(set(np.sort(v)[::-1][:c.K_top].tolist())) for _, v in lists[0])
    f["all_equal"] = all(len(set(v.tolist())) == 1 for _, v in lists[0])
    # the most entries of a list that one thread of the picker reads (fp64 and fp32 state), and how many values lie above the
    # picker's first lower bound: the K_top-th largest of what 256 lists of eight retain
    f["in_one_lane"] = {epv: max(int(np.bincount(picker_lane(i, epv)).max()) for i, _ in lists[0]) for epv in (2, 4)}
    gamma = GC.oracle_ref(c, "dosage", 1)["gamma_t"]
    lane = picker_lane(np.arange(c.panel.K), 2)
    above = []
    for g in c.thin_grids:
        col = gamma[:, g]
        kept = np.concatenate([np.sort(col[lane == t])[::-1][:GC.KMAXTOP] for t in range(256)])
        bound = np.sort(kept)[::-1][c.K_top - 1] if len(kept) >= c.K_top else 0.0
        above.append(int((col > bound).sum()))
    f["above_first_bound"] = tuple(above)
    return f


def edges_of(f):
    K, K_top, lens = f["K"], f["K_top"], set(f["lens"])
    e = {f"K_top={K_top}"} if GC.KMAXTOP < K_top <= K_TOP_MAX else set()
    if lens == {K_top} and K > K_top:
        e.add("a list of exactly K_top")
    if all(K_top < n < K for n in lens):
        e.add("a list longer than K_top through a tie")
    if any(n > GC.LIST_CAP for n in f["lens"] + f["lens2"]):
        e.add("a list longer than 64")
    if K < K_top and lens == {K}:
        e.add("K < K_top")
    if K > K_top and f["all_equal"] and lens == {K}:
        e.add("all tie")
    last = (K - 1) // ROW
    if any(r >= 1 for r in f["rows_listed"]):
        e.add("listed haplotypes in a second chunk row")
    if last >= 1 and K % ROW and last in f["rows_listed"]:
        e.add("listed haplotypes in the last row, which is partial")
    if any(r >= ROWS_ON_CHIP for r in f["rows_listed"]):
        e.add("listed haplotypes in a streamed row")
    if all(n > GC.KMAXTOP for n in f["in_one_lane"].values()):
        e.add("more than 8 of a list in one lane of the picker" + (", threshold below them" if min(lens) > max(f["in_one_lane"].values())
                                                                  else ", threshold among them"))
    if all(K_top <= n <= WIDE_LIST for n in f["above_first_bound"]):
        e.add("the threshold comes from the gathered values")
    if all(n > WIDE_LIST for n in f["above_first_bound"]):
        e.add("more values above the first bound than the gather holds")
    return e


def required_edges():
    return {f"K_top={k}" for k in K_TOPS} | {
        "a list of exactly K_top", "a list longer than K_top through a tie", "a list longer than 64", "K < K_top", "all tie",
        "listed haplotypes in a second chunk row", "listed haplotypes in the last row, which is partial",
        "listed haplotypes in a streamed row", "more than 8 of a list in one lane of the picker, threshold below them",
        "more than 8 of a list in one lane of the picker, threshold among them", "the threshold comes from the gathered values",
        "more values above the first bound than the gather holds"}
