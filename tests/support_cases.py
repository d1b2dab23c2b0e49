"""Constructed inputs for the three integer kernel files around the hot path (helper, no test; imports no device code).

csrc/panel_build.hip ranks a grid's words in an LDS hash table of kHT slots that it reuses for every grid a workgroup takes, up to
kMaxDistinct distinct words; csrc/match.hip walks four haplotypes per thread and picks the longest runs with a 256-wide scan over a
histogram of kMaxRunLen lengths; csrc/select.hip goes through 64 candidates at a time and subsamples the rank that fills Knew.
Panels from quilt_amd.synth and lists from a real full-panel pass meet those constants by accident; the builders here place their
inputs ON them.  Every builder returns a case with a name and ``claims`` -- what the builder says about its input (distinct words
per grid, the zero word's rank, where a cut falls, which branch the selection takes).  tests/test_support_cases_cpu.py checks every
claim against the host restatements alone; tests/test_support_geometry_gpu.py runs the cases on the device.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

KHT = 8192              # panel_build.hip: constexpr int kHT (hash slots per grid)
KMAXDISTINCT = 4096     # panel_build.hip: constexpr int kMaxDistinct (distinct non-zero words the device ranks)
KBT = 256               # panel_build.hip: constexpr int kBT (threads of k_rank_words / k_list_specials)
RANK_BLOCKS = 512       # panel_build.hip: qa_panel_create_from_rhb, blocks = std::min(G, 512)
KMAXRUNLEN = 4096       # match.hip: constexpr int kMaxRunLen (positions per index the histogram holds)
HAPS_PER_BLOCK = 1024   # match.hip: k_best_run, 4 haplotypes per thread x 256 threads
PICK_CHUNK = 256        # match.hip: k_pick_runs, for (int k0 = 0; k0 < K; k0 += 256)
WAVE = 64               # select.hip: k_select, for (int base = 0; base < n_cand; base += 64)
SLAB = 64 << 20         # panel_build.hip: qa_make_rhb_t_from_rhi_t, ((int64_t)64 << 20) alleles per upload slab
LDS_BYTES = 160 << 10   # select.hip: launch_select, 160 KB per workgroup on gfx950
NMAXDH_ALL = (255, 40, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# panel build
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class RhbPanel:
    """What DevicePanel.from_rhb and make_rhb_t_equality read of a panel: the packed haplotypes and the scalars around them."""
    rhb_t: np.ndarray
    nSNPs: int
    nMaxDH: int = 255
    ref_error: float = 1e-3
    transMatRate_t: np.ndarray = None

    def __post_init__(self):
        self.rhb_t = np.asfortranarray(self.rhb_t, dtype=np.int32)
        self.K, self.nGrids = self.rhb_t.shape
        assert (self.nSNPs + 31) // 32 == self.nGrids
        if self.transMatRate_t is None:
            self.transMatRate_t = trans_mat(self.nGrids)


def trans_mat(G):
    """transMatRate_t (2 x (G - 1)).  G = 1 has no transition: the array keeps ONE unused column there;
    qa_panel_create_from_rhb reads G - 1 = 0 columns of whatever it is given (tests/test_grid_geometry_gpu.py passes it none)."""
    sigma = np.full(max(G - 1, 1), 0.97)
    return np.asfortranarray(np.stack([sigma, 1.0 - sigma], axis=0))


@dataclass
class PanelCase:
    name: str
    panel: RhbPanel
    nMaxDHs: tuple = NMAXDH_ALL
    claims: dict = field(default_factory=dict)


def hash_word(w):
    """panel_build.hip: hash_word, restated ONLY so that `clustered` can pick its words."""
    w = np.asarray(w, dtype=np.uint64) & 0xffffffff
    w ^= w >> 16
    w = (w * 0x7feb352d) & 0xffffffff
    w ^= w >> 15
    w = (w * 0x846ca68b) & 0xffffffff
    w ^= w >> 16
    return (w & (KHT - 1)).astype(np.int64)


def distinct_words(rng, n, zero=False):
    """n distinct int32 words, none of them 0, signs alternating (even entries negative); ``zero``: the last one replaced by 0."""
    mag = rng.choice(2 ** 31 - 2, size=n, replace=False).astype(np.int64) + 1
    w = np.where(np.arange(n) % 2 == 0, -mag, mag)
    if zero:
        w[-1] = 0
    return w.astype(np.int32)


def column_with_counts(rng, words, counts):
    col = np.repeat(np.asarray(words, dtype=np.int32), np.asarray(counts, dtype=np.int64))
    return col[rng.permutation(len(col))]


def rank_of_zero(col):
    """1-based rank of the zero word in a grid under the rule (count descending, signed value ascending), 0 = absent: a second
    statement of the ranking, next to make_rhb_t_equality."""
    vals, cnt = np.unique(np.asarray(col, dtype=np.int32), return_counts=True)
    order = np.lexsort((vals, -cnt))
    at = np.flatnonzero(vals[order] == 0)
    return int(at[0]) + 1 if len(at) else 0


def n_distinct_nonzero(col):
    v = np.unique(col)
    return int((v != 0).sum())


def many_grids(ragged=False):
    """K = 70, G = 520 > 512 workgroups: grids 512 .. 519 are the SECOND grid of workgroups 0 .. 7, on the LDS table, counters and
    sort scratch their first grid left behind.  A grid and its partner 512 further on differ in the number of distinct words and in
    whether the zero word occurs; grids 3, 200 and 519 hold one word only, so they have no special at any nMaxDH."""
    K, G = 70, 520
    rng = np.random.default_rng(101)
    one_word = (3, 200, 519)
    n_dist = np.array([1 if g in one_word else 2 + (g * 7) % 61 for g in range(G)])
    has_zero = np.array([(g % 2 == 0) != (g >= RANK_BLOCKS) for g in range(G)])
    rhb = np.zeros((K, G), dtype=np.int32, order="F")
    for g in range(G):
        w = distinct_words(rng, n_dist[g], zero=has_zero[g])
        cnt = np.ones(n_dist[g], dtype=np.int64)
        np.add.at(cnt, rng.integers(0, max(n_dist[g] // 3, 1), size=K - n_dist[g]), 1)   # a skewed spectrum
        rhb[:, g] = column_with_counts(rng, w, cnt)
    nSNPs = 32 * G
    if ragged:
        nSNPs -= 13
        assert (rhb[:, G - 1] == 0).all()   # the last grid holds 19 SNPs: its one word is 0, no bit beyond them is set
    claims = dict(G=G, n_distinct=n_dist, has_zero=has_zero, one_word=one_word)
    return PanelCase("many_grids_ragged" if ragged else "many_grids", RhbPanel(rhb, nSNPs), claims=claims)


def _full_grid(rng, K, n_nonzero, zero_count):
    """A grid of K haplotypes with n_nonzero distinct non-zero words (+ zero_count copies of 0): most words occur once, the first
    ten occur (10, 10, 6, 6, 4, 4, 3, 3, 2, 2 ...) times -- equal counts in pairs of a negative and a positive word -- and whatever
    is left goes to the first word."""
    w = distinct_words(rng, n_nonzero)
    cnt = np.ones(n_nonzero, dtype=np.int64)
    extra = K - n_nonzero - zero_count
    assert extra >= 0
    for i, a in enumerate((9, 9, 5, 5, 3, 3, 2, 2, 1, 1)):
        a = min(a, extra)
        cnt[i] += a
        extra -= a
    cnt[0] += extra
    return column_with_counts(rng, np.r_[w, np.int32(0)], np.r_[cnt, zero_count])


def table_full():
    """K = 4300.  Grids 0 / 1 / 2 hold 4095 / 4096 / 4097 distinct non-zero words: below the device ranker's capacity, AT it (with the
    zero word n = 4097 sort entries, padded to np2 = 8192, the whole scratch slice) and the first host-ranked shape; grid 3 is one
    word; grids 4 and 5 are grids 0 and 1 without the zero word (n = 4096 = np2 exactly for grid 5).  The zero word, where present,
    occurs 6 times: tied with a negative and a positive word."""
    K = 4300
    rng = np.random.default_rng(102)
    spec = [(KMAXDISTINCT - 1, 6), (KMAXDISTINCT, 6), (KMAXDISTINCT + 1, 6), None, (KMAXDISTINCT - 1, 0), (KMAXDISTINCT, 0)]
    rhb = np.zeros((K, len(spec)), dtype=np.int32, order="F")
    for g, s in enumerate(spec):
        rhb[:, g] = np.int32(-77) if s is None else _full_grid(rng, K, *s)
    claims = dict(n_nonzero=[KMAXDISTINCT - 1, KMAXDISTINCT, KMAXDISTINCT + 1, 1, KMAXDISTINCT - 1, KMAXDISTINCT],
                  has_zero=[True, True, True, False, False, False],
                  device_ranked=[True, True, False, True, True, True])
    return PanelCase("table_full", RhbPanel(rhb, 32 * len(spec)), claims=claims)


def ties_by_sign():
    """K = 3000, every word of a grid distinct (count 1), half of them with bit 31 set: below the device ranker's capacity, and the
    255 codes go to the 255 LOWEST SIGNED words -- all negative.  Grid 1 has the zero word among them."""
    K = 3000
    rng = np.random.default_rng(103)
    rhb = np.zeros((K, 2), dtype=np.int32, order="F")
    for g in range(2):
        rhb[:, g] = distinct_words(rng, K, zero=g == 1)[rng.permutation(K)]
    return PanelCase("ties_by_sign", RhbPanel(rhb, 64), nMaxDHs=(255,), claims=dict(K=K, n_negative=K // 2))


def _ranked_grid(rng, K, D, zero_at, tie=False):
    """D distinct words with strictly decreasing counts D, D - 1, .. 1 (the first takes what is left of K), so that the rank of
    every word is its position; the word at 1-based rank ``zero_at`` is 0 (None: absent).  ``tie``: the words ranked zero_at - 1,
    zero_at, zero_at + 1 get the same count and are (negative, 0, positive)."""
    w = distinct_words(rng, D)
    cnt = np.arange(D, 0, -1).astype(np.int64)
    cnt[0] += K - cnt.sum()
    if zero_at is not None:
        w[zero_at - 1] = 0
    if tie:
        w[zero_at - 2] = -abs(int(w[zero_at - 2]))
        w[zero_at] = abs(int(w[zero_at]))
        cnt[zero_at - 2:zero_at + 1] = cnt[zero_at - 1]      # (c + 1, c, c - 1) -> (c, c, c)
        cnt[0] += K - cnt.sum()
    return column_with_counts(rng, w, cnt)


ZERO_RANKS = (1, 40, 41, 2, 40, 0)   # per grid of zero_rank(); grid 4 is the tie; 0 = absent


def zero_rank():
    """K = 1500, 50 distinct words per grid, one grid per place of the zero word: rank 1 (the most frequent; = nMaxDH for nMaxDH = 1),
    rank 40 (= nMaxDH for 40), rank 41 (nMaxDH + 1 for 40: every zero haplotype is special), rank 2 (nMaxDH + 1 for 1), rank 40 by the
    tie rule alone (same count as a negative word, which comes before it, and a positive word, which comes after and is special
    at nMaxDH = 40), and absent."""
    K, D = 1500, 50
    rng = np.random.default_rng(104)
    rhb = np.zeros((K, len(ZERO_RANKS)), dtype=np.int32, order="F")
    for g, r in enumerate(ZERO_RANKS):
        rhb[:, g] = _ranked_grid(rng, K, D, r or None, tie=g == 4)
    return PanelCase("zero_rank", RhbPanel(rhb, 32 * len(ZERO_RANKS)), claims=dict(zero_rank=ZERO_RANKS, tie_grid=4))


TINY_K = (1, 2, 255, 256, 257)


def tiny_K(K, G):
    """K at or below the 256-thread block (and one above): k_list_specials gives thread t the haplotypes [t * per, min(K, t * per +
    per)), an empty range with k1 < k0 for the trailing threads.  Five words per grid and nMaxDH in {1, 2}: every grid has specials
    as soon as it has more words than codes -- K = 1 cannot have any, K = 2 has one at nMaxDH = 1 (two words, count 1 each: the
    lower signed value takes the code).  The last haplotype is special in every grid of K >= 255.  G = 1: no transition, see
    trans_mat()."""
    rng = np.random.default_rng(105 + 10 * K + G)
    rhb = np.zeros((K, G), dtype=np.int32, order="F")
    for g in range(G):
        w = distinct_words(rng, 5, zero=g == 1)
        if K <= 2:
            rhb[:, g] = w[:K]
        else:
            col = w[np.minimum(rng.geometric(0.5, size=K) - 1, 4)]
            col[:5] = w                                  # every word occurs
            vals, cnt = np.unique(col, return_counts=True)
            col[K - 1] = vals[np.argmin(cnt)]            # the last haplotype: the rarest word, outside the two codes
            rhb[:, g] = col
    return PanelCase(f"tiny_K{K}_G{G}", RhbPanel(rhb, 32 * G), nMaxDHs=(1, 2),
                     claims=dict(K=K, G=G, specials_everywhere={1: K >= 2, 2: K >= 255}, last_special=K >= 255))


@lru_cache(maxsize=None)
def _clustered_words(slot, n):
    rng = np.random.default_rng(106)
    cand = np.unique(rng.integers(1, 2 ** 32, size=5_000_000, dtype=np.int64))
    h = hash_word(cand)
    out = []
    for s in (slot, (slot - 1) % KHT):
        w = cand[h == s]
        assert len(w) >= n, "too few candidates for one slot: hash more"
        out.append(w[rng.permutation(len(w))[:n]])
    return np.concatenate(out).astype(np.uint32).view(np.int32)


CLUSTER_SLOT, CLUSTER_N = 8000, 300


def clustered():
    """300 distinct words that hash_word sends to slot 8000 and 300 that it sends to slot 7999: the 600 occupy slots 7999 .. 8191 and
    wrap round to 0 .. 406, so inserts, the rank write-back and the code lookup all probe linearly over hundreds of slots and across
    the table's end.  The words were picked by hashing five million candidates with the restated hash: IF THE KERNEL'S HASH EVER
    CHANGES THIS CASE DEGRADES TO AN ORDINARY ONE (600 scattered words) -- it stays correct, it no longer pins the probing.  Grid 1
    adds the zero word, which lives outside the table."""
    K = 1500
    rng = np.random.default_rng(107)
    w = _clustered_words(CLUSTER_SLOT, CLUSTER_N)
    rhb = np.zeros((K, 2), dtype=np.int32, order="F")
    for g in range(2):
        cnt = np.ones(len(w), dtype=np.int64)
        np.add.at(cnt, rng.integers(0, 100, size=K - len(w) - 20 * g), 1)
        rhb[:, g] = column_with_counts(rng, np.r_[w, np.int32(0)], np.r_[cnt, 20 * g])
    return PanelCase("clustered", RhbPanel(rhb, 64), claims=dict(slot=CLUSTER_SLOT, n=CLUSTER_N))


def panel_cases():
    out = [many_grids(), many_grids(ragged=True), table_full(), ties_by_sign(), zero_rank(), clustered()]
    out += [tiny_K(K, G) for K in TINY_K for G in (3, 1)]
    return out


# ---- rhi -> rhb
@dataclass
class RhiCase:
    name: str
    K: int
    nSNPs: int
    claims: dict = field(default_factory=dict)

    def build(self):
        """K x nSNPs alleles (int32, Fortran order); any non-zero entry is an alternate allele."""
        rng = np.random.default_rng(108 + self.nSNPs)
        rhi = np.empty((self.K, self.nSNPs), dtype=np.int32, order="F")
        for t in range(self.nSNPs):
            rhi[:, t] = rng.integers(0, 2, size=self.K, dtype=np.int8)
        rhi[:, self.nSNPs - 1] *= 7
        return rhi

    def expected(self, rhi):
        G = (self.nSNPs + 31) // 32
        exp = np.zeros((self.K, G), dtype=np.int32, order="F")
        for g in range(G):
            bits = np.zeros((self.K, 32), dtype=np.uint8)
            n = min(32, self.nSNPs - 32 * g)
            bits[:, :n] = rhi[:, 32 * g:32 * g + n] != 0
            exp[:, g] = np.packbits(bits, axis=1, bitorder="little").view("<u4").ravel().view(np.int32)
        return exp


def slab_plan(K, nSNPs):
    """qa_make_rhb_t_from_rhi_t's upload plan: per slab (first grid, grids, SNPs uploaded)."""
    G = (nSNPs + 31) // 32
    per = max(1, min(G, SLAB // (32 * K)))
    return [(g0, min(per, G - g0), min(32 * min(per, G - g0), nSNPs - 32 * g0)) for g0 in range(0, G, per)]


def rhi_cases():
    """`rhi_two_slabs`: K = 2^20 + 3, 33 SNPs (138 MB of alleles): 32 K alleles per grid exceed half the slab, so a slab holds one
    grid and the second slab holds a single SNP -- k_pack_rhi indexes ``rhi`` relative to the slab and bounds the SNP absolutely.
    At 33 SNPs no K up to 2^20 reaches a second slab.  The small shapes sit around the kernel's 256-thread block, one slab each."""
    big = RhiCase("rhi_two_slabs", 2 ** 20 + 3, 33, dict(slabs=[(0, 1, 32), (1, 1, 1)]))
    small = [RhiCase(f"rhi_K{K}_T{T}", K, T, dict(slabs=[(0, (T + 31) // 32, T)])) for K, T in ((255, 33), (256, 64), (257, 95))]
    return [big] + small


# ---------------------------------------------------------------------------------------------------------------------------
# match
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class MatchCase:
    name: str
    rhb_t: np.ndarray
    nMaxDH: int
    Zs: np.ndarray            # [query][G] int32 words
    params: tuple             # of (nindices, min_len, max_matches)
    claims: dict = field(default_factory=dict)

    @property
    def panel(self):
        return _match_panel(self)


_panels = {}


def _match_panel(case):
    from tests.util import panel_from_rhb
    if case.name not in _panels:
        K, G = case.rhb_t.shape
        _panels[case.name] = panel_from_rhb(case.rhb_t, trans_mat(G), 32 * G, case.nMaxDH, 1e-3)
    return _panels[case.name]


def full_length_run(G=KMAXRUNLEN):
    """K = 5, G = 4096 = kMaxRunLen, the query is haplotype 0's own words: with one index its run is 4096 positions, the last bin of
    the histogram (and the largest value the uint16 run length has to hold here); with three indices the runs are 1366, 1365, 1365
    (4096 = 3 * 1365 + 1).  Random 32-bit words: no other haplotype shares one."""
    rng = np.random.default_rng(201)
    rhb = np.asfortranarray(rng.integers(-2 ** 31, 2 ** 31, size=(5, G), dtype=np.int64).astype(np.int32))
    return MatchCase(f"full_length_run_G{G}", rhb, 8, rhb[:1].copy(), ((1, 1, 5), (3, 1, 5)),
                     claims=dict(longest={1: [G], 3: [len(range(i, G, 3)) for i in range(3)]}))


def over_length_panel():
    """G = 4097: one index would have 4097 positions, more than the histogram holds; two have 2049 and 2048."""
    rng = np.random.default_rng(202)
    rhb = np.asfortranarray(rng.integers(1, 4, size=(2, KMAXRUNLEN + 1)).astype(np.int32))
    return MatchCase("over_length", rhb, 4, rhb[:1].copy(), ((1, 1, 2), (2, 1, 2)))


TILING_K = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 8192, 8193)
TILING_DEVICE_BUILT = (1, 4, 255, 257, 1024, 8192)   # the others are host-created panels
TILING_G = 12


@lru_cache(maxsize=None)
def _tiling_base():
    rng = np.random.default_rng(203)
    K, G = max(TILING_K), TILING_G
    rhb = np.zeros((K, G), dtype=np.int32, order="F")
    for g in range(G):
        rhb[:, g] = distinct_words(rng, 4, zero=g % 3 == 0)[rng.integers(0, 4, size=K)]
    return rhb


def tiling(K):
    """Row prefixes of one K = 8193, G = 12 panel over a 4-word alphabet per grid (runs are plentiful): K around k_best_run's four
    haplotypes per thread and 1024 per block, k_pick_runs' 256-wide scan, and the 8192 that Kp pads to.  Queries: haplotype 0, a
    mosaic of the first and the last haplotype, the last haplotype with a word that is in no dictionary at grids 4 and 5, random
    symbols.  nindices 1, 5 (does not divide 12: three indices of 3 positions, two of 2) and 12 (one position per index);
    max_matches 40 cuts inside ties at the large K and exceeds K at the small ones."""
    rng = np.random.default_rng(204)
    base = _tiling_base()
    rhb = np.asfortranarray(base[:K])
    q1 = base[0].copy()
    q2 = np.where(np.arange(TILING_G) < 7, base[0], base[K - 1]).astype(np.int32)
    q3 = base[K - 1].copy()
    q3[4:6] = 123456789
    q4 = np.array([base[rng.integers(0, max(TILING_K)), g] for g in range(TILING_G)], dtype=np.int32)
    return MatchCase(f"tiling_K{K}", rhb, 255, np.stack([q1, q2, q3, q4]), ((1, 2, 40), (5, 1, 300), (12, 1, 1000), (1, 1, K)),
                     claims=dict(K=K))


TIE_K, TIE_G = 700, 10


@lru_cache(maxsize=None)
def _tie_wall_rows():
    rng = np.random.default_rng(205)
    types = np.stack([distinct_words(rng, 3) for _ in range(TIE_G)], axis=1)   # [type][grid], all different within a grid
    types[1, :TIE_G // 2] = types[0, :TIE_G // 2]                              # type B = type A over the first half
    kind = rng.integers(0, 3, size=TIE_K)
    return types, kind


def tie_wall():
    """K = 700 rows, copies of three haplotypes in shuffled order: A, B (= A over grids 0 .. 4, different after) and C (different
    everywhere); the query is A.  With one index every A row has the longest run (10), every B row the next (5), C rows none: two
    tie groups of hundreds.  max_matches puts the cut inside a tie group -- inside the first 256-chunk of k_pick_runs, exactly at
    the end of that chunk (the quota is used up by the chunk's last tie), and inside the third chunk -- once in the A group
    (nothing above the threshold) and once in the B group (A rows above it, interleaved with the ties: the ``ra + min(rb, quota_b)``
    slots); then 1, K - 1, K and 2000, a min_len nothing reaches (11) and one that only the A rows reach (10)."""
    types, kind = _tie_wall_rows()
    rhb = np.asfortranarray(types[kind])
    isA, isB = kind == 0, kind == 1
    nA = int(isA.sum())
    cuts = {}
    for name, group, above in (("A", isA, 0), ("B", isB, nA)):
        c0, c01 = int(group[:PICK_CHUNK].sum()), int(group[:2 * PICK_CHUNK].sum())
        cuts[name] = dict(first_chunk=above + c0 // 2, chunk_boundary=above + c0, third_chunk=above + c01 + 7)
    params = [(1, 1, m) for c in cuts.values() for m in c.values()]
    params += [(1, 1, 1), (1, 1, TIE_K - 1), (1, 1, TIE_K), (1, 1, 2000), (1, TIE_G + 1, 50), (1, TIE_G, 2000), (1, TIE_G, 30)]
    return MatchCase("tie_wall", rhb, 255, types[:1].astype(np.int32), tuple(params),
                     claims=dict(cuts=cuts, nA=nA, nB=int(isB.sum()), isA=isA, isB=isB))


def no_symbol(zero_is_word, nMaxDH=255):
    """K = 300, G = 6, five words per grid.  ``zero_is_word`` False: no grid has the zero word and distinctHapsB has fewer than nMaxDH
    words, so its rows 6 .. are zero padding -- an all-zero query finds the FIRST padding row as its symbol, which no haplotype
    carries: no match.  True: zero is one of the five words and the same query matches the haplotypes that carry it.  The other
    queries: haplotype 7 with words of no dictionary at grids 1 and 4; haplotype 7 itself.  nMaxDH = 2 makes most haplotypes
    special (code 0): a query word that is a special's word is in no dictionary and matches nothing."""
    rng = np.random.default_rng(206 + int(zero_is_word))
    K, G = 300, 6
    rhb = np.zeros((K, G), dtype=np.int32, order="F")
    for g in range(G):
        rhb[:, g] = distinct_words(rng, 5, zero=zero_is_word)[np.minimum(rng.geometric(0.4, size=K) - 1, 4)]
    q_bad = rhb[7].copy()
    q_bad[[1, 4]] = [987654321, -5]
    Zs = np.stack([np.zeros(G, dtype=np.int32), q_bad, rhb[7].copy()])
    return MatchCase(f"no_symbol_zero{int(zero_is_word)}_dh{nMaxDH}", rhb, nMaxDH, Zs, ((1, 1, 50), (2, 1, 400), (6, 1, 10)),
                     claims=dict(zero_is_word=zero_is_word))


def match_cases():
    out = [full_length_run(), tie_wall(), no_symbol(False), no_symbol(True), no_symbol(False, 2), no_symbol(True, 2)]
    return out + [tiling(K) for K in TILING_K]


# ---------------------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------------------
SENTINEL = -7   # what the output rows hold before the call


@dataclass
class SelectCase:
    name: str
    K: int
    Ksubset: int
    Knew: int
    K_top_matches: int
    top_width: int
    top: np.ndarray           # [chain][label][thin][top_width], 0-based, -1 = no entry
    which: np.ndarray         # [chain][Ksubset], 1-based
    seeds: np.ndarray         # [chain] uint64
    want: np.ndarray          # [chain]
    claims: dict = field(default_factory=dict)   # per chain: ("subsample", rank, n_new - room) | ("exhausted",) | ("unwanted",)

    @property
    def n_chain(self):
        return self.top.shape[0]

    @property
    def n_cand(self):
        return self.top.shape[1] * self.top.shape[2]


def select_lds_bytes(K, n_cand, Ksubset):
    """select.hip: select_lds_bytes."""
    n_words = (K + 31) // 32
    return 4 * ((n_words + n_cand + 1) & ~1) + 8 * max(n_cand, Ksubset)


def trace_selection(case, chain):
    """The walk of everything_select_good_haps_dense over the ranks the device looks at, written a second time for the claims:
    per rank (n_new, room), and how it ends -- ("subsample", rank, n_new - room) or ("exhausted",)."""
    from quilt_amd.driver import previously_selected
    if not case.want[chain]:
        return [], ("unwanted",)
    prev = previously_selected(case.which[chain], case.Ksubset - case.Knew, int(case.seeds[chain]))
    seen = set((prev - 1).tolist())
    kept, steps = 0, []
    cols = case.top[chain].reshape(case.n_cand, case.top_width)
    for i in range(min(case.K_top_matches, case.top_width)):
        new = []
        for v in cols[:, i].tolist():
            if v >= 0 and v not in seen:
                seen.add(v)
                new.append(v)
        room = case.Knew - kept
        steps.append((len(new), room))
        if len(new) >= room:
            return steps, ("subsample", i, len(new) - room)
        kept += len(new)
    return steps, ("exhausted",)


class _Chain:
    """One chain's table under construction: columns of candidates per rank, filled from haplotypes that are new to the chain
    (``fresh``), haplotypes the chain keeps (``prev``), repeats and holes."""

    def __init__(self, rng, K, Ksubset, Knew, n_cand, width, seed):
        from quilt_amd.driver import previously_selected
        self.rng, self.n_cand, self.width = rng, n_cand, width
        self.which = np.sort(rng.choice(K, Ksubset, replace=False) + 1).astype(np.int32)
        self.seed = np.uint64(seed)
        self.prev0 = previously_selected(self.which, Ksubset - Knew, int(seed)).astype(np.int64) - 1
        pool = np.setdiff1d(np.arange(K), self.prev0)
        self.fresh = list(pool[rng.permutation(len(pool))])
        self.used = []
        self.cols = np.full((n_cand, width), -1, dtype=np.int32)

    def take(self, n):
        out, self.fresh = self.fresh[:n], self.fresh[n:]
        assert len(out) == n, "the panel has too few haplotypes for this table"
        return out

    def rank(self, i, n_new, junk=True):
        """n_new candidates new to the chain at scattered places of rank i; elsewhere kept haplotypes, repeats of earlier
        candidates and holes."""
        assert n_new <= self.n_cand
        at = self.rng.permutation(self.n_cand)
        new = self.take(n_new)
        self.cols[at[:n_new], i] = new
        for c in at[n_new:]:
            kind = self.rng.integers(0, 3) if junk else 2
            if kind == 0 and len(self.prev0):
                self.cols[c, i] = self.rng.choice(self.prev0)
            elif kind == 1 and (self.used or new):
                self.cols[c, i] = self.rng.choice(self.used + new)
        self.used += new


def _assemble(name, K, Ksubset, Knew, K_top, width, n_label, n_thin, chains, want=None, **claims):
    top = np.stack([c.cols.reshape(n_label, n_thin, width) for c in chains]).astype(np.int32)
    case = SelectCase(name, K, Ksubset, Knew, K_top, width, np.ascontiguousarray(top), np.stack([c.which for c in chains]),
                      np.array([c.seed for c in chains], dtype=np.uint64),
                      np.ones(len(chains), dtype=np.int32) if want is None else np.asarray(want, dtype=np.int32), claims)
    return case


def _chains(n, seed, K, Ksubset, Knew, n_cand, width):
    rng = np.random.default_rng(seed)
    return [_Chain(rng, K, Ksubset, Knew, n_cand, width, int(rng.integers(0, 2 ** 63))) for _ in range(n)]


def fill_cases():
    """`exact_fill` at rank 0 and at rank 2 (n_new == room: the subsample branch, which reorders the rank by key), `one_over`
    (n_new = room + 1) and `one_under` (n_new = room - 1: appended in list order, the next rank is subsampled).  Three chains each,
    different seeds."""
    K, Ksubset, Knew, n_label, n_thin, width = 900, 100, 30, 2, 20, 5
    out = []
    for name, per_rank, ends in (("exact_fill_rank0", (30,), ("subsample", 0, 0)),
                                 ("exact_fill_rank2", (8, 7, 15), ("subsample", 2, 0)),
                                 ("one_over", (8, 23), ("subsample", 1, 1)),
                                 ("one_under", (29, 12), ("subsample", 1, 11))):
        chains = _chains(3, 300 + len(out), K, Ksubset, Knew, n_label * n_thin, width)
        for c in chains:
            for i, n in enumerate(per_rank):
                c.rank(i, n)
            for i in range(len(per_rank), width):
                c.rank(i, 5)
        out.append(_assemble(name, K, Ksubset, Knew, width, width, n_label, n_thin, chains, ends=[ends] * 3))
    return out


def duplicates():
    """n_cand = 130 (three chunks of 64, 64, 2).  Rank 0 has haplotype X at lanes 0, 62 and 63 of the first chunk, at lane 3 of the
    second and in the third; Y twice in the second chunk; a kept haplotype at lanes 1 and 64.  Rank 1 repeats X and Y (an earlier
    rank) next to new ones.  Rank 0 is one short of Knew, so its order shows in the output; rank 1 is subsampled."""
    K, Ksubset, n_label, n_thin, width = 600, 40, 2, 65, 3
    n_first = 12
    Knew = n_first + 1
    chains = _chains(2, 310, K, Ksubset, Knew, n_label * n_thin, width)
    for c in chains:
        X, Y = c.take(2)
        new0 = c.take(n_first - 2)
        c.cols[[0, 62, 63, 64 + 3, 128], 0] = X
        c.cols[[64 + 10, 64 + 63], 0] = Y
        c.cols[[1, 64], 0] = c.prev0[0]
        c.cols[[5, 9, 20, 33, 61, 70, 90, 100, 120, 129], 0] = new0
        c.used += [X, Y] + new0
        c.cols[[0, 63, 64], 1] = [X, Y, X]
        c.cols[[2, 62, 65, 127, 128], 1] = c.take(5)
        c.cols[[3, 4], 1] = new0[:2]
    return _assemble("duplicates", K, Ksubset, Knew, width, width, n_label, n_thin, chains, ends=[("subsample", 1, 4)] * 2,
                     n_rank0=n_first)


N_CAND = ((1, 63), (1, 64), (1, 65), (3, 43))


def n_cand_cases():
    """63, 64, 65 and 129 (= 3 labels x 43) candidates: one chunk less a lane, one chunk, a chunk and one lane, two chunks and one
    lane.  Rank 0 has a hole at the last lane of every chunk (candidates 63, 127 where they exist, and the last candidate) and is
    short of Knew; rank 1 has new haplotypes exactly there."""
    out = []
    for n_label, n_thin in N_CAND:
        n = n_label * n_thin
        K, Ksubset, Knew, width = 800, 60, 50, 4
        chains = _chains(2, 320 + n, K, Ksubset, Knew, n, width)
        last = sorted({c for c in (63, 127, n - 1) if c < n})
        for c in chains:
            c.rank(0, 40, junk=False)
            c.cols[last, 0] = -1
            c.rank(1, 25)
            c.cols[last, 1] = c.take(len(last))
        out.append(_assemble(f"n_cand{n}", K, Ksubset, Knew, width, width, n_label, n_thin, chains, last_lanes=last))
    return out


BIT_K = (32, 33, 64, 65)


def bit_edges(K):
    """K at a word edge of the membership bits: the chain's panel and its candidates sit on haplotypes 0, 31, 32 and K - 1."""
    rng = np.random.default_rng(330 + K)
    edge = sorted({0, 31, min(32, K - 1), K - 1})
    Ksubset, Knew, n_thin, width = 6, 3, 8, 2
    chains = []
    for j in range(3):
        c = _Chain(rng, K, Ksubset, Knew, n_thin, width, int(rng.integers(0, 2 ** 63)))
        others = np.setdiff1d(np.arange(K), edge)
        c.which = (np.sort(np.r_[edge, rng.choice(others, Ksubset - len(edge), replace=False)]) + 1).astype(np.int32)
        c.cols[:, 0] = np.r_[edge, rng.choice(others, n_thin - len(edge), replace=False)][rng.permutation(n_thin)]
        c.cols[:, 1] = rng.permutation(K)[:n_thin]
        chains.append(c)
    return _assemble(f"bit_edges_K{K}", K, Ksubset, Knew, width, width, 1, n_thin, chains, edge=edge)


def Knew_extremes():
    """Knew == 0: the output is the chain's own panel in key order, status 0 (the first rank "overshoots" an empty room).
    Knew == Ksubset: nothing is kept.  Ksubset = 1 with both."""
    out = []
    for Ksubset, Knew in ((50, 0), (50, 50), (1, 0), (1, 1)):
        chains = _chains(2, 340 + Ksubset + Knew, 700, Ksubset, Knew, 2 * 30, 3)
        for c in chains:
            for i in range(3):
                c.rank(i, 40)
        out.append(_assemble(f"Knew{Knew}_of{Ksubset}", 700, Ksubset, Knew, 3, 3, 2, 30, chains,
                             ends=[("subsample", 0, 40 - Knew) if Knew <= 40 else ("subsample", 1, 80 - Knew)] * 2))
    return out


def width_cases():
    """top_width = K_top_matches = 64 on two candidates per rank: Knew = 127 is filled at the LAST rank (63), Knew = 129 never (status
    1).  top_width = 8 with K_top_matches = 3: ranks 3 .. 7 hold plenty of new candidates that must not be used -- chain 0 is short
    after rank 2 and is handed back, chain 1 is filled at rank 2."""
    out = []
    for Knew, ends in ((127, ("subsample", 63, 1)), (129, ("exhausted",))):
        chains = _chains(2, 350 + Knew, 2000, 200, Knew, 2, 64)
        for c in chains:
            for i in range(64):
                c.rank(i, 2)
        out.append(_assemble(f"width64_Knew{Knew}", 2000, 200, Knew, 64, 64, 1, 2, chains, ends=[ends] * 2))
    chains = _chains(2, 360, 900, 80, 30, 20, 8)
    for j, c in enumerate(chains):
        for i, n in enumerate((8, 7, 5 if j == 0 else 16, 20, 20, 20, 20, 20)):
            c.rank(i, n)
    out.append(_assemble("width8_top3", 900, 80, 30, 3, 8, 2, 10, chains, ends=[("exhausted",), ("subsample", 2, 1)]))
    return out


def exhausted():
    """The ranks run out for chains 0 and 3 (status 1); chain 1 is not wanted (status -1, its output row untouched) and sits between
    wanted chains; chain 2 is filled."""
    chains = _chains(4, 370, 900, 100, 60, 20, 4)
    for j, c in enumerate(chains):
        for i in range(4):
            c.rank(i, 20 if j == 2 else 10)
    return _assemble("exhausted", 900, 100, 60, 4, 4, 2, 10, chains, want=[1, 0, 1, 1],
                     ends=[("exhausted",), ("unwanted",), ("subsample", 2, 0), ("exhausted",)])


def too_large():
    """Ksubset = 20 600 on K = 21 000: 8 B x 20 600 keys alone exceed the 160 KB of LDS a workgroup can have, launch_select launches
    nothing and every wanted chain is handed back (status 1), the unwanted one reports -1."""
    K, Ksubset, Knew = 21000, 20600, 100
    chains = _chains(3, 380, K, Ksubset, Knew, 6, 2)
    for c in chains:
        c.rank(0, 6)
        c.rank(1, 6)
    return _assemble("too_large", K, Ksubset, Knew, 2, 2, 2, 3, chains, want=[1, 0, 1],
                     ends=[("exhausted",), ("unwanted",), ("exhausted",)], lds=select_lds_bytes(K, 6, Ksubset))


def shared():
    """Chains 0 and 2 share table, panel and seed and must agree; chain 1 has the same table and panel under another seed."""
    chains = _chains(1, 390, 900, 100, 30, 40, 3)
    c = chains[0]
    for i, n in enumerate((10, 35, 20)):
        c.rank(i, n)
    import copy
    other = copy.copy(c)
    other.seed = np.uint64(int(c.seed) ^ 0x5555)
    return _assemble("shared", 900, 100, 30, 3, 3, 2, 20, [c, other, c], twins=(0, 2))


def select_cases():
    out = fill_cases() + [duplicates()] + n_cand_cases() + [bit_edges(K) for K in BIT_K] + Knew_extremes() + width_cases()
    return out + [exhausted(), too_large(), shared()]
