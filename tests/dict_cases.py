"""Constructed inputs for the dictionary axis of the full-panel passes (helper, no test; imports no device code).

A panel reaches the kernels as a per-grid dictionary: ``nMaxDH`` words per grid (``distinctHapsB``), a code per haplotype and grid
(``hapMatcherR``; code 0 = "special": the haplotype's own word is in the CSR lists), optionally ``distinctHapsIE``.  csrc/fullpass.hip
builds the emission table from these and the genotype likelihoods (k_emat: thread t = table row t, ``nrow = nMaxDH + 1`` rows over
four waves, the block's minimum and maximum through ``s_red[.][4]``, specials 256 at a time), the backward kernels fold gamma x sigma
into a histogram by code (fold_histogram: ``code < nrow``) and k_dosage turns that into the dosage (codes 1 + q, 9 + q .. into eight
partial sums; specials eight at a time; the ``prm.IE`` table where the panel's distinctHapsIE is not the expansion of its words).
Random panels put none of this ON an edge; the builders here do.

Every word of a planted grid is ``j << 21 | random << 11 | private``: bits 21 .. 29 hold the word's number j, bit 31 is set in the
first half of a grid's words and bit 30 in its last quarter, so the signed values ascend with j, and the counts never ascend with
j -- the word with number j is table row j + 1 (make_rhb_t_equality ranks by descending count, ties by ascending value) and the
words beyond nMaxDH are special.  Bits 11 .. 20 are random and carry the weak background reads.  Bits 0 .. 10 are PRIVATE SNPs: bit i
is set in one word of the grid only, so that one strong base on SNP i makes that word's emission the grid's largest (the base calls
the alternate allele) or smallest (it calls the reference allele), whatever the background says.  tests/test_dict_cases_cpu.py
proves every claim on the oracle; tests/test_dict_geometry_gpu.py runs the cases on the device.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import grid_cases as GC

WAVE = 64               # fullpass.hip k_emat: `const int wv = t >> 6` -- table row t belongs to wave t / 64, four entries in s_red
DOSAGE_SUMS = 8         # fullpass.hip k_dosage: `for (int d0 = 1; d0 < prm.nrow; d0 += 8)` -- eight partial sums acc0[q] / acc1[q]
KMAXROW = 256           # fullpass_dev.hpp: constexpr int kMaxRow (rows of a grid's table; nrow = nMaxDH + 1 <= kMaxRow)
SPECIAL_STRIDE = 256    # fullpass.hip k_emat: `for (int i = t; i < sn; i += 256)` -- a grid's specials, 256 at a time
SPECIAL_SUMS = 8        # fullpass.hip k_dosage: `for (int i0 = 0; i0 < sn; i0 += 8)`
CHUNK = 16              # haplotypes of a chunk: one uint4 of codes (apply_special_emissions, special_half<>)
CONSTANTS = ("WAVE", "DOSAGE_SUMS", "KMAXROW", "SPECIAL_STRIDE", "SPECIAL_SUMS", "CHUNK")

K, G, T = GC.K_BASE, 6, 192
K_TOP = 5
THIN = (0, 2, 3, 5)
MIN_GL = GC.MIN_GL
SEP_RTOL = GC.SEP_RTOL
PRIVATE_BITS = 11       # bits 0 .. 10
RANDOM_LO, RANDOM_BITS = 11, 10
J_SHIFT = 21
STRONG = 30             # phred of a base on a private SNP: 999 : 1 between match and mismatch, more than the background can undo
SEED = 9100
FP32_BAR, FP64_BAR = 2e-4, 1e-10     # the dosage bars of the fp32-state and of the fp64 dosage passes
BIN_WIDTHS = (8, 9, 64, 255)
SPECIAL_WIDTHS = (1, 8)
REF_ERROR = 1e-3


def widths():
    """The nMaxDH of the suite: both sides of every constant the row loops step by, and the ends."""
    out = {1, 2, KMAXROW - 2, KMAXROW - 1}
    for m in (DOSAGE_SUMS, 2 * DOSAGE_SUMS, WAVE, 2 * WAVE, 3 * WAVE):
        out |= {m - 1, m, m + 1}
    return tuple(sorted(out))


def special_counts(n):
    """Specials per grid at nMaxDH = n: none, one, both sides of k_dosage's eight, both sides of k_emat's 256, and every haplotype
    a word of its own -- all but the n that the dictionary holds are special (n = 1: K - 1, every haplotype but the commonest
    word's; a grid has specials only beyond n distinct words, so K - n is the most there can be)."""
    return (0, 1, SPECIAL_SUMS - 1, SPECIAL_SUMS, SPECIAL_SUMS + 1, SPECIAL_STRIDE - 1, SPECIAL_STRIDE, SPECIAL_STRIDE + 1, K - n)


def planted_rows(n):
    """Table rows (1-based: row r is thread r of k_emat) that carry a private SNP: the ends and both sides of every wave edge."""
    rows = {1, n}
    for w in (WAVE, 2 * WAVE, 3 * WAVE):
        rows |= {w - 1, w, w + 1}
    rows = sorted(r for r in rows if 1 <= r <= n)
    assert len(rows) <= PRIVATE_BITS
    return rows


# ---------------------------------------------------------------------------------------------------------------------------
# the case
# ---------------------------------------------------------------------------------------------------------------------------
@dataclass
class DictCase(GC.GridCase):
    symbols: bool = False             # use_eMatDH_special_symbols of the device panel and of the oracle
    threshold: float = 1e-100         # min_emission_prob_normalization_threshold the case is run under (lazy passes)
    fp32: bool = True                 # compared under the fp32-state bars too (False: the fp64 families only; claims say why)

    @property
    def has_reads(self):
        return self.sample is not None


def oracle_ref(c, kind, label=1, *, always_normalize=False, normalize_emissions=True, threshold=None, panel=None):
    """The oracle on one label of a case (``thin`` / ``dosage`` / ``full`` as tests.grid_cases.oracle_ref) under the options the
    single-pass entry takes.  ``panel``: the case's inputs on another panel of the same shape.  Shared: do not write into it."""
    from oracle import oracle as O
    threshold = c.threshold if threshold is None else threshold
    p = c.panel if panel is None else panel
    key = (c.name, id(p), kind, label, bool(always_normalize), bool(normalize_emissions), float(threshold))
    if key not in _ref:
        gl = c.gl if label == 1 else GC.label_gl(c, label)
        kw = dict(K_top_matches=c.K_top, get_best_haps_from_thinned_sites=True, always_normalize=always_normalize,
                  normalize_emissions=normalize_emissions, min_emission_prob_normalization_threshold=threshold,
                  use_eMatDH_special_symbols=c.symbols)
        if kind == "thin":
            r = O.haploid_dosage_versus_refs(p, gl, c.cols, return_dosage=False, **kw)
        elif kind == "dosage":
            r = O.haploid_dosage_versus_refs(p, gl, c.cols, return_dosage=True, return_gamma_t=True, **kw)
        elif kind == "full":
            r = O.haploid_dosage_versus_refs(p, gl, c.cols, return_dosage=True, return_gamma_t=True, return_betaHat_t=True, **kw)
        else:
            raise ValueError(kind)
        _ref[key] = (r, p)     # (the panel is held: its id is part of the key)
    return _ref[key][0]


_ref = {}


# ---------------------------------------------------------------------------------------------------------------------------
# words, grids, panels
# ---------------------------------------------------------------------------------------------------------------------------
def make_words(m, rng):
    """m words with ascending signed values: number j in bits 21 .. 29, random bits 11 .. 20, private bits clear; bit 31 (the sign)
    on the first half and bit 30 on the last quarter, which keeps the order and lets SNPs 30 and 31 tell words apart.  From two
    words on, the last word's random bits are the complement of the first's: the two are far apart whatever the seed."""
    assert m <= 1 << (30 - J_SHIFT)
    w = (np.arange(m, dtype=np.uint32) << np.uint32(J_SHIFT)) | (rng.integers(0, 1 << RANDOM_BITS, size=m).astype(np.uint32)
                                                                  << np.uint32(RANDOM_LO))
    if m >= 2:
        mask = np.uint32(((1 << RANDOM_BITS) - 1) << RANDOM_LO)
        w[m - 1] = (w[m - 1] & ~mask) | (~w[0] & mask)
    h1 = (m + 1) // 2
    h2 = (m + h1 + 1) // 2
    w[:h1] |= np.uint32(1 << 31)
    w[h2:] |= np.uint32(1 << 30)
    assert np.all(np.diff(w.view(np.int32).astype(np.int64)) > 0)
    return w


def even_counts(total, m):
    """``total`` haplotypes over m words, never ascending."""
    c = np.full(m, total // m, dtype=np.int64)
    c[:total % m] += 1
    assert c.min() >= 1 and c.sum() == total
    return c


def grid_column(words, counts, rng, Kn=K, fixed=None):
    """The word of every haplotype of a grid: word j on counts[j] haplotypes, dealt at random; ``fixed`` {haplotype: j} first."""
    pool = np.repeat(np.arange(len(words)), counts)
    assert len(pool) == Kn
    col = np.full(Kn, -1, dtype=np.int64)
    if fixed:
        pool = pool.tolist()
        for k, j in fixed.items():
            pool.remove(j)
            col[k] = j
        pool = np.array(pool, dtype=np.int64)
    free = np.flatnonzero(col < 0)
    col[free] = rng.permutation(pool)
    return words[col], col


def _panel(rhb_words, nMaxDH, nSNPs=T, ref_error=REF_ERROR):
    from tests.util import panel_from_rhb
    Gn = rhb_words.shape[1]
    like = GC.base_panel(G, T)
    tm = like.transMatRate_t[:, :Gn - 1]
    rhb = np.asfortranarray(rhb_words.astype(np.uint32).view(np.int32))
    p = panel_from_rhb(rhb, tm, nSNPs, nMaxDH, ref_error)
    assert p.nMaxDH == nMaxDH
    return p


KINDS = ("full", "plus_one", "fewer", "single", "full", "plus_one")     # the grids of a width panel


def _grid_kind_words(kind, n):
    """(number of words, counts) of a grid of kind ``kind`` at nMaxDH = n."""
    if kind == "fewer" and n == 1:
        kind = "single"                       # (no grid has fewer than one word)
    if kind == "full":
        return n, even_counts(K, n)
    if kind == "plus_one":                    # the last word on ONE haplotype: it ties with the rarest and has the largest value
        return n + 1, np.r_[even_counts(K - 1, n), 1]
    if kind == "fewer":
        return n // 2, even_counts(K, n // 2)
    return 1, np.array([K])


@lru_cache(maxsize=None)
def width_panel(n, nSNPs=T, ref_error=REF_ERROR):
    """K = 300, G = 6 at nMaxDH = n: grid 0 and 4 hold exactly n words (no special), grids 1 and 5 n + 1 (one special haplotype),
    grid 2 n / 2 (zero-word padding rows), grid 3 one word.  The planted rows of every grid carry their private SNPs.  ``nSNPs`` <
    192: a ragged last grid, bits beyond it clear."""
    rng = np.random.default_rng(SEED + n)
    rows = planted_rows(n)
    rhb = np.zeros((K, G), dtype=np.uint32)
    for g, kind in enumerate(KINDS):
        m, counts = _grid_kind_words(kind, n)
        words = make_words(m, rng)
        for i, r in enumerate(rows):
            if r <= min(m, n):
                words[r - 1] |= np.uint32(1 << i)
        rhb[:, g], _ = grid_column(words, counts, rng)
    n_last = nSNPs - 32 * (G - 1)
    if n_last < 32:
        rhb[:, G - 1] &= np.uint32((1 << n_last) - 1)
    return _panel(rhb, n, nSNPs, ref_error)


def n_words(panel, g):
    return len(np.unique(np.asarray(panel.rhb_t)[:, g]))


def n_special(panel, g):
    return int((np.asarray(panel.hapMatcherR)[:, g] == 0).sum())


# ---------------------------------------------------------------------------------------------------------------------------
# reads
# ---------------------------------------------------------------------------------------------------------------------------
def background_reads(panel, seed, label, per_grid=2, phred=(1, 4), along=None):
    """Weak single-base reads along one haplotype (``along``, or one drawn from the seed) on the random bits (11 .. 20) of every
    grid: they never touch a private SNP.  Two bases of phred 4 or less: at most 20 : 1 between the best and the worst word,
    far less than the 750 : 1 of one strong base."""
    from quilt_amd.synth import panel_hap_bits
    rng = np.random.default_rng(seed)
    k = int(rng.integers(0, panel.K))
    bits = panel_hap_bits(panel, k if along is None else along)
    reads = []
    for g in range(panel.nGrids):
        n = min(32, panel.nSNPs - 32 * g)
        pool = np.arange(RANDOM_LO, min(RANDOM_LO + RANDOM_BITS, n))
        if not len(pool):
            pool = np.arange(n)
        for t in np.sort(rng.choice(pool, size=min(per_grid, len(pool)), replace=False)):
            t = 32 * g + int(t)
            q = int(rng.integers(phred[0], phred[1] + 1))
            reads.append(([t], [q if bits[t] else -q], label))
    return reads


def private_reads(i_min, i_max, label=1, n_grids=G):
    """One strong base per grid on private SNP i_min calling the reference allele (its word mismatches: the grid's minimum) and one
    on private SNP i_max calling the alternate (its word alone matches: the grid's maximum)."""
    reads = []
    for g in range(n_grids):
        if i_min is not None:
            reads.append(([32 * g + i_min], [-STRONG], label))
        if i_max is not None and i_max != i_min:
            reads.append(([32 * g + i_max], [STRONG], label))
    return reads


def _reads_case(name, panel, reads, group, claims, **kw):
    s, H = GC.sample_of(reads, panel.nGrids)
    return DictCase(name, panel, s, H, GC.cols_of(panel.nGrids, THIN), K_top=K_TOP, claims=claims, group=group, **kw)


def _gl_case(name, panel, gl, group, claims, thin=THIN, K_top=K_TOP, **kw):
    return DictCase(name, panel, None, None, GC.cols_of(panel.nGrids, thin), K_top=K_top, claims=claims, group=group,
                    _gl=np.asfortranarray(gl, dtype=np.float64), **kw)


def gl_of_reads(panel, reads):
    from oracle import oracle as O
    u = np.array([t for r in reads for t in r[0]], dtype=np.int32)
    bq = np.array([b for r in reads for b in r[1]], dtype=np.int32)
    return O.make_gl_from_u_bq(u, bq, panel.nSNPs, MIN_GL)


# ---------------------------------------------------------------------------------------------------------------------------
# emission tables restated (what the claims are made of)
# ---------------------------------------------------------------------------------------------------------------------------
def word_emissions(words, gl, g, ref_error):
    """The emission of 32-bit words at grid g: the product over the grid's SNPs of the (eps, 1 - eps) mix of gl."""
    Tn = gl.shape[1]
    s, n = 32 * g, min(32, Tn - 32 * g)
    words = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    out = np.ones(len(words))
    for b in range(n):
        x, y = gl[0, s + b], gl[1, s + b]
        e_ref, e_alt = x * (1 - ref_error) + y * ref_error, x * ref_error + y * (1 - ref_error)
        out = out * np.where((words >> b) & 1, e_alt, e_ref)
    return out


def table(panel, gl, g, normalize_emissions=True):
    """What the reference holds for grid g: (table rows 1 .. nMaxDH after normalisation, the specials' emissions after theirs, the
    grid's min_emission_prob, emission_max) -- reference-single.cpp:985-1057 restated; row 0 of the reference's table is the
    minimum of the others."""
    from oracle import oracle as O
    e = O.build_eMatDH(panel.distinctHapsB, gl, panel.nGrids, panel.nSNPs, panel.ref_error, add_zero_row=True)[:, g]
    emax = e.max()
    rows = e.copy()
    sp_scale = 1.0
    if normalize_emissions:
        if emax < 1:
            rows = rows * (1 / emax)
        sp_scale = 1 / emax
    ks = np.flatnonzero(np.asarray(panel.hapMatcherR)[:, g] == 0)
    sp = word_emissions(np.asarray(panel.rhb_t)[ks, g], gl, g, panel.ref_error) * sp_scale
    return rows[1:], sp, min(rows.min(), sp.min(initial=np.inf)), emax


def has_variant(gl, g):
    return not (gl[:, 32 * g:32 * g + 32] == 1).all()


def running_minimum(panel, gl, upto, normalize_emissions=True, skip_row=None):
    """The running product of min_emission_prob over grids 1 .. ``upto`` (no renormalisation in between); ``skip_row`` (grid, row):
    with that table row left out of that grid's minimum."""
    run = 1.0
    for g in range(1, upto + 1):
        if not (has_variant(gl, g) or g == 1):
            continue
        rows, sp, emin, _ = table(panel, gl, g, normalize_emissions)
        if skip_row is not None and skip_row[0] == g:
            emin = min(np.delete(rows, skip_row[1] - 1).min(initial=np.inf), sp.min(initial=np.inf))
        run *= emin
    return run


# ---------------------------------------------------------------------------------------------------------------------------
# 1. dictionary width: the minimum and the maximum on every planted row
# ---------------------------------------------------------------------------------------------------------------------------
MINMAX_GRID = 4         # a full grid past grid 0: its minimum is the one the planted threshold hangs on


@lru_cache(maxsize=None)
def width_cases(n):
    """One case per planted row i of the nMaxDH = n panel: the grids' minimum on planted row i, their maximum on planted row
    i + 1 (cyclic).  The threshold is planted between the running product of the minima up to MINMAX_GRID and what that product
    would be without the minimum row of MINMAX_GRID: the lazy passes renormalise at that grid, and would not with any other
    row's emission for the minimum."""
    p = width_panel(n)
    rows = planted_rows(n)
    out = []
    for i, r in enumerate(rows):
        i_max = (i + 1) % len(rows)
        name = f"dh{n}_min{r}_max{rows[i_max]}"
        reads = private_reads(i, i_max) + background_reads(p, SEED + 31 * n + i, 1) + background_reads(p, SEED + 31 * n + i + 500, 2)
        c = _reads_case(name, p, reads, f"dh{n}", dict(nMaxDH=n, min_row=r, max_row=rows[i_max], renorm=()))
        if len(rows) > 1:      # (nMaxDH = 1: one row is minimum and maximum, nothing to plant)
            true = running_minimum(p, c.gl, MINMAX_GRID)
            other = running_minimum(p, c.gl, MINMAX_GRID, skip_row=(MINMAX_GRID, r))
            c.threshold = float(np.sqrt(true * other))
            c.claims["renorm"] = (MINMAX_GRID,)
        out.append(c)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. code to bin
# ---------------------------------------------------------------------------------------------------------------------------
BIN_FP32 = {8: True, 9: True, 64: False, 255: False}    # whether the masses are far enough apart for the fp32 bar (CPU file)


@lru_cache(maxsize=None)
def bin_case(n):
    """Reads of moderate total weight on the nMaxDH = n panel: one base of phred 1 or 2 on every random SNP of every grid, so that
    any two words of a grid differ in emission; in the full grids every code is a word of its own and holds its own share of
    gamma.  (The seed is the first of SEED + 7000 + n + 50 i for which the two narrow widths meet the fp32 bar's condition in
    tests/test_dict_cases_cpu.py.)"""
    p = width_panel(n)
    reads = background_reads(p, SEED + 7100 + n, 1, per_grid=RANDOM_BITS, phred=(1, 2)) + background_reads(p, SEED + 7500 + n, 2)
    return _reads_case(f"bins_dh{n}", p, reads, f"bins_dh{n}", dict(nMaxDH=n, bins=True, fp32=BIN_FP32[n]), fp32=BIN_FP32[n])


def masses(c, g, label=1):
    """m_d of grid g, d = 0 .. nMaxDH: the oracle's gamma summed by code (bin 0: the specials)."""
    gamma = oracle_ref(c, "dosage", label)["gamma_t"][:, g]
    codes = np.asarray(c.panel.hapMatcherR)[:, g]
    return np.bincount(codes, weights=gamma, minlength=c.panel.nMaxDH + 1)


def dosage_from_masses(panel, g, m, gamma_col, IE=None):
    """k_dosage restated: dosage[32 g + b] = sum_d IE[d, b] m_d + sum over the specials of gamma_k (bit ? 1 - eps : eps), divided
    by the mass the histogram holds (gamma sums to 1 over a grid).  ``m``: nMaxDH + 1 masses, bin 0 the specials'."""
    n = min(32, panel.nSNPs - 32 * g)
    IE = panel.distinctHapsIE if IE is None else IE
    ks = np.flatnonzero(np.asarray(panel.hapMatcherR)[:, g] == 0)
    w = np.asarray(panel.rhb_t)[ks, g].astype(np.int64) & 0xFFFFFFFF
    eps = panel.ref_error
    out = np.zeros(n)
    for b in range(n):
        sp = (gamma_col[ks] * np.where((w >> b) & 1, 1 - eps, eps)).sum()
        out[b] = (IE[:, 32 * g + b] * m[1:]).sum() + sp
    return out / m.sum()


def bin_sensitivity(c, g):
    """The smallest change of any dosage of grid g, over every code d, when bin d is lost or swapped with bin d +- 1 or d +- 8:
    (lost, swapped), each the minimum over d of the largest change over the grid's SNPs."""
    p = c.panel
    m = masses(c, g)
    gamma = oracle_ref(c, "dosage")["gamma_t"][:, g]
    base = dosage_from_masses(p, g, m, gamma)
    lost, swapped = np.inf, np.inf
    for d in range(1, p.nMaxDH + 1):
        x = m.copy()
        x[d] = 0
        lost = min(lost, np.abs(dosage_from_masses(p, g, x, gamma) - base).max())
        for e in (d - DOSAGE_SUMS, d - 1, d + 1, d + DOSAGE_SUMS):
            if 1 <= e <= p.nMaxDH:
                x = m.copy()
                x[d], x[e] = m[e], m[d]
                swapped = min(swapped, np.abs(dosage_from_masses(p, g, x, gamma) - base).max())
    return lost, swapped


# ---------------------------------------------------------------------------------------------------------------------------
# 3. specials
# ---------------------------------------------------------------------------------------------------------------------------
SPECIAL_LAYOUTS = dict(g0_only=(SPECIAL_STRIDE + 1, 0, 0, 0, 0, 0), last_only=(0, 0, 0, 0, 0, SPECIAL_STRIDE),
                       mid_only=(0, 0, 0, SPECIAL_STRIDE - 1, 0, 0),
                       every_a=(1, SPECIAL_SUMS - 1, SPECIAL_SUMS, SPECIAL_SUMS + 1, SPECIAL_STRIDE - 1, "all"),
                       every_b=("all", SPECIAL_STRIDE, SPECIAL_STRIDE + 1, 1, SPECIAL_SUMS + 1, SPECIAL_SUMS - 1))
BIT_HI, BIT_LO = 0, 1     # the private SNPs of a grid's first special (emission above every table row) and of its last (the minimum)


def _special_grid(n, count, rng, Kn=K, special_haps=None):
    """A grid with ``count`` special haplotypes at nMaxDH = n: n common words share the others, every special has a word of its
    own (one haplotype each: rarer than, or tied with and larger than, every common word).  The first special (ascending haplotype) carries private bit 0, the last (if there are two)
    private bit 1."""
    assert Kn - count >= n
    words = make_words(n + count, rng)
    counts = np.r_[even_counts(Kn - count, n), np.ones(count, dtype=np.int64)]
    fixed = None
    if special_haps is not None:
        assert len(special_haps) == count
        fixed = {int(k): n + i for i, k in enumerate(sorted(special_haps))}
    col_words, col = grid_column(words, counts, rng, Kn, fixed)
    ks = np.flatnonzero(col >= n)
    if len(ks):
        col_words[ks[0]] |= np.uint32(1 << BIT_HI)
    if len(ks) >= 2:
        col_words[ks[-1]] |= np.uint32(1 << BIT_LO)
    return col_words


@lru_cache(maxsize=None)
def special_panel(n, layout):
    rng = np.random.default_rng(SEED + 100 * n + sorted(SPECIAL_LAYOUTS).index(layout))
    rhb = np.zeros((K, G), dtype=np.uint32)
    for g, count in enumerate(SPECIAL_LAYOUTS[layout]):
        rhb[:, g] = _special_grid(n, K - n if count == "all" else count, rng)
    return _panel(rhb, n)


def _special_reads(p, seed):
    """Label 1: on every grid a strong alternate base on the first special's private SNP and a strong reference base on the last
    special's, over the weak background; label 2 the background alone."""
    return private_reads(BIT_LO, BIT_HI, n_grids=p.nGrids) + background_reads(p, seed, 1) + background_reads(p, seed + 500, 2)


@lru_cache(maxsize=None)
def special_case(n, layout, symbols=False):
    p = special_panel(n, layout)
    name = f"sp_dh{n}_{layout}" + ("_symbols" if symbols else "")
    counts = tuple(n_special(p, g) for g in range(G))
    return _reads_case(name, p, _special_reads(p, SEED + 3000 + 10 * n + sorted(SPECIAL_LAYOUTS).index(layout)), name,
                       dict(nMaxDH=n, special_counts=counts, layout=layout), symbols=symbols)


# chunks of 16 haplotypes whose specials are planted by position
CHUNK_PATTERNS = ("all", "low", "high")


@lru_cache(maxsize=None)
def chunk_K():
    """The smallest K (no multiple of 16, one whole chunk past the edge) at which the fp32 family runs two chunk rows."""
    from tests import k_cases as KC
    k = 16
    while KC.geometry(k, "f32")["NCH"] < 2:
        k += 16
    return k - 15 + 16 + 12


def chunk_positions(Kn):
    """{where: chunk}: the first chunk, the first chunk of the fp32 family's second chunk row, the chunk that holds K - 1."""
    from tests import k_cases as KC
    geo = KC.geometry(Kn, "f32")
    assert geo["NCH"] >= 2
    return dict(first=0, second_row=geo["NT"], last=(Kn - 1) // CHUNK)


def chunk_special_haps(Kn, g):
    """The special haplotypes of grid g of the chunk panel: pattern (g + i) mod 3 at position i -- over three grids every pattern
    at every position; grids 3 .. 5 repeat 0 .. 2."""
    out = set()
    for i, (where, ch) in enumerate(sorted(chunk_positions(Kn).items())):
        pat = CHUNK_PATTERNS[(g + i) % 3]
        lo, hi = {"all": (0, 16), "low": (0, 8), "high": (8, 16)}[pat]
        out |= {k for k in range(CHUNK * ch + lo, CHUNK * ch + hi) if k < Kn}
    return sorted(out)


@lru_cache(maxsize=None)
def chunk_panel():
    Kn, n = chunk_K(), 8
    rng = np.random.default_rng(SEED + 555)
    rhb = np.zeros((Kn, G), dtype=np.uint32)
    for g in range(G):
        sp = chunk_special_haps(Kn, g)
        rhb[:, g] = _special_grid(n, len(sp), rng, Kn, sp)
    return _panel(rhb, n)


@lru_cache(maxsize=None)
def chunk_case(symbols=False):
    p = chunk_panel()
    name = "sp_chunks" + ("_symbols" if symbols else "")
    return _reads_case(name, p, _special_reads(p, SEED + 5550), name, dict(nMaxDH=8, chunks=True), symbols=symbols)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. emissions: gl inputs
# ---------------------------------------------------------------------------------------------------------------------------
EMIT_DH = 9             # the panel of the variant-position and no-variant cases
MIN_GL_DH = 255         # ... of the MIN_GL cases: enough words that some table rows fall below fp32's range
ONE_BELOW = 1 - 2.0 ** -53


def _background_gl(p, seed):
    return gl_of_reads(p, background_reads(p, seed, 1))


def _only_variant(p, seed, g, b):
    """The weak background with grid g silent but for local SNP b, where gl = (0.2, 1)."""
    gl = _background_gl(p, seed)
    gl[:, 32 * g:32 * g + 32] = 1
    gl[:, 32 * g + b] = (0.2, 1.0)
    return gl


@lru_cache(maxsize=None)
def emission_cases():
    out = []
    p = width_panel(EMIT_DH)
    seed = SEED + 9000
    for name, g, b in (("only_snp0", 2, 0), ("only_snp31", 2, 31), ("only_snp31_g0", 0, 31), ("only_snp31_g1", 1, 31),
                       ("only_snp31_last", G - 1, 31)):
        out.append(_gl_case(f"emit_{name}", p, _only_variant(p, seed, g, b), "emit", dict(only_variant=(g, b))))
    for n_last in (1, 31):
        pr = width_panel(EMIT_DH, 32 * (G - 1) + n_last)
        out.append(_gl_case(f"emit_ragged{n_last}_last_snp", pr, _only_variant(pr, seed, G - 1, n_last - 1), f"emit_ragged{n_last}",
                            dict(only_variant=(G - 1, n_last - 1), last_grid_snps=n_last)))
    for name, quiet in (("g0", (0,)), ("g1", (1,)), ("g0_g1", (0, 1)), ("g2", (2,)), ("g1_g2", (1, 2)), ("all", tuple(range(G)))):
        gl = _background_gl(p, seed + 1)
        for g in quiet:
            gl[:, 32 * g:32 * g + 32] = 1
        out.append(_gl_case(f"emit_novar_{name}", p, gl, "emit", dict(novar=quiet)))
    # the largest table row exactly 1.0 (every word that holds the reference allele at the one variant SNP), and just below
    for name, pair in (("emax_one", (1.0, ONE_BELOW)), ("emax_below_one", (ONE_BELOW, ONE_BELOW))):
        gl = _background_gl(p, seed + 2)
        gl[:, 32 * 3:32 * 4] = 1
        gl[:, 32 * 3 + 12] = pair
        gl[:, 32 * 4:32 * 5] = 1
        gl[:, 32 * 4 + 12] = pair
        # (no thinned grid: words that differ at that SNP alone differ by one rounding in emission, and so do the gammas of their
        # haplotypes -- no order to compare)
        out.append(_gl_case(f"emit_{name}", p, gl, "emit_emax", dict(emax=name, emax_grids=(3, 4)), thin=()))
    # MIN_GL on all 32 SNPs of grid 4, along the word of table row 1: that row alone keeps an emission near 1
    for eps in (1e-3, 1e-4):
        pm = width_panel(MIN_GL_DH, T, eps)
        gl = _background_gl(pm, seed + 3)
        w = int(np.asarray(pm.distinctHapsB)[0, 4]) & 0xFFFFFFFF
        for b in range(32):
            gl[:, 32 * 4 + b] = (MIN_GL, 1.0) if (w >> b) & 1 else (1.0, MIN_GL)
        # (K_top = 2: the two haplotypes of that word lead every list; all others keep 1e-12 of their history through this grid
        # and are told apart by less than the separation rule asks)
        out.append(_gl_case(f"emit_min_gl_eps{eps:g}", pm, gl, f"emit_min_gl_eps{eps:g}", dict(min_gl_grid=4, ref_error=eps), K_top=2))
    return tuple(out)


SCHEDULE_THRESHOLD = 1e-30   # planted: the weak background of the schedule panel reaches about 1e-71 over the region


@lru_cache(maxsize=None)
def threshold_cases():
    """The schedule cases of the grid suite that never renormalise under the default (`none`) or at the block edge only, again
    under a threshold the background alone crosses."""
    out = []
    for which in ("none", "block_edge"):
        c = GC.schedule_case(which)
        out.append(DictCase(f"thr_{which}", c.panel, c.sample, c.labels, c.cols, K_top=c.K_top, group="thr",
                            claims=dict(default_renorm=tuple(GC.SCHEDULES[which])), threshold=SCHEDULE_THRESHOLD))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a free distinctHapsIE
# ---------------------------------------------------------------------------------------------------------------------------
IE_DH = 9
IE_OTHER_ERROR = 5e-3
IE_ENTRY = 0.25


@lru_cache(maxsize=None)
def ie_panels():
    """(the derived panel, {name: the same panel with another distinctHapsIE})"""
    from quilt_amd.panel import int_expand
    p = width_panel(IE_DH)
    bits = int_expand(p.distinctHapsB).reshape(IE_DH, G * 32)[:, :T]
    other = np.asfortranarray(np.where(bits == 1, 1 - IE_OTHER_ERROR, IE_OTHER_ERROR).astype(np.float64))
    entry = np.array(p.distinctHapsIE, order="F")
    entry[IE_DH - 1, T - 1] = IE_ENTRY
    return p, dict(other_error=dataclasses.replace(p, distinctHapsIE=other), one_entry=dataclasses.replace(p, distinctHapsIE=entry))


@lru_cache(maxsize=None)
def ie_cases():
    """Moderate reads along a haplotype that holds the LAST code in the last grid, on each panel: {name: (case on the free panel,
    the same case on the derived one)}."""
    derived, free = ie_panels()
    k = int(np.flatnonzero(np.asarray(derived.hapMatcherR)[:, G - 1] == IE_DH)[0])
    reads = background_reads(derived, SEED + 8000, 1, per_grid=6, phred=(3, 8), along=k) + background_reads(derived, SEED + 8500, 2)
    base = _reads_case("ie_base", derived, reads, "ie", {})
    out = {}
    for name, p in free.items():
        mk = lambda panel, nm: DictCase(nm, panel, base.sample, base.labels, base.cols, K_top=K_TOP, group=nm, claims=dict(ie=name))
        out[name] = (mk(p, f"ie_{name}"), mk(derived, f"ie_{name}_derived"))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the lists
# ---------------------------------------------------------------------------------------------------------------------------
def special_cases():
    out = [special_case(n, layout, sym) for n in SPECIAL_WIDTHS for layout in SPECIAL_LAYOUTS for sym in (False, True)]
    return out + [chunk_case(False), chunk_case(True)]


@lru_cache(maxsize=None)
def all_cases():
    out = [c for n in widths() for c in width_cases(n)] + [bin_case(n) for n in BIN_WIDTHS] + special_cases()
    out += list(emission_cases()) + list(threshold_cases()) + [c for pair in ie_cases().values() for c in pair]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return {c.name: c for c in all_cases()}[name]


def groups():
    """The cases that can share one qa_fullpass_batch call (one panel, one set of columns, the default form of the specials), two
    or more."""
    out = {}
    for c in all_cases():
        if not c.symbols:
            out.setdefault(c.group, []).append(c)
    return {g: cs for g, cs in out.items() if len(cs) > 1}


def separation(c, width=None):
    """tests.grid_cases.separation among the first ``width`` + 1 ranks, for the labels the case has."""
    worst = np.inf
    width = c.K_top if width is None else width
    for label in ((1, 2) if c.has_reads else (1,)):
        gamma = oracle_ref(c, "dosage", label)["gamma_t"]
        for g in c.thin_grids:
            v = np.sort(gamma[:, g])[::-1][:width + 1]
            hi, lo = v[:-1], v[1:]
            gap = (hi - lo)[hi != lo] / hi[hi != lo]
            worst = min(worst, gap.min(initial=np.inf))
    return float(worst)
