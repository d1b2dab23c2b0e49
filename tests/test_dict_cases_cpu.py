"""The claims of tests/dict_cases.py, checked without a device: the panel tables and the oracle alone must say of every constructed
input what its builder says -- how many words and specials a grid holds, which table row is a grid's minimum and which its
maximum, where the lazy passes renormalise under the planted threshold, how much gamma every code holds, which specials sit where
-- and its gammas must be separate enough that the device's lists can be compared with no "allowed to differ" branch.  A case whose
claim fails here is a broken builder, and tests/test_dict_geometry_gpu.py would pin nothing with it.  No case is skipped; the
coverage table is derived from the same facts, never from a case's name."""
import numpy as np
import pytest

from tests import dict_cases as DC
from tests import grid_cases as GC

WIDTHS = DC.widths()
K, G = DC.K, DC.G


def _finite(c):
    kinds = [("thin", False), ("dosage", False), ("full", True)]
    for kind, always in kinds:
        r = DC.oracle_ref(c, kind, always_normalize=always)
        assert np.isfinite(r["c"]).all() and (r["c"] > 0).all()
        if kind != "thin":
            assert np.isfinite(r["dosage"]).all() and r["dosage"].min() >= 0 and r["dosage"].max() <= 1 + 1e-12
        assert len(r["best_haps"]) == len(c.thin_grids)
        for idx, val in r["best_haps"]:
            assert len(idx) >= min(c.K_top, c.panel.K) and np.isfinite(val).all() and (val > 0).all() and np.all(np.diff(idx) > 0)
    assert DC.separation(c) > DC.SEP_RTOL, "unequal gammas among the first K_top + 1 ranks of a thinned grid are apart"
    if c.has_reads:
        assert len(c.labels) == c.sample.nReads and np.all(np.diff(c.sample.wif) >= 0)


def _row_of_min_max(c, g):
    rows, sp, emin, emax = DC.table(c.panel, c.gl, g)
    return int(np.argmin(rows)) + 1, int(np.argmax(rows)) + 1, rows, sp, emin


# ---------------------------------------------------------------------------------------------------------------------------
# 1. dictionary width
# ---------------------------------------------------------------------------------------------------------------------------
def test_the_widths_are_the_edges_of_the_named_constants():
    assert WIDTHS == (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255)
    assert (DC.WAVE, DC.DOSAGE_SUMS, DC.KMAXROW) == (64, 8, 256)
    assert DC.special_counts(1) == (0, 1, 7, 8, 9, 255, 256, 257, K - 1) and DC.special_counts(8)[-1] == K - 8


@pytest.mark.parametrize("n", WIDTHS)
def test_width_panel(n):
    """Grid by grid: exactly n words and no special; n + 1 and one special haplotype; fewer, with zero-word padding rows; one
    word.  Word number j is table row j + 1, and a planted row's private SNP is set in that word alone."""
    p = DC.width_panel(n)
    assert (p.K, p.nGrids, p.nSNPs, p.nMaxDH) == (K, G, DC.T, n) and p.distinctHapsB.shape == (n, G)
    words = [DC.n_words(p, g) for g in range(G)]
    special = [DC.n_special(p, g) for g in range(G)]
    fewer = max(1, n // 2)
    assert words == [n, n + 1, fewer, 1, n, n + 1] and special == [0, 1, 0, 0, 0, 1]
    hm, B, rhb = np.asarray(p.hapMatcherR), np.asarray(p.distinctHapsB), np.asarray(p.rhb_t)
    assert hm.max() == n, "the last code is in use"
    for g in range(G):
        used = min(words[g], n)
        assert np.all(np.diff(B[:used, g].astype(np.int64)) > 0), "rows ascend in value: the word with number j is row j + 1"
        assert (B[used:, g] == 0).all(), "padding rows hold the zero word"
        assert np.all(np.diff(np.bincount(hm[:, g], minlength=n + 1)[1:used + 1]) <= 0)
        codes = hm[:, g]
        assert np.array_equal(B[codes[codes > 0] - 1, g], rhb[codes > 0, g])
        for i, r in enumerate(DC.planted_rows(n)):
            col = (rhb[:, g].astype(np.int64) >> i) & 1
            assert ((col == 1) == (codes == r)).all() if r <= used else not col.any(), (g, r)
    if n >= 2:
        assert words[2] < n and (B[fewer:, 2] == 0).all() and B.shape[0] > fewer
    # SNPs 30 and 31 tell words apart wherever a grid holds two
    for g in (0, 4):
        if n >= 2:
            assert len(set(((rhb[:, g].astype(np.int64) >> 31) & 1).tolist())) == 2


@pytest.mark.parametrize("n", WIDTHS)
def test_minimum_and_maximum_on_every_planted_row(n):
    """Per case of the width: in both full grids the smallest table row is the claimed one and the largest the other, each alone by
    a factor of ten; the padding rows of the `fewer` grid take part in both as the reference's zero words do; under the planted
    threshold the oracle renormalises at MINMAX_GRID and nowhere else, under the default nowhere, and with ANY other row for the
    minimum of that grid the running product would stay above the threshold."""
    cases = DC.width_cases(n)
    rows = DC.planted_rows(n)
    assert [c.claims["min_row"] for c in cases] == rows and sorted(c.claims["max_row"] for c in cases) == rows
    for c in cases:
        _finite(c)
        for g in (0, DC.MINMAX_GRID):
            lo, hi, e, sp, emin = _row_of_min_max(c, g)
            assert len(sp) == 0
            if n > 1:
                assert (lo, hi) == (c.claims["min_row"], c.claims["max_row"]), (c.name, g)
                s = np.sort(e)
                assert s[0] * 10 < s[1] and s[-2] * 10 < s[-1] and s[-1] >= 1 - 1e-15
        # the `fewer` grid: its padding rows are the zero word's emission, part of minimum and maximum
        e2 = DC.table(c.panel, c.gl, 2)[0]
        used = max(1, n // 2)
        if n >= 2:
            assert np.allclose(e2[used:], DC.word_emissions([0], c.gl, 2, c.panel.ref_error)[0] / DC.table(c.panel, c.gl, 2)[3])
        lazy = DC.oracle_ref(c, "thin")
        assert GC.renormalised(c, lazy["c"]) == c.claims["renorm"], c.name
        assert GC.renormalised(c, DC.oracle_ref(c, "thin", threshold=1e-100)["c"]) == ()
        if n > 1:
            true = DC.running_minimum(c.panel, c.gl, DC.MINMAX_GRID)
            other = DC.running_minimum(c.panel, c.gl, DC.MINMAX_GRID, skip_row=(DC.MINMAX_GRID, c.claims["min_row"]))
            assert true * 3 < c.threshold < other / 3 and c.threshold < DC.running_minimum(c.panel, c.gl, DC.MINMAX_GRID - 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. code to bin
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", DC.BIN_WIDTHS)
def test_every_code_holds_mass_that_a_mix_up_would_move(n):
    """The mat-vec restated in NumPy gives the oracle's dosage; and in the full grids, losing the mass of any one code, or
    swapping it with the code 1 or 8 away, moves some dosage by ten times the loosest bar the case is compared under.  Where
    the masses (about 1 / nMaxDH each) cannot reach ten times the fp32 bar the case is compared under the fp64 families only."""
    c = DC.bin_case(n)
    _finite(c)
    ref = DC.oracle_ref(c, "dosage")
    worst = np.inf
    for g in (0, DC.MINMAX_GRID):
        m = DC.masses(c, g)
        assert m[0] == 0 and (m[1:] > 0).all() and abs(m.sum() - 1) < 1e-12
        got = DC.dosage_from_masses(c.panel, g, m, ref["gamma_t"][:, g])
        assert np.abs(got - ref["dosage"][32 * g:32 * g + 32]).max() < 1e-12
        worst = min(worst, *DC.bin_sensitivity(c, g))
    print(f"nMaxDH = {n}: smallest movement {worst:.3g}")
    assert worst >= 10 * DC.FP64_BAR
    assert c.fp32 == c.claims["fp32"] == (worst >= 10 * DC.FP32_BAR), "the fp32 families take the case exactly where their bar can show it"


# ---------------------------------------------------------------------------------------------------------------------------
# 3. specials
# ---------------------------------------------------------------------------------------------------------------------------
def _resolved(n, layout):
    return tuple(K - n if x == "all" else x for x in DC.SPECIAL_LAYOUTS[layout])


@pytest.mark.parametrize("n", DC.SPECIAL_WIDTHS)
@pytest.mark.parametrize("layout", sorted(DC.SPECIAL_LAYOUTS))
def test_special_panel(n, layout):
    """The grids hold the stated numbers of specials; on every grid with specials the first one's emission exceeds every table
    row (after the reference's division by emission_max it is above 1) and, where there are two, the last one's is the grid's
    min_emission_prob, below every table row."""
    c = DC.special_case(n, layout)
    p = c.panel
    counts = tuple(DC.n_special(p, g) for g in range(G))
    assert counts == _resolved(n, layout) == c.claims["special_counts"] and p.nMaxDH == n
    for g in range(G):
        rows, sp, emin, emax = DC.table(p, c.gl, g)
        assert len(sp) == counts[g]
        if counts[g] >= 1:
            assert sp[0] > 10 * rows.max() and sp[0] > 1 and rows.max() >= 1 - 1e-15
            assert DC.n_words(p, g) == n + counts[g], "every special has a word of its own"
        if counts[g] >= 2:
            assert sp[-1] == emin and sp[-1] * 10 < min(rows.min(), np.delete(sp, -1).min())
    _finite(c)
    sym = DC.special_case(n, layout, True)
    assert sym.panel is p and sym.symbols
    _finite(sym)
    if 1 in counts:   # the reference's search gives the zero word for a grid's only special: the two forms differ there
        assert not np.array_equal(DC.oracle_ref(sym, "dosage")["dosage"], DC.oracle_ref(c, "dosage")["dosage"])


def test_special_layouts_cover_counts_and_places():
    for n in DC.SPECIAL_WIDTHS:
        seen = set()
        for layout in DC.SPECIAL_LAYOUTS:
            seen |= set(_resolved(n, layout))
        assert seen == set(DC.special_counts(n))
    only = {k: [g for g, x in enumerate(v) if x] for k, v in DC.SPECIAL_LAYOUTS.items()}
    assert only["g0_only"] == [0] and only["last_only"] == [G - 1] and only["mid_only"] == [3]
    assert only["every_a"] == only["every_b"] == list(range(G))


def test_chunk_panel():
    """Per grid and position (first chunk, first chunk of the fp32 family's second chunk row, the chunk with K - 1) the specials
    are a whole chunk, its low half or its high half -- every pattern at every position within grids 0 .. 2, and again in 3 .. 5."""
    from tests import k_cases as KC
    p = DC.chunk_panel()
    Kn = p.K
    pos = DC.chunk_positions(Kn)
    geo = KC.geometry(Kn, "f32")
    assert geo["NCH"] == 2 and pos == dict(first=0, second_row=geo["NT"], last=(Kn - 1) // 16) and Kn % 16
    assert KC.geometry(Kn - Kn % 16 - 16, "f32")["NCH"] == 1, "one chunk fewer and the family runs one chunk row"
    hm = np.asarray(p.hapMatcherR)
    seen = set()
    for g in range(G):
        sp = set(np.flatnonzero(hm[:, g] == 0).tolist())
        assert sp == set(DC.chunk_special_haps(Kn, g))
        for where, ch in pos.items():
            inside = sorted(k - 16 * ch for k in sp if k // 16 == ch)
            n_in = min(16, Kn - 16 * ch)
            pat = {tuple(range(n_in)): "all", tuple(range(min(8, n_in))): "low", tuple(range(8, n_in)): "high"}[tuple(inside)]
            seen.add((g // 3, where, pat))
        assert sp <= {k for ch in pos.values() for k in range(16 * ch, 16 * ch + 16)}
    assert seen == {(h, w, q) for h in (0, 1) for w in pos for q in DC.CHUNK_PATTERNS}
    for sym in (False, True):
        _finite(DC.chunk_case(sym))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. emissions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in DC.emission_cases()])
def test_emission_case(name):
    c = DC.case(name)
    cl, gl, p = c.claims, c.gl, c.panel
    Gn, Tn = p.nGrids, p.nSNPs
    assert not c.has_reads and gl.shape == (2, Tn)
    _finite(c)
    for norm in (True, False):
        for kind, always in (("thin", False), ("dosage", False), ("full", True)):
            r = DC.oracle_ref(c, kind, always_normalize=always, normalize_emissions=norm)
            assert np.isfinite(r["c"]).all() and (kind == "thin" or np.isfinite(r["dosage"]).all())
    if "only_variant" in cl:
        g, b = cl["only_variant"]
        n_local = min(32, Tn - 32 * g)
        block = gl[:, 32 * g:32 * g + n_local]
        assert b == n_local - 1 or b == 0
        assert (np.delete(block, b, axis=1) == 1).all() and tuple(block[:, b]) == (0.2, 1.0)
        assert cl.get("last_grid_snps", 32) == Tn - 32 * (Gn - 1)
        # the SNP tells words apart (or the grid's table would be all ones after normalisation, variant or not)
        rows = DC.table(p, gl, g)[0]
        assert len(set(np.round(rows, 12).tolist())) >= 2, name
    if "novar" in cl:
        assert tuple(GC.no_variant_grids(gl, Gn)) == tuple(cl["novar"])
    if "emax" in cl:
        for g in cl["emax_grids"]:
            assert DC.has_variant(gl, g)
            emax = DC.table(p, gl, g)[3]
            assert (emax == 1.0) if cl["emax"] == "emax_one" else (1 - 1e-15 < emax < 1.0), (name, g, emax)
    if "min_gl_grid" in cl:
        g = cl["min_gl_grid"]
        assert p.ref_error == cl["ref_error"] and set(gl[:, 32 * g:32 * g + 32].ravel().tolist()) == {DC.MIN_GL, 1.0}
        assert (gl[:, 32 * g:32 * g + 32].min(axis=0) == DC.MIN_GL).all(), "MIN_GL on all 32 SNPs"
        rows = DC.table(p, gl, g)[0]
        assert rows[0] == rows.max() >= 1 - 1e-15
        gone = np.flatnonzero(rows.astype(np.float32) == 0) + 1      # the table rows fp32 rounds to 0
        assert len(gone) >= 1 and len(gone) < p.nMaxDH
        mass = DC.masses(c, g)
        print(f"{name}: {len(gone)} rows round to 0 in fp32, e.g. {gone[:8].tolist()}; they hold {mass[gone].sum():.3g} of gamma")
        assert mass[gone].sum() < 1e-30, "... and carry no gamma to speak of"


def test_planted_threshold_moves_the_schedule():
    """The schedule cases under the planted threshold renormalise where the weak background alone takes the running product
    below it -- other grids than under the default 1e-100."""
    for c in DC.threshold_cases():
        planted = GC.renormalised(c, DC.oracle_ref(c, "thin")["c"])
        default = GC.renormalised(c, DC.oracle_ref(c, "thin", threshold=1e-100)["c"])
        print(f"{c.name}: 1e-100 renormalises at {default}, {c.threshold:g} at {planted}")
        assert default == c.claims["default_renorm"] and set(planted) - set(default) and c.threshold == DC.SCHEDULE_THRESHOLD
        assert DC.separation(c) > DC.SEP_RTOL


# ---------------------------------------------------------------------------------------------------------------------------
# 5. a free distinctHapsIE
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["other_error", "one_entry"])
def test_free_ie_panel(name):
    """The table is not the (eps, 1 - eps) expansion of the words; the oracle's dosage follows the table (the restated mat-vec
    with it gives the oracle's dosage, and the dosage differs from the derived panel's by far more than any bar) while c, alpha
    and the lists do not look at it."""
    free, derived = DC.ie_cases()[name]
    p, d = free.panel, derived.panel
    differs = np.asarray(p.distinctHapsIE) != np.asarray(d.distinctHapsIE)
    assert differs.any() and np.array_equal(p.distinctHapsB, d.distinctHapsB) and np.array_equal(p.hapMatcherR, d.hapMatcherR)
    if name == "one_entry":
        assert differs.sum() == 1 and differs[p.nMaxDH - 1, p.nSNPs - 1]
    a, b = DC.oracle_ref(free, "dosage"), DC.oracle_ref(derived, "dosage")
    assert np.abs(a["dosage"] - b["dosage"]).max() > 10 * DC.FP32_BAR, "every family's bar can tell the two tables apart"
    assert np.array_equal(a["c"], b["c"]) and np.array_equal(a["gamma_t"], b["gamma_t"])
    for (ia, va), (ib, vb) in zip(a["best_haps"], b["best_haps"]):
        assert np.array_equal(ia, ib) and np.array_equal(va, vb)
    for g in range(G):
        got = DC.dosage_from_masses(p, g, DC.masses(free, g), a["gamma_t"][:, g])
        assert np.abs(got - a["dosage"][32 * g:32 * g + 32]).max() < 1e-12
    _finite(free)


# ---------------------------------------------------------------------------------------------------------------------------
# groups and coverage
# ---------------------------------------------------------------------------------------------------------------------------
def test_groups():
    groups = DC.groups()
    assert {f"dh{n}" for n in WIDTHS if n > 1} | {"emit", "thr"} <= set(groups)
    for cs in groups.values():
        assert all(c.panel is cs[0].panel and np.array_equal(c.cols, cs[0].cols) and c.K_top == cs[0].K_top for c in cs)


def _edges():
    """{edge: [cases]} from the tables and the oracle."""
    table = {}

    def add(e, c):
        table.setdefault(e, []).append(c.name)
    for c in DC.all_cases():
        p = c.panel
        n = p.nMaxDH
        if "min_row" in c.claims:
            add(f"nMaxDH={n}", c)
            lo, hi = _row_of_min_max(c, DC.MINMAX_GRID)[:2]
            if n > 1:
                add(f"minimum on row {lo}", c)
                add(f"maximum on row {hi}", c)
            for g in range(G):
                w, s = DC.n_words(p, g), DC.n_special(p, g)
                add(f"nMaxDH={n}: " + ("exactly nMaxDH words" if w == n and not s else "one special" if s == 1 else "fewer words"), c)
                if w == 1:
                    add(f"nMaxDH={n}: one word", c)
        if c.claims.get("bins"):
            add(f"bins at nMaxDH={n}", c)
        if "special_counts" in c.claims:
            for g in range(G):
                add(f"nMaxDH={n}: {DC.n_special(p, g)} specials" + (" (symbols)" if c.symbols else ""), c)
        if c.claims.get("chunks"):
            add("chunks" + (" (symbols)" if c.symbols else ""), c)
    return table


REQUIRED = dict(
    WAVE={f"nMaxDH={w + d}" for w in (64, 128, 192) for d in (-1, 0, 1)} |
         {f"{m} on row {w + d}" for m in ("minimum", "maximum") for w in (64, 128, 192) for d in (-1, 0, 1)},
    DOSAGE_SUMS={f"nMaxDH={m + d}" for m in (8, 16) for d in (-1, 0, 1)} | {"bins at nMaxDH=8", "bins at nMaxDH=9"},
    KMAXROW={"nMaxDH=254", "nMaxDH=255", "nMaxDH=1", "nMaxDH=2", "minimum on row 255", "maximum on row 255", "minimum on row 1",
             "maximum on row 1", "bins at nMaxDH=255"} |
            {f"nMaxDH={n}: {k}" for n in WIDTHS for k in ("exactly nMaxDH words", "one special", "one word")} |
            {f"nMaxDH={n}: fewer words" for n in WIDTHS if n > 3},
    SPECIAL_STRIDE={f"nMaxDH={n}: {k} specials{s}" for n in (1, 8) for k in (255, 256, 257) for s in ("", " (symbols)")},
    SPECIAL_SUMS={f"nMaxDH={n}: {k} specials{s}" for n in (1, 8) for k in (0, 1, 7, 8, 9, K - n) for s in ("", " (symbols)")},
    CHUNK={"chunks", "chunks (symbols)"},
)


def test_coverage_table():
    """Every constant named at the top of tests/dict_cases.py is hit: each edge it stands for by at least one case."""
    table = _edges()
    assert set(REQUIRED) == set(DC.CONSTANTS)
    for constant in DC.CONSTANTS:
        missing = REQUIRED[constant] - set(table)
        assert not missing, (constant, sorted(missing))
    for e in sorted(table):
        print(f"{e}: {len(table[e])} cases, e.g. {table[e][0]}")
    names = [c.name for c in DC.all_cases()]
    assert len(names) == len(set(names))
