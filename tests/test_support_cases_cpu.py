"""The claims of tests/support_cases.py, checked without a device: every constructed input must hit the edge its builder names, by
the host restatements alone (quilt_amd.panel.make_rhb_t_equality, tests.oracle_backend.find_good_matches_bruteforce,
quilt_amd.driver.everything_select_good_haps_dense) -- a case whose claim fails here is a broken builder, and
tests/test_support_geometry_gpu.py would pin nothing with it.  No case is skipped or filtered."""
import numpy as np
import pytest

from tests import support_cases as S


# ---------------------------------------------------------------------------------------------------------------------------
# panel build
# ---------------------------------------------------------------------------------------------------------------------------
def _tables(panel, nMaxDH):
    from quilt_amd.panel import make_rhb_t_equality
    return make_rhb_t_equality(panel.rhb_t, nMaxDH, panel.nSNPs, panel.ref_error)


def _second_ranking(col, nMaxDH):
    """make_rhb_t_equality's codes of one grid, stated a second time: np.unique + lexsort (count descending, signed value
    ascending), the first nMaxDH ranks are the codes."""
    vals, inv, cnt = np.unique(col, return_inverse=True, return_counts=True)
    order = np.lexsort((vals, -cnt))
    rank = np.empty(len(vals), dtype=np.int64)
    rank[order] = np.arange(1, len(vals) + 1)
    B = np.zeros(nMaxDH, dtype=np.int32)
    B[:min(nMaxDH, len(vals))] = vals[order][:nMaxDH]
    return np.where(rank[inv] <= nMaxDH, rank[inv], 0), B


@pytest.mark.parametrize("ragged", [False, True])
def test_many_grids(ragged):
    case = S.many_grids(ragged)
    p, c = case.panel, case.claims
    assert p.nGrids == c["G"] == 520 > S.RANK_BLOCKS and p.K == 70
    assert p.nSNPs == 32 * 520 - (13 if ragged else 0)
    nd = np.array([len(np.unique(p.rhb_t[:, g])) for g in range(p.nGrids)])
    hz = (p.rhb_t == 0).any(axis=0)
    assert np.array_equal(nd, c["n_distinct"]) and np.array_equal(hz, c["has_zero"])
    for g in range(p.nGrids - S.RANK_BLOCKS):   # a workgroup's first and second grid differ in kind
        assert nd[g] != nd[g + S.RANK_BLOCKS] and hz[g] != hz[g + S.RANK_BLOCKS]
    for nMaxDH in (40, 1):
        hm = _tables(p, nMaxDH)["hapMatcherR"]
        has_sp = (hm == 0).any(axis=0)
        assert not has_sp[list(c["one_word"])].any(), "the one-word grids: the `continue` of k_list_specials"
        assert has_sp.sum() > 100 and (~has_sp).sum() >= 3
        assert np.array_equal(has_sp, nd > nMaxDH)
    assert not (_tables(p, 255)["hapMatcherR"] == 0).any()   # K = 70: nothing is special at 255, k_list_specials is not launched


def test_table_full():
    case = S.table_full()
    p, c = case.panel, case.claims
    assert p.K == 4300
    nz = [S.n_distinct_nonzero(p.rhb_t[:, g]) for g in range(p.nGrids)]
    assert nz == c["n_nonzero"] == [4095, 4096, 4097, 1, 4095, 4096]
    assert [bool((p.rhb_t[:, g] == 0).any()) for g in range(p.nGrids)] == c["has_zero"]
    assert [n <= S.KMAXDISTINCT for n in nz] == c["device_ranked"]
    # grid 1: 4096 words in the table + the zero word = 4097 sort entries, padded to the whole scratch slice
    n = nz[1] + 1
    assert n == S.KMAXDISTINCT + 1 and 1 << (n - 1).bit_length() == 2 * S.KMAXDISTINCT
    assert nz[5] == 1 << (nz[5] - 1).bit_length() == S.KMAXDISTINCT   # grid 5: no padding entry at all
    for g in (0, 1, 2):   # unequal counts, and the zero word tied with a negative and a positive word
        vals, cnt = np.unique(p.rhb_t[:, g], return_counts=True)
        assert len(np.unique(cnt)) >= 5
        tied = vals[cnt == cnt[vals == 0][0]]
        assert (tied < 0).any() and (tied > 0).any()
    for nMaxDH in case.nMaxDHs:
        t = _tables(p, nMaxDH)
        for g in range(p.nGrids):
            codes, B = _second_ranking(p.rhb_t[:, g], nMaxDH)
            assert np.array_equal(t["hapMatcherR"][:, g], codes) and np.array_equal(t["distinctHapsB"][:, g], B)


def test_ties_by_sign():
    case = S.ties_by_sign()
    p = case.panel
    assert case.nMaxDHs == (255,) and p.K == 3000 <= S.KMAXDISTINCT
    t = _tables(p, 255)
    for g in range(p.nGrids):
        col = p.rhb_t[:, g]
        assert len(np.unique(col)) == p.K and (col < 0).sum() == case.claims["n_negative"] == 1500
        coded = col[t["hapMatcherR"][:, g] != 0]
        assert len(coded) == 255 and np.array_equal(np.sort(coded), np.sort(col)[:255]) and (coded < 0).all()
        assert np.array_equal(t["distinctHapsB"][:, g], np.sort(col)[:255])
        # an unsigned tie order would code the 255 lowest NON-NEGATIVE words instead: a disjoint set
        assert not np.isin(np.sort(col.view(np.uint32))[:255].view(np.int32), coded).any()


def test_zero_rank():
    case = S.zero_rank()
    p = case.panel
    assert case.claims["zero_rank"] == (1, 40, 41, 2, 40, 0)
    for g, want in enumerate(case.claims["zero_rank"]):
        assert S.rank_of_zero(p.rhb_t[:, g]) == want
    g = case.claims["tie_grid"]   # the zero word between a negative and a positive word of the same count
    vals, cnt = np.unique(p.rhb_t[:, g], return_counts=True)
    tied = np.sort(vals[cnt == cnt[vals == 0][0]])
    assert len(tied) == 3 and tied[0] < 0 == tied[1] < tied[2]
    for nMaxDH in case.nMaxDHs:
        t = _tables(p, nMaxDH)
        for g, r in enumerate(case.claims["zero_rank"]):
            codes, B = _second_ranking(p.rhb_t[:, g], nMaxDH)
            assert np.array_equal(t["hapMatcherR"][:, g], codes) and np.array_equal(t["distinctHapsB"][:, g], B)
            zero = p.rhb_t[:, g] == 0
            if r:   # the zero haplotypes carry the code `r` up to nMaxDH and are special from nMaxDH + 1 on
                assert (t["hapMatcherR"][zero, g] == (r if r <= nMaxDH else 0)).all()
        if nMaxDH == 40:
            hm = t["hapMatcherR"]
            assert (hm[p.rhb_t[:, 1] == 0, 1] == 40).all() and (hm[p.rhb_t[:, 2] == 0, 2] == 0).all()
            pos = np.sort(np.unique(p.rhb_t[:, 4])[np.unique(p.rhb_t[:, 4], return_counts=True)[1] == (p.rhb_t[:, 4] == 0).sum()])[2]
            assert (hm[p.rhb_t[:, 4] == pos, 4] == 0).all()   # the tie's positive word falls behind the cut


@pytest.mark.parametrize("G", [3, 1])
@pytest.mark.parametrize("K", S.TINY_K)
def test_tiny_K(K, G):
    case = S.tiny_K(K, G)
    p = case.panel
    assert (p.K, p.nGrids) == (K, G) and case.nMaxDHs == (1, 2)
    assert p.transMatRate_t.shape == (2, max(G - 1, 1)) and p.transMatRate_t.ctypes.data != 0
    per = (K + S.KBT - 1) // S.KBT
    if K <= S.KBT:   # trailing threads of k_list_specials: k0 = t * per at or beyond K
        assert (S.KBT - 1) * per >= K or K == S.KBT
    if K == S.KBT + 1:
        assert per == 2 and 129 * per > K   # thread 129: k0 = 258 > k1 = 257
    for nMaxDH in case.nMaxDHs:
        hm = _tables(p, nMaxDH)["hapMatcherR"]
        assert bool((hm == 0).any(axis=0).all()) == case.claims["specials_everywhere"][nMaxDH]
        if case.claims["last_special"]:
            assert (hm[K - 1] == 0).all()
    if K == 1:
        assert not (_tables(p, 1)["hapMatcherR"] == 0).any()
    if K == 2:   # two words, one haplotype each: the lower signed value takes the code
        hm = _tables(p, 1)["hapMatcherR"]
        for g in range(G):
            assert hm[np.argmin(p.rhb_t[:, g]), g] == 1 and hm[np.argmax(p.rhb_t[:, g]), g] == 0


def test_clustered():
    case = S.clustered()
    p = case.panel
    for g in range(p.nGrids):
        w = np.unique(p.rhb_t[:, g])
        w = w[w != 0]
        slots = S.hash_word(w.view(np.uint32))
        assert len(w) == 600 <= S.KMAXDISTINCT
        assert (slots == case.claims["slot"]).sum() == 300 and (slots == case.claims["slot"] - 1).sum() == 300
        assert case.claims["slot"] - 1 + 600 > S.KHT   # the occupied run wraps round the table's end
    assert (p.rhb_t[:, 1] == 0).any() and not (p.rhb_t[:, 0] == 0).any()
    for nMaxDH in case.nMaxDHs:
        assert ((_tables(p, nMaxDH)["hapMatcherR"] == 0).any(axis=0)).all()


def test_panel_case_list_is_complete():
    names = [c.name for c in S.panel_cases()]
    assert len(set(names)) == len(names) == 6 + 2 * len(S.TINY_K)


def test_rhi_cases():
    cases = S.rhi_cases()
    for c in cases:
        assert S.slab_plan(c.K, c.nSNPs) == c.claims["slabs"]
    big = cases[0]
    assert big.name == "rhi_two_slabs" and (big.K, big.nSNPs) == (2 ** 20 + 3, 33)
    assert S.slab_plan(big.K, 33) == [(0, 1, 32), (1, 1, 1)]
    assert len(S.slab_plan(2 ** 20, 33)) == 1 and len(S.slab_plan(2 ** 20 + 1, 33)) == 2   # where the second slab begins
    assert [c.K for c in cases[1:]] == [255, 256, 257]
    # the expectation (packbits per grid) against the bit definition, on a small shape
    c = cases[3]
    rhi = c.build()
    exp = c.expected(rhi)
    for k in (0, 100, c.K - 1):
        for g in range(exp.shape[1]):
            bits = (rhi[k, 32 * g:32 * g + 32] != 0).astype(np.int64)
            assert int(exp[k, g]) & 0xffffffff == int((bits << np.arange(len(bits))).sum())
    assert rhi.max() == 7


# ---------------------------------------------------------------------------------------------------------------------------
# match
# ---------------------------------------------------------------------------------------------------------------------------
def _ref(case, prm):
    from tests.oracle_backend import find_good_matches_bruteforce
    return find_good_matches_bruteforce(case.panel, case.Zs, *prm)


def test_full_length_run():
    case = S.full_length_run()
    assert case.rhb_t.shape == (5, S.KMAXRUNLEN)
    ref = _ref(case, (1, 1, 5))
    assert ref[0][0].tolist() == [[0, 0, S.KMAXRUNLEN]]
    ref = _ref(case, (3, 1, 5))
    assert [r.tolist() for r in ref[0]] == [[[0, 0, 1366]], [[0, 0, 1365]], [[0, 0, 1365]]]
    assert case.claims["longest"] == {1: [4096], 3: [1366, 1365, 1365]}
    over = S.over_length_panel()
    G = over.rhb_t.shape[1]
    assert G == S.KMAXRUNLEN + 1 and -(-G // 1) > S.KMAXRUNLEN and -(-G // 2) <= S.KMAXRUNLEN


def test_tiling():
    assert S.TILING_K == (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 8192, 8193)
    for edge in (4, S.PICK_CHUNK, S.HAPS_PER_BLOCK):   # below, at and above every tile
        assert {edge - 1, edge, edge + 1} <= set(S.TILING_K)
    assert {8192, 8193} <= set(S.TILING_K)                # Kp: one padded row of 8192, and the first K with two
    assert set(S.TILING_DEVICE_BUILT) < set(S.TILING_K)
    for K in S.TILING_K:
        case = S.tiling(K)
        assert case.rhb_t.shape == (K, 12) and np.array_equal(case.rhb_t, S.tiling(max(S.TILING_K)).rhb_t[:K])
        assert {p[0] for p in case.params} == {1, 5, 12} and 12 % 5 and any(p[2] >= K for p in case.params)
    case = S.tiling(8193)   # runs are plentiful: ties at the cut, and the cut is a real one
    for prm in case.params[:3]:
        for per_index in _ref(case, prm):
            lens = np.concatenate([m[:, 2] for m in per_index])
            assert len(lens) and lens.max() >= 2 if prm[0] == 1 else len(lens)
    ref = _ref(case, (1, 2, 40))
    assert all(len(r[0]) == 40 for r in ref[:2])
    assert (case.panel.hapMatcherR == 0).sum() == 0
    q3 = _ref(S.tiling(1025), (1, 1, 1025))[2][0]   # the query with two words of no dictionary: no run crosses grids 4 and 5
    assert len(q3) and ((q3[:, 1] + q3[:, 2] <= 4) | (q3[:, 1] >= 6)).all()


def test_tie_wall():
    case = S.tie_wall()
    c = case.claims
    isA, isB, nA = c["isA"], c["isB"], c["nA"]
    assert case.rhb_t.shape == (700, 10) and len(np.unique(case.rhb_t, axis=0)) == 3 and nA > 150 and c["nB"] > 150
    full = _ref(case, (1, 1, 2000))[0][0]
    assert np.array_equal(full[:, 0], np.flatnonzero(isA | isB))
    assert (full[isA[full[:, 0]], 2] == 10).all() and (full[isB[full[:, 0]], 2] == 5).all()
    for name, group in (("A", isA), ("B", isB)):
        above = 0 if name == "A" else nA
        ks = np.flatnonzero(group)
        cuts = c["cuts"][name]
        for where, m in cuts.items():
            assert m in [p[2] for p in case.params]
            n_tie = m - above                       # ties accepted: the cut falls INSIDE the group
            assert 0 < n_tie < len(ks)
            last_in, first_out = ks[n_tie - 1], ks[n_tie]
            if where == "first_chunk":
                assert last_in < S.PICK_CHUNK and first_out < S.PICK_CHUNK
            elif where == "chunk_boundary":         # the quota is used up by the last tie of chunk 0
                assert last_in < S.PICK_CHUNK <= first_out
            else:
                assert 2 * S.PICK_CHUNK <= last_in and 2 * S.PICK_CHUNK <= first_out
            got = _ref(case, (1, 1, m))[0][0]
            want = np.sort(np.r_[np.flatnonzero(isA) if above else [], ks[:n_tie]]).astype(np.int64)
            assert np.array_equal(got[:, 0], want)
        if name == "B":                             # rows above the threshold come after ties that were cut off
            assert (np.flatnonzero(isA) > ks[cuts["first_chunk"] - above]).sum() > 100
    assert len(_ref(case, (1, 11, 50))[0][0]) == 0 and len(_ref(case, (1, 10, 2000))[0][0]) == nA
    assert {1, 699, 700, 2000} <= {p[2] for p in case.params}


def test_no_symbol():
    for dh in (255, 2):
        a, b = S.no_symbol(False, dh), S.no_symbol(True, dh)
        assert not (a.rhb_t == 0).any() and (b.rhb_t == 0).any(axis=0).all()
        Ba = a.panel.distinctHapsB
        if dh == 255:   # fewer words than rows: zero padding that an all-zero query "finds"
            assert (Ba[5:] == 0).all() and (Ba[:5] != 0).all()
            assert (a.panel.hapMatcherR != 0).all()
        else:
            assert (a.panel.hapMatcherR == 0).any(axis=0).all()
        for prm in a.params:
            ra, rb = _ref(a, prm), _ref(b, prm)
            assert all(len(m) == 0 for m in ra[0]), "the all-zero query on a panel without the zero word"
            if prm[0] == 1:   # words of no dictionary at grids 1 and 4: no run covers them
                s, e = ra[1][0][:, 1], ra[1][0][:, 1] + ra[1][0][:, 2]
                assert len(s) and ((e <= 1) | ((s >= 2) & (e <= 4)) | (s >= 5)).all()
        zero_coded = (b.panel.hapMatcherR != 0) & (b.rhb_t == 0)
        assert sum(len(m) for m in _ref(b, (1, 1, 50))[0]) == min(50, int(zero_coded.any(axis=1).sum()))
        assert any(len(m) for m in _ref(a, (1, 1, 50))[2])
    assert len(S.match_cases()) == 6 + len(S.TILING_K)


# ---------------------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------------------
def _host_selection(case, c):
    """previously_selected + everything_select_good_haps_dense(truncated=True): the row, or None where the host raises."""
    from quilt_amd.driver import ListsTruncated, everything_select_good_haps_dense, previously_selected
    prev = previously_selected(case.which[c], case.Ksubset - case.Knew, int(case.seeds[c]))
    try:
        sel = everything_select_good_haps_dense(case.Knew, case.K_top_matches, case.top[c].astype(np.int64) + 1, prev, case.K,
                                                int(case.seeds[c]), truncated=True)
    except ListsTruncated:
        return prev, None
    return prev, sel


_select = {c.name: c for c in S.select_cases()}


@pytest.mark.parametrize("name", list(_select))
def test_select_case(name):
    from quilt_amd.rng import SELECT_OFFSET_RANK, keyed_subset
    case = _select[name]
    assert case.top.shape[0] == case.n_chain == len(case.which) == len(case.seeds) == len(case.want)
    assert case.top.shape[3] == case.top_width <= 64 and 1 <= case.K_top_matches <= case.top_width
    assert case.top.min() >= -1 and case.top.max() < case.K and case.which.min() >= 1 and case.which.max() <= case.K
    assert all(len(set(w.tolist())) == case.Ksubset for w in case.which)
    ends = case.claims.get("ends")
    for c in range(case.n_chain):
        steps, end = S.trace_selection(case, c)
        if ends is not None:
            assert end == ends[c], (c, steps)
        if end == ("unwanted",):
            continue
        prev, sel = _host_selection(case, c)
        assert (sel is None) == (end == ("exhausted",)), "the host takes the branch the trace names"
        if sel is None:
            assert sum(n for n, _ in steps) < case.Knew
            continue
        _, rank, over = end
        n_new, room = steps[rank]
        assert n_new - room == over >= 0 and all(n < r for n, r in steps[:rank])
        row = np.concatenate([prev, sel])
        assert len(set(row.tolist())) == case.Ksubset and row.min() >= 1 and row.max() <= case.K
        # the ranks before the last are appended in list order, the last one by key
        cols = case.top[c].reshape(case.n_cand, case.top_width)
        seen, at = set((prev - 1).tolist()), 0
        for i in range(rank + 1):
            new = []
            for v in cols[:, i].tolist():
                if v >= 0 and v not in seen:
                    seen.add(v)
                    new.append(v)
            if i < rank:
                assert sel[at:at + len(new)].tolist() == [v + 1 for v in new]
                at += len(new)
            else:
                pick = keyed_subset(int(case.seeds[c]), len(new), room, SELECT_OFFSET_RANK)
                assert sel[at:].tolist() == [new[j] + 1 for j in pick]


def test_select_edges():
    c = _select
    for name in ("exact_fill_rank0", "exact_fill_rank2"):   # len(new) == Knew - len(to_keep): the subsample branch, reordered by key
        case = c[name]
        for ch in range(case.n_chain):
            steps, end = S.trace_selection(case, ch)
            n_new, room = steps[end[1]]
            assert n_new == room and end[2] == 0
            prev, sel = _host_selection(case, ch)
            assert sel[-room:].tolist() != sorted(sel[-room:].tolist())
    assert [S.trace_selection(c["one_over"], 0)[0][1], S.trace_selection(c["one_under"], 0)[0][0]] == [(23, 22), (29, 30)]
    # duplicates: X at lanes 0, 62, 63, in the second and the third chunk, a kept haplotype, and repeats at the next rank
    case = c["duplicates"]
    assert case.n_cand == 130 > 2 * S.WAVE
    for ch in range(case.n_chain):
        col0, col1 = case.top[ch].reshape(130, -1)[:, 0], case.top[ch].reshape(130, -1)[:, 1]
        X = col0[0]
        assert X >= 0 and (col0[[62, 63, 67, 128]] == X).all() and (col1[[0, 64]] == X).all()
        assert col0[74] == col0[127] >= 0 and col1[63] == col0[74]
        prev, _ = _host_selection(case, ch)
        assert col0[1] + 1 in prev and col0[64] == col0[1]
        assert S.trace_selection(case, ch)[0][0] == (case.claims["n_rank0"], case.Knew)
    assert sorted(c[f"n_cand{n}"].n_cand for n in (63, 64, 65, 129)) == [63, 64, 65, 129] and c["n_cand129"].top.shape[1] == 3
    for n in (63, 64, 65, 129):
        case = c[f"n_cand{n}"]
        last = case.claims["last_lanes"]
        assert n - 1 in last and (63 in last) == (n > 63) and (127 in last) == (n > 127)
        cols = case.top[0].reshape(n, -1)
        assert (cols[last, 0] == -1).all() and (cols[last, 1] >= 0).all()
        assert S.trace_selection(case, 0)[1][:2] == ("subsample", 1)
    for K in S.BIT_K:
        case = c[f"bit_edges_K{K}"]
        assert case.K == K and case.claims["edge"] == sorted({0, 31, min(32, K - 1), K - 1})
        for ch in range(case.n_chain):
            assert set(case.claims["edge"]) <= set((case.which[ch] - 1).tolist())
            assert set(case.claims["edge"]) <= set(case.top[ch][..., 0].ravel().tolist())
    for name, Ksubset, Knew in (("Knew0_of50", 50, 0), ("Knew50_of50", 50, 50), ("Knew0_of1", 1, 0), ("Knew1_of1", 1, 1)):
        case = c[name]
        assert (case.Ksubset, case.Knew) == (Ksubset, Knew)
        prev, sel = _host_selection(case, 0)
        assert len(prev) == Ksubset - Knew and len(sel) == Knew
        if Knew == 0:
            assert sorted(prev.tolist()) == sorted(case.which[0].tolist())
    assert (c["width64_Knew127"].top_width, c["width64_Knew127"].K_top_matches) == (64, 64)
    assert S.trace_selection(c["width64_Knew127"], 0)[1] == ("subsample", 63, 1)
    case = c["width8_top3"]
    assert (case.top_width, case.K_top_matches) == (8, 3)
    wide = S.SelectCase(**{**case.__dict__, "K_top_matches": 8})       # the candidates at ranks 3 .. 7 WOULD fill chain 0
    assert S.trace_selection(case, 0)[1] == ("exhausted",) and S.trace_selection(wide, 0)[1][0] == "subsample"
    case = c["exhausted"]
    assert case.want.tolist() == [1, 0, 1, 1]
    case = c["too_large"]
    lds = S.select_lds_bytes(case.K, case.n_cand, case.Ksubset)
    assert lds == case.claims["lds"] == 4 * ((657 + 6 + 1) & ~1) + 8 * 20600 > S.LDS_BYTES
    assert all(S.select_lds_bytes(x.K, x.n_cand, x.Ksubset) <= S.LDS_BYTES for x in c.values() if x.name != "too_large")
    case = c["shared"]
    a, b = case.claims["twins"]
    assert np.array_equal(case.top[a], case.top[b]) and case.seeds[a] == case.seeds[b] and case.seeds[1] != case.seeds[a]
    assert np.array_equal(_host_selection(case, a)[1], _host_selection(case, b)[1])
    assert not np.array_equal(_host_selection(case, a)[1], _host_selection(case, 1)[1])
    assert sum(len(set(x.seeds.tolist())) > 1 for x in c.values()) >= 10   # several chains per call, different seeds
