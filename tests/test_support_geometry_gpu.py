"""Every geometry of the three integer kernel files around the hot path -- csrc/panel_build.hip, csrc/match.hip, csrc/select.hip --
on the constructed inputs of tests/support_cases.py (whose claims tests/test_support_cases_cpu.py proves), each against its host
restatement with np.array_equal: quilt_amd.panel.make_rhb_t_equality, tests.oracle_backend.find_good_matches_bruteforce, and
previously_selected + everything_select_good_haps_dense of quilt_amd.driver.  The selection kernel is reached through the private
entry qa_select_from_lists (csrc/fullpass_testhook.h): a real full-panel pass cannot be steered to the lists these cases need; one
test here ties that entry to the public call."""
import ctypes as C

import numpy as np
import pytest

from tests import support_cases as S
from tests.util import check_panel_tables

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------
# panel build
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def panel_cases():
    return {c.name: c for c in S.panel_cases()}


_PANEL_NAMES = ["many_grids", "many_grids_ragged", "table_full", "ties_by_sign", "zero_rank", "clustered"]
_PANEL_NAMES += [f"tiny_K{K}_G{G}" for K in S.TINY_K for G in (3, 1)]


@pytest.mark.parametrize("name", _PANEL_NAMES)
def test_device_built_tables(panel_cases, name):
    case = panel_cases[name]
    for nMaxDH in case.nMaxDHs:
        check_panel_tables(case.panel, nMaxDH)


def test_panel_names_cover_every_case(panel_cases):
    assert sorted(_PANEL_NAMES) == sorted(panel_cases)


@pytest.mark.parametrize("name", ["many_grids", "many_grids_ragged"])
@pytest.mark.parametrize("nMaxDH", [40, 1])
def test_many_grids_special_symbols_mode(panel_cases, name, nMaxDH):
    """use_eMatDH_special_symbols on more grids than workgroups: the tables built on the device against the panel created from the
    host's tables."""
    from quilt_amd.native import DevicePanel
    from tests.util import panel_from_rhb
    p = panel_cases[name].panel
    panel = panel_from_rhb(p.rhb_t, p.transMatRate_t, p.nSNPs, nMaxDH, p.ref_error)
    a = DevicePanel(panel, use_eMatDH_special_symbols=True)
    b = DevicePanel.from_rhb(panel, use_eMatDH_special_symbols=True)
    ta, tb = a.export_tables(), b.export_tables()
    a.close()
    b.close()
    assert ta[2][-1] > 0
    for x, y in zip(ta, tb):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("case", S.rhi_cases(), ids=lambda c: c.name)
def test_make_rhb_t_from_rhi_t(case):
    from quilt_amd.native import check, lib, ptr
    rhi = case.build()
    G = (case.nSNPs + 31) // 32
    out = np.full((case.K, G), -1, dtype=np.int32, order="F")
    check(lib().qa_make_rhb_t_from_rhi_t(ptr(rhi), C.c_int32(case.K), C.c_int32(case.nSNPs), ptr(out)))
    assert np.array_equal(out, case.expected(rhi))


# ---------------------------------------------------------------------------------------------------------------------------
# match
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def match_cases():
    return {c.name: c for c in S.match_cases()}


def _device_panel(case, device_built):
    from quilt_amd.native import DevicePanel
    return DevicePanel.from_rhb(case.panel) if device_built else DevicePanel(case.panel)


def _check_matches(case, dev):
    from quilt_amd.mspbwt import find_good_matches, match_tables_as_lists
    from tests.oracle_backend import find_good_matches_bruteforce
    for nind, min_len, n_max in case.params:
        match, n = find_good_matches(dev, case.Zs, nind, min_len, n_max)
        got = match_tables_as_lists(match, n)
        ref = find_good_matches_bruteforce(case.panel, case.Zs, nind, min_len, n_max)
        for q in range(len(case.Zs)):
            for i in range(nind):
                assert n[q, i] == len(ref[q][i]), (case.name, nind, min_len, n_max, q, i)
                assert np.array_equal(got[q][i], ref[q][i]), (case.name, nind, min_len, n_max, q, i)


_MATCH_NAMES = ["full_length_run_G4096", "tie_wall", "no_symbol_zero0_dh255", "no_symbol_zero1_dh255", "no_symbol_zero0_dh2",
                "no_symbol_zero1_dh2"] + [f"tiling_K{K}" for K in S.TILING_K]


@pytest.mark.parametrize("name", _MATCH_NAMES)
def test_device_search(match_cases, name):
    case = match_cases[name]
    device_built = case.claims.get("K") in S.TILING_DEVICE_BUILT or name.endswith("zero1_dh2")
    dev = _device_panel(case, device_built)
    try:
        _check_matches(case, dev)
    finally:
        dev.close()


def test_match_names_cover_every_case(match_cases):
    assert sorted(_MATCH_NAMES) == sorted(match_cases)


def test_more_positions_than_the_histogram_holds():
    """G = 4097: one index would have 4097 positions (kMaxRunLen = 4096) and is refused; two indices are served."""
    from quilt_amd.mspbwt import find_good_matches
    from quilt_amd.native import QA_ERR_INVALID, QuiltAmdError
    case = S.over_length_panel()
    dev = _device_panel(case, False)
    try:
        with pytest.raises(QuiltAmdError) as e:
            find_good_matches(dev, case.Zs, 1, 1, 2)
        assert e.value.status == QA_ERR_INVALID
        case.params = ((2, 1, 2),)
        _check_matches(case, dev)
    finally:
        dev.close()


# ---------------------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------------------
def select_from_lists(top, which, seeds, want, K, Ksubset, Knew, K_top_matches, top_width):
    """qa_select_from_lists (csrc/fullpass_testhook.h): which_next [chain][Ksubset], pre-filled with SENTINEL, and status."""
    from quilt_amd.native import check, ptr
    from tests.testhooks import hook_lib
    top = np.ascontiguousarray(top, dtype=np.int32)
    n_chain, n_label, n_thin, width = top.shape
    assert width == top_width
    which = np.ascontiguousarray(which, dtype=np.int32)
    seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    want = np.ascontiguousarray(want, dtype=np.int32)
    nxt = np.full((n_chain, Ksubset), S.SENTINEL, dtype=np.int32)
    status = np.full(n_chain, -99, dtype=np.int32)
    check(hook_lib().qa_select_from_lists(C.c_int32(n_chain), C.c_int32(n_label), C.c_int32(n_thin), C.c_int32(top_width),
                                     C.c_int32(K_top_matches), C.c_int32(K), C.c_int32(Ksubset), C.c_int32(Knew), ptr(top),
                                     ptr(which), ptr(seeds), ptr(want), ptr(nxt), ptr(status)))
    return nxt, status


@pytest.fixture(scope="module")
def select_cases():
    return {c.name: c for c in S.select_cases()}


_SELECT_NAMES = ["exact_fill_rank0", "exact_fill_rank2", "one_over", "one_under", "duplicates", "n_cand63", "n_cand64", "n_cand65",
                 "n_cand129", "bit_edges_K32", "bit_edges_K33", "bit_edges_K64", "bit_edges_K65", "Knew0_of50", "Knew50_of50",
                 "Knew0_of1", "Knew1_of1", "width64_Knew127", "width64_Knew129", "width8_top3", "exhausted", "too_large", "shared"]


@pytest.mark.parametrize("name", _SELECT_NAMES)
def test_device_selection(select_cases, name):
    from quilt_amd.driver import ListsTruncated, everything_select_good_haps_dense, previously_selected
    case = select_cases[name]
    nxt, status = select_from_lists(case.top, case.which, case.seeds, case.want, case.K, case.Ksubset, case.Knew,
                                    case.K_top_matches, case.top_width)
    for c in range(case.n_chain):
        if not case.want[c]:
            assert status[c] == -1 and (nxt[c] == S.SENTINEL).all(), "a chain without a selection: its row is untouched"
            continue
        prev = previously_selected(case.which[c], case.Ksubset - case.Knew, int(case.seeds[c]))
        try:
            sel = everything_select_good_haps_dense(case.Knew, case.K_top_matches, case.top[c].astype(np.int64) + 1, prev, case.K,
                                                    int(case.seeds[c]), truncated=True)
        except ListsTruncated:
            assert status[c] == 1, "ranks exhausted on the host: the device must hand the chain back"
            continue
        assert status[c] == 0
        assert np.array_equal(nxt[c], np.concatenate([prev, sel])), (name, c)
        assert len(set(nxt[c].tolist())) == case.Ksubset and nxt[c].min() >= 1 and nxt[c].max() <= case.K
    if name == "too_large":      # nothing was launched
        assert status.tolist() == [1, -1, 1] and (nxt == S.SENTINEL).all()
    if name == "shared":
        a, b = case.claims["twins"]
        assert np.array_equal(nxt[a], nxt[b]) and not np.array_equal(nxt[a], nxt[1])


def test_select_names_cover_every_case(select_cases):
    assert sorted(_SELECT_NAMES) == sorted(select_cases)


def test_selection_entry_checks_its_arguments(select_cases):
    """The checks of qa_fullpass_reads_select_batch: top_width in K_top_matches .. 64, K_top_matches >= 1, Ksubset in 1 .. K, Knew in
    0 .. Ksubset."""
    from quilt_amd.native import QA_ERR_INVALID, QuiltAmdError
    case = select_cases["one_over"]
    ok = dict(K=case.K, Ksubset=case.Ksubset, Knew=case.Knew, K_top_matches=2, top_width=case.top_width)
    wide = np.full(case.top.shape[:3] + (65,), -1, dtype=np.int32)
    bad = [dict(ok, top_width=65, top=wide), dict(ok, K_top_matches=0), dict(ok, K_top_matches=case.top_width + 1),
           dict(ok, Knew=case.Ksubset + 1), dict(ok, Knew=-1), dict(ok, K=case.Ksubset - 1)]
    for kw in bad:
        with pytest.raises(QuiltAmdError) as e:
            select_from_lists(kw.pop("top", case.top), case.which, case.seeds, case.want, **kw)
        assert e.value.status == QA_ERR_INVALID, kw
    with pytest.raises(QuiltAmdError):
        select_from_lists(case.top, case.which[:, :-1], case.seeds, case.want, **dict(ok, Ksubset=0))
    select_from_lists(case.top, case.which, case.seeds, case.want, **ok)


def test_entry_and_public_call_select_alike(small_panel):
    """What keeps the private entry honest: a real qa_fullpass_reads_select_batch (top_width = 64, K_top_matches = 5) against
    qa_select_from_lists on the lists the same passes return without the selection -- the same which_next and status."""
    from tests.test_select_gpu import _both
    Ksubset, K_top = 100, 5
    for Knew, filled in ((12, True), (40, False)):   # 2 labels x 8 thinned grids x 5 ranks: 12 are found, 40 distinct ones are not
        top, cnt, which, seeds, nxt, status, want_top = _both(small_panel, 3, 7, Ksubset, Knew, K_top, thin=0.5, top_width=64)
        got, st = select_from_lists(top, np.stack(which), seeds, want_top, small_panel.K, Ksubset, Knew, K_top, 64)
        assert np.array_equal(st, status) and status[1] == -1
        assert (status[np.array(want_top) == 1] == (0 if filled else 1)).all()
        for c in np.flatnonzero(status == 0):
            assert np.array_equal(got[c], nxt[c])
