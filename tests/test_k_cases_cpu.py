"""What tests/k_cases.py says about its table of K values and its planted panels, proved on the host tables
(qa_fullpass_geometry, no device) and on the fp64 oracle alone: tests/test_k_geometry_gpu.py compares the device with the oracle
on these cases without a branch on the device's result, and that is sound only if the claims here hold."""
import numpy as np
import pytest

from tests import k_cases as KC

KS = KC.k_table()
ROWS = (64, 128, 192, 256, 320, 384, 448, 512)


# ---------------------------------------------------------------------------------------------------------------------------
# the table against the launchers' built lists
# ---------------------------------------------------------------------------------------------------------------------------
def test_hook_needs_no_device_and_checks_its_arguments():
    from tests.testhooks import hook_lib
    import ctypes as C
    f = hook_lib().qa_fullpass_geometry
    out = (C.c_int32 * 8)()
    assert f(C.c_int32(0), C.c_int32(0), out) != 0 and f(C.c_int32(5), C.c_int32(9), out) != 0 and f(C.c_int32(5), C.c_int32(0), None) != 0
    # (3 125 chunks of 16 over 7 per lane: 447 lanes, rounded up to whole waves)
    assert KC.geometry(50000, "f32") == dict(NT=448, NCH=7, NR=0, NL=0, n_last=0, NS=0, Kq=50176, built=1)
    assert KC.geometry(50000, "rank") == dict(NT=512, NCH=7, NR=5, NL=2, n_last=64, NS=0, Kq=57344, built=1)
    assert KC.geometry(65537, "dos") == dict(NT=512, NCH=9, NR=5, NL=2, n_last=512, NS=2, Kq=9 * 8192, built=1)
    assert KC.geometry(5000, "full") == dict(NT=256, NCH=2, NR=0, NL=0, n_last=0, NS=0, Kq=8192, built=1)
    assert KC.geometry(57345, "full")["NT"] == 0 and KC.geometry(98305, "f32")["NT"] == 0


def test_every_launcher_case_is_reached():
    """Every entry of the launchers' built lists (csrc/fullpass.hip: Nch32Built, Nch64Built; csrc/fullpass64.hip: Rows64Built and
    the streamed build) is run by some K of the table.  The ranking pair's <4, 3> build is the one exception K cannot reach: launch_fb64 sends every
    seven-row panel to <5, 2> unless QA_FB64_FOUR_ROWS=1 is in the environment when the library loads."""
    assert set(KC.reached("f32")) == {(n,) for n in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12)}
    assert set(KC.reached("full")) == {(n,) for n in (1, 2, 4, 6, 8, 10, 12, 13, 14)}
    on_chip = {(1, 0), (2, 0), (3, 0), (4, 0), (4, 1), (4, 2), (5, 2), ("SP",)}
    assert set(KC.reached("rank")) == on_chip
    assert set(KC.reached("dos")) == on_chip | {(4, 3)}


def test_both_forms_of_the_dosage_seven_row_choice():
    """launch_fb64_dosage keeps <4, 3> while three LDS rows fit beside k_bwd64d's histogram and takes <5, 2> beyond: the last K
    of the first and the first K of the second are in the table, and the ranking pair runs <5, 2> on both."""
    sw = [k for k in KC.switches()["dos"] if KC.variant(k, "dos") == (4, 3)]
    assert len(sw) == 1 and {sw[0], sw[0] + 1} <= set(KS)
    assert KC.variant(sw[0] + 1, "dos") == (5, 2) and KC.variant(sw[0], "rank") == KC.variant(sw[0] + 1, "rank") == (5, 2)
    assert KC.geometry(sw[0], "dos")["n_last"] == 64 and KC.geometry(sw[0] + 1, "dos")["n_last"] == 128


def test_every_switch_has_its_last_K_and_the_next():
    for kind, ks in KC.switches().items():
        assert ks, kind
        for k in ks:
            assert {k, k + 1} <= set(KS), (kind, k)
    assert set(KC.TINY) | {57345, 65537} <= set(KS)
    assert {m + d for m in [2048, *range(4096, 57345, 4096), 65536, 81920, 98304] for d in (0, 1)} <= set(KS)
    assert 55 <= len(KS) <= 70


@pytest.mark.parametrize("rows,variant", [(2, (2, 0)), (6, (4, 2))])
def test_every_width_of_the_last_row(rows, variant):
    """All eight n_last at a geometry whose last row is in registers and at one whose last row is in LDS, K no multiple of 16."""
    ks = KC.n_last_sweep(rows)
    assert set(ks) <= set(KS) and all(k % 16 for k in ks)
    for kind in ("rank", "dos"):
        assert [KC.variant(k, kind) for k in ks] == [variant] * 8
        assert tuple(KC.geometry(k, kind)["n_last"] for k in ks) == ROWS
    # and the streamed build runs whole rows
    assert KC.geometry(57345, "rank")["n_last"] == 512 and KC.geometry(57345, "rank")["NS"] == 1


def test_no_K_reaches_a_geometry_that_is_not_built():
    """Whatever pick_geometry / geo64 choose, the launcher's built list holds: `geometry not built` cannot be reached by K
    (run_passes refuses a build without that entry with QA_ERR_UNSUPPORTED before any device work)."""
    for kind in KC.KINDS:
        for k in [*range(1, 40), *range(16, KC.K_SCAN + 1, 16), *range(17, KC.K_SCAN + 2, 16), 131072, 1 << 20]:
            g = KC.geometry(k, kind)
            assert g["built"] == (1 if g["NT"] else 0), (kind, k, g)
            assert g["Kq"] == g["NT"] * g["NCH"] * 16 and (g["NT"] == 0 or g["Kq"] >= k)


# ---------------------------------------------------------------------------------------------------------------------------
# the planted panels, K by K
# ---------------------------------------------------------------------------------------------------------------------------
def _ranked(ref, j):
    idx, v = ref["best_haps"][j]
    return idx[np.argsort(-v, kind="stable")]


@pytest.mark.parametrize("K", KS)
def test_planted_rows_head_every_list(K):
    """Per case and label: the oracle's lists have the stated length; where a label has K_top planted rows or more, every list is
    its promoted rows in the promoted order; the K_top + 1 first gammas of every thinned grid are exact copies or SEP_RTOL apart;
    and over the cases of the K every edge haplotype is within the first K_top ranks of some list."""
    cases = KC.cases_of(K)
    r1, r2 = KC.planted_rows(K)
    assert set(KC.edge_rows(K)) <= set(r1) | set(r2) and not set(r1) & set(r2)
    seen = set()
    for c in cases:
        assert c.panel.K == K and c.panel.nGrids == KC.G and c.K_top == KC.K_TOP
        for label in (1, 2):
            ref = KC.oracle_ref(c, "dosage", label)
            thin = KC.oracle_ref(c, "thin", label)
            assert len(ref["best_haps"]) == len(KC.THIN)
            promoted = c.claims["promoted"][label]
            for j, g in enumerate(KC.THIN):
                idx, v = ref["best_haps"][j]
                assert len(idx) == c.claims["list_len"][label], (c.name, label, g)
                assert np.array_equal(idx, thin["best_haps"][j][0])
                order = _ranked(ref, j)
                if len(promoted) >= KC.K_TOP:
                    assert order.tolist() == promoted, (c.name, label, g)
                elif promoted:      # fewer planted rows than K_top: they head the list, the tie of all others follows
                    assert order[:len(promoted)].tolist() == promoted
                seen |= set(order[:KC.K_TOP].tolist())
                top = np.sort(ref["gamma_t"][:, g])[::-1][:KC.K_TOP + 1]
                hi, lo = top[:-1], top[1:]
                assert ((hi == lo) | (hi - lo >= KC.SEP_RTOL * hi)).all(), (c.name, label, g, top)
        # the oracle's own K-wide sums: what c_without_summation_error takes out of c is within the bound of adding K positive
        # numbers one after the other, (K - 1) x 2^-53 relative, for the two sums in it (and the roundings of the correction)
        ref = KC.oracle_ref(c, "dosage", 1)
        assert np.abs(KC.c_without_summation_error(c, ref) / ref["c"] - 1).max() <= (2 * K + 2) * 2.0 ** -53
        if c.claims["no_reads"]:
            assert (c.gl == 1).all() and c.claims["list_len"][1] == K
            assert np.abs(KC.oracle_ref(c, "full", 1, True)["c"] - 1).max() <= K * 2.0 ** -53
            for j in range(len(KC.THIN)):
                assert np.array_equal(KC.oracle_ref(c, "thin", 1)["best_haps"][j][0], np.arange(K))
    assert set(KC.edge_rows(K)) <= seen


@pytest.mark.parametrize("K", KS)
def test_small_nMaxDH_makes_the_planted_rows_special(K):
    """nMaxDH = 8: from K = 1 024 on every planted row has code 0 at every grid (its words are rarer than the eight commonest of
    the background); the nMaxDH = 255 panel of the same K holds no special at all.  Below that the few rows of the panel all
    have codes, and the case says so."""
    p255, p8, _, rows = KC.panels(K)
    planted = np.array(rows[0] + rows[1])
    assert p8.nMaxDH <= 8 and not (np.asarray(p255.hapMatcherR) == 0).any()
    assert np.array_equal(p8.rhb_t, p255.rhb_t)
    if K >= KC.MIN_SPECIAL_K:
        assert (np.asarray(p8.hapMatcherR)[planted, :] == 0).all()
    else:
        assert K <= 17
