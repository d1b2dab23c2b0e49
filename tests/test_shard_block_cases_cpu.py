"""The block-wise shard pass on the CPU: the reference of tests/shard_block_cases.py alone -- every case shows the table features
it was built for -- and the conditions under which the device can be compared with it without a tolerance on a decision: no
uniform within 1e-6 of the probability it is compared with, and no cut that a relative change of 1e-9 in the switch rate (far
more than the device's rounding of a Ks-wide sum) can move.  Also: the library's host-side block table on each case's rate, and
the new ABI member in the header and in its ctypes mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import rtwin
from tests import shard_block_cases as SB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["g40_readless", "g130_ks600_end63", "g130_ks40_end64", "g40_ks600_one_block"]


@pytest.mark.parametrize("name", NAMES)
def test_every_pass_has_a_consistent_table(name):
    case = SB.cases()[name]
    ref = case.reference()
    assert len(ref["trace"]) == len(SB.BLOCK_ITS)
    assert 120 <= case.sample.nReads <= 250
    for t in ref["trace"]:
        n = t["n_blocks"]
        # (a read-less run at the right end leaves the last block ending at G - 2: gibbs-nipt-block.cpp:1432-1490, kept as it is)
        assert t["grid_start"][0] == 0 and t["grid_end"][-1] in (case.G - 1, case.G - 2)
        assert all(t["grid_start"][b + 1] == t["grid_end"][b] + 1 for b in range(n - 1))
        assert [g for g in range(case.G) if t["grid_where"][g] >= 0] == t["grid_end"]
        assert len(t["p_stay"]) == n - 1 and list(t["block"]) == list(range(n - 1))


def test_readless_runs_are_merged_at_the_left_in_the_middle_and_at_the_right():
    case = SB.cases()["g40_readless"]
    wif = case.sample.wif
    for t in case.reference()["trace"]:
        bg = t["blocked_grid"]
        has = sorted(set(int(bg[g]) for g in wif))
        nb = int(bg.max()) + 1
        gone = [b for b in range(nb) if b not in has]
        assert 0 in gone and nb - 1 in gone, "read-less blocks at both ends"
        runs = np.split(np.array(gone), np.where(np.diff(gone) != 1)[0] + 1)
        assert any(len(r) >= 2 and r[0] > 0 and r[-1] < nb - 1 for r in runs), "a run of two read-less blocks in the middle"
        assert t["n_blocks"] == nb - len(gone)
        for b in range(t["n_blocks"]):   # every block that is left holds a read
            assert ((wif >= t["grid_start"][b]) & (wif <= t["grid_end"][b])).any()


def test_blocks_end_at_the_staging_edges():
    assert all(63 in t["grid_end"] for t in SB.cases()["g130_ks600_end63"].reference()["trace"])
    assert all(64 in t["grid_end"] for t in SB.cases()["g130_ks40_end64"].reference()["trace"])


def test_no_available_boundary_means_one_block_and_no_decision():
    for t in SB.cases()["g40_ks600_one_block"].reference()["trace"]:
        assert t["n_blocks"] == 1 and len(t["p_stay"]) == 0 and len(t["u"]) == 0


@pytest.mark.parametrize("name", NAMES[:3])
def test_planted_decisions(name):
    case = SB.cases()[name]
    tr = case.reference()["trace"]
    t0 = tr[0]
    assert t0["u"][0] == 1 - 3 * 2.0 ** -53 and t0["u"][1] == 0.0 and t0["flip_mode"][0] == 1 and t0["flip_mode"][1] == 0
    assert t0["u"][-1] == 1 - 2.0 ** -53 and t0["flip_mode"][-1] == 1, "a flip decided at the last considered block"
    flips = np.concatenate([t["flip_mode"] for t in tr])
    assert flips.sum() >= 1 and (flips == 0).sum() >= 1


@pytest.mark.parametrize("name", NAMES)
def test_no_decision_is_close(name):
    for t in SB.cases()[name].reference()["trace"]:
        assert np.all(np.abs(t["u"] - t["p_stay"]) >= 1e-6)


def _table_from_rate(case, rate2):
    grid = np.arange(case.panel.nSNPs) // 32
    G = case.G
    sm = rtwin.make_smoothed_rate(rate2, case.L_grid, case.radius)
    # the rest of the block definition takes the state only through rate2: drive rtwin's own function with a state whose rate2
    # is the given one -- K = 1, sigma = 1, alpha = beta = 1, e(g + 1) = 1 - rate2(g) / 2 for both labels
    al = [np.ones((1, G)) for _ in range(3)]
    be = [np.ones((1, G)) for _ in range(3)]
    eg = [np.ones((1, G)) for _ in range(3)]
    for h in range(2):
        eg[h][0, 1:G - 1] = 1 - rate2[:G - 2] / 2
    tm = np.ones((2, G - 1))
    cc = [np.ones(G) for _ in range(3)]
    b = rtwin.R_define_blocked_snps_using_gamma_on_the_fly(al, be, cc, eg, tm, case.radius, case.L_grid, grid, case.q, 0.0)
    np.testing.assert_allclose(b["smoothed_rate"], sm, rtol=1e-12, atol=1e-15)
    return b["blocked_grid"], rtwin.R_make_gibbs_considers(b["blocked_snps"], grid, case.sample.wif, G)


@pytest.mark.parametrize("name", NAMES)
def test_rounding_of_the_rate_cannot_move_a_cut(name):
    case = SB.cases()[name]
    ref = case.reference()
    rng = np.random.default_rng(5)
    for rate2, t in zip(ref["rate2"], ref["trace"]):
        for _ in range(20):
            eps = rng.uniform(-1, 1, size=len(rate2))
            bg, cons = _table_from_rate(case, rate2 * (1 + 1e-9 * eps))
            assert np.array_equal(bg, t["blocked_grid"])
            assert cons["n_blocks"] == t["n_blocks"] and list(cons["grid_where"]) == list(t["grid_where"])


@pytest.mark.parametrize("name", NAMES)
def test_host_block_table_matches_the_reference(name):
    """qa_nipt_block_table (host code, no device) on each pass's rate2."""
    from quilt_amd import native
    lib = native.lib()
    case = SB.cases()[name]
    ref = case.reference()
    G, wif = case.G, np.ascontiguousarray(case.sample.wif, dtype=np.int32)
    Lg = np.ascontiguousarray(case.L_grid, dtype=np.int32)
    for rate2, t in zip(ref["rate2"], ref["trace"]):
        arrs = [np.zeros(G, dtype=np.int32) for _ in range(6)]
        n = C.c_int32()
        r2 = np.ascontiguousarray(rate2, dtype=np.float64)
        native.check(lib.qa_nipt_block_table(native.ptr(r2), native.ptr(Lg), C.c_int32(G), C.c_int32(case.radius), C.c_double(case.q),
                                             native.ptr(wif), C.c_int32(len(wif)), *[native.ptr(a) for a in arrs], C.byref(n)))
        assert np.array_equal(arrs[0], t["blocked_grid"])
        assert n.value == t["n_blocks"]
        assert list(arrs[1][:n.value]) == t["grid_start"] and list(arrs[2][:n.value]) == t["grid_end"]
        assert list(arrs[5]) == t["grid_where"]


def test_header_and_mirror_carry_shard_by_blocks(tmp_path):
    """qa_gibbs_opts_t.shard_by_blocks follows draw_uniforms_ctx in the header and in the ctypes mirror, at the same offset."""
    from quilt_amd.gibbs_nipt import GibbsOpts
    names = [f[0] for f in GibbsOpts._fields_]
    assert names[-2:] == ["draw_uniforms_ctx", "shard_by_blocks"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quilt_amd.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu\\n", offsetof(qa_gibbs_opts_t, draw_uniforms_ctx), offsetof(qa_gibbs_opts_t, shard_by_blocks),\n'
                   '           sizeof(qa_gibbs_opts_t));\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    ctx, flag, size = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert GibbsOpts.draw_uniforms_ctx.offset == ctx and GibbsOpts.shard_by_blocks.offset == flag and C.sizeof(GibbsOpts) == size
    from quilt_amd import native
    assert native.lib().qa_abi_version() == 5


def test_header_and_mirror_carry_the_loops_shard_blocks(tmp_path):
    """qa_impute_params_t.shard_blocks (last member) and qa_impute_shard_blocks_t against their ctypes mirrors."""
    from quilt_amd.impute import ImputeParams, ImputeShardBlocks
    assert [f[0] for f in ImputeParams._fields_][-2:] == ["sample_source", "shard_blocks"]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quilt_amd.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(qa_impute_params_t, shard_blocks), sizeof(qa_impute_params_t),\n'
                   '           offsetof(qa_impute_shard_blocks_t, L_grid), offsetof(qa_impute_shard_blocks_t, shuffle_bin_radius),\n'
                   '           offsetof(qa_impute_shard_blocks_t, block_gibbs_quantile_prob), sizeof(qa_impute_shard_blocks_t));\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert [ImputeParams.shard_blocks.offset, C.sizeof(ImputeParams), ImputeShardBlocks.L_grid.offset,
            ImputeShardBlocks.shuffle_bin_radius.offset, ImputeShardBlocks.block_gibbs_quantile_prob.offset,
            C.sizeof(ImputeShardBlocks)] == v
