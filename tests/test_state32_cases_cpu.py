"""What tests/state32_cases.py says about its cases, proven on the CPU with the reference alone: the storage error E, the margin
DELTA = max(1e-5, 20 E), the admission of every case at its fixed seed, the argument rules that need no device, and the ABI:
the mode is a setting of the panel handle and the two option structs keep their layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import state32_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = {"g1": (1, 40, 3), "g2_ks1": (2, 1, 4), "g65_ks63": (65, 63, 40), "g65_ks65": (65, 65, 40), "g129_ks600": (129, 600, 60),
         "g129_ks640": (129, 640, 60), "g40_ks1024": (40, 1024, 30), "g130_ks600_blocks": (130, 600, 60), "rc_small": (None, 64, None),
         "readless_run": (70, 600, None)}


def test_every_case_of_the_table_exists():
    assert set(S.NAMES) == set(TABLE) and set(S.SEEDS) == set(TABLE)
    for name, (G, Ks, R) in TABLE.items():
        c = S.case(name)
        assert c.Ks == Ks and (G is None or c.G == G) and (R is None or c.sample.nReads == R), name
        assert len(c.runif_reads) == c.sample.nReads * 21 and len(c.runif_shard) == 3 * (c.G - 1)
        assert 0 <= S.SEEDS[name] < S.MAX_SEEDS
    assert (S.N_BURN + S.N_SAMPLE, S.BLOCK_ITS) == (21, (3, 6, 9))
    wif = S.case("readless_run").sample.wif
    assert set(np.unique(wif)) == set(range(4)) | set(range(66, 70))
    rc = S.case("rc_small")
    assert rc.rc is not None and rc.G == rc.rc.nGrids_all and rc.G > rc.panel.nGrids
    b = S.case("g130_ks600_blocks")
    assert b.blocks is not None and b.blocks.planted == (20, 63, 100) and b.device_kwargs()["shard_check_every_pair"] is False


def test_storage_error_and_margin():
    """E is a rounding to nearest of a 24-bit mantissa -- at most 2^-24 -- and comes out there; DELTA is then the 1e-5 floor."""
    E, delta = S.E(), S.DELTA()
    print(f"E = {E:.6e}  (2^-24 = {2.0 ** -24:.6e})   DELTA = {delta:.3e}   4 E = {4 * E:.6e}")
    assert 0.5 * 2.0 ** -24 < E <= 2.0 ** -24
    assert delta == max(1e-5, 20 * E) == 1e-5


@pytest.mark.parametrize("name", S.NAMES)
def test_case_is_admitted(name):
    c = S.case(name)
    why = S.admission(c, S.DELTA())
    print(name, "seed", c.seed, "admitted" if why is None else f"NOT admitted: {why}")
    assert why is None, why


def test_the_cases_show_something():
    """labels move, both shard decisions occur over the cases, and the block case has blocks to decide on"""
    moved = {n: int((S.reference(S.case(n))["H"] != S.case(n).H0).sum()) for n in S.NAMES}
    print(moved)
    assert all(moved[n] > 0 for n in ("g65_ks63", "g65_ks65", "g129_ks600", "g129_ks640", "g40_ks1024", "g130_ks600_blocks"))
    c = S.case("g130_ks600_blocks")
    trace = []
    from tests import shard_block_cases as SB
    from oracle import rtwin
    saved = rtwin.R_shard_block_gibbs_resampler
    rtwin.R_shard_block_gibbs_resampler = SB.blockwise_resampler(c.blocks.L_grid, c.blocks.radius, c.blocks.q, c.panel.nSNPs)
    try:
        rtwin.forwardBackwardGibbsNIPT(c.panel, c.sample, c.which, c.H0, c.runif_reads, c.first_read, n_gibbs_burn_in_its=S.N_BURN,
                                       n_gibbs_sample_its=S.N_SAMPLE, block_gibbs_iterations=S.BLOCK_ITS, runif_shard=c.runif_shard,
                                       trace=trace)
    finally:
        rtwin.R_shard_block_gibbs_resampler = saved
    assert len(trace) == 3 and all(t["n_blocks"] >= 2 for t in trace), [t["n_blocks"] for t in trace]


def _probe(tmp_path, body):
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quilt_amd.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()


def test_the_mode_is_a_setting_of_the_handle_and_the_option_structs_keep_their_layout(tmp_path):
    """The width is set on the panel handle (qa_panel_set_gibbs_state_bits, beside the two precision setters), so that
    qa_gibbs_opts_t and qa_impute_params_t end where ABI 5 has them end: shard_by_blocks and shard_blocks stay the last members
    of the headers' structs and of their ctypes mirrors, and the compiler sees the setter's prototype."""
    from quilt_amd import native
    from quilt_amd.gibbs_nipt import GibbsOpts
    from quilt_amd.impute import ImputeParams
    assert [f[0] for f in GibbsOpts._fields_][-1] == "shard_by_blocks" and [f[0] for f in ImputeParams._fields_][-1] == "shard_blocks"
    # (unevaluated calls: the compiler checks them against the prototypes, the probe links nothing)
    out = _probe(tmp_path, '    qa_panel_t *h = NULL;\n'
                           '    size_t set = sizeof(qa_panel_set_gibbs_state_bits(h, (int32_t)32)), get = sizeof(qa_panel_get_gibbs_state_bits(h));\n'
                           '    printf("%zu %zu %zu %zu %d\\n", offsetof(qa_gibbs_opts_t, shard_by_blocks), sizeof(qa_gibbs_opts_t),\n'
                           '           offsetof(qa_impute_params_t, shard_blocks), sizeof(qa_impute_params_t), set == sizeof(int) && get == sizeof(int));\n')
    flag, gsize, blocks, isize, ok = map(int, out)
    assert (GibbsOpts.shard_by_blocks.offset, C.sizeof(GibbsOpts), ImputeParams.shard_blocks.offset, C.sizeof(ImputeParams)) == (flag, gsize, blocks, isize)
    assert gsize - flag <= 8 and isize - blocks == 8 and ok == 1, "nothing but padding follows the last members"
    L = native.lib()
    assert L.qa_abi_version() == 5
    assert L.qa_panel_set_gibbs_state_bits.argtypes == [C.c_void_p, C.c_int32] and L.qa_panel_get_gibbs_state_bits.argtypes == [C.c_void_p]


def test_argument_rules_without_a_device():
    """a NULL handle is refused by both entries, whatever the width (no device is touched)"""
    from quilt_amd import native
    L = native.lib()
    for bits in (0, 32, 64, 16):
        assert L.qa_panel_set_gibbs_state_bits(None, C.c_int32(bits)) == native.QA_ERR_INVALID
    assert b"qa_panel_set_gibbs_state_bits" in L.qa_last_error()
    assert L.qa_panel_get_gibbs_state_bits(None) == native.QA_ERR_INVALID
