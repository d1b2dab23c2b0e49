"""Test infrastructure for output_read_label_prob and hla_run from BAM paths: the native loop and the range call with the new
options over the CPU oracle's entry points (the private test hook, csrc/impute_testhook.h: qa_impute_samples_backend_reads,
qa_impute_bam_range_backend_ex), and one small BAM file that exercises every clause of the loader's rule for a read's name
(include/quilt_amd_io.h).  Nothing in the product imports this."""
import ctypes as C

import numpy as np

from quilt_amd.impute import (STAT_NAMES, ImputeReadsOut, flatten_samples, make_hla, make_nipt, make_params, make_rare_common,
                              wrap_results)
from quilt_amd.native import ptr
from tests.testhooks import hook_lib


def impute_samples_reads_on_oracle(panel, samples, params, sample_offset=0, samples_per_launch_set=256, n_threads=1, rare_common=None,
                                   output_read_label_prob=True, hla_grid=None):
    """qa_impute_samples_backend_reads over the oracle table, flat reads: results (with read_label_prob when asked, with the gamma
    fields when ``hla_grid`` is given)."""
    from tests.hla_backend import OracleTableHLA
    P = params
    rcq = keep_rc = None
    if P.impute_rare_common:
        rcq, keep_rc = make_rare_common(rare_common, [C.c_void_p(100 + w) for w in range(n_threads)], samples)
    nq = fd = fg = keep_n = None
    if P.method == "nipt":
        nq, fd, fg, keep_n = make_nipt(panel, samples, P.shuffle_bin_radius, rare_common.nSNPs_all if P.impute_rare_common else None)
    q, keep = make_params(P, samples_per_launch_set, None, True, rcq, nq)
    tab = OracleTableHLA(panel, rare_common=rare_common)
    read_off, read_ptr, u, bq, wif = flatten_samples(samples)
    n, T, K = len(samples), (rare_common.nSNPs_all if P.impute_rare_common else panel.nSNPs), panel.K
    dosage, gp_t, haps = np.zeros((n, T)), np.zeros((n, 3, T)), np.zeros((n, 3 if P.method == "nipt" else 2, T))
    labels = np.zeros(int(read_off[-1]), dtype=np.int32)
    nDosage, stats = np.zeros(n, dtype=np.int32), np.zeros(11, dtype=np.int64)
    prob = np.full(int(read_off[-1]), -1.0) if output_read_label_prob else None
    ro = ImputeReadsOut(None if prob is None else prob.ctypes.data, None, None)
    hq = hla = None
    if hla_grid is not None:
        hq, hla = make_hla(hla_grid, n, P.nGibbsSamples, K)
    handles = (C.c_void_p * n_threads)(*[C.c_void_p(w + 1) for w in range(n_threads)])
    L = hook_lib()
    st = L.qa_impute_samples_backend_reads(C.byref(tab.table), tab.select_gamma_cb if hq is not None else None, handles, C.c_int32(n_threads),
                                           C.c_int32(K), C.c_int32(panel.nGrids), C.c_int32(panel.nSNPs), C.byref(q), C.c_int32(n),
                                           C.c_int64(sample_offset), ptr(read_off), ptr(read_ptr), ptr(u), ptr(bq), ptr(wif), ptr(dosage),
                                           ptr(gp_t), ptr(haps), ptr(labels), ptr(nDosage), ptr(stats),
                                           None if hq is None else C.byref(hq), None if prob is None else C.byref(ro))
    del keep, keep_rc, keep_n
    if tab.error is not None:
        raise tab.error
    if st != 0:
        raise RuntimeError(f"qa_impute_samples_backend_reads: status {st}: {L.qa_last_error().decode()}")
    return wrap_results(samples, dosage, gp_t, haps, labels, nDosage, read_off, fd, fg, hla, prob)


def impute_bam_range_ex_on_oracle(panel, bam_files, chr, ref, alt, params, n_threads=1, rare_common=None, **kw):
    """qa_impute_bam_range_backend_ex over the oracle table with the gamma-column entry (the loader then keeps the names)."""
    from quilt_amd.impute import BamRangeExtras
    from tests.hla_backend import OracleTableHLA
    from tests.native_driver_backend import bam_range_on_table

    def call(fn, tab, handles, n_threads, q, io, n, paths, sidx, ffv, h, ex=None, **bx):
        if ex is None:   # (a call without an option: the zeroed struct, which is qa_impute_bam_range)
            ex = BamRangeExtras(int(bx["use_bx_tag"].value) if bx else 0, int(bx["bxTagUpperLimit"].value) if bx else 0, 0, -1)
        return fn(C.byref(tab.table), tab.select_gamma_cb, handles, n_threads, panel.K, panel.nGrids, C.byref(q), C.byref(io), C.byref(ex), n,
                  paths, ptr(sidx), ptr(ffv), C.byref(h))
    return bam_range_on_table(OracleTableHLA(panel, rare_common=rare_common), "qa_impute_bam_range_backend_ex", call, bam_files, chr, ref,
                              alt, params, n_threads, rare_common, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# one file for the loader's names: forty sites a kilobase apart, four to a grid (the sites of tests/test_bx_loader_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------
NAMES_LIMIT = 1500      # bxTagUpperLimit the file is made for
NAMES_CAP = 3           # downsampleToCov the file is made for


def names_file_alignments():
    """Alignments in FILE order (the file is written unsorted, header SO:unsorted), holding
      * a mate pair that merges ("pair": sites 10 and 11),
      * alignments written against the order of their grids (later grids first), so the ordering by grid permutes the reads,
      * site 20 under six reads: above NAMES_CAP, reads are removed,
      * the barcode MOL on three fragments at sites 1, 2, 3, the LAST of them written first (its slot and name are the molecule's),
      * the barcode SPL at sites 5 and 30: further apart than NAMES_LIMIT, split."""
    from tests.test_bx_loader_cpu import L, aln
    at = lambda t: int(L[t]) - 7
    alns = [
        aln(at(36), {36: ("a", 30)}, "late_grid9"),
        aln(at(3), {3: ("r", 31)}, "mol_c", tag="MOL"),
        aln(at(30), {30: ("a", 33)}, "spl_far", tag="SPL"),
        aln(at(10), {10: ("a", 35)}, "pair", flag=0x1 | 0x40),
        aln(at(25), {25: ("r", 28)}, "grid6"),
        aln(at(1), {1: ("a", 30)}, "mol_a", tag="MOL"),
        aln(at(11), {11: ("r", 36)}, "pair", flag=0x1 | 0x80),
        aln(at(5), {5: ("a", 32)}, "spl_near", tag="SPL"),
        aln(at(2), {2: ("a", 29)}, "mol_b", tag="MOL"),
        aln(at(0), {0: ("r", 30)}, "first_site"),
    ]
    alns += [aln(at(20), {20: ("a" if i % 2 else "r", 20 + i)}, f"deep{i}") for i in range(6)]
    alns.append(aln(at(15), {15: ("a", 30)}, "grid3"))
    return alns
