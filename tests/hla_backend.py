"""Test infrastructure for hla_run (qa_impute_samples_hla, include/quilt_amd.h): the CPU oracle's passes with the reference's
gamma_t kept at one grid, for quilt_amd/driver.py (OracleBackendHLA) and for the native loop through the private test hook
qa_impute_samples_backend_hla (OracleTableHLA + impute_samples_hla_on_oracle).  The gamma column is
oracle.haploid_dosage_versus_refs(..., return_gamma_t=True)["gamma_t"][:, grid]: reference-single.cpp's gamma_t_col."""
import ctypes as C
import threading

import numpy as np

from oracle import oracle as O
from quilt_amd.impute import STAT_NAMES, flatten_samples, make_hla, make_params, wrap_results
from quilt_amd.native import ptr
from tests.native_driver_backend import F32P, F64P, I32P, U64P, OracleTable
from tests.oracle_backend import OracleBackend
from tests.testhooks import hook_lib

SELECT_GAMMA_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, I32P, I32P, I32P, I32P, I32P, I32P, I32P, I32P,
                              I32P, C.c_int32, C.c_double, F64P, C.c_int32, I32P, F32P, I32P, C.c_int32, C.c_int32, I32P, U64P, I32P,
                              I32P, C.c_int32, F64P)


class OracleBackendHLA(OracleBackend):
    """OracleBackend whose full-panel passes also return the gamma column of ``gamma_grid`` (the driver's hla_run rounds).
    ``pending_grid`` set: the same for a caller that cannot pass the argument (OracleTableHLA); the columns go to
    ``last_gamma``.  Both per calling thread: the native loop's host threads call in concurrently."""
    _tls = threading.local()

    @property
    def pending_grid(self):
        return getattr(self._tls, "pending_grid", None)

    @pending_grid.setter
    def pending_grid(self, g):
        self._tls.pending_grid = g

    @property
    def last_gamma(self):
        return getattr(self._tls, "last_gamma", None)

    @last_gamma.setter
    def last_gamma(self, g):
        self._tls.last_gamma = g

    def fullpass_reads_batch(self, samples, chain_sample, labels, want_dosage, want_top, cols, K_top_matches, minGLValue,
                             top_width, n_label=2, gamma_grid=None):
        grid = gamma_grid if gamma_grid is not None else self.pending_grid
        if grid is None:
            return super().fullpass_reads_batch(samples, chain_sample, labels, want_dosage, want_top, cols, K_top_matches,
                                                minGLValue, top_width, n_label=n_label)
        from quilt_amd.driver import make_gl_from_u_bq
        T, K = self.panel.nSNPs, self.panel.K
        n_chain = len(chain_sample)
        n_thin = int((np.asarray(cols) >= 0).sum())
        dosage = np.zeros((n_chain, n_label, T))
        gamma = np.zeros((n_chain, n_label, K))
        top = np.full((n_chain, n_label, n_thin, top_width), -1, dtype=np.int32)
        cnt = np.zeros((n_chain, n_label, n_thin), dtype=np.int32)

        def one(c):
            s = samples[chain_sample[c]]
            per_base = np.repeat(labels[c], np.diff(s.read_ptr))
            for l in range(1, n_label + 1):
                sel = (per_base == l) & (s.bq != 0)
                gl = make_gl_from_u_bq(s.u[sel], s.bq[sel], T, minGLValue, self.make_gl_bound)
                r = O.haploid_dosage_versus_refs(self.panel, gl, cols, K_top_matches=K_top_matches,
                                                 return_dosage=bool(want_dosage[c]), return_gamma_t=bool(want_dosage[c]),
                                                 get_best_haps_from_thinned_sites=bool(want_top[c]))
                dosage[c, l - 1] = r["dosage"]
                if want_dosage[c]:
                    gamma[c, l - 1] = r["gamma_t"][:, grid]
                for j, (idx, v) in enumerate(r["best_haps"] if want_top[c] else []):
                    order = np.argsort(-v, kind="stable")      # everything_per_hap_rejig_haps (functions.R:2161-2170)
                    k = idx[order][:top_width]
                    top[c, l - 1, j, : len(k)] = k
                    cnt[c, l - 1, j] = len(idx)
        self._map(one, list(range(n_chain)))
        if gamma_grid is not None:
            return dosage, top, cnt, gamma
        self.last_gamma = gamma
        return dosage, top, cnt


class OracleTableHLA(OracleTable):
    """OracleTable plus the select_gamma entry of qa_impute_samples_backend_hla: the oracle's passes with the gamma column,
    then the same host selection as OracleTable.select."""

    def __init__(self, panel, **kw):
        super().__init__(panel, **kw)
        self.ob = OracleBackendHLA(panel, kw.get("rare_common"))
        self.calls["select_gamma"] = 0
        self.select_gamma_cb = SELECT_GAMMA_FN(self._guard(self.select_gamma, "select_gamma"))

    def select_gamma(self, handle, n_chain, n_label, n_sample, cs, read_off, read_ptr, u, bq, H, wd, wt, cols, Ktop, minGL, dosage,
                     top_width, top_idx, top_val, top_cnt, Ksubset, Knew, which, seed, which_next, status, grid, gamma_col):
        self.ob.pending_grid = int(grid)
        try:
            st = self.select(handle, n_chain, n_label, n_sample, cs, read_off, read_ptr, u, bq, H, wd, wt, cols, Ktop, minGL, dosage,
                             top_width, top_idx, top_val, top_cnt, Ksubset, Knew, which, seed, which_next, status)
        finally:
            self.ob.pending_grid = None
        g = np.ctypeslib.as_array(gamma_col, shape=(n_chain, n_label, self.panel.K))
        wda = np.ctypeslib.as_array(wd, shape=(n_chain,))
        for c in range(n_chain):
            if wda[c]:
                g[c] = self.ob.last_gamma[c]
        return st


def impute_samples_hla_on_oracle(panel, samples, params, grid, sample_offset=0, samples_per_launch_set=256, n_threads=1,
                                 fuse_tails=True, source=None, q_edit=None):
    """qa_impute_samples_backend_hla over the oracle table: (results with the four gamma fields, native counters, table).
    ``source``: the samples handed over one by one (qa_sample_source_t).  ``q_edit(q)``: changes the parameter struct before
    the call (refusal tests).  Raises RuntimeError with qa_last_error's text on a non-zero status."""
    q, keep = make_params(params, samples_per_launch_set, None, fuse_tails)
    if q_edit is not None:
        keep = (keep, q_edit(q))
    tab = OracleTableHLA(panel)
    read_off, read_ptr, u, bq, wif = flatten_samples(samples)
    n, T, K = len(samples), panel.nSNPs, panel.K
    keep_s = None
    labels = np.zeros(int(read_off[-1]), dtype=np.int32)
    per_sample_labels = None
    if source:
        from quilt_amd.impute import sample_source_over
        per_sample_labels = [np.zeros(s.nReads, dtype=np.int32) for s in samples]
        src, keep_s = sample_source_over(samples, per_sample_labels)
        q.sample_source = C.cast(C.pointer(src), C.c_void_p)
    hq, hla = make_hla(grid, n, params.nGibbsSamples, K)
    dosage, gp_t, haps = np.zeros((n, T)), np.zeros((n, 3, T)), np.zeros((n, 2, T))
    nDosage = np.zeros(n, dtype=np.int32)
    stats = np.zeros(11, dtype=np.int64)
    handles = (C.c_void_p * n_threads)(*[C.c_void_p(w + 1) for w in range(n_threads)])
    L = hook_lib()
    st = L.qa_impute_samples_backend_hla(C.byref(tab.table), tab.select_gamma_cb, handles, C.c_int32(n_threads), C.c_int32(K),
                                         C.c_int32(panel.nGrids), C.c_int32(T), C.byref(q), C.c_int32(n), C.c_int64(sample_offset),
                                         *((None,) * 5 if source else (ptr(read_off), ptr(read_ptr), ptr(u), ptr(bq), ptr(wif))),
                                         ptr(dosage), ptr(gp_t), ptr(haps), None if source else ptr(labels), ptr(nDosage), ptr(stats),
                                         C.byref(hq))
    if source:
        labels = np.concatenate(per_sample_labels)
    del keep, keep_s
    if tab.error is not None:
        raise tab.error
    if st != 0:
        raise RuntimeError(f"qa_impute_samples_backend_hla: status {st}: {L.qa_last_error().decode()}")
    return wrap_results(samples, dosage, gp_t, haps, labels, nDosage, read_off, hla=hla), dict(zip(STAT_NAMES, stats.tolist())), tab


def oracle_gamma_t(panel, samples, chain_sample, labels, minGLValue=1e-10):
    """The oracle's whole gamma_t (K x nGrids) of every (chain, label) pass, from the genotype likelihoods the driver's passes
    build from the chain's reads and labels: [n_chain][2] arrays."""
    from quilt_amd.driver import make_gl_from_u_bq
    out = []
    for c, si in enumerate(chain_sample):
        s = samples[si]
        per_base = np.repeat(labels[c], np.diff(s.read_ptr))
        row = []
        for l in (1, 2):
            sel = (per_base == l) & (s.bq != 0)
            gl = make_gl_from_u_bq(s.u[sel], s.bq[sel], panel.nSNPs, minGLValue, O.make_gl_bound)
            row.append(O.haploid_dosage_versus_refs(panel, gl, return_gamma_t=True)["gamma_t"])
        out.append(row)
    return out
