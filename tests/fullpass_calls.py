"""The calls the geometry suites of the full-panel passes make on the device (helper, no test): the single-pass entry with lists at
a case's thinned grids, qa_fullpass_batch on label 1 of several cases, and the comparison of two sets of lists.  A case is a
tests.grid_cases.GridCase (or a subclass): panel, gl, cols, K_top."""
import ctypes as C

import numpy as np


def single(dev, c, *, dosage, alpha=False, gamma=False, beta=False, always_normalize=False, normalize_emissions=True,
           threshold=1e-100):
    """One call of the single-pass entry with lists at the thinned grids."""
    from quilt_amd.reference_single import Rcpp_haploid_dosage_versus_refs
    K, G, T = c.panel.K, c.panel.nGrids, c.panel.nSNPs
    out = dict(c=np.ones(G), best_haps_stuff_list=[None] * len(c.thin_grids))
    if dosage:
        out["dosage"] = np.zeros(T)
    for want, name in ((alpha, "alphaHat_t"), (gamma, "gamma_t"), (beta, "betaHat_t")):
        if want:
            out[name] = np.zeros((K, G), order="F")
    Rcpp_haploid_dosage_versus_refs(dev, c.gl, gammaSmall_cols_to_get=c.cols, K_top_matches=c.K_top, return_dosage=dosage,
                                    return_gamma_t=gamma, return_betaHat_t=beta, get_best_haps_from_thinned_sites=True,
                                    always_normalize=always_normalize, normalize_emissions=normalize_emissions,
                                    min_emission_prob_normalization_threshold=threshold, **out)
    return out


def batch(dev, cases, want):
    """qa_fullpass_batch on label 1 of ``cases`` (one panel, one set of columns): dosage [P][T] and per pass the lists."""
    from quilt_amd.native import check, lib, ptr
    c0 = cases[0]
    P, T, n_thin = len(cases), c0.panel.nSNPs, len(c0.thin_grids)
    gl = np.ascontiguousarray(np.stack([np.ascontiguousarray(c.gl.T) for c in cases]))   # [P][T][2]
    wd = np.array(want, dtype=np.int32)
    dosage = np.zeros((P, T))
    bptr = np.zeros(P * n_thin + 1, dtype=np.int32)
    cap = max(P * n_thin * c0.panel.K, 1)
    bidx, bval = np.zeros(cap, dtype=np.int32), np.zeros(cap)
    check(lib().qa_fullpass_batch(dev.handle, C.c_int32(P), ptr(gl), ptr(wd), ptr(c0.cols), C.c_int32(c0.K_top), ptr(dosage),
                                  ptr(bptr), ptr(bidx), ptr(bval), C.c_int64(cap)))
    lists = [[dict(top_matches=bidx[bptr[p * n_thin + j]:bptr[p * n_thin + j + 1]].copy(),
                   top_matches_values=bval[bptr[p * n_thin + j]:bptr[p * n_thin + j + 1]].copy()) for j in range(n_thin)]
             for p in range(P)]
    return dosage, lists


def lists_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x["top_matches"], y["top_matches"]) and
                                    np.array_equal(x["top_matches_values"], y["top_matches_values"]) for x, y in zip(a, b))


def lists_equal_oracle(got, best_haps):
    """The device's lists against the oracle's (index array, value array) pairs, bit for bit."""
    return len(got) == len(best_haps) and all(np.array_equal(e["top_matches"], oi) and np.array_equal(e["top_matches_values"], ov)
                                              for e, (oi, ov) in zip(got, best_haps))
