/*
 * quilt_amd_shim.c -- the R side of the drop-in boundary: a shared object whose registered `.Call` routines have the
 * reference's own names and arities and forward to libquilt_amd.so (include/quilt_amd.h).
 *
 * What it replaces.  QUILT's R code reaches its native hot path through `.Call('_QUILT_<fn>', PACKAGE = 'QUILT', ...)`
 * (QUILT/R/RcppExports.R); the routines are registered in QUILT/src/RcppExports.cpp:1703-1782 (`CallEntries[]`,
 * `R_init_QUILT`).  This file registers, under the same symbol names and with the same number of arguments:
 *
 *   _QUILT_Rcpp_haploid_dosage_versus_refs   38 arguments   RcppExports.cpp:1580-1625   -> qa_Rcpp_haploid_dosage_versus_refs
 *   _QUILT_rcpp_forwardBackwardGibbsNIPT     63 arguments   RcppExports.cpp:966-1038    -> qa_gibbs_batch(_rare_common)
 *   _QUILT_Rcpp_make_gl_bound                 3 arguments   RcppExports.cpp:1263-1273   -> qa_Rcpp_make_gl_bound
 *   _QUILT_rcpp_make_eMatRead_t              15 arguments   RcppExports.cpp:15-38       -> qa_rcpp_make_eMatRead_t
 *
 * The C functions are called qa_QUILT_<fn> -- NOT _QUILT_<fn>: RcppExports.cpp defines those symbols itself, and this
 * file is compiled INTO QUILT.so (shim/QUILT-src.patch adds it to QUILT/src and points the four rows of RcppExports.cpp's
 * CallEntries[] at the functions here; R_init_QUILT then registers them under the reference's names, so every
 * `.Call('_QUILT_<fn>', PACKAGE = 'QUILT', ...)` of the unmodified R code lands here).  It can also be built as a DLL of its
 * own (R_init_quilt_amd_shim below) and swapped in with `assignInNamespace` (INTEGRATION.md shows both); no R function
 * changes its signature.  The prepared panel is uploaded on first use and cached in this file (keyed by the identity of the R
 * objects -- data pointer and dimensions of distinctHapsB / hapMatcherR -- plus ref_error and a checksum over transMatRate and
 * samples of both tables, so that a different panel that lands on a recycled address is not mistaken for the cached one), so
 * the 38- and 63-argument entries keep their arity; `qa_shim_release()` (0 arguments) drops the cache.  R owns every buffer it passes: results are copied back into
 * them before returning (SURVEY.md 8(b) "Ownership").
 *
 * Random numbers.  The reference draws inside the native call from R's generator (`Rcpp::runif`, `Rcpp::sample`:
 * gibbs-nipt.cpp:2845-2848, 3013-3018; gibbs-nipt-block.cpp:2054) under `Rcpp::RNGScope` (RcppExports.cpp:971).  The
 * shim draws the same uniforms, in the same order, with unif_rand() (`sample(nReads, 1)` = one unif_rand() scaled by nReads,
 * as Rcpp's sugar EmpiricalSample does) between GetRNGstate() / PutRNGstate() and passes them down; the device never generates R-incompatible numbers on this
 * path.  The shard pass draws nGrids - 1 uniforms per block iteration: what gibbs-nipt-block.cpp:2054 draws with
 * shard_check_every_pair = TRUE, the production value (quilt.R:178); with FALSE a pass draws n_blocks - 1, asked for through
 * draw_shard_uniforms_from_R below once the pass's table exists (not with the rare + common call, which refuses FALSE).  Where the reference's draw count depends on
 * intermediate results (`Rcpp::sample(1:3, 1, prob)` per read whose class leaves a choice, in rcpp_sample_H_using_H_class, NIPT
 * only) the stream cannot be pre-drawn: since round 6 the library asks for those uniforms WHEN the reference draws them
 * (qa_gibbs_opts_t.draw_uniforms -> draw_uniforms_from_R below: runif_proposed / runif_block / runif_total before a block pass,
 * one unif_rand() per drawing read after its relabelling), so the NIPT entry consumes R's generator in the reference's order and
 * number as well (tests/test_shim_gpu.py counts them against the oracle run on the same stream).
 *
 * Type-checked without R by `make -C shim check` against shim/qa_r_api.h (declarations only), and EXECUTED without R by
 * tests/test_shim_gpu.py / tests/test_shim_cpu.py under tests/c/mini_r.c, a test runtime behind the same declarations (objects
 * with type, length, names and dim; `.Call` by registered name with R's arity check; Rf_error as an exception; unif_rand() from a
 * loaded sequence): every routine below is called with R-shaped arguments and compared with the Python mirror's call.
 */
#ifdef QA_HAVE_R
#include <R.h>
#include <Rinternals.h>
#include <R_ext/Random.h>
#include <R_ext/Rdynload.h>
#else
#include "qa_r_api.h"
#endif

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include "../include/quilt_amd.h"
#include "../include/quilt_amd_io.h"   /* qa_impute_bam_range */

/* ---- small helpers ---------------------------------------------------------------------------------------------- */

static SEXP list_get(SEXP list, const char *name) {
    SEXP names = Rf_getAttrib(list, R_NamesSymbol);
    for (R_xlen_t i = 0; i < Rf_xlength(list); i++)
        if (names != R_NilValue && strcmp(CHAR(STRING_ELT(names, i)), name) == 0) return VECTOR_ELT(list, i);
    return R_NilValue;
}
static int flag(SEXP param_list, const char *name, int dflt) {
    SEXP v = list_get(param_list, name);
    return v == R_NilValue ? dflt : Rf_asLogical(v);
}
static double num_or(SEXP list, const char *name, double dflt) {
    SEXP v = list_get(list, name);
    return (v == R_NilValue || Rf_length(v) < 1) ? dflt : Rf_asReal(v);
}
static const char *one_string(SEXP list, const char *name) {
    SEXP v = list_get(list, name);
    return (v != R_NilValue && TYPEOF(v) == STRSXP && Rf_length(v) == 1) ? CHAR(STRING_ELT(v, 0)) : NULL;
}
static void check_status(int st, const char *what) {
    if (st < 0) Rf_error("%s: libquilt_amd status %d: %s", what, st, qa_last_error());
}
static int is_nipt(SEXP paramsSEXP) {   /* params$method == "nipt" (absent: "diploid") */
    const char *m = one_string(paramsSEXP, "method");
    return m != NULL && strcmp(m, "nipt") == 0;
}

/* ---- each conversion of an R object, once -------------------------------------------------------------------------- */

/* element i of an integer-or-double vector (every int32 is a double, so the integer case loses nothing) */
static double num_at(SEXP v, int i) { return TYPEOF(v) == INTSXP ? INTEGER(v)[i] : REAL(v)[i]; }
/* an integer-or-double vector of length n as int32_t[] / int64_t[] (malloc); NULL when it is not one, or out of memory */
static int32_t *ints_of(SEXP v, int n) {
    if (v == R_NilValue || (TYPEOF(v) != INTSXP && TYPEOF(v) != REALSXP) || Rf_length(v) != n) return NULL;
    int32_t *out = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n > 0 ? n : 1));
    for (int i = 0; out && i < n; i++) out[i] = (int32_t)num_at(v, i);
    return out;
}
static int64_t *int64s_of(SEXP v, int n) {   /* (a sample's global index: kept as wide as the library takes it) */
    if (v == R_NilValue || (TYPEOF(v) != INTSXP && TYPEOF(v) != REALSXP) || Rf_length(v) != n) return NULL;
    int64_t *out = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n > 0 ? n : 1));
    for (int i = 0; out && i < n; i++) out[i] = (int64_t)num_at(v, i);
    return out;
}
/* C arrays as fresh R vectors (the caller roots them: result_add below, or PROTECT) */
static SEXP int_vector(const int32_t *v, int n) {
    SEXP out = Rf_allocVector(INTSXP, n);
    if (n > 0) memcpy(INTEGER(out), v, sizeof(int) * (size_t)n);
    return out;
}
static SEXP real_vector(const double *v, int n) {
    SEXP out = Rf_allocVector(REALSXP, n);
    if (n > 0) memcpy(REAL(out), v, sizeof(double) * (size_t)n);
    return out;
}
static void counters_to_real(const int64_t *v, int n, SEXP out) {   /* the library's int64 counters (stats, bx_stats) as R numbers */
    for (int i = 0; i < n; i++) REAL(out)[i] = (double)v[i];
}

/* sites$<name>: one TRUE or FALSE (NA is neither); absent: dflt */
static int strict_flag(SEXP sitesSEXP, const char *name, int dflt, const char *who) {
    SEXP v = list_get(sitesSEXP, name);
    if (v == R_NilValue) return dflt;
    if (TYPEOF(v) != LGLSXP || Rf_length(v) != 1 || (LOGICAL(v)[0] != 0 && LOGICAL(v)[0] != 1))
        Rf_error("quilt_amd: %s: sites$%s must be TRUE or FALSE", who, name);
    return LOGICAL(v)[0] != 0;
}
/* hla_run (functions.R:1261-1280): params$hla_grid, the 0-based grid of gamma1 / gamma2; -1 when absent */
static int hla_grid_of(SEXP paramsSEXP, const char *who, int G) {
    SEXP hg = list_get(paramsSEXP, "hla_grid");
    if (hg == R_NilValue) return -1;
    const double v = Rf_length(hg) == 1 && (TYPEOF(hg) == INTSXP || TYPEOF(hg) == REALSXP) ? Rf_asReal(hg) : -1;
    if (!(v >= 0 && v < G && v == floor(v)))   /* (NA and NaN fail every comparison) */
        Rf_error("quilt_amd: %s: params$hla_grid must be one whole number in [0, nGrids = %d) (iGrid - 1)", who, G);
    return (int)v;
}

/* A result list built by appending (name, value) pairs: names and values cannot go out of step and nobody counts positions.
 * A value is reachable from the builder's protected slots from the moment it is added, so `result_add(&r, "x", Rf_alloc...)` needs
 * no PROTECT of its own.  result_begin leaves ONE object on the PROTECT stack and result_end takes it off again: whatever a
 * routine PROTECTs in between it UNPROTECTs in between. */
#define RESULT_MAX 16
typedef struct { SEXP slots; const char *names[RESULT_MAX]; int n; } result_t;
static void result_begin(result_t *r) { r->slots = PROTECT(Rf_allocVector(VECSXP, RESULT_MAX)); r->n = 0; }
static SEXP result_add(result_t *r, const char *name, SEXP value) {
    r->names[r->n] = name;
    return SET_VECTOR_ELT(r->slots, r->n++, value);
}
static SEXP result_end(result_t *r) {
    SEXP out = PROTECT(Rf_allocVector(VECSXP, r->n)), nm = PROTECT(Rf_allocVector(STRSXP, r->n));
    for (int i = 0; i < r->n; i++) {
        SET_VECTOR_ELT(out, i, VECTOR_ELT(r->slots, i));
        SET_STRING_ELT(nm, i, Rf_mkChar(r->names[i]));
    }
    Rf_setAttrib(out, R_NamesSymbol, nm);
    UNPROTECT(3);
    return out;
}

/* sampleReads (list over reads of list(J, wif, bq matrix, u matrix): copied-from-stitch.cpp:153-160) in the flattened form of
 * include/quilt_amd.h: read_off n + 1; per sample read_ptr R + 1 (at read_off[i] + i); bases back to back; wif per read. */
typedef struct { int32_t *read_off, *read_ptr, *wif, *u, *bq; } flat_reads_t;
static void flat_reads_free(flat_reads_t *f) {
    free(f->read_off); free(f->read_ptr); free(f->wif); free(f->u); free(f->bq);
    memset(f, 0, sizeof *f);
}
/* `nested`: a list of sampleReads (the range call); otherwise ONE sampleReads (the per-call entries: read_off = {0, R}).  wif is
 * filled only when asked for.  Returns 0, or -1 when an allocation failed -- everything it allocated is then freed again and the
 * caller raises the R error.  Raises none itself: what the range call passes has been through validate_reads_list. */
static int pack_reads(SEXP readsSEXP, int nested, int want_wif, flat_reads_t *f) {
    const int n = nested ? Rf_length(readsSEXP) : 1;
    memset(f, 0, sizeof *f);
    f->read_off = (int32_t *)malloc(sizeof(int32_t) * ((size_t)n + 1));
    if (!f->read_off) return -1;
    f->read_off[0] = 0;
    size_t nbases = 0;
    for (int i = 0; i < n; i++) {
        SEXP sr = nested ? VECTOR_ELT(readsSEXP, i) : readsSEXP;
        const int R = Rf_length(sr);
        f->read_off[i + 1] = f->read_off[i] + R;
        for (int r = 0; r < R; r++) nbases += (size_t)Rf_length(VECTOR_ELT(VECTOR_ELT(sr, r), 3));
    }
    const int totR = f->read_off[n];
    f->read_ptr = (int32_t *)malloc(sizeof(int32_t) * ((size_t)totR + (size_t)n + 1));
    if (want_wif) f->wif = (int32_t *)malloc(sizeof(int32_t) * (size_t)(totR > 0 ? totR : 1));
    f->u = (int32_t *)malloc(sizeof(int32_t) * (nbases > 0 ? nbases : 1));
    f->bq = (int32_t *)malloc(sizeof(int32_t) * (nbases > 0 ? nbases : 1));
    if (!f->read_ptr || (want_wif && !f->wif) || !f->u || !f->bq) {
        flat_reads_free(f);
        return -1;
    }
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        SEXP sr = nested ? VECTOR_ELT(readsSEXP, i) : readsSEXP;
        const int R = Rf_length(sr);
        int32_t *rp = f->read_ptr + f->read_off[i] + i;
        rp[0] = 0;
        for (int r = 0; r < R; r++) {
            SEXP rd = VECTOR_ELT(sr, r);
            const int nb = Rf_length(VECTOR_ELT(rd, 3));
            if (want_wif) f->wif[f->read_off[i] + r] = Rf_asInteger(VECTOR_ELT(rd, 1));
            memcpy(f->bq + at, INTEGER(VECTOR_ELT(rd, 2)), sizeof(int) * (size_t)nb);
            memcpy(f->u + at, INTEGER(VECTOR_ELT(rd, 3)), sizeof(int) * (size_t)nb);
            at += (size_t)nb;
            rp[r + 1] = rp[r] + nb;
        }
    }
    return 0;
}

/* The rare + common inputs of qa_rare_common_create: rare_per_hap_info (list over the K haplotypes of 1-based all-SNP indices,
 * rare_common.R:222-247) as CSR, snp_is_common as bytes.  0, or -1 when an allocation failed (nothing stays allocated then). */
typedef struct { int64_t *rare_ptr; int32_t *rare_snp; uint8_t *is_common; } rare_inputs_t;
static void rare_inputs_free(rare_inputs_t *ri) {
    free(ri->rare_ptr); free(ri->rare_snp); free(ri->is_common);
    memset(ri, 0, sizeof *ri);
}
static int rare_inputs_pack(SEXP rare_per_hap_infoSEXP, SEXP snp_is_commonSEXP, int K, rare_inputs_t *ri) {
    const int T = Rf_length(snp_is_commonSEXP);
    memset(ri, 0, sizeof *ri);
    ri->is_common = (uint8_t *)malloc((size_t)(T > 0 ? T : 1));
    ri->rare_ptr = (int64_t *)malloc(sizeof(int64_t) * ((size_t)K + 1));
    if (ri->is_common && ri->rare_ptr) {
        for (int t = 0; t < T; t++) ri->is_common[t] = LOGICAL(snp_is_commonSEXP)[t] ? 1 : 0;
        ri->rare_ptr[0] = 0;
        for (int k = 0; k < K; k++) ri->rare_ptr[k + 1] = ri->rare_ptr[k] + Rf_length(VECTOR_ELT(rare_per_hap_infoSEXP, k));
        ri->rare_snp = (int32_t *)malloc(sizeof(int32_t) * (size_t)(ri->rare_ptr[K] > 0 ? ri->rare_ptr[K] : 1));
    }
    if (!ri->is_common || !ri->rare_ptr || !ri->rare_snp) {
        rare_inputs_free(ri);
        return -1;
    }
    for (int k = 0; k < K; k++)
        if (ri->rare_ptr[k + 1] > ri->rare_ptr[k])
            memcpy(ri->rare_snp + ri->rare_ptr[k], INTEGER(VECTOR_ELT(rare_per_hap_infoSEXP, k)),
                   sizeof(int) * (size_t)(ri->rare_ptr[k + 1] - ri->rare_ptr[k]));
    return 0;
}

/* ---- the prepared panel, uploaded once per process ---------------------------------------------------------------- */

static struct {
    qa_panel_t *panel;
    qa_rare_common_t *rc;
    const void *key_B, *key_hm, *key_rare;
    int K, G, T, nMaxDH;
    double ref_error;
    uint64_t checksum;
} g_cache;

/* FNV-1a over the transition rates and evenly spaced samples of the two panel tables: cheap next to any call it guards */
static uint64_t fnv(uint64_t h, const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}
static uint64_t panel_checksum(const void *hm, size_t hm_bytes, const int *B, size_t nB, const double *tm, size_t n_tm) {
    uint64_t h = 1469598103934665603ull;
    h = fnv(h, tm, n_tm * sizeof(double));
    const size_t step_h = hm_bytes / 4096 + 1, step_B = nB / 4096 + 1;
    for (size_t i = 0; i < hm_bytes; i += step_h) h = fnv(h, (const unsigned char *)hm + i, 1);
    for (size_t i = 0; i < nB; i += step_B) h = fnv(h, B + i, sizeof(int));
    return h;
}

static void cache_drop(void) {
    if (g_cache.rc) qa_rare_common_destroy(g_cache.rc);
    if (g_cache.panel) qa_panel_destroy(g_cache.panel);
    memset(&g_cache, 0, sizeof g_cache);
}

/* transMatRate: 2 x (G - 1) doubles (column-major), the first slice of transMatRate_tc_H or transMatRate_t itself */
static qa_panel_t *panel_for(SEXP hapMatcher, SEXP hapMatcherR, int use_hapMatcherR, SEXP distinctHapsB, SEXP distinctHapsIE,
                             SEXP special_helper, SEXP special_matrix, SEXP special_grid_which, SEXP rhb_t, double ref_error,
                             int use_eMatDH_special_symbols, const double *transMatRate) {
    const int nMaxDH = Rf_nrows(distinctHapsB), G = Rf_ncols(distinctHapsB), T = Rf_ncols(distinctHapsIE);
    SEXP hm = use_hapMatcherR ? hapMatcherR : hapMatcher;
    const int K = Rf_nrows(hm);
    const void *kB = INTEGER(distinctHapsB), *kh = use_hapMatcherR ? (const void *)RAW(hapMatcherR) : (const void *)INTEGER(hapMatcher);
    const uint64_t sum = panel_checksum(kh, (size_t)K * G * (use_hapMatcherR ? 1 : sizeof(int)), INTEGER(distinctHapsB),
                                        (size_t)nMaxDH * G, transMatRate, 2 * (size_t)(G > 1 ? G - 1 : 0));
    if (g_cache.panel && g_cache.key_B == kB && g_cache.key_hm == kh && g_cache.K == K && g_cache.G == G && g_cache.T == T &&
        g_cache.nMaxDH == nMaxDH && g_cache.ref_error == ref_error && g_cache.checksum == sum)
        return g_cache.panel;
    cache_drop();
    qa_panel_desc_t d;
    memset(&d, 0, sizeof d);
    d.K = K; d.nGrids = G; d.nSNPs = T; d.nMaxDH = nMaxDH;
    d.hapMatcherR = use_hapMatcherR ? RAW(hapMatcherR) : NULL;
    d.hapMatcher = use_hapMatcherR ? NULL : INTEGER(hapMatcher);
    const int have_rhb = Rf_nrows(rhb_t) == K && Rf_ncols(rhb_t) == G;   /* 1 x 1 in msPBWT mode (quilt.R:551-563) */
    d.rhb_t = have_rhb ? INTEGER(rhb_t) : NULL;
    d.distinctHapsB = INTEGER(distinctHapsB);
    d.distinctHapsIE = REAL(distinctHapsIE);
    int *which = NULL;
    if (special_grid_which != R_NilValue) {
        d.eMatDH_special_grid_which = INTEGER(special_grid_which);
    } else {   /* the Gibbs entry does not receive it: a grid holds specials iff its helper row is set (first row > 0) */
        which = (int *)calloc((size_t)G, sizeof(int));
        int n = 0;
        for (int g = 0; g < G; g++)
            if (Rf_nrows(special_helper) == G && INTEGER(special_helper)[g] > 0) which[g] = ++n;
        d.eMatDH_special_grid_which = which;
    }
    d.eMatDH_special_matrix_helper = Rf_nrows(special_helper) == G ? INTEGER(special_helper) : NULL;
    d.eMatDH_special_matrix = INTEGER(special_matrix);
    d.eMatDH_special_matrix_nrow = Rf_nrows(special_matrix);
    d.use_eMatDH_special_symbols = use_eMatDH_special_symbols || !have_rhb;
    d.transMatRate_t = transMatRate;
    d.ref_error = ref_error;
    qa_panel_t *p = NULL;
    const int st = qa_panel_create(&d, &p);
    free(which);
    check_status(st, "qa_panel_create");
    {   /* QUILT_AMD_SUM_ORDER (Sys.setenv before the first call; read when the panel is uploaded): 1 / 2 = the VALIDATION MODE of
         * the full-panel passes (include/quilt_amd.h, qa_panel_set_sum_order) for the per-call entries as well */
        const char *e = getenv("QUILT_AMD_SUM_ORDER");
        if (e && (e[0] == '1' || e[0] == '2') && e[1] == 0) check_status(qa_panel_set_sum_order(p, e[0] - '0'), "qa_panel_set_sum_order");
    }
    g_cache.panel = p; g_cache.key_B = kB; g_cache.key_hm = kh;
    g_cache.K = K; g_cache.G = G; g_cache.T = T; g_cache.nMaxDH = nMaxDH;
    g_cache.ref_error = ref_error; g_cache.checksum = sum;
    return p;
}

SEXP qa_shim_release(void) {
    cache_drop();
    (void)qa_impute_release_buffers();   /* pinned transfer buffers of qa_impute_samples, if any are still kept */
    return R_NilValue;
}

/* ---- _QUILT_Rcpp_make_gl_bound(gl, minGLValue, to_fix)  (reference-single.cpp:68-94; to_fix 0-based) --------------- */

SEXP qa_QUILT_Rcpp_make_gl_bound(SEXP glSEXP, SEXP minGLValueSEXP, SEXP to_fixSEXP) {
    check_status(qa_Rcpp_make_gl_bound(REAL(glSEXP), Rf_asReal(minGLValueSEXP), INTEGER(to_fixSEXP), Rf_length(to_fixSEXP)),
                 "qa_Rcpp_make_gl_bound");
    return R_NilValue;
}

/* ---- _QUILT_Rcpp_haploid_dosage_versus_refs: the 38 arguments of RcppExports.cpp:1582, in order ------------------------- */

SEXP qa_QUILT_Rcpp_haploid_dosage_versus_refs(
    SEXP glSEXP, SEXP arma_alphaHat_tSEXP, SEXP eigen_alphaHat_tSEXP, SEXP betaHat_tSEXP, SEXP cSEXP, SEXP gamma_tSEXP,
    SEXP gammaSmall_tSEXP, SEXP best_haps_stuff_listSEXP, SEXP dosageSEXP, SEXP transMatRate_tSEXP, SEXP rhb_tSEXP,
    SEXP ref_errorSEXP, SEXP use_eMatDHSEXP, SEXP distinctHapsBSEXP, SEXP distinctHapsIESEXP,
    SEXP eMatDH_special_matrix_helperSEXP, SEXP eMatDH_special_matrixSEXP, SEXP use_eMatDH_special_symbolsSEXP,
    SEXP hapMatcherSEXP, SEXP hapMatcherRSEXP, SEXP use_hapMatcherRSEXP, SEXP gammaSmall_cols_to_getSEXP,
    SEXP eMatDH_special_grid_whichSEXP, SEXP eMatDH_special_values_listSEXP, SEXP K_top_matchesSEXP, SEXP suppressOutputSEXP,
    SEXP min_emission_prob_normalization_thresholdSEXP, SEXP return_betaHat_tSEXP, SEXP return_dosageSEXP,
    SEXP return_gamma_tSEXP, SEXP return_gammaSmall_tSEXP, SEXP get_best_haps_from_thinned_sitesSEXP, SEXP is_version_2SEXP,
    SEXP is_version_3SEXP, SEXP return_extraSEXP, SEXP always_normalizeSEXP, SEXP use_eigenSEXP, SEXP normalize_emissionsSEXP) {
    (void)eMatDH_special_values_listSEXP; (void)is_version_2SEXP; (void)return_extraSEXP; (void)use_eigenSEXP;
    if (!Rf_asLogical(use_eMatDHSEXP)) Rf_error("quilt_amd: use_eMatDH = FALSE is not supported (the production path uses TRUE)");
    qa_panel_t *panel = panel_for(hapMatcherSEXP, hapMatcherRSEXP, Rf_asLogical(use_hapMatcherRSEXP), distinctHapsBSEXP,
                                  distinctHapsIESEXP, eMatDH_special_matrix_helperSEXP, eMatDH_special_matrixSEXP,
                                  eMatDH_special_grid_whichSEXP, rhb_tSEXP, Rf_asReal(ref_errorSEXP),
                                  Rf_asLogical(use_eMatDH_special_symbolsSEXP), REAL(transMatRate_tSEXP));
    qa_fullpass_opts_t o;
    memset(&o, 0, sizeof o);
    o.K_top_matches = Rf_asInteger(K_top_matchesSEXP);
    o.return_betaHat_t = Rf_asLogical(return_betaHat_tSEXP);
    o.return_dosage = Rf_asLogical(return_dosageSEXP);
    o.return_gamma_t = Rf_asLogical(return_gamma_tSEXP);
    o.return_gammaSmall_t = Rf_asLogical(return_gammaSmall_tSEXP);
    o.get_best_haps_from_thinned_sites = Rf_asLogical(get_best_haps_from_thinned_sitesSEXP);
    o.always_normalize = Rf_asLogical(always_normalizeSEXP);
    o.normalize_emissions = Rf_asLogical(normalize_emissionsSEXP);
    o.min_emission_prob_normalization_threshold = Rf_asReal(min_emission_prob_normalization_thresholdSEXP);
    o.suppressOutput = Rf_asInteger(suppressOutputSEXP);
    /* version 3 writes alpha through the Eigen map, versions 1 / 2 through the arma matrix: both alias R's matrix */
    SEXP alphaSEXP = Rf_asLogical(is_version_3SEXP) ? eigen_alphaHat_tSEXP : arma_alphaHat_tSEXP;
    const int G = g_cache.G, K = g_cache.K;
    double *alpha = (Rf_nrows(alphaSEXP) == K && Rf_ncols(alphaSEXP) == G) ? REAL(alphaSEXP) : NULL;
    const int *cols = INTEGER(gammaSmall_cols_to_getSEXP);
    int n_thin = 0;
    for (int g = 0; g < G; g++) if (cols[g] + 1 > n_thin) n_thin = cols[g] + 1;
    int32_t *bptr = (int32_t *)calloc((size_t)n_thin + 1, sizeof(int32_t));
    int64_t cap = 64 * (int64_t)(n_thin > 0 ? n_thin : 1);
    int32_t *bidx = NULL;
    double *bval = NULL;
    int st = QA_OK;
    for (int attempt = 0; attempt < 2; attempt++) {
        bidx = (int32_t *)realloc(bidx, sizeof(int32_t) * (size_t)cap);
        bval = (double *)realloc(bval, sizeof(double) * (size_t)cap);
        st = qa_Rcpp_haploid_dosage_versus_refs(panel, REAL(glSEXP), cols, &o, alpha,
                                                o.return_betaHat_t ? REAL(betaHat_tSEXP) : NULL, REAL(cSEXP),
                                                o.return_gamma_t ? REAL(gamma_tSEXP) : NULL,
                                                o.return_gammaSmall_t ? REAL(gammaSmall_tSEXP) : NULL,
                                                o.return_dosage ? REAL(dosageSEXP) : NULL, bptr, bidx, bval, cap);
        if (st != QA_ERR_CAPACITY) break;
        cap = bptr[n_thin];   /* needed sizes are in bptr */
    }
    if (st >= 0 && o.get_best_haps_from_thinned_sites) {
        /* best_haps_stuff_list[[i]] <- list(top_matches = <0-based k>, top_matches_values = <gamma>) (reference-single.cpp:2024-2030) */
        for (int i = 0; i < n_thin && i < Rf_length(best_haps_stuff_listSEXP); i++) {
            const int n = bptr[i + 1] - bptr[i];
            result_t e;
            result_begin(&e);
            result_add(&e, "top_matches", int_vector(bidx + bptr[i], n));
            result_add(&e, "top_matches_values", real_vector(bval + bptr[i], n));
            SET_VECTOR_ELT(best_haps_stuff_listSEXP, i, result_end(&e));
        }
    }
    free(bptr); free(bidx); free(bval);
    check_status(st, "qa_Rcpp_haploid_dosage_versus_refs");
    return R_NilValue;
}

/* ---- _QUILT_rcpp_forwardBackwardGibbsNIPT: the 63 arguments of RcppExports.cpp:968, in order -------------------------- */

/* calculate_likelihoods_values + add_to_per_it_likelihoods (gibbs-nipt.cpp:1463-1621) from the per-sweep record */
/* qa_gibbs_opts_t.draw_uniforms for the 63-argument entry (NIPT): the block passes' uniforms drawn from R's generator WHEN the
 * reference draws them.  At a block iteration the reference draws runif_proposed (6 x nReads, unused by block_approach 6),
 * runif_block (nReads) and runif_total (nReads, read only by the total relabelling, which is off) -- gibbs-nipt.cpp:3013-3017 --
 * and then, inside rcpp_sample_H_using_H_class (gibbs-nipt-block.cpp:213-246), one uniform per Rcpp::sample(1:3, 1, prob), i.e.
 * per read whose class leaves a choice, in read order.  The library asks for the first kind before the pass (what = 0) and for
 * the second after its relabelling (what = 1), from the thread that made the .Call. */
static void draw_uniforms_from_R(void *ctx, int32_t chain, int32_t pass, int32_t what, int32_t n, double *out) {
    (void)ctx; (void)chain; (void)pass;
    if (what == 0) {
        for (long i = 0; i < 6L * n; i++) (void)unif_rand();   /* :3013-3015 runif_proposed */
        for (int r = 0; r < n; r++) out[r] = unif_rand();     /* :3016 runif_block */
        for (int r = 0; r < n; r++) (void)unif_rand();        /* :3017 runif_total */
    } else {
        for (int r = 0; r < n; r++) out[r] = unif_rand();     /* Rcpp::sample(one_through_3, 1, false, probs): one unif_rand() each */
    }
}

/* The same for a diploid call with shard_check_every_pair = FALSE (what = 2): at a block iteration the reference draws the
 * 8 x nReads above, none of which a diploid call uses (gibbs-nipt.cpp:3013-3018), and then, inside the shard resampler,
 * runif(n_blocks - 1) for the table it has just made (gibbs-nipt-block.cpp:2054).  The library asks only where n_blocks > 1, so
 * the 8 x nReads of the passes it did not ask for are made up before the next pass's draws, and after the call. */
typedef struct { int n_reads, next_pass; } shard_draws_t;
static void burn_block_iterations(shard_draws_t *d, int upto_pass) {
    for (; d->next_pass <= upto_pass; d->next_pass++)
        for (long i = 0; i < 8L * d->n_reads; i++) (void)unif_rand();
}
static void draw_shard_uniforms_from_R(void *ctx, int32_t chain, int32_t pass, int32_t what, int32_t n, double *out) {
    (void)chain; (void)what;
    burn_block_iterations((shard_draws_t *)ctx, pass);
    for (int b = 0; b < n; b++) out[b] = unif_rand();
}

static double lgamma1(double x) { return lgamma(x + 1.0); }
static void fill_per_it_row(double *m, int nrow, int row, const double *rec, double ff, int it, double p_H_class) {
    const double prior[3] = {0.5, (1 - ff) / 2, ff / 2};
    const double d1 = rec[0], d2 = rec[1], d3 = rec[2], rc[3] = {rec[3], rec[4], rec[5]};
    double dH = 0, set = lgamma1(rc[0] + rc[1] + rc[2]);
    for (int h = 0; h < 3; h++) {
        if (rc[h] > 0) dH += rc[h] * log(prior[h]);
        if (prior[h] > 0) set += rc[h] * log(prior[h]) - lgamma1(rc[h]);
    }
    const double v[13] = {1, 1, it + 1, 1, d1, d2, d3, d1 + d2 + d3, dH, d1 + d2 + d3 + dH, set, 0, p_H_class};
    for (int j = 0; j < 13; j++) m[(size_t)j * nrow + row] = v[j];
}
static double log_p_H_class(const int *H_class, int n, double ff) {   /* rcpp_get_log_p_H_class, gibbs-nipt-block.cpp:146-164 */
    const double vals[8] = {0, log(0.5), log(0.5 - ff * 0.5), log(ff * 0.5), log(1.0 - ff * 0.5), log(0.5 + ff * 0.5), log(0.5), 0};
    double out = 0;
    for (int i = 0; i < n; i++) out += vals[H_class[i] & 7];
    return out;
}

/* per_it_likelihoods: one row per sweep, the 13 columns of gibbs-nipt.cpp:2767-2768 */
static SEXP per_it_likelihoods(const double *per_it, int n_its, const int32_t *H_class, int R, double ff) {
    static const char *cn[13] = {"s", "i_samp", "i_it", "i_result_it", "p_O1_given_H1_L", "p_O2_given_H2_L", "p_O3_given_H3_L",
                                 "p_O_given_H_L", "p_H_given_L", "p_O_H_given_L_up_to_C", "p_set_H_given_L", "relabel",
                                 "p_H_class_given_L"};
    SEXP pit = PROTECT(Rf_allocMatrix(REALSXP, n_its, 13));
    for (int it = 0; it < n_its; it++)   /* H_class is recorded by the last sweep only: NA before */
        fill_per_it_row(REAL(pit), n_its, it, per_it + (size_t)it * 8, ff, it,
                        it == n_its - 1 ? log_p_H_class(H_class, R, ff) : NA_REAL);
    SEXP dn = PROTECT(Rf_allocVector(VECSXP, 2)), cns = PROTECT(Rf_allocVector(STRSXP, 13));
    for (int j = 0; j < 13; j++) SET_STRING_ELT(cns, j, Rf_mkChar(cn[j]));
    SET_VECTOR_ELT(dn, 0, R_NilValue);
    SET_VECTOR_ELT(dn, 1, cns);
    Rf_setAttrib(pit, R_DimNamesSymbol, dn);
    UNPROTECT(3);
    return pit;
}

/* Everything one call of the 63-argument entry mallocs, freed in one place, and what its draws leave for the call */
typedef struct {
    flat_reads_t reads;
    double *per_it, *runif_reads, *runif_pass, *state;
    int32_t *H, *H_class, first_read;
    int by_blocks, n_passes;   /* the block-wise shard passes (shard_check_every_pair = FALSE) and how many the library runs */
    shard_draws_t shard_draws;
} gibbs_call_t;
static void gibbs_call_free(gibbs_call_t *c) {
    flat_reads_free(&c->reads);
    free(c->per_it); free(c->runif_reads); free(c->runif_pass); free(c->H); free(c->H_class); free(c->state);
}

/* stage 1: arguments the production caller holds constant with another value */
static void gibbs_refuse_non_production(SEXP pl, SEXP n_gibbs_startsSEXP, SEXP generate_fb_snp_offsetsSEXP) {
    if (Rf_asInteger(n_gibbs_startsSEXP) != 1 || flag(pl, "run_fb_subset", 0) || Rf_asLogical(generate_fb_snp_offsetsSEXP) ||
        !flag(pl, "use_starting_read_labels", 1) || flag(pl, "pass_in_eMatRead_t", 0) || flag(pl, "use_small_eHapsCurrent_tc", 0))
        Rf_error("quilt_amd: only the production form of rcpp_forwardBackwardGibbsNIPT is supported (n_gibbs_starts = 1, "
                 "run_fb_subset = FALSE, use_starting_read_labels = TRUE, pass_in_eMatRead_t = FALSE, packed panel)");
    if (!flag(pl, "shard_check_every_pair", 1) && flag(pl, "make_eMatRead_t_rare_common", 0))
        Rf_error("quilt_amd: shard_check_every_pair = FALSE is not supported with make_eMatRead_t_rare_common = TRUE");
}

/* stage 2, rare + common: the all-SNP handle beside the cached panel, made on first use and kept while snp_is_common is the same
 * R object.  transMatRate_tc_H is the all-SNP grid's here. */
static void cache_rare_common(qa_panel_t *panel, SEXP rare_per_hap_infoSEXP, SEXP snp_is_commonSEXP, SEXP transMatRate_tc_HSEXP) {
    if (g_cache.rc && g_cache.key_rare == (const void *)LOGICAL(snp_is_commonSEXP)) return;
    if (g_cache.rc) { qa_rare_common_destroy(g_cache.rc); g_cache.rc = NULL; }
    rare_inputs_t ri;
    if (rare_inputs_pack(rare_per_hap_infoSEXP, snp_is_commonSEXP, g_cache.K, &ri) != 0)
        Rf_error("quilt_amd: rcpp_forwardBackwardGibbsNIPT: out of memory");
    const int st = qa_rare_common_create(panel, Rf_length(snp_is_commonSEXP), ri.is_common, ri.rare_ptr, ri.rare_snp,
                                         REAL(transMatRate_tc_HSEXP), &g_cache.rc);
    rare_inputs_free(&ri);
    check_status(st, "qa_rare_common_create");
    g_cache.key_rare = LOGICAL(snp_is_commonSEXP);
}

/* stage 5: the reference's draws, in its order (RcppExports.cpp:971 RNGScope).  Opens R's generator and leaves it open: the entry
 * closes it after the call, because the library draws through the callbacks above while it runs. */
static void gibbs_draw(gibbs_call_t *c, qa_gibbs_opts_t *o, SEXP pl, SEXP block_gibbs_iterationsSEXP, double ff, int R, int G,
                       int n_its, int every_pair) {
    const int nb = Rf_length(block_gibbs_iterationsSEXP);
    const size_t n_pass_unif = ff != 0 ? (size_t)nb * 2 * (size_t)R : (size_t)nb * (size_t)(G - 1);
    double *runif_reads = (double *)malloc(sizeof(double) * ((size_t)R * (size_t)n_its + 1));
    double *runif_pass = (double *)calloc(n_pass_unif + 1, sizeof(double));   /* (NIPT: filled by the library through draw_uniforms) */
    int32_t first_read = 0;
    GetRNGstate();
    for (size_t i = 0; i < (size_t)R * (size_t)n_its; i++) runif_reads[i] = unif_rand();         /* gibbs-nipt.cpp:2845 */
    if (!flag(pl, "gibbs_initialize_at_first_read", 0) && R > 0) {
        /* :2846-2848 Rcpp::sample(nReads, 1) - 1.  Rcpp's sugar (sugar/functions/sample.h, EmpiricalSample, size < 2) draws
         * static_cast<int>(n * unif_rand() + 1): ONE unif_rand(), no rejection loop (R_unif_index under sample.kind =
         * "Rejection" would consume a data-dependent number of draws and return another value). */
        first_read = (int32_t)(unif_rand() * (double)R);
        if (first_read >= R) first_read = R - 1;
    }
    if (o->perform_block_gibbs && ff != 0) {
        /* NIPT: the block passes' draws depend on the passes' own results (one Rcpp::sample per read whose class leaves a choice),
         * so they are made when the reference makes them, through the library's callback; the generator stays open until the call
         * returns (PutRNGstate below the call) */
        o->draw_uniforms = draw_uniforms_from_R;
        o->draw_uniforms_ctx = NULL;
    }
    /* diploid, shard_check_every_pair = FALSE: a pass draws n_blocks - 1 uniforms for the table it makes itself -- through the
     * callback as well (qa_gibbs_opts_t.shard_by_blocks) */
    const int by_blocks = ff == 0 && !every_pair && o->perform_block_gibbs && o->do_shard_block_gibbs && nb > 0;
    c->shard_draws.n_reads = R; c->shard_draws.next_pass = 0;
    int n_passes = 0;   /* block iterations that name a sweep of the call, each once: the passes the library runs */
    if (by_blocks) {
        for (int ib = 0; ib < nb; ib++) {
            const int b = INTEGER(block_gibbs_iterationsSEXP)[ib];
            int seen = 0;
            for (int jb = 0; jb < ib; jb++) seen |= INTEGER(block_gibbs_iterationsSEXP)[jb] == b;
            n_passes += b >= 0 && b < n_its && !seen;
        }
        o->shard_by_blocks = 1;
        o->draw_uniforms = draw_shard_uniforms_from_R;
        o->draw_uniforms_ctx = &c->shard_draws;
    }
    if (o->perform_block_gibbs && ff == 0 && !by_blocks) {
        for (int ib = 0; ib < nb; ib++) {
            for (size_t i = 0; i < 6 * (size_t)R; i++) (void)unif_rand();                        /* :3013-3015 runif_proposed (unused by approach 6) */
            {
                for (size_t i = 0; i < 2 * (size_t)R; i++) (void)unif_rand();                    /* :3016-3017, no effect for diploid samples */
                if (o->do_shard_block_gibbs)
                    for (int g = 0; g < G - 1; g++) runif_pass[(size_t)ib * (G - 1) + g] = unif_rand();   /* gibbs-nipt-block.cpp:2054 */
            }
        }
    }
    c->runif_reads = runif_reads; c->runif_pass = runif_pass; c->first_read = first_read;
    c->by_blocks = by_blocks; c->n_passes = n_passes;
}

/* stage 7: the matrices the reference mutates in place (pass_in_alphaBeta = TRUE: R's buffers, quilt.R:731-745) */
static void gibbs_copy_state_back(const double *state, int Ks, int G, SEXP *dst, int n_dst) {
    const size_t m = (size_t)Ks * G;
    for (int i = 0; i < n_dst; i++)
        if (Rf_nrows(dst[i]) == Ks && Rf_ncols(dst[i]) == G) memcpy(REAL(dst[i]), state + (size_t)i * m, sizeof(double) * m);
}

/* stage 8: the result list, names as gibbs-nipt.cpp:3217-3306 (gm / gf / hap are the caller's, protected there) */
static SEXP gibbs_result_list(const gibbs_call_t *c, int R, int n_its, double ff, SEXP gm, SEXP gf, SEXP hap, int want_gen, int want_hap) {
    result_t r;
    result_begin(&r);
    result_add(&r, "underflow_problem", Rf_ScalarLogical(0));
    if (want_gen) { result_add(&r, "genProbsM_t", gm); result_add(&r, "genProbsF_t", gf); }
    if (want_hap) result_add(&r, "hapProbs_t", hap);
    SEXP Hs = result_add(&r, "H", int_vector(c->H, R));
    SEXP l1 = result_add(&r, "double_list_of_ending_read_labels", Rf_allocVector(VECSXP, 1));   /* [[s]][[i_gibbs_sampling]] */
    SEXP l2 = SET_VECTOR_ELT(l1, 0, Rf_allocVector(VECSXP, 1));
    SET_VECTOR_ELT(l2, 0, Hs);
    result_add(&r, "per_it_likelihoods", per_it_likelihoods(c->per_it, n_its, c->H_class, R, ff));
    result_add(&r, "H_class", int_vector(c->H_class, R));
    return result_end(&r);
}
/* ... or, after an underflow, only `underflow_problem = TRUE` (gibbs-nipt.cpp:2959-2969); impute_one_sample retries
 * (functions.R:2704-2715) */
static SEXP gibbs_underflow_list(void) {
    result_t r;
    result_begin(&r);
    result_add(&r, "underflow_problem", Rf_ScalarLogical(1));
    return result_end(&r);
}

SEXP qa_QUILT_rcpp_forwardBackwardGibbsNIPT(
    SEXP sampleReadsSEXP, SEXP eMatRead_tSEXP, SEXP priorCurrent_mSEXP, SEXP alphaMatCurrent_tcSEXP, SEXP eHapsCurrent_tcSEXP,
    SEXP transMatRate_tc_HSEXP, SEXP ffSEXP, SEXP blocks_for_outputSEXP, SEXP alphaHat_t1SEXP, SEXP betaHat_t1SEXP,
    SEXP alphaHat_t2SEXP, SEXP betaHat_t2SEXP, SEXP alphaHat_t3SEXP, SEXP betaHat_t3SEXP, SEXP eMatGrid_t1SEXP,
    SEXP eMatGrid_t2SEXP, SEXP eMatGrid_t3SEXP, SEXP gammaMT_t_localSEXP, SEXP gammaMU_t_localSEXP, SEXP gammaP_t_localSEXP,
    SEXP hapSum_tcSEXP, SEXP hapMatcherSEXP, SEXP hapMatcherRSEXP, SEXP use_hapMatcherRSEXP, SEXP distinctHapsBSEXP,
    SEXP distinctHapsIESEXP, SEXP eMatDH_special_matrix_helperSEXP, SEXP eMatDH_special_matrixSEXP, SEXP rhb_tSEXP,
    SEXP ref_errorSEXP, SEXP which_haps_to_useSEXP, SEXP wif0SEXP, SEXP grid_has_readSEXP, SEXP L_gridSEXP, SEXP smooth_cmSEXP,
    SEXP param_listSEXP, SEXP skip_read_iterationSEXP, SEXP Jmax_localSEXP, SEXP maxDifferenceBetweenReadsSEXP,
    SEXP maxEmissionMatrixDifferenceSEXP, SEXP run_fb_grid_offsetSEXP, SEXP gridSEXP, SEXP snp_start_1_basedSEXP,
    SEXP snp_end_1_basedSEXP, SEXP generate_fb_snp_offsetsSEXP, SEXP suppressOutputSEXP, SEXP n_gibbs_startsSEXP,
    SEXP n_gibbs_sample_itsSEXP, SEXP n_gibbs_burn_in_itsSEXP, SEXP double_list_of_starting_read_labelsSEXP,
    SEXP seed_vectorSEXP, SEXP prev_list_of_alphaBetaBlocksSEXP, SEXP i_snp_block_for_alpha_betaSEXP,
    SEXP do_block_resamplingSEXP, SEXP artificial_relabelSEXP, SEXP class_sum_cutoffSEXP, SEXP shuffle_bin_radiusSEXP,
    SEXP block_gibbs_iterationsSEXP, SEXP block_gibbs_quantile_probSEXP, SEXP rare_per_hap_infoSEXP,
    SEXP common_snp_indexSEXP, SEXP snp_is_commonSEXP, SEXP rare_per_snp_infoSEXP) {
    /* arguments the production caller holds constant or that only the unused code paths read */
    (void)eMatRead_tSEXP; (void)priorCurrent_mSEXP; (void)alphaMatCurrent_tcSEXP; (void)eHapsCurrent_tcSEXP;
    (void)blocks_for_outputSEXP; (void)alphaHat_t3SEXP; (void)betaHat_t3SEXP; (void)eMatGrid_t3SEXP; (void)gammaMT_t_localSEXP;
    (void)gammaMU_t_localSEXP; (void)gammaP_t_localSEXP; (void)hapSum_tcSEXP; (void)grid_has_readSEXP; (void)smooth_cmSEXP;
    (void)skip_read_iterationSEXP; (void)maxEmissionMatrixDifferenceSEXP; (void)run_fb_grid_offsetSEXP; (void)gridSEXP;
    (void)snp_start_1_basedSEXP; (void)snp_end_1_basedSEXP; (void)suppressOutputSEXP; (void)seed_vectorSEXP;
    (void)prev_list_of_alphaBetaBlocksSEXP; (void)i_snp_block_for_alpha_betaSEXP; (void)do_block_resamplingSEXP;
    (void)artificial_relabelSEXP; (void)common_snp_indexSEXP; (void)rare_per_snp_infoSEXP;
    SEXP pl = param_listSEXP;
    /* 1. refuse non-production forms */
    gibbs_refuse_non_production(pl, n_gibbs_startsSEXP, generate_fb_snp_offsetsSEXP);
    const double ff = Rf_asReal(ffSEXP);
    const int rare_common = flag(pl, "make_eMatRead_t_rare_common", 0), every_pair = flag(pl, "shard_check_every_pair", 1);
    /* 2. panel and rare + common handle from the cache.  transMatRate_tc_H: 2 x (G - 1) x S; with rare + common it is the all-SNP
     * grid's and the panel's own is not passed: the panel handle must then exist already (created by a full-panel call or an
     * earlier common-SNP Gibbs call) */
    const int G = Rf_nrows(transMatRate_tc_HSEXP) == 2 ? (int)(Rf_xlength(transMatRate_tc_HSEXP) / 2) + 1 : Rf_ncols(distinctHapsBSEXP);
    if (rare_common && !g_cache.panel) Rf_error("quilt_amd: the rare + common call needs the panel of an earlier common-SNP call");
    qa_panel_t *panel = rare_common ? g_cache.panel :
        panel_for(hapMatcherSEXP, hapMatcherRSEXP, Rf_asLogical(use_hapMatcherRSEXP), distinctHapsBSEXP, distinctHapsIESEXP,
                  eMatDH_special_matrix_helperSEXP, eMatDH_special_matrixSEXP, R_NilValue, rhb_tSEXP, Rf_asReal(ref_errorSEXP),
                  flag(pl, "use_eMatDH_special_symbols", 0), REAL(transMatRate_tc_HSEXP));
    if (rare_common) cache_rare_common(panel, rare_per_hap_infoSEXP, snp_is_commonSEXP, transMatRate_tc_HSEXP);
    const int T = rare_common ? Rf_length(snp_is_commonSEXP) : g_cache.T;
    /* 3. pack reads (the central grids come as wif0) */
    gibbs_call_t c;
    memset(&c, 0, sizeof c);
    const int R = Rf_length(sampleReadsSEXP), Ks = Rf_length(which_haps_to_useSEXP);
    if (pack_reads(sampleReadsSEXP, 0, 0, &c.reads) != 0) Rf_error("quilt_amd: rcpp_forwardBackwardGibbsNIPT: out of memory");
    /* 4. options */
    const int n_burn = Rf_asInteger(n_gibbs_burn_in_itsSEXP), n_samp = Rf_asInteger(n_gibbs_sample_itsSEXP), n_its = n_burn + n_samp;
    qa_gibbs_opts_t o;
    memset(&o, 0, sizeof o);
    o.Ks = Ks; o.ff = ff; o.sample_is_diploid = flag(pl, "sample_is_diploid", ff == 0);
    o.Jmax = Rf_asInteger(Jmax_localSEXP);
    o.maxDifferenceBetweenReads = Rf_asReal(maxDifferenceBetweenReadsSEXP);
    o.rescale_eMatRead_t = flag(pl, "rescale_eMatRead_t", 1);
    o.n_gibbs_burn_in_its = n_burn; o.n_gibbs_sample_its = n_samp;
    o.block_gibbs_iterations = INTEGER(block_gibbs_iterationsSEXP); o.n_block_gibbs_iterations = Rf_length(block_gibbs_iterationsSEXP);
    o.perform_block_gibbs = flag(pl, "perform_block_gibbs", 0);
    o.do_shard_block_gibbs = flag(pl, "do_shard_block_gibbs", 1);
    o.gibbs_initialize_iteratively = flag(pl, "gibbs_initialize_iteratively", 0);
    o.disable_read_category_usage = flag(pl, "disable_read_category_usage", 0);
    o.class_sum_cutoff = Rf_asReal(class_sum_cutoffSEXP);
    o.L_grid = INTEGER(L_gridSEXP); o.shuffle_bin_radius = Rf_asInteger(shuffle_bin_radiusSEXP);
    o.block_gibbs_quantile_prob = Rf_asReal(block_gibbs_quantile_probSEXP);
    o.per_it_out = c.per_it = (double *)calloc((size_t)(n_its > 0 ? n_its : 1) * 8, sizeof(double));
    /* 5. the reference's draws (R's generator stays open until the call has returned) */
    gibbs_draw(&c, &o, pl, block_gibbs_iterationsSEXP, ff, R, G, n_its, every_pair);
    /* 6. call: starting labels in, ending labels out */
    SEXP start = VECTOR_ELT(VECTOR_ELT(double_list_of_starting_read_labelsSEXP, 0), 0);
    c.H = (int32_t *)malloc(sizeof(int32_t) * (size_t)(R > 0 ? R : 1));
    c.H_class = (int32_t *)calloc((size_t)(R > 0 ? R : 1), sizeof(int32_t));
    memcpy(c.H, INTEGER(start), sizeof(int) * (size_t)R);
    const int want_hap = flag(pl, "return_hapProbs", 0), want_gen = flag(pl, "return_genProbs", 0);
    SEXP hap = PROTECT(Rf_allocMatrix(REALSXP, 3, T)), gm = PROTECT(Rf_allocMatrix(REALSXP, 3, T)), gf = PROTECT(Rf_allocMatrix(REALSXP, 3, T));
    c.state = (double *)malloc(sizeof(double) * ((size_t)6 * Ks * G + (size_t)3 * G));
    int32_t underflow = 0;
    const flat_reads_t *fr = &c.reads;
    const int st = rare_common
        ? qa_gibbs_batch_rare_common(panel, g_cache.rc, &o, 1, INTEGER(which_haps_to_useSEXP), fr->read_off, fr->read_ptr, fr->u, fr->bq,
                                     INTEGER(wif0SEXP), c.runif_reads, &c.first_read, c.runif_pass, c.H, c.H_class,
                                     (want_hap || want_gen) ? REAL(hap) : NULL, want_gen ? REAL(gm) : NULL,
                                     want_gen ? REAL(gf) : NULL, &underflow, c.state, NULL, NULL)
        : qa_gibbs_batch(panel, &o, 1, INTEGER(which_haps_to_useSEXP), fr->read_off, fr->read_ptr, fr->u, fr->bq, INTEGER(wif0SEXP),
                         c.runif_reads, &c.first_read, c.runif_pass, c.H, c.H_class, (want_hap || want_gen) ? REAL(hap) : NULL,
                         want_gen ? REAL(gm) : NULL, want_gen ? REAL(gf) : NULL, &underflow, c.state, NULL, NULL);
    if (c.by_blocks && st >= 0 && !underflow) burn_block_iterations(&c.shard_draws, c.n_passes - 1);
    PutRNGstate();   /* (after the call: with NIPT block passes the library draws through draw_uniforms_from_R while it runs) */
    SEXP out = R_NilValue;
    if (st >= 0 && !underflow) {
        /* 7. copy state back */
        SEXP dst[6] = {alphaHat_t1SEXP, alphaHat_t2SEXP, betaHat_t1SEXP, betaHat_t2SEXP, eMatGrid_t1SEXP, eMatGrid_t2SEXP};
        gibbs_copy_state_back(c.state, Ks, G, dst, 6);
        /* 8. result list ... */
        out = gibbs_result_list(&c, R, n_its, ff, gm, gf, hap, want_gen, want_hap);
    } else if (st >= 0) {
        out = gibbs_underflow_list();   /* ... or the underflow list */
    }
    gibbs_call_free(&c);
    UNPROTECT(3);
    check_status(st, "qa_gibbs_batch");
    return out;
}

/* ---- _QUILT_rcpp_make_eMatRead_t: the 15 arguments of RcppExports.cpp:17, in order ----------------------------------
 * Read likelihoods against the K rows of eHapsCurrent_tc[, , s + 1] (copied-from-stitch.cpp:115-229), written into the
 * caller's K x nReads eMatRead_t; production caller: calculate_eMatRead_t_vs_haplotypes (functions.R:2975-3020, K = 2 or 3).
 * Needs the device context of a panel handle: the calls that precede it in the driver loop have created one. */
#ifdef QA_INSIDE_QUILT_SO
/* Compiled into QUILT.so (shim/QUILT-src.patch): the package's own Rcpp wrapper is still there and takes every call this
 * entry does not cover -- the other callers of rcpp_make_eMatRead_t (K = KL rows: functions.R:2903, reference-single.R:545,
 * gibbs-nipt.R:126/1634, the test drivers), pseudo-haploid mode, and calls made before any panel was uploaded. */
extern SEXP _QUILT_rcpp_make_eMatRead_t(SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP, SEXP);
#define QA_EMATREAD_NOT_COVERED(msg)                                                                                          \
    return _QUILT_rcpp_make_eMatRead_t(eMatRead_tSEXP, sampleReadsSEXP, eHapsCurrent_tcSEXP, sSEXP, maxDifferenceBetweenReadsSEXP, \
                                       JmaxSEXP, eMatHapOri_tSEXP, pRgivenH1SEXP, pRgivenH2SEXP, prevSEXP, suppressOutputSEXP,  \
                                       prev_sectionSEXP, next_sectionSEXP, run_pseudo_haploidSEXP, rescale_eMatRead_tSEXP)
#else
#define QA_EMATREAD_NOT_COVERED(msg) Rf_error("quilt_amd: rcpp_make_eMatRead_t: " msg)
#endif
#define QA_EMATREAD_MAX_K 3   /* the device form serves the driver loop's caller (K = 2 or 3 sampled haplotypes) */

SEXP qa_QUILT_rcpp_make_eMatRead_t(SEXP eMatRead_tSEXP, SEXP sampleReadsSEXP, SEXP eHapsCurrent_tcSEXP, SEXP sSEXP,
                                   SEXP maxDifferenceBetweenReadsSEXP, SEXP JmaxSEXP, SEXP eMatHapOri_tSEXP, SEXP pRgivenH1SEXP,
                                   SEXP pRgivenH2SEXP, SEXP prevSEXP, SEXP suppressOutputSEXP, SEXP prev_sectionSEXP,
                                   SEXP next_sectionSEXP, SEXP run_pseudo_haploidSEXP, SEXP rescale_eMatRead_tSEXP) {
    (void)eMatHapOri_tSEXP; (void)pRgivenH1SEXP; (void)pRgivenH2SEXP; (void)prevSEXP; (void)suppressOutputSEXP;
    (void)prev_sectionSEXP; (void)next_sectionSEXP;
    if (Rf_asLogical(run_pseudo_haploidSEXP)) QA_EMATREAD_NOT_COVERED("run_pseudo_haploid = TRUE is not supported");
    if (!g_cache.panel) QA_EMATREAD_NOT_COVERED("needs the panel of an earlier full-panel or Gibbs call");
    const int K = Rf_nrows(eMatRead_tSEXP), R = Rf_length(sampleReadsSEXP), s = Rf_asInteger(sSEXP);
    if (K > QA_EMATREAD_MAX_K) QA_EMATREAD_NOT_COVERED("more than 3 haplotype rows");
    SEXP dim = Rf_getAttrib(eHapsCurrent_tcSEXP, R_DimSymbol);
    if (Rf_length(dim) != 3 || INTEGER(dim)[0] != K || s < 0 || s >= INTEGER(dim)[2] || Rf_ncols(eMatRead_tSEXP) != R)
        Rf_error("quilt_amd: rcpp_make_eMatRead_t: eHapsCurrent_tc must be K x nSNPs x S with K = nrow(eMatRead_t), 0 <= s < S");
    const int T = INTEGER(dim)[1];
    flat_reads_t fr;
    if (pack_reads(sampleReadsSEXP, 0, 0, &fr) != 0) Rf_error("quilt_amd: rcpp_make_eMatRead_t: out of memory");
    const int st = qa_rcpp_make_eMatRead_t_nsnps(g_cache.panel, T, 1, K, REAL(eHapsCurrent_tcSEXP) + (size_t)s * K * T, fr.read_off,
                                                 fr.read_ptr, fr.u, fr.bq, Rf_asReal(maxDifferenceBetweenReadsSEXP), Rf_asInteger(JmaxSEXP),
                                                 Rf_asLogical(rescale_eMatRead_tSEXP), REAL(eMatRead_tSEXP));
    flat_reads_free(&fr);
    check_status(st, "qa_rcpp_make_eMatRead_t");
    return R_NilValue;
}


/* ---- qa_impute_sample_range: the body of QUILT()'s loop over a core's samples as ONE `.Call` -----------------------------
 * QUILT/R/quilt.R:688-996 runs `for(iSample in sampleRange[1]:sampleRange[2]) get_and_impute_one_sample(...)` inside
 * mclapply; with the GPU library the whole range goes to qa_impute_samples (include/quilt_amd.h; csrc/impute.cpp: the loop of
 * functions.R:3-1500 in host C++ over the batched kernels), n_handles host threads sharing the device.  R-side (INTEGRATION.md
 * 4a has the replacement of the mclapply body):
 *     out <- .Call("qa_impute_sample_range", list_of_sampleReads, panel_objects, params, sample_offset, n_handles,
 *                  list_of_allSNP_sampleReads)
 *   list_of_sampleReads   one sampleReads (list of list(J, wif, bq, u), copied-from-stitch.cpp:153-160) per sample of the range
 *   panel_objects         named list: hapMatcherR, distinctHapsB, distinctHapsIE, eMatDH_special_matrix_helper,
 *                         eMatDH_special_matrix, rhb_t, transMatRate_t (2 x (nGrids - 1)), ref_error, use_eMatDH_special_symbols;
 *                         method = "nipt": L_grid (nGrids);
 *                         impute_rare_common = TRUE: rare_common = list(snp_is_common, rare_per_hap_info, transMatRate_t
 *                         (2 x (nGrids_all - 1)), L_grid) of special_rare_common_objects (prepare_reference_functions.R:172-247)
 *   params                named list of QUILT()'s arguments the path sees (missing entries = the reference's defaults):
 *                         nGibbsSamples, n_seek_its, n_burn_in_seek_its, Ksubset, Knew, K_top_matches, heuristic_match_thin,
 *                         small_ref_panel_gibbs_iterations, small_ref_panel_block_gibbs_iterations (0-based), maxDifferenceBetweenReads,
 *                         minGLValue, Jmax, seed (a non-negative whole number below 2^53), samples_per_launch_set, device (0-based GPU of
 *                         this worker, taken modulo the number of devices: mclapply's iCore - 1; absent: the current device);
 *                         use_mspbwt, mspbwtL, mspbwtM, mspbwt_nindices;
 *                         impute_rare_common; method ("diploid" / "nipt"), ff (one fetal fraction per sample), shuffle_bin_radius;
 *                         hla_grid (hla_run = TRUE: iGrid - 1, 0-based; qa_impute_samples_hla)
 *   sample_offset         0-based index of the range's first sample among ALL samples (keys the random streams: a sample's
 *                         result does not depend on the range it lands in)
 *   list_of_allSNP_sampleReads   impute_rare_common = TRUE: allSNP_sampleReads per sample (functions.R:162-172: u over all SNPs,
 *                         wif on the all-SNP grid); NULL otherwise
 * Returns list(dosage = nSNPs x n, gp_t = 3 nSNPs x n (per sample 3 x nSNPs, row-major as the library writes it),
 * phasing_haps = 2 nSNPs x n (nipt: 3 nSNPs x n), read_labels = list of integer vectors, nDosage, stats[, fet_dosage, fet_gp_t]);
 * nSNPs = all SNPs with impute_rare_common.  With params$output_read_label_prob = TRUE also read_label_prob (list of numeric
 * vectors: per read the confidence of its label, qa_impute_samples_reads).  With params$hla_grid also gamma1, gamma2, gamma_total (K x n: a sample's column is
 * its vector) and list_of_gammas ((K x 2 x nGibbsSamples) x n: per sample the nGibbsSamples pairs (gamma1, gamma2) of
 * functions.R:1276-1278, each column an R array of dim c(K, 2, nGibbsSamples)).  Draws: the library's counter streams (R's stream cannot be handed to 2 048 chains
 * advancing in lock-step); `seed` plays set.seed's part.  use_mspbwt: the panel's msPBWT indices are built here by
 * qa_mspbwt_create (the `ms_indices` the reference loads are the mspbwt package's own structures). */

/* Every R-level check of a list of sampleReads, BEFORE anything is allocated: an R error longjmps out of the routine, so it must
 * not be raised (by INTEGER() on a REALSXP, say) while panel handles, the msPBWT index or malloc'd buffers are live. */
static void validate_reads_list(SEXP readsListSEXP, const char *what) {
    if (TYPEOF(readsListSEXP) != VECSXP) Rf_error("quilt_amd: qa_impute_sample_range: %s must be a list of sampleReads", what);
    const int n = Rf_length(readsListSEXP);
    for (int i = 0; i < n; i++) {
        SEXP sr = VECTOR_ELT(readsListSEXP, i);
        if (TYPEOF(sr) != VECSXP) Rf_error("quilt_amd: qa_impute_sample_range: %s[[%d]] is not a list of reads", what, i + 1);
        const int R = Rf_length(sr);
        for (int r = 0; r < R; r++) {
            SEXP rd = VECTOR_ELT(sr, r);
            if (TYPEOF(rd) != VECSXP || Rf_length(rd) < 4)
                Rf_error("quilt_amd: qa_impute_sample_range: %s[[%d]][[%d]] is not list(J, wif, bq, u)", what, i + 1, r + 1);
            SEXP bq = VECTOR_ELT(rd, 2), u = VECTOR_ELT(rd, 3), wif = VECTOR_ELT(rd, 1);
            if (TYPEOF(bq) != INTSXP || TYPEOF(u) != INTSXP || Rf_length(bq) != Rf_length(u))
                Rf_error("quilt_amd: qa_impute_sample_range: %s[[%d]][[%d]]: bq and u must be integer vectors of one length "
                         "(sampleReads as loadBamAndConvert writes them)", what, i + 1, r + 1);
            if ((TYPEOF(wif) != INTSXP && TYPEOF(wif) != REALSXP) || Rf_length(wif) < 1)
                Rf_error("quilt_amd: qa_impute_sample_range: %s[[%d]][[%d]]: the central grid (element 2) must be a number", what, i + 1, r + 1);
        }
    }
}

/* What the two range routines share: the panel handles (one per host thread), the parameter struct with its msPBWT index,
 * all-SNP handles and NIPT block, from the R objects `panel_objects` and `params`. */
typedef struct {
    int K, G, T, T_out, n_handles, nipt, rare;
    qa_panel_t *handles[16];
    int made;
    qa_impute_params_t ip;
    qa_mspbwt_t *index;
    qa_impute_rare_common_t rcq;
    qa_rare_common_t *rcs[16];
    int n_rc;
    rare_inputs_t rin;
    int32_t *L_grid_all, *L_grid;
    qa_impute_nipt_t nq;
    qa_impute_shard_blocks_t sb;
    char msg[512];
} range_ctx_t;

/* Every check that can raise an R error comes first: nothing is allocated yet, nothing can leak (an R error longjmps). */
static void range_validate(SEXP panelSEXP, SEXP paramsSEXP, const char *who) {
    SEXP hapMatcherR = list_get(panelSEXP, "hapMatcherR"), distinctHapsB = list_get(panelSEXP, "distinctHapsB");
    SEXP distinctHapsIE = list_get(panelSEXP, "distinctHapsIE"), tm = list_get(panelSEXP, "transMatRate_t");
    SEXP helper = list_get(panelSEXP, "eMatDH_special_matrix_helper"), spmat = list_get(panelSEXP, "eMatDH_special_matrix");
    SEXP rhb_t = list_get(panelSEXP, "rhb_t");
    if (hapMatcherR == R_NilValue || distinctHapsB == R_NilValue || distinctHapsIE == R_NilValue || tm == R_NilValue ||
        helper == R_NilValue || spmat == R_NilValue)
        Rf_error("quilt_amd: %s: panel_objects needs hapMatcherR, distinctHapsB, distinctHapsIE, "
                 "eMatDH_special_matrix_helper, eMatDH_special_matrix, transMatRate_t", who);
    if (TYPEOF(hapMatcherR) != RAWSXP || TYPEOF(distinctHapsB) != INTSXP || TYPEOF(distinctHapsIE) != REALSXP || TYPEOF(tm) != REALSXP ||
        TYPEOF(helper) != INTSXP || TYPEOF(spmat) != INTSXP || (rhb_t != R_NilValue && TYPEOF(rhb_t) != INTSXP))
        Rf_error("quilt_amd: %s: panel_objects: hapMatcherR must be raw, distinctHapsB / eMatDH_special_matrix(_helper) / "
                 "rhb_t integer, distinctHapsIE / transMatRate_t numeric", who);
    const int G = Rf_ncols(hapMatcherR);
    if (Rf_length(tm) != 2 * (G > 1 ? G - 1 : 0))
        Rf_error("quilt_amd: %s: panel_objects$transMatRate_t must be 2 x (nGrids - 1)", who);
    SEXP rc0 = list_get(panelSEXP, "rare_common");
    SEXP rph0 = rc0 == R_NilValue ? R_NilValue : list_get(rc0, "rare_per_hap_info");
    if (rph0 != R_NilValue) {
        if (TYPEOF(rph0) != VECSXP) Rf_error("quilt_amd: %s: rare_common$rare_per_hap_info must be a list", who);
        for (int k = 0; k < Rf_length(rph0); k++)
            if (TYPEOF(VECTOR_ELT(rph0, k)) != INTSXP && Rf_length(VECTOR_ELT(rph0, k)) > 0)
                Rf_error("quilt_amd: %s: rare_common$rare_per_hap_info[[%d]] must be an integer vector", who, k + 1);
        SEXP sic0 = list_get(rc0, "snp_is_common"), tma0 = list_get(rc0, "transMatRate_t");
        if ((sic0 != R_NilValue && TYPEOF(sic0) != LGLSXP) || (tma0 != R_NilValue && TYPEOF(tma0) != REALSXP))
            Rf_error("quilt_amd: %s: rare_common$snp_is_common must be logical, $transMatRate_t numeric", who);
    }
    {   /* grid positions (method = "nipt": the block definition): numbers, wherever they are given */
        SEXP lg = list_get(panelSEXP, "L_grid"), lga = rc0 == R_NilValue ? R_NilValue : list_get(rc0, "L_grid");
        if ((lg != R_NilValue && TYPEOF(lg) != INTSXP && TYPEOF(lg) != REALSXP) || (lga != R_NilValue && TYPEOF(lga) != INTSXP && TYPEOF(lga) != REALSXP))
            Rf_error("quilt_amd: %s: L_grid must be numeric", who);
        SEXP ff = list_get(paramsSEXP, "ff");
        if (ff != R_NilValue && TYPEOF(ff) != REALSXP) Rf_error("quilt_amd: %s: params$ff must be numeric (as.numeric)", who);
    }
    {   /* the small panel the samplers are built for (include/quilt_amd.h: QA_KSUBSET_MAX*), after quilt.R:453-463's reset to the
         * panel's size: refused here, before the panel is uploaded, not by the first sample's first Gibbs call */
        const int K = Rf_nrows(hapMatcherR);
        const double ks_asked = num_or(paramsSEXP, "Ksubset", 600), ks = K < ks_asked ? K : ks_asked;
        const int nipt = is_nipt(paramsSEXP);
        const int ks_max = nipt ? QA_KSUBSET_MAX_NIPT : QA_KSUBSET_MAX;
        if (ks > ks_max)
            Rf_error("quilt_amd: %s: Ksubset = %d (the smaller of params$Ksubset and the panel's %d haplotypes) is not built for "
                     "method = \"%s\", which runs every Ksubset in 1..%d (method = \"diploid\": 1..%d, method = \"nipt\": 1..%d)",
                     who, (int)ks, K, nipt ? "nipt" : "diploid", ks_max, QA_KSUBSET_MAX, QA_KSUBSET_MAX_NIPT);
    }
    const double seed_d = num_or(paramsSEXP, "seed", 1);
    if (!(seed_d >= 0) || seed_d > 9007199254740992.0 /* 2^53 */ || seed_d != floor(seed_d))   /* (NA / NaN fail the first test) */
        Rf_error("quilt_amd: %s: params$seed must be a non-negative whole number below 2^53", who);
    const double so = num_or(paramsSEXP, "sum_order", 0);
    if (!(so == 0 || so == 1 || so == 2)) Rf_error("quilt_amd: %s: params$sum_order must be 0, 1 or 2 (include/quilt_amd.h: qa_panel_set_sum_order)", who);
    const double sob = num_or(paramsSEXP, "sum_order_batched", 0);
    if (!(sob == 0 || sob == 1)) Rf_error("quilt_amd: %s: params$sum_order_batched must be 0 or 1 (include/quilt_amd.h: qa_panel_set_sum_order_batched)", who);
    SEXP blocks = list_get(paramsSEXP, "small_ref_panel_block_gibbs_iterations");
    if (blocks != R_NilValue && TYPEOF(blocks) != INTSXP)
        Rf_error("quilt_amd: %s: params$small_ref_panel_block_gibbs_iterations must be an integer vector (0-based sweeps)", who);
    /* which GPU: params$device (0-based; taken modulo the number of devices, so that mclapply's iCore - 1 can be passed as it
     * is); absent: the process's current device.  Forked workers must make their first HIP call after the fork -- this one. */
    const double dev_d = num_or(paramsSEXP, "device", -1);
    if (dev_d >= 0) {
        const int n_dev = qa_device_count();
        if (n_dev < 1) Rf_error("quilt_amd: %s: no gfx950 device (libquilt_amd has no CPU fallback)", who);
        check_status(qa_set_device((int)dev_d % n_dev), "qa_set_device");
    }
}

static void range_teardown(range_ctx_t *cx) {
    for (int i = 0; i < cx->n_rc; i++) if (cx->rcs[i]) qa_rare_common_destroy(cx->rcs[i]);
    if (cx->index) qa_mspbwt_destroy(cx->index);
    rare_inputs_free(&cx->rin);
    free(cx->L_grid); free(cx->L_grid_all);
    for (int i = 0; i < cx->made; i++) if (cx->handles[i]) qa_panel_destroy(cx->handles[i]);
    cx->n_rc = 0; cx->made = 0; cx->index = NULL;
    cx->L_grid = NULL; cx->L_grid_all = NULL;
}

/* The stages of range_setup, in its order.  None raises an R error: each returns a QA status with the text in cx->msg, and
 * range_teardown undoes whatever the stages before a failure made. */

/* 1. panel handles: one per host thread, replicas of the panel on this process's device, taking the device in turn */
static int setup_panel_handles(range_ctx_t *cx, SEXP panelSEXP, SEXP paramsSEXP, int n_handles) {
    SEXP hapMatcherR = list_get(panelSEXP, "hapMatcherR"), distinctHapsB = list_get(panelSEXP, "distinctHapsB");
    SEXP distinctHapsIE = list_get(panelSEXP, "distinctHapsIE"), tm = list_get(panelSEXP, "transMatRate_t");
    SEXP helper = list_get(panelSEXP, "eMatDH_special_matrix_helper"), spmat = list_get(panelSEXP, "eMatDH_special_matrix");
    SEXP rhb_t = list_get(panelSEXP, "rhb_t");
    const int K = cx->K = Rf_nrows(hapMatcherR), G = cx->G = Rf_ncols(hapMatcherR), T = cx->T = Rf_ncols(distinctHapsIE);
    cx->T_out = T;
    if (n_handles < 1) n_handles = 1;
    if (n_handles > 16) n_handles = 16;
    cx->n_handles = n_handles;
    qa_panel_desc_t d;
    memset(&d, 0, sizeof d);
    d.K = K; d.nGrids = G; d.nSNPs = T; d.nMaxDH = Rf_nrows(distinctHapsB);
    d.hapMatcherR = RAW(hapMatcherR);
    const int have_rhb = rhb_t != R_NilValue && Rf_nrows(rhb_t) == K && Rf_ncols(rhb_t) == G;
    d.rhb_t = have_rhb ? INTEGER(rhb_t) : NULL;
    d.distinctHapsB = INTEGER(distinctHapsB);
    d.distinctHapsIE = REAL(distinctHapsIE);
    int *which = (int *)calloc((size_t)(G > 0 ? G : 1), sizeof(int));
    if (!which) { snprintf(cx->msg, sizeof cx->msg, "out of memory"); return QA_ERR_INVALID; }
    int nsp = 0;
    for (int g = 0; g < G; g++)
        if (Rf_nrows(helper) == G && INTEGER(helper)[g] > 0) which[g] = ++nsp;
    d.eMatDH_special_grid_which = which;
    d.eMatDH_special_matrix_helper = Rf_nrows(helper) == G ? INTEGER(helper) : NULL;
    d.eMatDH_special_matrix = INTEGER(spmat);
    d.eMatDH_special_matrix_nrow = Rf_nrows(spmat);
    d.use_eMatDH_special_symbols = !have_rhb || (int)num_or(panelSEXP, "use_eMatDH_special_symbols", 0);
    d.transMatRate_t = REAL(tm);
    d.ref_error = num_or(panelSEXP, "ref_error", 1e-3);
    /* params$sum_order (quilt-amd.R takes it from QUILT_AMD_SUM_ORDER): 0 = production kernels; 1 = VALIDATION MODE, every K-wide
     * sum of the full-panel passes in the order the reference's code adds it (bit-identical to the CPU package's lists, 20-50x
     * slower passes); 2 = the same with grid 0's Armadillo sum read left to right (include/quilt_amd.h) */
    const int sum_order = (int)num_or(paramsSEXP, "sum_order", 0);
    /* params$sum_order_batched (QUILT_AMD_SUM_ORDER_BATCHED) beside a sum_order of 1 or 2: the same sums, hence the same bits, from
     * the kernels laid out for many passes at once (qa_panel_set_sum_order_batched) */
    const int sum_order_batched = sum_order ? (int)num_or(paramsSEXP, "sum_order_batched", 0) : 0;
    /* params$gibbs_state_bits (quilt-amd.R takes it from QUILT_AMD_GIBBS_STATE_BITS): 0 / 64 = fp64 Gibbs state; 32 = alphaHat_t and
     * betaHat_t stored as fp32 (qa_panel_set_gibbs_state_bits: method = "diploid" only -- the library refuses a "nipt" range on such
     * handles before its first sample, and any other value here).  Both range entries; the per-call entries' handle stays at fp64
     * (set.seed parity). */
    const int gibbs_state_bits = (int)num_or(paramsSEXP, "gibbs_state_bits", 0);
    int st = QA_OK;
    for (; cx->made < n_handles && st == QA_OK; cx->made++) {
        cx->handles[cx->made] = NULL;
        st = qa_panel_create(&d, &cx->handles[cx->made]);
        if (st == QA_OK) st = qa_panel_set_device_share(cx->handles[cx->made], n_handles);
        if (st == QA_OK && n_handles > 1) st = qa_panel_set_exclusive(cx->handles[cx->made], 1);
        if (st == QA_OK) st = qa_panel_set_dosage_precision(cx->handles[cx->made], 64);   /* the reference computes in double */
        if (st == QA_OK && sum_order) st = qa_panel_set_sum_order(cx->handles[cx->made], sum_order);
        if (st == QA_OK && sum_order_batched) st = qa_panel_set_sum_order_batched(cx->handles[cx->made], 1);
        if (st == QA_OK && gibbs_state_bits) st = qa_panel_set_gibbs_state_bits(cx->handles[cx->made], gibbs_state_bits);
    }
    free(which);
    if (st != QA_OK) snprintf(cx->msg, sizeof cx->msg, "qa_panel_create: %s", qa_last_error());
    return st;
}

/* 2. plain parameters: params' numbers over the library's defaults */
static void setup_plain_params(range_ctx_t *cx, SEXP paramsSEXP) {
    qa_impute_params_t *ip = &cx->ip;
    qa_impute_params_default(ip);
    ip->nGibbsSamples = (int)num_or(paramsSEXP, "nGibbsSamples", ip->nGibbsSamples);
    ip->n_seek_its = (int)num_or(paramsSEXP, "n_seek_its", ip->n_seek_its);
    ip->n_burn_in_seek_its = (int)num_or(paramsSEXP, "n_burn_in_seek_its", -1);   /* NA -> n_seek_its - 1 (quilt.R:248-250) */
    ip->Ksubset = (int)num_or(paramsSEXP, "Ksubset", ip->Ksubset);
    ip->Knew = (int)num_or(paramsSEXP, "Knew", ip->Knew);
    ip->K_top_matches = (int)num_or(paramsSEXP, "K_top_matches", ip->K_top_matches);
    ip->heuristic_match_thin = num_or(paramsSEXP, "heuristic_match_thin", ip->heuristic_match_thin);
    ip->small_ref_panel_gibbs_iterations = (int)num_or(paramsSEXP, "small_ref_panel_gibbs_iterations", ip->small_ref_panel_gibbs_iterations);
    SEXP blocks = list_get(paramsSEXP, "small_ref_panel_block_gibbs_iterations");
    if (blocks != R_NilValue && TYPEOF(blocks) == INTSXP) {
        ip->small_ref_panel_block_gibbs_iterations = INTEGER(blocks);
        ip->n_block_gibbs_iterations = Rf_length(blocks);
    }
    ip->maxDifferenceBetweenReads = num_or(paramsSEXP, "maxDifferenceBetweenReads", ip->maxDifferenceBetweenReads);
    ip->minGLValue = num_or(paramsSEXP, "minGLValue", ip->minGLValue);
    ip->Jmax = (int)num_or(paramsSEXP, "Jmax", ip->Jmax);
    ip->seed = (uint64_t)num_or(paramsSEXP, "seed", 1);   /* (range-checked by range_validate) */
    ip->samples_per_launch_set = (int)num_or(paramsSEXP, "samples_per_launch_set", 0);
}

/* 3. msPBWT index: use_mspbwt = TRUE (QUILT2's default; mspbwt.R:225-474): the panel's indices, built here */
static int setup_mspbwt(range_ctx_t *cx, SEXP panelSEXP, SEXP paramsSEXP) {
    if (!flag(paramsSEXP, "use_mspbwt", 0)) return QA_OK;
    SEXP hapMatcherR = list_get(panelSEXP, "hapMatcherR"), distinctHapsB = list_get(panelSEXP, "distinctHapsB");
    qa_impute_params_t *ip = &cx->ip;
    ip->use_mspbwt = 1;
    ip->mspbwtL = (int)num_or(paramsSEXP, "mspbwtL", ip->mspbwtL);
    ip->mspbwtM = (int)num_or(paramsSEXP, "mspbwtM", ip->mspbwtM);
    cx->index = qa_mspbwt_create(cx->K, cx->G, RAW(hapMatcherR), Rf_nrows(distinctHapsB), INTEGER(distinctHapsB),
                                 (int)num_or(paramsSEXP, "mspbwt_nindices", 4));
    ip->mspbwt_index = cx->index;
    if (cx->index) return QA_OK;
    snprintf(cx->msg, sizeof cx->msg, "qa_mspbwt_create: %s", qa_last_error());
    return QA_ERR_INVALID;
}

/* 4. rare-and-common handles: impute_rare_common = TRUE (functions.R:1042-1123): one all-SNP handle per panel handle (the all-SNP
 * reads are the caller's) */
static int setup_rare_common(range_ctx_t *cx, SEXP panelSEXP, SEXP paramsSEXP) {
    cx->rare = flag(paramsSEXP, "impute_rare_common", 0);
    if (!cx->rare) return QA_OK;
    SEXP rc = list_get(panelSEXP, "rare_common");
    SEXP sic = rc == R_NilValue ? R_NilValue : list_get(rc, "snp_is_common"), rph = rc == R_NilValue ? R_NilValue : list_get(rc, "rare_per_hap_info");
    SEXP tma = rc == R_NilValue ? R_NilValue : list_get(rc, "transMatRate_t"), lga = rc == R_NilValue ? R_NilValue : list_get(rc, "L_grid");
    if (sic == R_NilValue || rph == R_NilValue || tma == R_NilValue || Rf_length(rph) != cx->K) {
        snprintf(cx->msg, sizeof cx->msg, "impute_rare_common: panel_objects$rare_common needs snp_is_common, rare_per_hap_info (one entry per "
                                          "haplotype), transMatRate_t");
        return QA_ERR_INVALID;
    }
    const int T_out = cx->T_out = Rf_length(sic);
    if (rare_inputs_pack(rph, sic, cx->K, &cx->rin) != 0) {
        snprintf(cx->msg, sizeof cx->msg, "out of memory preparing the rare + common inputs");
        return QA_ERR_INVALID;
    }
    int st = QA_OK;
    for (; cx->n_rc < cx->n_handles && st == QA_OK; cx->n_rc++) {
        cx->rcs[cx->n_rc] = NULL;
        st = qa_rare_common_create(cx->handles[cx->n_rc], T_out, cx->rin.is_common, cx->rin.rare_ptr, cx->rin.rare_snp, REAL(tma), &cx->rcs[cx->n_rc]);
    }
    if (st != QA_OK) {
        snprintf(cx->msg, sizeof cx->msg, "qa_rare_common_create: %s", qa_last_error());
        return st;
    }
    cx->rcq.handles = (const qa_rare_common_t *const *)cx->rcs;
    cx->rcq.nSNPs_all = T_out;
    cx->rcq.nGrids_all = (T_out + 31) / 32;
    cx->rcq.snp_is_common = cx->rin.is_common;
    cx->rcq.L_grid_all = cx->L_grid_all = ints_of(lga, cx->rcq.nGrids_all);   /* (optional: NULL when absent or of another length) */
    cx->ip.rare_common = &cx->rcq;
    return QA_OK;
}

/* the grid positions a block definition needs: panel_objects$L_grid (nGrids) into cx->L_grid; `missing` is the text when absent */
static int setup_L_grid(range_ctx_t *cx, SEXP panelSEXP, int have_the_rest, const char *missing) {
    SEXP lg = list_get(panelSEXP, "L_grid");
    if (!have_the_rest || lg == R_NilValue || Rf_length(lg) != cx->G) {
        snprintf(cx->msg, sizeof cx->msg, "%s", missing);
        return QA_ERR_INVALID;
    }
    cx->L_grid = ints_of(lg, cx->G);
    if (cx->L_grid) return QA_OK;
    snprintf(cx->msg, sizeof cx->msg, "out of memory");
    return QA_ERR_INVALID;
}

/* 5. NIPT block: method = "nipt" (functions.R:586, :1009-1016, :1218-1231): one fetal fraction per sample (`n_sample` of them;
 * the fetus' outputs are the caller's to set), the block definition's grid */
static int setup_nipt(range_ctx_t *cx, SEXP panelSEXP, SEXP paramsSEXP, int n_sample) {
    cx->nipt = is_nipt(paramsSEXP);
    if (!cx->nipt) return QA_OK;
    SEXP ff = list_get(paramsSEXP, "ff");
    const int st = setup_L_grid(cx, panelSEXP, ff != R_NilValue && TYPEOF(ff) == REALSXP && Rf_length(ff) == n_sample,
                                "method = \"nipt\": params$ff (one per sample, numeric) and panel_objects$L_grid (nGrids) are needed");
    if (st != QA_OK) return st;
    cx->nq.ff = REAL(ff);
    cx->nq.L_grid = cx->L_grid;
    cx->nq.shuffle_bin_radius = (int)num_or(paramsSEXP, "shuffle_bin_radius", 5000);
    cx->ip.nipt = &cx->nq;
    return QA_OK;
}

/* 6. block-wise shard passes: shard_check_every_pair = FALSE (quilt.R:178; absent: TRUE), method = "diploid": the shard passes go
 * block by block and the block definition needs the grid positions (qa_impute_params_t.shard_blocks) */
static int setup_shard_blocks(range_ctx_t *cx, SEXP panelSEXP, SEXP paramsSEXP) {
    if (cx->nipt || flag(paramsSEXP, "shard_check_every_pair", 1)) return QA_OK;
    const int st = setup_L_grid(cx, panelSEXP, 1, "shard_check_every_pair = FALSE: panel_objects$L_grid (nGrids) is needed");
    if (st != QA_OK) return st;
    cx->sb.L_grid = cx->L_grid;
    cx->sb.shuffle_bin_radius = (int)num_or(paramsSEXP, "shuffle_bin_radius", 5000);
    cx->sb.block_gibbs_quantile_prob = num_or(paramsSEXP, "block_gibbs_quantile_prob", 0.95);
    cx->ip.shard_blocks = &cx->sb;
    return QA_OK;
}

/* Raises no R error: returns a QA status with the text in cx->msg; on failure everything made so far is torn down again. */
static int range_setup(range_ctx_t *cx, SEXP panelSEXP, SEXP paramsSEXP, int n_handles, int n_sample) {
    memset(cx, 0, sizeof *cx);
    int st = setup_panel_handles(cx, panelSEXP, paramsSEXP, n_handles);
    if (st == QA_OK) setup_plain_params(cx, paramsSEXP);
    if (st == QA_OK) st = setup_mspbwt(cx, panelSEXP, paramsSEXP);
    if (st == QA_OK) st = setup_rare_common(cx, panelSEXP, paramsSEXP);
    if (st == QA_OK) st = setup_nipt(cx, panelSEXP, paramsSEXP, n_sample);
    if (st == QA_OK) st = setup_shard_blocks(cx, panelSEXP, paramsSEXP);
    if (st != QA_OK) range_teardown(cx);
    return st;
}

/* sample_offset: ONE number (sample i of the call is global sample offset + i) or one 0-based global index PER SAMPLE -- the
 * form quilt-amd.R uses, so that a sample skipped for too few reads does not shift the streams of the samples behind it */
static int64_t *sample_index_of(SEXP sample_offsetSEXP, int n) {
    if (Rf_length(sample_offsetSEXP) != n || n <= 1) return NULL;   /* (n == 1: offset and index are the same thing) */
    return int64s_of(sample_offsetSEXP, n);
}

/* what the caller asked for beyond the plain outputs; filled by the validation stage */
typedef struct { int hla_grid, want_prob; } range_opts_t;

/* stage 1: every R-level check of the six arguments, before anything is made */
static void sample_range_validate(SEXP readsListSEXP, SEXP panelSEXP, SEXP paramsSEXP, SEXP sample_offsetSEXP, SEXP allReadsListSEXP,
                                  const char *who, range_opts_t *opt) {
    const int n = Rf_length(readsListSEXP);
    validate_reads_list(readsListSEXP, "list_of_sampleReads");
    if (allReadsListSEXP != R_NilValue) validate_reads_list(allReadsListSEXP, "list_of_allSNP_sampleReads");
    range_validate(panelSEXP, paramsSEXP, who);
    if ((TYPEOF(sample_offsetSEXP) != REALSXP && TYPEOF(sample_offsetSEXP) != INTSXP) ||
        (Rf_length(sample_offsetSEXP) != 1 && Rf_length(sample_offsetSEXP) != n))
        Rf_error("quilt_amd: %s: sample_offset must be one number or one global index per sample", who);
    if (flag(paramsSEXP, "impute_rare_common", 0) && (allReadsListSEXP == R_NilValue || Rf_length(allReadsListSEXP) != n))
        Rf_error("quilt_amd: %s: impute_rare_common needs one allSNP_sampleReads per sample", who);
    opt->hla_grid = hla_grid_of(paramsSEXP, who, Rf_ncols(list_get(panelSEXP, "hapMatcherR")));
    /* output_read_label_prob (functions.R:1164-1166): params$output_read_label_prob -> read_label_prob, one vector per sample */
    opt->want_prob = flag(paramsSEXP, "output_read_label_prob", 0);
}

/* The range's outputs: the R objects the library writes into (each PROTECTed, `n_prot` of them) and the malloc'd per-read arrays */
typedef struct {
    SEXP dosage, gp_t, haps, nDosage, stats, fet_dosage, fet_gp_t, g1, g2, gtot, glist, lab, probs;
    int n_prot;
    int32_t *labels;
    double *prob;
    int64_t *sidx, st64[11];
    qa_impute_hla_t hq;
} range_out_t;
static SEXP keep(range_out_t *o, SEXP x) { o->n_prot++; return PROTECT(x); }

/* stage 4: allocate results (R's before the library runs; cx->nq gets the fetus' outputs).  QA_OK, or the status with `msg` set. */
static int range_out_alloc(range_out_t *o, range_ctx_t *cx, const range_opts_t *opt, SEXP sample_offsetSEXP, int n, int totR, char *msg,
                           size_t n_msg) {
    const int T_out = cx->T_out, nL = cx->nipt ? 3 : 2;
    memset(o, 0, sizeof *o);
    o->fet_dosage = o->fet_gp_t = o->g1 = o->g2 = o->gtot = o->glist = R_NilValue;
    if (cx->nipt) {
        o->fet_dosage = keep(o, Rf_allocMatrix(REALSXP, T_out, n));
        o->fet_gp_t = keep(o, Rf_allocMatrix(REALSXP, 3 * T_out, n));
        cx->nq.fet_dosage = REAL(o->fet_dosage);
        cx->nq.fet_gp_t = REAL(o->fet_gp_t);
    }
    o->dosage = keep(o, Rf_allocMatrix(REALSXP, T_out, n));
    o->gp_t = keep(o, Rf_allocMatrix(REALSXP, 3 * T_out, n));
    o->haps = keep(o, Rf_allocMatrix(REALSXP, nL * T_out, n));
    o->nDosage = keep(o, Rf_allocVector(INTSXP, n));
    o->stats = keep(o, Rf_allocVector(REALSXP, 11));
    if (opt->hla_grid >= 0) {
        o->g1 = keep(o, Rf_allocMatrix(REALSXP, cx->K, n)); o->g2 = keep(o, Rf_allocMatrix(REALSXP, cx->K, n));
        o->gtot = keep(o, Rf_allocMatrix(REALSXP, cx->K, n));
        o->glist = keep(o, Rf_allocMatrix(REALSXP, cx->K * 2 * cx->ip.nGibbsSamples, n));
        o->hq.grid = opt->hla_grid;
        o->hq.gamma1 = REAL(o->g1); o->hq.gamma2 = REAL(o->g2); o->hq.gamma_total = REAL(o->gtot); o->hq.list_of_gammas = REAL(o->glist);
    }
    o->labels = (int32_t *)malloc(sizeof(int32_t) * (size_t)(totR > 0 ? totR : 1));
    o->prob = opt->want_prob ? (double *)malloc(sizeof(double) * (size_t)(totR > 0 ? totR : 1)) : NULL;
    o->sidx = sample_index_of(sample_offsetSEXP, n);
    if (o->labels && (!opt->want_prob || o->prob) && !(Rf_length(sample_offsetSEXP) == n && n > 1 && !o->sidx)) return QA_OK;
    snprintf(msg, n_msg, "out of memory");
    return QA_ERR_INVALID;
}

/* stage 5: call the library -- the entry of the options asked for */
static int range_call(range_ctx_t *cx, const range_opts_t *opt, const flat_reads_t *fr, range_out_t *o, SEXP sample_offsetSEXP, int n,
                      char *msg, size_t n_msg) {
    const int hla = opt->hla_grid >= 0;
    int st;
    cx->ip.sample_index = o->sidx;
    const int64_t off = o->sidx ? 0 : (int64_t)Rf_asReal(sample_offsetSEXP);
    if (opt->want_prob) {
        qa_impute_reads_out_t ro;
        memset(&ro, 0, sizeof ro);
        ro.read_label_prob = o->prob;
        st = qa_impute_samples_reads(cx->handles, cx->n_handles, &cx->ip, n, off, fr->read_off, fr->read_ptr, fr->u, fr->bq, fr->wif,
                                     REAL(o->dosage), REAL(o->gp_t), REAL(o->haps), o->labels, INTEGER(o->nDosage), o->st64,
                                     hla ? &o->hq : NULL, &ro);
    } else if (hla)
        st = qa_impute_samples_hla(cx->handles, cx->n_handles, &cx->ip, n, off, fr->read_off, fr->read_ptr, fr->u, fr->bq, fr->wif,
                                   REAL(o->dosage), REAL(o->gp_t), REAL(o->haps), o->labels, INTEGER(o->nDosage), o->st64, &o->hq);
    else
        st = qa_impute_samples(cx->handles, cx->n_handles, &cx->ip, n, off, fr->read_off, fr->read_ptr, fr->u, fr->bq, fr->wif,
                               REAL(o->dosage), REAL(o->gp_t), REAL(o->haps), o->labels, INTEGER(o->nDosage), o->st64);
    if (st != QA_OK) snprintf(msg, n_msg, "%s: %s", hla ? "qa_impute_samples_hla" : "qa_impute_samples", qa_last_error());
    return st;
}

/* stage 6: label lists -- per sample the read labels and, when asked for, their confidences */
static void range_label_lists(range_out_t *o, const int32_t *read_off, int n, int want_prob, int filled) {
    o->lab = keep(o, Rf_allocVector(VECSXP, n));
    o->probs = keep(o, want_prob ? Rf_allocVector(VECSXP, n) : R_NilValue);
    for (int i = 0; filled && i < n; i++) {
        const int R = read_off[i + 1] - read_off[i];
        SET_VECTOR_ELT(o->lab, i, int_vector(o->labels + read_off[i], R));
        if (want_prob) SET_VECTOR_ELT(o->probs, i, real_vector(o->prob + read_off[i], R));
    }
}

/* stage 7: result list */
static SEXP range_result_list(const range_out_t *o, int nipt, int hla, int want_prob) {
    result_t r;
    result_begin(&r);
    result_add(&r, "dosage", o->dosage); result_add(&r, "gp_t", o->gp_t); result_add(&r, "phasing_haps", o->haps);
    result_add(&r, "read_labels", o->lab); result_add(&r, "nDosage", o->nDosage); result_add(&r, "stats", o->stats);
    if (hla) {
        result_add(&r, "gamma1", o->g1); result_add(&r, "gamma2", o->g2);
        result_add(&r, "gamma_total", o->gtot); result_add(&r, "list_of_gammas", o->glist);
    } else if (nipt) {
        result_add(&r, "fet_dosage", o->fet_dosage); result_add(&r, "fet_gp_t", o->fet_gp_t);
    }
    if (want_prob) result_add(&r, "read_label_prob", o->probs);
    return result_end(&r);
}

SEXP qa_impute_sample_range(SEXP readsListSEXP, SEXP panelSEXP, SEXP paramsSEXP, SEXP sample_offsetSEXP, SEXP n_handlesSEXP,
                            SEXP allReadsListSEXP) {
    static const char *who = "qa_impute_sample_range";
    const int n = Rf_length(readsListSEXP);
    /* 1. validate */
    range_opts_t opt;
    sample_range_validate(readsListSEXP, panelSEXP, paramsSEXP, sample_offsetSEXP, allReadsListSEXP, who, &opt);
    /* 2. set up */
    range_ctx_t cx;
    int st = range_setup(&cx, panelSEXP, paramsSEXP, Rf_asInteger(n_handlesSEXP), n);
    if (st != QA_OK) Rf_error("quilt_amd: %s: %s", who, cx.msg);
    /* 3. flatten reads: the range's sampleReads and, with rare + common, its all-SNP ones */
    flat_reads_t fr, fa;
    memset(&fa, 0, sizeof fa);
    if (pack_reads(readsListSEXP, 1, 1, &fr) != 0 || (cx.rare && pack_reads(allReadsListSEXP, 1, 1, &fa) != 0)) {
        flat_reads_free(&fr);
        range_teardown(&cx);
        Rf_error("quilt_amd: %s: out of memory flattening the sampleReads", who);
    }
    if (cx.rare) { cx.rcq.read_off = fa.read_off; cx.rcq.read_ptr = fa.read_ptr; cx.rcq.u = fa.u; cx.rcq.bq = fa.bq; cx.rcq.wif = fa.wif; }
    /* 4. allocate results */
    range_out_t o;
    char msg[512];
    msg[0] = 0;
    st = range_out_alloc(&o, &cx, &opt, sample_offsetSEXP, n, fr.read_off[n], msg, sizeof msg);
    /* 5. call the library */
    if (st == QA_OK) st = range_call(&cx, &opt, &fr, &o, sample_offsetSEXP, n, msg, sizeof msg);
    range_teardown(&cx);
    free(o.sidx); flat_reads_free(&fa);
    /* 6. label lists */
    range_label_lists(&o, fr.read_off, n, opt.want_prob, st == QA_OK);
    flat_reads_free(&fr);
    free(o.labels); free(o.prob);
    if (st != QA_OK) {
        UNPROTECT(o.n_prot);
        Rf_error("quilt_amd: %s: %s", who, msg);
    }
    counters_to_real(o.st64, 11, o.stats);
    /* 7. result list */
    SEXP out = range_result_list(&o, cx.nipt, opt.hla_grid >= 0, opt.want_prob);
    UNPROTECT(o.n_prot);
    return out;
}

/* ---- qa_impute_bam_range: the same loop body from BAM PATHS to VCF COLUMNS, natively ------------------------------------------
 * qa_impute_sample_range above leaves both ends of get_and_impute_one_sample to R: STITCH's loadBamAndConvert + load() +
 * snap_sampleReads_to_grid per sample in front of the call (functions.R:243-298) and the per-sample column / count code behind
 * it (functions.R:1380-1463) -- about a second per sample on the R worker that owns a GPU which imputes ~40 per second.  This
 * routine is the whole body of the loop over a core's samples (quilt.R:832-982) behind one `.Call`:
 *     out <- .Call("qa_impute_bam_range", bam_files, sites, panel_objects, params, sample_index, n_handles)
 *   bam_files       character vector: the range's BAM files (bamlist order)
 *   sites           named list: chr; L (pos[, 2]), ref, alt (pos[, 3:4] as character vectors of single letters), grid (0-based);
 *                   impute_rare_common: L_all / ref_all / alt_all / grid_all (pos_all, special_rare_common_objects$grid);
 *                   loader options bqFilter, iSizeUpperLimit, useSoftClippedBases, downsampleToCov, chrStart, chrEnd (the
 *                   window of functions.R:262-263); minimum_number_of_sample_reads, output_gt_phased_genotypes, n_io_threads;
 *                   optional: use_bx_tag (logical) and bxTagUpperLimit (a whole number >= 0; default 50000, quilt.R:47) -- the
 *                   loader's linked-read rule (include/quilt_amd_io.h: qa_bam_load_sample_reads_bx); absent means off
 *   panel_objects, params, n_handles   as for qa_impute_sample_range (params$ff: one per FILE)
 *   sample_index    0-based global index of every file's sample (iSample - 1)
 * Returns list(sample_was_imputed (logical), n_reads (integer), per_sample_vcf_col (list: character vector per imputed sample,
 * NULL otherwise), read_labels (list), infoCount (nSNPs x 2), afCount, hweCount (nSNPs x 3), alleleCount (nSNPs x 2): the
 * range's sums in sample order as quilt.R:955-961 forms them; seconds (load, impute, format, total), stats, bx_stats (the BX rule's
 * four counters summed over the files: qa_bam_range_bx_stats; zeros without use_bx_tag)).  With sites$output_read_label_prob = TRUE
 * also final_read_labels_prob (per file list(names, prob, labels), NULL when not imputed); with params$hla_grid (iGrid - 1) also
 * gamma1, gamma2, gamma_total (K x n) and list_of_gammas ((K x 2 x nGibbsSamples) x n) as qa_impute_sample_range returns them (NA
 * columns for files not imputed).  Both go through qa_impute_bam_range_ex (include/quilt_amd_io.h).  The loader is
 * csrc/hostio.cpp's (include/quilt_amd_io.h says where it is unpinned against STITCH: CRAM is refused); quilt-amd.R calls this
 * routine only for the options it implements and falls back to the R loader otherwise. */
/* a character vector of single letters -> n bytes; NULL when an entry is not one letter (nothing allocated then) */
static char *letters_of(SEXP v, int n) {
    if (v == R_NilValue || TYPEOF(v) != STRSXP || Rf_length(v) != n) return NULL;
    for (int i = 0; i < n; i++) if (strlen(CHAR(STRING_ELT(v, i))) != 1) return NULL;
    char *out = (char *)malloc((size_t)(n > 0 ? n : 1));
    for (int i = 0; out && i < n; i++) out[i] = CHAR(STRING_ELT(v, i))[0];
    return out;
}
static void range_result_finalizer(SEXP p) {
    qa_bam_range_result_t *r = (qa_bam_range_result_t *)R_ExternalPtrAddr(p);
    if (r) qa_bam_range_destroy(r);
    R_ClearExternalPtr(p);
}

/* the options of one call, all checked before anything is made */
typedef struct { int use_bx_tag, bx_limit, want_prob, hla_grid, rare, T, Ta; const char *chr; } bam_opts_t;

/* stage 1: validate options (and everything else that can raise an R error) */
static void bam_range_validate(SEXP bamFilesSEXP, SEXP sitesSEXP, SEXP panelSEXP, SEXP paramsSEXP, SEXP sample_indexSEXP, const char *who,
                               bam_opts_t *opt) {
    if (TYPEOF(bamFilesSEXP) != STRSXP) Rf_error("quilt_amd: %s: bam_files must be a character vector", who);
    if ((TYPEOF(sample_indexSEXP) != REALSXP && TYPEOF(sample_indexSEXP) != INTSXP) || Rf_length(sample_indexSEXP) != Rf_length(bamFilesSEXP))
        Rf_error("quilt_amd: %s: sample_index must hold one 0-based global index per file", who);
    range_validate(panelSEXP, paramsSEXP, who);
    /* the BX pair */
    opt->use_bx_tag = strict_flag(sitesSEXP, "use_bx_tag", 0, who);
    opt->bx_limit = 50000;
    SEXP bl = list_get(sitesSEXP, "bxTagUpperLimit");
    if (bl != R_NilValue) {
        const double v = ((TYPEOF(bl) == INTSXP || TYPEOF(bl) == REALSXP) && Rf_length(bl) == 1) ? Rf_asReal(bl) : -1.0;
        if (!(v >= 0 && v <= 2147483647.0 && v == (double)(int)v))   /* (NA and NaN fail every comparison) */
            Rf_error("quilt_amd: %s: sites$bxTagUpperLimit must be one whole number >= 0 (below 2^31)", who);
        opt->bx_limit = (int)v;
    }
    /* the two options of qa_bam_range_extras_t beyond the tag: sites$output_read_label_prob, params$hla_grid (0-based, as for
     * qa_impute_sample_range) */
    opt->want_prob = strict_flag(sitesSEXP, "output_read_label_prob", 0, who);
    opt->hla_grid = hla_grid_of(paramsSEXP, who, Rf_ncols(list_get(panelSEXP, "hapMatcherR")));
    opt->chr = one_string(sitesSEXP, "chr");
    SEXP Lx = list_get(sitesSEXP, "L");
    if (!opt->chr || Lx == R_NilValue) Rf_error("quilt_amd: %s: sites needs chr, L, ref, alt, grid", who);
    opt->T = Rf_length(Lx);
    if (opt->T != Rf_ncols(list_get(panelSEXP, "distinctHapsIE"))) Rf_error("quilt_amd: %s: sites$L must have one entry per SNP of the panel", who);
    opt->rare = flag(paramsSEXP, "impute_rare_common", 0);
    opt->Ta = opt->rare ? Rf_length(list_get(sitesSEXP, "L_all")) : 0;
}

/* stage 2: the sites, the paths and the sample indices as plain arrays (malloc; one free for every path) */
typedef struct { int32_t *L, *grid, *La, *grida; char *ref, *alt, *refa, *alta; const char **paths; int64_t *sidx; } site_arrays_t;
static void site_arrays_free(site_arrays_t *a) {
    free(a->L); free(a->grid); free(a->ref); free(a->alt); free(a->La); free(a->grida); free(a->refa); free(a->alta);
    free((void *)a->paths); free(a->sidx);
    memset(a, 0, sizeof *a);
}
/* 1, or 0 when an entry of `sites` is of the wrong kind or length (or memory ran out): the caller frees and reports */
static int site_arrays_make(site_arrays_t *a, SEXP sitesSEXP, SEXP bamFilesSEXP, SEXP sample_indexSEXP, const bam_opts_t *opt) {
    const int n = Rf_length(bamFilesSEXP), T = opt->T, Ta = opt->Ta;
    memset(a, 0, sizeof *a);
    a->L = ints_of(list_get(sitesSEXP, "L"), T); a->grid = ints_of(list_get(sitesSEXP, "grid"), T);
    a->ref = letters_of(list_get(sitesSEXP, "ref"), T); a->alt = letters_of(list_get(sitesSEXP, "alt"), T);
    if (opt->rare) {
        a->La = ints_of(list_get(sitesSEXP, "L_all"), Ta); a->grida = ints_of(list_get(sitesSEXP, "grid_all"), Ta);
        a->refa = letters_of(list_get(sitesSEXP, "ref_all"), Ta); a->alta = letters_of(list_get(sitesSEXP, "alt_all"), Ta);
    }
    a->paths = (const char **)malloc(sizeof(char *) * (size_t)(n > 0 ? n : 1));
    a->sidx = int64s_of(sample_indexSEXP, n);
    for (int i = 0; a->paths && i < n; i++) a->paths[i] = CHAR(STRING_ELT(bamFilesSEXP, i));
    return a->L && a->grid && a->ref && a->alt && a->paths && a->sidx && (!opt->rare || (a->La && a->grida && a->refa && a->alta));
}

/* stage 4: qa_bam_range_io_t from the site arrays and sites' loader options, the extras from the checked options */
static void bam_io_fill(qa_bam_range_io_t *io, qa_bam_range_extras_t *ex, SEXP sitesSEXP, const bam_opts_t *opt, const site_arrays_t *a) {
    memset(io, 0, sizeof *io);
    io->chr = opt->chr; io->nSNPs = opt->T; io->L = a->L; io->ref = a->ref; io->alt = a->alt; io->grid = a->grid;
    io->nSNPs_all = opt->Ta; io->L_all = a->La; io->ref_all = a->refa; io->alt_all = a->alta; io->grid_all = a->grida;
    qa_bam_opts_default(&io->bam);
    io->bam.bqFilter = (int)num_or(sitesSEXP, "bqFilter", io->bam.bqFilter);
    const double isz = num_or(sitesSEXP, "iSizeUpperLimit", io->bam.iSizeUpperLimit);
    io->bam.iSizeUpperLimit = isz > 2147483647.0 ? 2147483647 : (int)isz;
    io->bam.useSoftClippedBases = flag(sitesSEXP, "useSoftClippedBases", 0);
    io->bam.downsampleToCov = (int)num_or(sitesSEXP, "downsampleToCov", io->bam.downsampleToCov);
    io->bam.chrStart = (int)num_or(sitesSEXP, "chrStart", 0);
    io->bam.chrEnd = (int)num_or(sitesSEXP, "chrEnd", 0);
    io->minimum_number_of_sample_reads = (int)num_or(sitesSEXP, "minimum_number_of_sample_reads", 2);
    io->output_gt_phased_genotypes = flag(sitesSEXP, "output_gt_phased_genotypes", 1);
    io->n_io_threads = (int)num_or(sitesSEXP, "n_io_threads", 0);
    io->discard_sample_arrays = 1;   /* (columns, labels and counts go back to R: the per-SNP numbers behind them are not kept) */
    memset(ex, 0, sizeof *ex);
    ex->use_bx_tag = opt->use_bx_tag; ex->bxTagUpperLimit = opt->bx_limit;
    ex->output_read_label_prob = opt->want_prob; ex->hla_grid = opt->hla_grid;
}

/* stage 6, the result as R objects: each part appends its entries to the list and balances its own PROTECTs */

/* sample_was_imputed, n_reads, per_sample_vcf_col, read_labels; returns read_labels (the confidences' lists share its vectors) */
static SEXP bam_columns_and_labels(result_t *r, const qa_bam_range_result_t *res, int n) {
    const int T_out = qa_bam_range_n_snps(res);
    SEXP imputed = result_add(r, "sample_was_imputed", Rf_allocVector(LGLSXP, n));
    SEXP n_reads = result_add(r, "n_reads", Rf_allocVector(INTSXP, n));
    SEXP cols = result_add(r, "per_sample_vcf_col", Rf_allocVector(VECSXP, n));
    SEXP labs = result_add(r, "read_labels", Rf_allocVector(VECSXP, n));
    for (int i = 0; i < n; i++) {
        LOGICAL(imputed)[i] = qa_bam_range_imputed(res, i);
        INTEGER(n_reads)[i] = qa_bam_range_n_reads(res, i);
        const char *buf = NULL;
        const int64_t *off = NULL;
        qa_bam_range_column(res, i, &buf, &off);
        if (!buf) continue;
        SEXP col = PROTECT(Rf_allocVector(STRSXP, T_out));
        for (int t = 0; t < T_out; t++) SET_STRING_ELT(col, t, Rf_mkChar(buf + off[t]));
        SET_VECTOR_ELT(cols, i, col);
        UNPROTECT(1);
        const int32_t *rl = NULL;
        int32_t nl = 0;
        qa_bam_range_sample(res, i, NULL, NULL, NULL, NULL, NULL, &rl, &nl, NULL);
        SET_VECTOR_ELT(labs, i, int_vector(rl, nl));
    }
    return labs;
}
/* infoCount, afCount, hweCount, alleleCount: the range's sums */
static void bam_counts(result_t *r, const qa_bam_range_result_t *res) {
    const int T_out = qa_bam_range_n_snps(res);
    SEXP info = result_add(r, "infoCount", Rf_allocMatrix(REALSXP, T_out, 2)), af = result_add(r, "afCount", Rf_allocVector(REALSXP, T_out));
    SEXP hwe = result_add(r, "hweCount", Rf_allocMatrix(REALSXP, T_out, 3)), ac = result_add(r, "alleleCount", Rf_allocMatrix(REALSXP, T_out, 2));
    qa_bam_range_counts(res, REAL(info), REAL(af), REAL(hwe), REAL(ac));
}
/* seconds, stats, bx_stats */
static void bam_timings_and_stats(result_t *r, const qa_bam_range_result_t *res) {
    SEXP sec = result_add(r, "seconds", Rf_allocVector(REALSXP, 4)), stats = result_add(r, "stats", Rf_allocVector(REALSXP, 11));
    int64_t st64[11] = {0}, bx64[4] = {0};
    qa_bam_range_timings(res, REAL(sec), st64, NULL);
    counters_to_real(st64, 11, stats);
    qa_bam_range_bx_stats(res, bx64);
    counters_to_real(bx64, 4, result_add(r, "bx_stats", Rf_allocVector(REALSXP, 4)));
}
/* final_read_labels_prob: per sample list(names, prob, labels) (functions.R:318-319, :1165, :1203); NULL when not imputed */
static void bam_read_label_prob(result_t *r, const qa_bam_range_result_t *res, int n, SEXP labs) {
    SEXP frlp = result_add(r, "final_read_labels_prob", Rf_allocVector(VECSXP, n));
    for (int i = 0; i < n; i++) {
        const char *nb = NULL;
        const int64_t *no = NULL;
        const double *pr = NULL;
        int32_t nr = 0;
        qa_bam_range_read_label_prob(res, i, &nb, &no, &pr, &nr);
        if (!no) continue;
        SEXP three = SET_VECTOR_ELT(frlp, i, Rf_allocVector(VECSXP, 3));
        SEXP nm = SET_VECTOR_ELT(three, 0, Rf_allocVector(STRSXP, nr));
        for (int q = 0; q < nr; q++) SET_STRING_ELT(nm, q, Rf_mkChar(nb + no[q]));
        SET_VECTOR_ELT(three, 1, real_vector(pr, nr));
        SET_VECTOR_ELT(three, 2, VECTOR_ELT(labs, i));
    }
}
/* gamma1, gamma2, gamma_total, list_of_gammas: the shapes of qa_impute_sample_range (K x n, and (K x 2 x nGibbsSamples) x n); NA
 * for a file not imputed */
static void bam_hla_matrices(result_t *r, const qa_bam_range_result_t *res, int n, int32_t K, int32_t nG) {
    static const char *names[4] = {"gamma1", "gamma2", "gamma_total", "list_of_gammas"};
    const size_t rows[4] = {(size_t)K, (size_t)K, (size_t)K, (size_t)K * 2 * (size_t)nG};
    for (int q = 0; q < 4; q++) {
        SEXP m = result_add(r, names[q], Rf_allocMatrix(REALSXP, (int)rows[q], n));
        for (int i = 0; i < n; i++) {
            const double *g[4] = {NULL, NULL, NULL, NULL};
            int32_t k2 = 0, g2 = 0;
            qa_bam_range_hla(res, i, &g[0], &g[1], &g[2], &g[3], &k2, &g2);
            double *dst = REAL(m) + (size_t)i * rows[q];
            if (g[q] && k2 == K && g2 == nG) memcpy(dst, g[q], sizeof(double) * rows[q]);
            else for (size_t k = 0; k < rows[q]; k++) dst[k] = NA_REAL;
        }
    }
}
/* (An allocation failure inside R longjmps past the end of the routine: the result is handed to an external pointer with a
 * finalizer first, so that the collector frees it in that case; it is freed explicitly at the end otherwise.) */
static SEXP bam_result_to_R(qa_bam_range_result_t *res, int n, const bam_opts_t *opt, int32_t K, int32_t nG) {
    SEXP guard = PROTECT(R_MakeExternalPtr(res, R_NilValue, R_NilValue));
    R_RegisterCFinalizerEx(guard, range_result_finalizer, TRUE);
    result_t r;
    result_begin(&r);
    SEXP labs = bam_columns_and_labels(&r, res, n);
    bam_counts(&r, res);
    bam_timings_and_stats(&r, res);
    if (opt->want_prob) bam_read_label_prob(&r, res, n, labs);
    if (opt->hla_grid >= 0) bam_hla_matrices(&r, res, n, K, nG);
    SEXP out = result_end(&r);
    range_result_finalizer(guard);
    UNPROTECT(1);
    return out;
}

SEXP qa_impute_bam_range_call(SEXP bamFilesSEXP, SEXP sitesSEXP, SEXP panelSEXP, SEXP paramsSEXP, SEXP sample_indexSEXP, SEXP n_handlesSEXP) {
    static const char *who = "qa_impute_bam_range";
    /* 1. validate options */
    bam_opts_t opt;
    bam_range_validate(bamFilesSEXP, sitesSEXP, panelSEXP, paramsSEXP, sample_indexSEXP, who, &opt);
    const int n = Rf_length(bamFilesSEXP);
    /* 2. site arrays (R errors are raised only before they exist or after they are freed) */
    site_arrays_t sa;
    range_ctx_t cx;
    memset(&cx, 0, sizeof cx);
    int st = QA_OK;
    char msg[512];
    msg[0] = 0;
    if (!site_arrays_make(&sa, sitesSEXP, bamFilesSEXP, sample_indexSEXP, &opt)) {
        st = QA_ERR_INVALID;
        snprintf(msg, sizeof msg, "sites: L / grid numeric, ref / alt character vectors of single letters, all of the panel's length%s",
                 opt.rare ? " (and L_all / grid_all / ref_all / alt_all over all SNPs)" : "");
    }
    /* 3. set up */
    if (st == QA_OK) {
        st = range_setup(&cx, panelSEXP, paramsSEXP, Rf_asInteger(n_handlesSEXP), n);
        if (st != QA_OK) snprintf(msg, sizeof msg, "%s", cx.msg);
    }
    qa_bam_range_result_t *res = NULL;
    if (st == QA_OK) {
        /* 4. fill qa_bam_range_io_t and the extras */
        qa_bam_range_io_t io;
        qa_bam_range_extras_t ex;
        bam_io_fill(&io, &ex, sitesSEXP, &opt, &sa);
        /* 5. call */
        st = qa_impute_bam_range_ex(cx.handles, cx.n_handles, &cx.ip, &io, &ex, n, sa.paths, sa.sidx, cx.nipt ? cx.nq.ff : NULL, &res);
        if (st != QA_OK) snprintf(msg, sizeof msg, "%s", qa_last_error());
        range_teardown(&cx);
    }
    site_arrays_free(&sa);
    if (st != QA_OK) {
        if (res) qa_bam_range_destroy(res);
        Rf_error("quilt_amd: %s: %s", who, msg);
    }
    /* 6. result to R objects (K and nGibbsSamples are plain numbers of the context: they outlive its teardown) */
    return bam_result_to_R(res, n, &opt, cx.K, cx.ip.nGibbsSamples);
}

/* ---- registration (RcppExports.cpp:1703-1782) ----------------------------------------------------------------------
 * Inside QUILT.so (shim/QUILT-src.patch): RcppExports.cpp's own CallEntries[] names these functions in the four rows, and
 * R_init_QUILT registers them.  As a DLL of its own: R_init_quilt_amd_shim. */

static const R_CallMethodDef CallEntries[] = {
    {"_QUILT_rcpp_forwardBackwardGibbsNIPT", (DL_FUNC)&qa_QUILT_rcpp_forwardBackwardGibbsNIPT, 63},
    {"_QUILT_Rcpp_haploid_dosage_versus_refs", (DL_FUNC)&qa_QUILT_Rcpp_haploid_dosage_versus_refs, 38},
    {"_QUILT_Rcpp_make_gl_bound", (DL_FUNC)&qa_QUILT_Rcpp_make_gl_bound, 3},
    {"_QUILT_rcpp_make_eMatRead_t", (DL_FUNC)&qa_QUILT_rcpp_make_eMatRead_t, 15},
    {"qa_shim_release", (DL_FUNC)&qa_shim_release, 0},
    {"qa_impute_sample_range", (DL_FUNC)&qa_impute_sample_range, 6},
    {"qa_impute_bam_range", (DL_FUNC)&qa_impute_bam_range_call, 6},
    {NULL, NULL, 0}};

void R_init_quilt_amd_shim(DllInfo *dll) {
    R_registerRoutines(dll, NULL, CallEntries, NULL, NULL);
    R_useDynamicSymbols(dll, FALSE);
}
