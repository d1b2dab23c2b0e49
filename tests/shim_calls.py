"""R-shaped arguments for the `.Call` entries of shim/quilt_amd_shim.c (helper, no test): `params` from a DriverParams, the panel
arguments the 38- and 63-argument entries share, a call of a `_QUILT_*` entry by argument name, and the 63- and 15-argument
entries as the driver loop makes them.  ``R`` is a tests.mini_r.R."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(R, prm, **more):
    d = dict(nGibbsSamples=R.integer([prm.nGibbsSamples]), n_seek_its=R.integer([prm.n_seek_its]), Ksubset=R.integer([prm.Ksubset]),
             Knew=R.integer([prm.Knew]), K_top_matches=R.integer([prm.K_top_matches]), heuristic_match_thin=R.real([prm.heuristic_match_thin]),
             small_ref_panel_gibbs_iterations=R.integer([prm.small_ref_panel_gibbs_iterations]),
             small_ref_panel_block_gibbs_iterations=R.integer(list(prm.small_ref_panel_block_gibbs_iterations)),
             maxDifferenceBetweenReads=R.real([prm.maxDifferenceBetweenReads]), minGLValue=R.real([prm.minGLValue]), Jmax=R.integer([prm.Jmax]),
             seed=R.real([float(prm.seed)]), samples_per_launch_set=R.integer([2]))
    d.update(more)
    return R.named(d)


def entry_args(name):
    return json.load(open(os.path.join(ROOT, "tests", "golden", "callentries.json")))[name]["args"]


def call_by_name(R, name, vals):
    """`.Call(name, ...)` with the arguments in the reference's order (tests/golden/callentries.json, from RcppExports.cpp);
    arguments the test does not name are NULL."""
    order = entry_args(name)
    assert set(vals) <= set(order), set(vals) - set(order)
    return R.dotcall(name, *[vals.get(a, R.nil) for a in order])


def panel_args(R, panel):
    return dict(hapMatcher=R.integer(np.zeros((1, 1), dtype=np.int32)), hapMatcherR=R.raw(panel.hapMatcherR), use_hapMatcherR=R.logical([1]),
                distinctHapsB=R.integer(panel.distinctHapsB), distinctHapsIE=R.real(panel.distinctHapsIE),
                eMatDH_special_matrix_helper=R.integer(panel.eMatDH_special_matrix_helper), eMatDH_special_matrix=R.integer(panel.eMatDH_special_matrix),
                rhb_t=R.integer(panel.rhb_t), ref_error=R.real([panel.ref_error]))


def gibbs_args(R, panel, s, which, start, n_burn, n_samp, blocks=(), param_list=None, **more):
    """The 63-argument entry's named arguments for a common-SNP diploid call on ``s`` (impute_one_sample, functions.R:2385-2700);
    ``param_list`` and ``more`` replace or add entries."""
    G, Ks = panel.nGrids, len(which)
    z = lambda: R.real(np.zeros((Ks, G)))
    pl = dict(perform_block_gibbs=R.logical([1 if len(blocks) else 0]), return_hapProbs=R.logical([1]), return_genProbs=R.logical([1]))
    pl.update(param_list or {})
    a = dict(sampleReads=R.sample_reads(s), transMatRate_tc_H=R.real(np.asarray(panel.transMatRate_t).reshape(2, G - 1, 1, order="F")), ff=R.real([0.0]),
             alphaHat_t1=z(), betaHat_t1=z(), alphaHat_t2=z(), betaHat_t2=z(), eMatGrid_t1=z(), eMatGrid_t2=z(),
             which_haps_to_use=R.integer(which), wif0=R.integer(s.wif), L_grid=R.integer(panel.L_grid), param_list=R.named(pl),
             Jmax_local=R.integer([10000]), maxDifferenceBetweenReads=R.real([1e10]), generate_fb_snp_offsets=R.logical([0]),
             n_gibbs_starts=R.integer([1]), n_gibbs_sample_its=R.integer([n_samp]), n_gibbs_burn_in_its=R.integer([n_burn]),
             double_list_of_starting_read_labels=R.list([R.list([R.integer(start)])]), class_sum_cutoff=R.real([0.06]),
             shuffle_bin_radius=R.integer([5000]), block_gibbs_iterations=R.integer(np.asarray(blocks, dtype=np.int32)),
             block_gibbs_quantile_prob=R.real([0.95]))
    a.update(panel_args(R, panel))
    a.update(more)
    return a


def ematread_args(R, s, eMatRead_t, eHaps, slice_, pseudo_haploid=0):
    """The 15 arguments of `_QUILT_rcpp_make_eMatRead_t` as calculate_eMatRead_t_vs_haplotypes passes them (functions.R:2975-3020)."""
    return [eMatRead_t, R.sample_reads(s), R.real(eHaps), R.integer([slice_]), R.real([1000.0]), R.integer([1000]), R.real(np.zeros((1, 1))),
            R.real([0.0]), R.real([0.0]), R.integer([0]), R.integer([1]), R.string("N"), R.string("N"), R.logical([pseudo_haploid]), R.logical([0])]
