"""Every refusal shim/quilt_amd_shim.c raises BEFORE its first library call that needs a device, as a whole string: the text of
each R error and, where a call has two faults, which of them decides the text (the first failing check).  The expected texts are
tests/golden/shim_refusals.json, recorded by running this file's case table against the shim of the commit the file names
(`python -m tests.test_shim_refusals_cpu --record <commit>`): a restructuring of the shim must leave every one of them byte for
byte.  Refusals raised after the panel handles exist (method = "nipt" without ff, a missing L_grid, ...) need a device and stay
with tests/test_shim_gpu.py.  K = 64, 320-SNP panel, one 40-read sample; the Ksubset case needs a panel above the built maximum."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "shim_refusals.json")


class Ctx:
    """The R runtime and the objects every case starts from; a case replaces what it breaks."""

    def __init__(self):
        from quilt_amd.driver import DriverParams
        from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample
        from tests.mini_r import R as Runtime
        self.R = Runtime()
        self.R.dotcall("qa_shim_release")   # (no cached panel: the per-call entries' "needs the panel" refusals are about that state)
        self.panel = make_synthetic_panel(K=64, nSNPs=320, seed=2)
        self.big = make_synthetic_panel(K=2048, nSNPs=320, seed=2)
        self.s = make_synthetic_sample(self.panel, seed=3, n_reads=40)
        self.prm = DriverParams(nGibbsSamples=2, Ksubset=64, Knew=64)

    # ---- qa_impute_sample_range(list_of_sampleReads, panel_objects, params, sample_offset, n_handles, list_of_allSNP_sampleReads)
    def sample_range(self, reads=None, panel=None, params=None, offset=None, all_reads=None, **more_params):
        from tests.shim_calls import params as mk
        R = self.R
        return R.dotcall("qa_impute_sample_range", R.list([R.sample_reads(self.s)]) if reads is None else reads,
                         R.panel_objects(self.panel) if panel is None else panel,
                         mk(R, self.prm, **more_params) if params is None else params,
                         R.real([0.0]) if offset is None else offset, R.integer([1]), R.nil if all_reads is None else all_reads)

    # ---- qa_impute_bam_range(bam_files, sites, panel_objects, params, sample_index, n_handles)
    def sites(self, drop=(), **more):
        R, p = self.R, self.panel
        d = dict(chr=R.string("chr20"), L=R.integer(p.L), ref=R.strings(["A"] * p.nSNPs), alt=R.strings(["C"] * p.nSNPs),
                 grid=R.integer(np.arange(p.nSNPs) // 32))
        d.update(more)
        return R.named({k: v for k, v in d.items() if k not in drop})

    def bam_range(self, bams=None, sites=None, panel=None, index=None, **more_params):
        from tests.shim_calls import params as mk
        R = self.R
        return R.dotcall("qa_impute_bam_range", R.strings(["a.bam"]) if bams is None else bams, self.sites() if sites is None else sites,
                         R.panel_objects(self.panel) if panel is None else panel, mk(R, self.prm, **more_params),
                         R.real([0.0]) if index is None else index, R.integer([1]))

    # ---- the per-call entries
    def gibbs(self, param_list=None, **more):
        from tests.shim_calls import call_by_name, gibbs_args
        R, s = self.R, self.s
        a = gibbs_args(R, self.panel, s, np.arange(1, 33, dtype=np.int32), np.ones(s.nReads, dtype=np.int32), 1, 1, param_list=param_list, **more)
        return call_by_name(R, "_QUILT_rcpp_forwardBackwardGibbsNIPT", a)

    def ematread(self, pseudo_haploid=0):
        from tests.shim_calls import ematread_args
        R, s = self.R, self.s
        return R.dotcall("_QUILT_rcpp_make_eMatRead_t", *ematread_args(R, s, R.real(np.zeros((2, s.nReads))), np.full((2, self.panel.nSNPs, 1), 0.5), 0,
                                                                       pseudo_haploid=pseudo_haploid))

    def fullpass(self):
        from tests.shim_calls import call_by_name
        return call_by_name(self.R, "_QUILT_Rcpp_haploid_dosage_versus_refs", dict(use_eMatDH=self.R.logical([0])))


def _read(R, J=None, wif=None, bq=None, u=None, n=4):
    """One read list(J, wif, bq, u) with the given entries replaced (n < 4: a list too short)."""
    items = [R.integer([1]) if J is None else J, R.integer([0]) if wif is None else wif, R.integer([[20], [20]]) if bq is None else bq,
             R.integer([[3], [4]]) if u is None else u]
    return R.list(items[:n])


def _rare_common(R, panel, **more):
    d = dict(snp_is_common=R.logical(np.ones(panel.nSNPs, dtype=np.int32)), rare_per_hap_info=R.list([R.integer([])] * panel.K),
             transMatRate_t=R.real(panel.transMatRate_t))
    d.update(more)
    return R.named(d)


def _panel_without(c, *drop, **more):
    """panel_objects with entries dropped or replaced."""
    R, p = c.R, c.panel
    d = dict(hapMatcherR=R.raw(p.hapMatcherR), distinctHapsB=R.integer(p.distinctHapsB), distinctHapsIE=R.real(p.distinctHapsIE),
             eMatDH_special_matrix_helper=R.integer(p.eMatDH_special_matrix_helper), eMatDH_special_matrix=R.integer(p.eMatDH_special_matrix),
             rhb_t=R.integer(p.rhb_t), transMatRate_t=R.real(p.transMatRate_t), ref_error=R.real([p.ref_error]))
    d.update(more)
    return R.named({k: v for k, v in d.items() if k not in drop})


# id -> the call that must be refused.  Ids say which entry and what is wrong; "a+b" names two faults in the order the shim checks them.
CASES = {
    # ---- sample range: the reads
    "range/reads_not_a_list": lambda c: c.sample_range(reads=c.R.integer([1])),
    "range/sample_not_a_list": lambda c: c.sample_range(reads=c.R.list([c.R.integer([1])])),
    "range/read_too_short": lambda c: c.sample_range(reads=c.R.list([c.R.list([_read(c.R), _read(c.R, n=3)])])),
    "range/read_not_a_list": lambda c: c.sample_range(reads=c.R.list([c.R.list([c.R.integer([1])])])),
    "range/bq_not_integer": lambda c: c.sample_range(reads=c.R.list([c.R.list([_read(c.R, bq=c.R.real([[20.0], [20.0]]))])])),
    "range/bq_u_lengths_differ": lambda c: c.sample_range(reads=c.R.list([c.R.list([_read(c.R, u=c.R.integer([[3]]))])])),
    "range/wif_not_a_number": lambda c: c.sample_range(reads=c.R.list([c.R.list([_read(c.R, wif=c.R.string("0"))])])),
    "range/wif_empty": lambda c: c.sample_range(reads=c.R.list([c.R.list([_read(c.R, wif=c.R.integer([]))])])),
    "range/all_reads_not_a_list": lambda c: c.sample_range(all_reads=c.R.real([1.0])),
    "range/all_reads_sample_not_a_list": lambda c: c.sample_range(all_reads=c.R.list([c.R.list([]), c.R.real([1.0])])),
    # ---- sample range: panel_objects and params (range_validate)
    "range/panel_objects_empty": lambda c: c.sample_range(panel=c.R.named({})),
    "range/panel_objects_without_transMatRate_t": lambda c: c.sample_range(panel=_panel_without(c, "transMatRate_t")),
    "range/hapMatcherR_not_raw": lambda c: c.sample_range(panel=_panel_without(c, hapMatcherR=c.R.integer(c.panel.hapMatcherR))),
    "range/rhb_t_not_integer": lambda c: c.sample_range(panel=_panel_without(c, rhb_t=c.R.real(np.zeros((1, 1))))),
    "range/transMatRate_t_size": lambda c: c.sample_range(panel=_panel_without(c, transMatRate_t=c.R.real(np.zeros((2, 5))))),
    "range/rare_per_hap_info_not_a_list": lambda c: c.sample_range(
        panel=_panel_without(c, rare_common=_rare_common(c.R, c.panel, rare_per_hap_info=c.R.integer([1])))),
    "range/rare_per_hap_info_entry_not_integer": lambda c: c.sample_range(
        panel=_panel_without(c, rare_common=_rare_common(c.R, c.panel, rare_per_hap_info=c.R.list([c.R.integer([]), c.R.integer([]), c.R.real([5.0])])))),
    "range/snp_is_common_not_logical": lambda c: c.sample_range(
        panel=_panel_without(c, rare_common=_rare_common(c.R, c.panel, snp_is_common=c.R.integer(np.ones(c.panel.nSNPs, dtype=np.int32))))),
    "range/rare_transMatRate_t_not_numeric": lambda c: c.sample_range(
        panel=_panel_without(c, rare_common=_rare_common(c.R, c.panel, transMatRate_t=c.R.integer([1, 2])))),
    "range/L_grid_not_numeric": lambda c: c.sample_range(panel=_panel_without(c, L_grid=c.R.strings(["1"] * c.panel.nGrids))),
    "range/rare_L_grid_not_numeric": lambda c: c.sample_range(
        panel=_panel_without(c, rare_common=_rare_common(c.R, c.panel, L_grid=c.R.logical([1] * c.panel.nGrids)))),
    "range/ff_not_numeric": lambda c: c.sample_range(ff=c.R.integer([0])),
    "range/Ksubset_above_the_built_maximum": lambda c: c.sample_range(panel=c.R.panel_objects(c.big), Ksubset=c.R.integer([2000])),
    "range/Ksubset_above_the_built_maximum_nipt": lambda c: c.sample_range(panel=c.R.panel_objects(c.big), Ksubset=c.R.integer([700]),
                                                                            method=c.R.string("nipt")),
    "range/Ksubset_is_the_panels_size": lambda c: c.sample_range(panel=c.R.panel_objects(c.big), Ksubset=c.R.integer([5000])),
    "range/seed_negative": lambda c: c.sample_range(seed=c.R.real([-1.0])),
    "range/seed_fraction": lambda c: c.sample_range(seed=c.R.real([1.5])),
    "range/seed_nan": lambda c: c.sample_range(seed=c.R.real([float("nan")])),
    "range/seed_above_2_53": lambda c: c.sample_range(seed=c.R.real([2.0 ** 60])),
    "range/sum_order": lambda c: c.sample_range(sum_order=c.R.integer([7])),
    "range/sum_order_batched": lambda c: c.sample_range(sum_order=c.R.integer([1]), sum_order_batched=c.R.integer([2])),
    "range/block_iterations_not_integer": lambda c: c.sample_range(small_ref_panel_block_gibbs_iterations=c.R.real([3.0])),
    # ---- sample range: the entry's own checks
    "range/sample_offset_length": lambda c: c.sample_range(offset=c.R.real([0.0, 1.0])),
    "range/sample_offset_type": lambda c: c.sample_range(offset=c.R.string("0")),
    "range/rare_common_without_all_reads": lambda c: c.sample_range(impute_rare_common=c.R.logical([1])),
    "range/rare_common_all_reads_of_another_length": lambda c: c.sample_range(impute_rare_common=c.R.logical([1]), all_reads=c.R.list([])),
    "range/hla_grid_out_of_range": lambda c: c.sample_range(hla_grid=c.R.integer([c.panel.nGrids])),
    "range/hla_grid_negative": lambda c: c.sample_range(hla_grid=c.R.integer([-1])),
    "range/hla_grid_fraction": lambda c: c.sample_range(hla_grid=c.R.real([1.5])),
    "range/hla_grid_two_numbers": lambda c: c.sample_range(hla_grid=c.R.integer([1, 2])),
    "range/hla_grid_not_a_number": lambda c: c.sample_range(hla_grid=c.R.string("1")),
    # ---- sample range: two faults, the first check decides
    "range/reads_not_a_list+panel_objects_empty": lambda c: c.sample_range(reads=c.R.integer([1]), panel=c.R.named({})),
    "range/all_reads_not_a_list+panel_objects_empty": lambda c: c.sample_range(all_reads=c.R.real([1.0]), panel=c.R.named({})),
    "range/hapMatcherR_not_raw+transMatRate_t_size": lambda c: c.sample_range(
        panel=_panel_without(c, hapMatcherR=c.R.integer(c.panel.hapMatcherR), transMatRate_t=c.R.real(np.zeros((2, 5))))),
    "range/L_grid_not_numeric+ff_not_numeric": lambda c: c.sample_range(panel=_panel_without(c, L_grid=c.R.strings(["1"])), ff=c.R.integer([0])),
    "range/Ksubset+seed": lambda c: c.sample_range(panel=c.R.panel_objects(c.big), Ksubset=c.R.integer([2000]), seed=c.R.real([-1.0])),
    "range/seed+sum_order": lambda c: c.sample_range(seed=c.R.real([-1.0]), sum_order=c.R.integer([7])),
    "range/sum_order+block_iterations": lambda c: c.sample_range(sum_order=c.R.integer([7]), small_ref_panel_block_gibbs_iterations=c.R.real([3.0])),
    "range/block_iterations+sample_offset": lambda c: c.sample_range(small_ref_panel_block_gibbs_iterations=c.R.real([3.0]), offset=c.R.string("0")),
    "range/sample_offset+rare_common_without_all_reads": lambda c: c.sample_range(offset=c.R.real([0.0, 1.0]), impute_rare_common=c.R.logical([1])),
    "range/rare_common_without_all_reads+hla_grid": lambda c: c.sample_range(impute_rare_common=c.R.logical([1]), hla_grid=c.R.integer([-1])),
    # ---- BAM range
    "bam/bam_files_type": lambda c: c.bam_range(bams=c.R.integer([1])),
    "bam/sample_index_length": lambda c: c.bam_range(index=c.R.real([0.0, 1.0])),
    "bam/sample_index_type": lambda c: c.bam_range(index=c.R.strings(["0"])),
    "bam/panel_objects_empty": lambda c: c.bam_range(panel=c.R.named({})),
    "bam/seed": lambda c: c.bam_range(seed=c.R.real([-1.0])),
    "bam/sum_order": lambda c: c.bam_range(sum_order=c.R.integer([7])),
    "bam/use_bx_tag_not_logical": lambda c: c.bam_range(sites=c.sites(use_bx_tag=c.R.integer([1]))),
    "bam/use_bx_tag_two_values": lambda c: c.bam_range(sites=c.sites(use_bx_tag=c.R.logical([1, 0]))),
    "bam/use_bx_tag_na": lambda c: c.bam_range(sites=c.sites(use_bx_tag=c.R.logical([-2147483648]))),
    "bam/bxTagUpperLimit_negative": lambda c: c.bam_range(sites=c.sites(bxTagUpperLimit=c.R.integer([-1]))),
    "bam/bxTagUpperLimit_fraction": lambda c: c.bam_range(sites=c.sites(bxTagUpperLimit=c.R.real([0.5]))),
    "bam/output_read_label_prob_not_logical": lambda c: c.bam_range(sites=c.sites(output_read_label_prob=c.R.real([1.0]))),
    "bam/hla_grid_out_of_range": lambda c: c.bam_range(hla_grid=c.R.integer([c.panel.nGrids])),
    "bam/hla_grid_fraction": lambda c: c.bam_range(hla_grid=c.R.real([1.5])),
    "bam/sites_without_chr": lambda c: c.bam_range(sites=c.sites(drop=("chr",))),
    "bam/sites_chr_two_strings": lambda c: c.bam_range(sites=c.sites(chr=c.R.strings(["chr1", "chr2"]))),
    "bam/sites_without_L": lambda c: c.bam_range(sites=c.sites(drop=("L",))),
    "bam/sites_L_of_another_length": lambda c: c.bam_range(sites=c.sites(L=c.R.integer(c.panel.L[:-1]))),
    "bam/sites_ref_not_character": lambda c: c.bam_range(sites=c.sites(ref=c.R.integer(np.zeros(c.panel.nSNPs, dtype=np.int32)))),
    "bam/sites_alt_two_letters": lambda c: c.bam_range(sites=c.sites(alt=c.R.strings(["AC"] * c.panel.nSNPs))),
    "bam/sites_grid_not_numeric": lambda c: c.bam_range(sites=c.sites(grid=c.R.strings(["0"] * c.panel.nSNPs))),
    "bam/sites_without_grid": lambda c: c.bam_range(sites=c.sites(drop=("grid",))),
    "bam/rare_common_without_the_all_snp_sites": lambda c: c.bam_range(impute_rare_common=c.R.logical([1])),
    # ---- BAM range: two faults
    "bam/bam_files_type+sample_index_length": lambda c: c.bam_range(bams=c.R.integer([1]), index=c.R.real([0.0, 1.0])),
    "bam/sample_index_length+panel_objects_empty": lambda c: c.bam_range(index=c.R.real([0.0, 1.0]), panel=c.R.named({})),
    "bam/seed+use_bx_tag": lambda c: c.bam_range(seed=c.R.real([-1.0]), sites=c.sites(use_bx_tag=c.R.integer([1]))),
    "bam/use_bx_tag+bxTagUpperLimit": lambda c: c.bam_range(sites=c.sites(use_bx_tag=c.R.integer([1]), bxTagUpperLimit=c.R.integer([-1]))),
    "bam/bxTagUpperLimit+output_read_label_prob": lambda c: c.bam_range(
        sites=c.sites(bxTagUpperLimit=c.R.integer([-1]), output_read_label_prob=c.R.real([1.0]))),
    "bam/output_read_label_prob+hla_grid": lambda c: c.bam_range(sites=c.sites(output_read_label_prob=c.R.real([1.0])), hla_grid=c.R.integer([-1])),
    "bam/hla_grid+sites_without_chr": lambda c: c.bam_range(hla_grid=c.R.integer([-1]), sites=c.sites(drop=("chr",))),
    "bam/sites_without_chr+ref_not_character": lambda c: c.bam_range(
        sites=c.sites(drop=("chr",), ref=c.R.integer(np.zeros(c.panel.nSNPs, dtype=np.int32)))),
    # ---- the per-call entries (no panel is cached)
    "gibbs/n_gibbs_starts": lambda c: c.gibbs(n_gibbs_starts=c.R.integer([2])),
    "gibbs/run_fb_subset": lambda c: c.gibbs(param_list=dict(run_fb_subset=c.R.logical([1]))),
    "gibbs/generate_fb_snp_offsets": lambda c: c.gibbs(generate_fb_snp_offsets=c.R.logical([1])),
    "gibbs/use_starting_read_labels": lambda c: c.gibbs(param_list=dict(use_starting_read_labels=c.R.logical([0]))),
    "gibbs/pass_in_eMatRead_t": lambda c: c.gibbs(param_list=dict(pass_in_eMatRead_t=c.R.logical([1]))),
    "gibbs/use_small_eHapsCurrent_tc": lambda c: c.gibbs(param_list=dict(use_small_eHapsCurrent_tc=c.R.logical([1]))),
    "gibbs/block_wise_shard_with_rare_common": lambda c: c.gibbs(
        param_list=dict(shard_check_every_pair=c.R.logical([0]), make_eMatRead_t_rare_common=c.R.logical([1]))),
    "gibbs/rare_common_without_a_panel": lambda c: c.gibbs(param_list=dict(make_eMatRead_t_rare_common=c.R.logical([1]))),
    "gibbs/n_gibbs_starts+block_wise_shard_with_rare_common": lambda c: c.gibbs(
        n_gibbs_starts=c.R.integer([2]), param_list=dict(shard_check_every_pair=c.R.logical([0]), make_eMatRead_t_rare_common=c.R.logical([1]))),
    "ematread/pseudo_haploid": lambda c: c.ematread(pseudo_haploid=1),
    "ematread/without_a_panel": lambda c: c.ematread(),
    "fullpass/use_eMatDH_false": lambda c: c.fullpass(),
}


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.R.dotcall("qa_shim_release")
    c.R.reset()


def refusal(c, case_id):
    """The R error's text, whole; None when the call was not refused."""
    from tests.mini_r import RError
    try:
        CASES[case_id](c)
    except RError as e:
        return str(e)
    return None


def test_the_golden_file_holds_exactly_the_case_table():
    golden = json.load(open(GOLDEN))
    assert sorted(golden["refusals"]) == sorted(CASES)
    assert len(golden["recorded_at_commit"]) == 40 and all(t.startswith("quilt_amd: ") for t in golden["refusals"].values())


@pytest.mark.parametrize("case_id", sorted(CASES))
def test_refusal_text(ctx, case_id):
    want = json.load(open(GOLDEN))["refusals"][case_id]
    assert refusal(ctx, case_id) == want


def test_the_issues_pairs_give_the_first_checks_text(ctx):
    """The order the texts of the golden file stand for, said once more without it: of two faults the earlier check's text arrives."""
    golden = json.load(open(GOLDEN))["refusals"]
    for pair in (c for c in CASES if "+" in c):
        entry, faults = pair.split("/")
        first = faults.split("+")[0]
        alone = [c for c in CASES if c.startswith(entry + "/" + first) and "+" not in c]
        assert alone, pair
        assert golden[pair] in {golden[a] for a in alone}, pair


if __name__ == "__main__":
    import sys
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: python -m tests.test_shim_refusals_cpu --record <commit of the shim>"
    c = Ctx()
    texts = {case_id: refusal(c, case_id) for case_id in sorted(CASES)}
    missing = [k for k, v in texts.items() if v is None]
    assert not missing, missing
    json.dump(dict(recorded_at_commit=sys.argv[2], refusals=texts), open(GOLDEN, "w"), indent=1, sort_keys=True)
    print(f"{len(texts)} refusals -> {GOLDEN}")
