"""hla_run = TRUE on the range call (qa_impute_samples_hla, include/quilt_amd.h) without a device: the native loop of
csrc/impute.cpp run over the CPU oracle through qa_impute_samples_backend_hla must equal quilt_amd/driver.py on the oracle, bit
for bit, for the four outputs get_and_impute_one_sample adds under hla_run (functions.R:1261-1280, :1489-1494) -- and leave
every other output exactly as the same run without hla_run produces it."""
import ctypes as C

import numpy as np
import pytest

from quilt_amd import native


def r_round_half_even(x):
    return int(np.round(x))   # numpy rounds half to even, as R's round() does


def igrid_0based(panel, closest_to=None):
    """functions.R:1264-1268: round(nGrids / 2) when gamma_physically_closest_to is NA, else
    grid[which.min(abs(L - gamma_physically_closest_to))] + 1; returned 0-based."""
    if closest_to is None:
        return r_round_half_even(panel.nGrids / 2) - 1
    return int(np.asarray(panel.grid)[int(np.argmin(np.abs(np.asarray(panel.L) - closest_to)))])


@pytest.fixture(scope="module")
def hla_panel():
    from quilt_amd.synth import make_synthetic_panel
    return make_synthetic_panel(K=400, nSNPs=3200, seed=77, ref_error=1e-3)


def _same_existing(a, b):
    assert a.nDosage == b.nDosage
    assert np.array_equal(a.read_labels, b.read_labels), "consensus read labels"
    assert np.array_equal(a.dosage, b.dosage), "dosage"
    assert np.array_equal(a.gp_t, b.gp_t), "genotype posteriors"
    assert np.array_equal(a.phasing_haps, b.phasing_haps), "phased haplotypes"


def _same_hla(a, b):
    for f in ("gamma1", "gamma2", "gamma_total", "list_of_gammas"):
        assert np.array_equal(np.asarray(getattr(a, f)), np.asarray(getattr(b, f))), f


def _check_total(r, nG, K):
    lg = np.asarray(r.list_of_gammas)
    assert lg.shape == (nG, 2, K)
    tot = np.zeros(K)
    for i in range(nG):
        tot = (tot + lg[i, 0]) + lg[i, 1]
    assert np.array_equal(np.asarray(r.gamma_total), tot), "gamma_total = ((0 + g1_1) + g2_1) + ... in Gibbs-sample order"


def test_new_symbols_are_exported_and_need_a_device():
    L = native.lib()
    for name in ("qa_fullpass_reads_select_gamma_batch", "qa_impute_samples_hla", "qa_impute_samples_backend_hla"):
        assert hasattr(L, name), name
    from quilt_amd.impute import make_hla
    hq, keep = make_hla(0, 1, 1, 1)
    gcol = np.zeros(1)
    if L.qa_device_count() < 1:
        # without a device both stop at the device check, before the (fake, never dereferenced) handle is looked at
        handle = C.c_void_p(1)
        panels = (C.c_void_p * 1)(handle)
        want = native.QA_ERR_NO_DEVICE
    else:   # with one: no handle at all, refused as a missing argument
        handle, panels, want = None, None, native.QA_ERR_INVALID
    st_f = L.qa_fullpass_reads_select_gamma_batch(handle, *([C.c_int32(0)] * 3), *([None] * 9), C.c_int32(0), C.c_double(0), None,
                                                  C.c_int32(0), None, None, None, C.c_int32(0), C.c_int32(0), None, None, None, None,
                                                  C.c_int32(0), gcol.ctypes.data_as(C.POINTER(C.c_double)))
    st_i = L.qa_impute_samples_hla(panels, C.c_int32(1), None, C.c_int32(0), C.c_int64(0), *([None] * 11), C.byref(hq))
    assert st_f == want and st_i == want


def test_hla_struct_mirror_has_the_headers_layout(tmp_path):
    import os
    import subprocess
    from quilt_amd.impute import ImputeHla
    from tests.test_struct_layout_cpu import INC, _header_text, _members
    names = _members("qa_impute_hla_t", _header_text())
    assert [f[0] for f in ImputeHla._fields_] == names
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "quilt_amd.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(qa_impute_hla_t));']
    lines += [f'    printf("{n} %zu\\n", offsetof(qa_impute_hla_t, {n}));' for n in names]
    lines += ["    return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", INC, str(src), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for n in names:
        assert getattr(ImputeHla, n).offset == int(out[n]), n
    assert C.sizeof(ImputeHla) == int(out["size"])
    assert os.path.exists(os.path.join(INC, "quilt_amd.h"))


@pytest.mark.parametrize("seed,closest,per_set,n_threads", [
    (11, None, 2, 1),
    (12, 151_000, 3, 2),
    (13, None, 256, 3),
    (14, 40_000, 1, 3),
], ids=["NA-sets2", "closest-sets3-threads2", "NA-sets256-threads3", "closest-sets1-threads3"])
def test_native_hla_loop_equals_python_driver(hla_panel, seed, closest, per_set, n_threads):
    from quilt_amd.driver import Driver, DriverParams, HlaDriverParams
    from quilt_amd.synth import make_synthetic_sample
    from tests.hla_backend import OracleBackendHLA, impute_samples_hla_on_oracle
    from tests.native_driver_backend import impute_samples_on_oracle
    panel = hla_panel
    grid = igrid_0based(panel, closest)
    assert 0 <= grid < panel.nGrids
    samples = [make_synthetic_sample(panel, seed=700 + 10 * seed + i, n_reads=180 + 7 * i) for i in range(4)]
    common = dict(nGibbsSamples=3, n_seek_its=2, Ksubset=48, Knew=32, small_ref_panel_gibbs_iterations=4,
                  small_ref_panel_block_gibbs_iterations=(2,), seed=seed)
    P = HlaDriverParams(**common, hla_grid=grid)
    want = Driver(panel, OracleBackendHLA(panel), P).run(samples, sample_offset=3)
    got, _, tab = impute_samples_hla_on_oracle(panel, samples, P, grid, sample_offset=3, samples_per_launch_set=per_set,
                                               n_threads=n_threads)
    plain, _, _ = impute_samples_on_oracle(panel, samples, DriverParams(**common), sample_offset=3, samples_per_launch_set=per_set,
                                           n_threads=n_threads)
    assert tab.calls["select_gamma"] >= 1
    for a, b, c in zip(got, want, plain):
        _same_existing(a, b)
        _same_existing(a, c)   # hla_run changes nothing else in the loop
        _same_hla(a, b)
        _check_total(a, P.nGibbsSamples, panel.K)
        assert np.asarray(a.gamma1).shape == (panel.K,) and np.asarray(a.gamma2).shape == (panel.K,)
        # a gamma column sums to 1 over the panel (colSums(gamma_t) == 1)
        assert abs(np.asarray(a.gamma1).sum() - 1) < 1e-9 and abs(np.asarray(a.gamma2).sum() - 1) < 1e-9


def test_native_hla_loop_with_a_sample_source(hla_panel):
    from quilt_amd.driver import DriverParams, HlaDriverParams
    from quilt_amd.synth import make_synthetic_sample
    from tests.hla_backend import impute_samples_hla_on_oracle
    panel = hla_panel
    grid = igrid_0based(panel)
    samples = [make_synthetic_sample(panel, seed=900 + i, n_reads=170) for i in range(3)]
    P = HlaDriverParams(nGibbsSamples=2, n_seek_its=2, Ksubset=48, Knew=48, small_ref_panel_gibbs_iterations=4,
                        small_ref_panel_block_gibbs_iterations=(2,), seed=5, hla_grid=grid)
    flat, _, _ = impute_samples_hla_on_oracle(panel, samples, P, grid, samples_per_launch_set=2, n_threads=2)
    src, _, _ = impute_samples_hla_on_oracle(panel, samples, P, grid, samples_per_launch_set=2, n_threads=2, source=True)
    for a, b in zip(flat, src):
        _same_existing(a, b)
        _same_hla(a, b)


def _r_function(text, name):
    at = text.index(name + " <- function(")
    depth, i = 0, text.index("{", text.index(") {", at))
    for j in range(i, len(text)):
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[at:j + 1]
    raise AssertionError(name)


def test_the_r_side_forms_igrid_with_the_reference_expressions():
    """shim/quilt-amd.R: quilt_amd_hla_iGrid is the reference's own two expressions (functions.R:1264-1268), the range call passes
    iGrid - 1, and a range whose iGrid is below 1 (nGrids = 1: round(1 / 2) = 0) is not covered."""
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    amd = open(os.path.join(root, "shim", "quilt-amd.R")).read()
    fn = _r_function(amd, "quilt_amd_hla_iGrid")
    exprs = ("iGrid <- round(nGrids / 2)", "iGrid <- grid[which.min(abs(L - gamma_physically_closest_to))] + 1")
    for e in exprs:
        assert e in fn
    ref = "/root/reference/QUILT/R/functions.R"
    if os.path.exists(ref):
        text = open(ref).read()
        for e in exprs:
            assert e in text
    covered = _r_function(amd, "quilt_amd_range_is_covered")
    assert "quilt_amd_hla_iGrid(gamma_physically_closest_to, L, grid, ncol(hapMatcherR)) >= 1" in covered
    assert 'params[["hla_grid"]] <- as.integer(iGrid - 1L)' in _r_function(amd, "quilt_amd_impute_sample_range")
    assert r_round_half_even(1 / 2) == 0   # nGrids = 1: iGrid 0, not covered


def test_igrid_follows_the_reference_expressions(hla_panel):
    assert igrid_0based(hla_panel) == 49                 # round(100 / 2) = 50, 1-based
    assert r_round_half_even(2.5) == 2 and r_round_half_even(3.5) == 4
    L, grid = np.asarray(hla_panel.L), np.asarray(hla_panel.grid)
    assert igrid_0based(hla_panel, int(L[-1]) + 10_000) == int(grid[-1])
    assert igrid_0based(hla_panel, int(L[0])) == 0


def _refusal(panel, P, grid, q_edit=None):
    from quilt_amd.synth import make_synthetic_sample
    from tests.hla_backend import impute_samples_hla_on_oracle
    samples = [make_synthetic_sample(panel, seed=950, n_reads=150)]
    with pytest.raises(RuntimeError) as e:
        impute_samples_hla_on_oracle(panel, samples, P, grid, q_edit=q_edit)
    return str(e.value)


def test_refusals(hla_panel):
    from quilt_amd.driver import DriverParams, HlaDriverParams
    from quilt_amd.impute import ImputeNipt
    panel = hla_panel
    base = dict(nGibbsSamples=2, n_seek_its=2, Ksubset=48, Knew=48, small_ref_panel_gibbs_iterations=4,
                small_ref_panel_block_gibbs_iterations=(2,), seed=5)
    P = DriverParams(**base)
    for g in (-1, panel.nGrids):
        assert "grid outside [0, nGrids)" in _refusal(panel, P, g)

    def mspbwt(q):
        q.use_mspbwt = 1
    assert "use_mspbwt" in _refusal(panel, P, 3, mspbwt)
    nq = ImputeNipt()

    def nipt(q):
        q.nipt = C.cast(C.pointer(nq), C.c_void_p)
        return nq
    assert "nipt" in _refusal(panel, P, 3, nipt)
    dummy = (C.c_char * 128)()

    def rare_common(q):
        q.rare_common = C.cast(dummy, C.c_void_p)
        return dummy
    assert "impute_rare_common" in _refusal(panel, P, 3, rare_common)

    def burn(q):
        q.n_burn_in_seek_its = 2
    assert "not a dosage pass" in _refusal(panel, P, 3, burn)
    # the Python driver refuses the same
    for kw in (dict(use_mspbwt=True), dict(method="nipt"), dict(impute_rare_common=True)):
        with pytest.raises(ValueError):
            HlaDriverParams(**base, **kw, hla_grid=3).resolved(panel.K)
    from quilt_amd.driver import Driver
    from tests.hla_backend import OracleBackendHLA
    with pytest.raises(ValueError):
        Driver(panel, OracleBackendHLA(panel), HlaDriverParams(**base, hla_grid=panel.nGrids))
