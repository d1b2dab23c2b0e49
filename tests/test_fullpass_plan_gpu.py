"""The launch planner of the full-panel passes against what run_passes carves (csrc/pass_layout.hpp: one layout serves both).
Through the private hook of csrc/fullpass_testhook.h: the calling thread's last launch set -- its passes, the planned bytes per
pass, the plan's fixed term, the arena bytes carved, the kernels that ran it."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.testhooks import last_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_F32, KIND_F64_RANK, KIND_F64_FULL, KIND_F64_DOS, KIND_F64_REF = range(5)   # PassKind (csrc/pass_layout.hpp)


def _carve_align():
    """The arena's carve alignment, as common.hpp states it."""
    src = open(os.path.join(ROOT, "quilt_amd", "csrc", "common.hpp")).read()
    return int(re.search(r"kCarveAlign\s*=\s*(\d+)\s*;", src).group(1))


@pytest.fixture(scope="module")
def two_row_panel():
    """K = 8 193: the first size with two fp64 chunk rows; 12 grids."""
    from quilt_amd.synth import make_synthetic_panel
    return make_synthetic_panel(K=8193, nSNPs=384, seed=93)


def _gls(panel, n, seed=3):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.uniform(0.05, 1.0, size=(n, panel.nSNPs, 2)))


def _batch(dev, panel, cols, want_dosage, K_top):
    """qa_fullpass_batch with P = 3 passes that all want the same."""
    from quilt_amd.native import check, lib, ptr
    n, T = 3, panel.nSNPs
    gl = _gls(panel, n)
    wd = np.full(n, want_dosage, dtype=np.int32)
    n_thin = int((cols >= 0).sum())
    cap = n * n_thin * 4096
    bptr, bidx, bval = np.zeros(n * n_thin + 1, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap)
    dosage = np.zeros((n, T))
    check(lib().qa_fullpass_batch(dev.handle, C.c_int32(n), ptr(gl), ptr(wd), ptr(cols), C.c_int32(K_top), ptr(dosage), ptr(bptr),
                                  ptr(bidx), ptr(bval), C.c_int64(cap)))


def _matrices(dev, panel, cols):
    """The single-pass entry, P = 1: dosage, gamma_t and betaHat_t."""
    from quilt_amd.reference_single import Rcpp_haploid_dosage_versus_refs
    K, G, T = panel.K, panel.nGrids, panel.nSNPs
    gl = np.asfortranarray(_gls(panel, 1)[0].T)
    Rcpp_haploid_dosage_versus_refs(dev, gl, dosage=np.zeros(T), gamma_t=np.zeros((K, G), order="F"),
                                    betaHat_t=np.zeros((K, G), order="F"), gammaSmall_cols_to_get=cols)


def _gamma_column(dev, panel, cols):
    """qa_fullpass_reads_select_gamma_batch for chains that want the dosage (and the gamma column) only."""
    from quilt_amd.driver import HipBackend
    from quilt_amd.synth import make_synthetic_sample
    rng = np.random.default_rng(5)
    samples = [make_synthetic_sample(panel, seed=800 + i, n_reads=120) for i in range(2)]
    cs = [0, 1, 0]
    labels = [rng.integers(1, 3, size=samples[s].nReads).astype(np.int32) for s in cs]
    which = [np.sort(rng.choice(panel.K, 64, replace=False) + 1).astype(np.int32) for _ in cs]
    sel = dict(Ksubset=64, Knew=32, which=which, seeds=[11, 12, 13])
    HipBackend(dev).fullpass_reads_batch(samples, cs, labels, [1] * 3, [0] * 3, cols, 5, 1e-10, 8, select=sel, gamma_grid=panel.nGrids // 2)


# kind -> (dosage bits, reference-order sums), and its request shapes: (what, ranking bits, call)
_DOSAGE = ("dosage", 64, lambda d, p, c: _batch(d, p, c, 1, 0))
_LISTS64 = ("thinned lists", 64, lambda d, p, c: _batch(d, p, c, 0, 5))
_LISTS32 = ("thinned lists", 32, lambda d, p, c: _batch(d, p, c, 0, 5))
_BOTH32 = ("dosage and lists", 32, lambda d, p, c: _batch(d, p, c, 1, 5))
_MATRICES32 = ("gamma and beta matrices", 32, _matrices)
_GAMMA_COL = ("gamma column", 64, _gamma_column)
_CASES = {
    KIND_F32: ((32, 0), [_DOSAGE, _LISTS32, _BOTH32, _MATRICES32]),
    KIND_F64_RANK: ((32, 0), [_LISTS64]),
    KIND_F64_DOS: ((64, 0), [_DOSAGE, _GAMMA_COL]),
    KIND_F64_FULL: ((64, 0), [_LISTS32, _BOTH32, _MATRICES32]),
    KIND_F64_REF: ((64, 1), [_DOSAGE, _LISTS64, _BOTH32, _MATRICES32, _GAMMA_COL]),
}


@pytest.mark.parametrize("kind", sorted(_CASES))
@pytest.mark.parametrize("which_panel", ["small", "two_rows"])
def test_plan_is_what_is_carved(kind, which_panel, small_panel, two_row_panel):
    """Every kind of kernels, every request shape it accepts: the launch set carves no more than the plan allows, and the plan
    exceeds the carve by no more than its fixed term plus one carve alignment per buffer and pass (the plan rounds every buffer
    of every pass; the carve rounds every buffer once)."""
    from quilt_amd.driver import thinned_grid_columns
    from quilt_amd.native import DevicePanel
    panel = small_panel if which_panel == "small" else two_row_panel
    cols = np.ascontiguousarray(thinned_grid_columns(panel.nGrids, 0.25), dtype=np.int32)
    assert (cols >= 0).sum() >= 2
    align = _carve_align()
    (bits, ref_order), shapes = _CASES[kind]
    dev = DevicePanel(panel)
    try:
        dev.set_dosage_precision(bits)
        dev.set_sum_order(ref_order)
        for what, rank_bits, call in shapes:
            dev.set_ranking_precision(rank_bits)
            call(dev, panel, cols)
            h = last_plan()
            print(what, h)
            assert h["kind"] == kind, (what, h)
            assert h["P"] == (1 if call is _matrices else 6 if call is _gamma_column else 3), (what, h)
            plan = h["fixed"] + h["P"] * h["planned"]
            assert h["carved"] <= plan, (what, h)
            assert plan - h["carved"] <= h["fixed"] + align * h["n_buf"] * h["P"], (what, h)
    finally:
        dev.close()


_CUT_SCRIPT = r"""
import ctypes as C, hashlib, sys
sys.path.insert(0, %r)
import numpy as np
from quilt_amd.driver import thinned_grid_columns
from quilt_amd.native import DevicePanel, QA_ERR_CAPACITY, check, lib, ptr
from quilt_amd.synth import make_synthetic_panel
from tests.testhooks import hook_lib
panel = make_synthetic_panel(K=30011, nSNPs=6400, seed=21)
T = panel.nSNPs
cols = np.ascontiguousarray(thinned_grid_columns(panel.nGrids, 0.1), dtype=np.int32)
n_thin = int((cols >= 0).sum())
dev = DevicePanel(panel)
dev.set_dosage_precision(64)
L = hook_lib()
hook = (C.c_int64 * 6)()
rows = np.random.default_rng(7).uniform(0.05, 1.0, size=(5, T, 2))

def run(want, K_top):
    n = len(want)
    gl = np.ascontiguousarray(rows[np.arange(n) %% 5])
    wd = np.ascontiguousarray(want, dtype=np.int32)
    dosage = np.zeros((n, T))
    bptr, cap = np.zeros(n * n_thin + 1, dtype=np.int32), n * n_thin * 16
    for _ in range(2):
        bidx, bval = np.zeros(cap, dtype=np.int32), np.zeros(cap)
        st = L.qa_fullpass_batch(dev.handle, C.c_int32(n), ptr(gl), ptr(wd), ptr(cols), C.c_int32(K_top), ptr(dosage), ptr(bptr),
                                 ptr(bidx), ptr(bval), C.c_int64(cap))
        if st == QA_ERR_CAPACITY:
            cap = int(bptr[-1])
            continue
        check(st)
        break
    check(L.qa_fullpass_last_plan(hook))
    return dosage, bptr, bidx[:bptr[-1]], bval[:bptr[-1]]

run([1], 0)                       # one fp64 dosage pass: its planned bytes
planned = int(hook[1])
free_b, total_b = C.c_size_t(), C.c_size_t()
from quilt_amd import native
hip = C.CDLL(native._soname_in(native.LIB_PATH, b"libamdhip64").decode())   # (the runtime the library already runs on)
assert hip.hipMemGetInfo(C.byref(free_b), C.byref(total_b)) == 0
n_pass = int(1.5 * 0.1 * total_b.value / planned) + 2
# dosage and list-only passes in turn: single passes, a run of list-only passes, then the run of dosage passes that memory cuts
want = [1, 0] * 8 + [0] * 64 + [1] * (n_pass - 80)
out = run(want, 5)
h = hashlib.sha256()
for a in out:
    h.update(np.ascontiguousarray(a).tobytes())
print("RESULT", h.hexdigest(), n_pass, int(hook[0]), planned)
dev.close()
"""


def test_launch_sets_cut_by_memory_give_the_same_results():
    """qa_fullpass_batch in fp64-dosage mode, dosage and list-only passes, more of them than a tenth of the device holds at once
    (planned bytes of a dosage pass x passes > 1.5 x 0.1 x the device's memory): with the arena at 10 % of the device the planner
    cuts the call into several launch sets, at the default it does not; the dosage rows and the packed lists are the same bytes."""
    out = {}
    for frac in ("0.1", None):
        env = dict(os.environ)
        env.pop("QA_ARENA_FRACTION", None)
        if frac:
            env["QA_ARENA_FRACTION"] = frac
        r = subprocess.run([sys.executable, "-c", _CUT_SCRIPT % ROOT], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        f = [l for l in r.stdout.splitlines() if l.startswith("RESULT")][0].split()
        out[frac] = dict(digest=f[1], n_pass=int(f[2]), last_P=int(f[3]), planned=int(f[4]))
        print(frac, out[frac])
    assert out["0.1"]["last_P"] < out["0.1"]["n_pass"], out
    assert out["0.1"]["last_P"] < out[None]["last_P"] == out[None]["n_pass"] - 80, out
    assert out["0.1"]["digest"] == out[None]["digest"], out
