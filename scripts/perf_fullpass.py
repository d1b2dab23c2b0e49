"""Developer aid: time the full-panel pass kernels at a given (K, nSNPs, P) on the GPU."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quilt_amd.native import DevicePanel, check, last_fullpass_timing_ms, lib, ptr  # noqa: E402
from quilt_amd.synth import make_synthetic_panel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--K", type=int, default=50000)
ap.add_argument("--T", type=int, default=64000)
ap.add_argument("--P", type=int, default=256)
ap.add_argument("--thin-frac", type=float, default=0.0, help="fraction of thin passes")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--ktop", type=int, default=5)
ap.add_argument("--fp64", action="store_true", help="dosage passes with fp64 state (k_fwd64 + k_bwd64d)")
ap.add_argument("--driver", action="store_true", help="time the driver path (qa_fullpass_reads_batch: fused top-K)")
ap.add_argument("--sum-order-batched", action="store_true",
                help="reference-order sums (qa_panel_set_sum_order 1): alternate the validation kernels and the batched ones "
                     "(qa_panel_set_sum_order_batched) in this process on the same inputs, for launch sets of --sets passes with "
                     "dosage and with ranking flags; passes/s of each, written to --json")
ap.add_argument("--validation-large-k", action="store_true",
                help="validation mode beyond 57 344 haplotypes: K = 64 976 x 500 grids (the HRC-sized shape; overrides --K / --T), "
                     "launch sets of --sets ranking passes and dosage passes in production mode (fp64 dosage), validation mode "
                     "(qa_panel_set_sum_order 1) and validation mode with the batched form, in this process on the same inputs; "
                     "passes/s of each, written to --json")
ap.add_argument("--sets", type=int, nargs="+", default=None, help="default: 256 1024 (--validation-large-k: 256)")
ap.add_argument("--json", default=None, help="default: profiles/sum_order_batched.json (--validation-large-k: "
                                             "profiles/validation_large_k.json)")
a = ap.parse_args()
PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
if a.validation_large_k:
    a.K, a.T = 64976, 16000
    a.sets = a.sets or [256]
    a.json = a.json or os.path.join(PROFILES, "validation_large_k.json")
a.sets = a.sets or [256, 1024]
a.json = a.json or os.path.join(PROFILES, "sum_order_batched.json")
if a.sum_order_batched or a.validation_large_k:
    a.P = max(a.sets)

t0 = time.time()
panel = make_synthetic_panel(K=a.K, nSNPs=a.T, seed=4916, keep_rhb_t=True)
print(f"panel built in {time.time() - t0:.1f}s: K={panel.K} G={panel.nGrids}", flush=True)
dev = DevicePanel(panel)
if a.fp64:
    dev.set_dosage_precision(64)
G, T = panel.nGrids, panel.nSNPs
rng = np.random.default_rng(1)
# synthetic gl: ~10 % of SNPs informative per label
gl = np.ones((a.P, T, 2))
for p in range(a.P):
    idx = rng.choice(T, size=T // 10, replace=False)
    ref = rng.random(len(idx)) < 0.7
    e = 10.0 ** (-rng.integers(20, 41, size=len(idx)) / 10.0)
    gl[p, idx, 0] = np.where(ref, 1 - e, e / 3)
    gl[p, idx, 1] = np.where(ref, e / 3, 1 - e)
cols = np.full(G, -1, dtype=np.int32)
w = np.sort(rng.choice(np.arange(1, G), size=max(1, G // 10), replace=False))
cols[w] = np.arange(len(w))
n_thin = len(w)
want = (np.arange(a.P) >= int(a.P * a.thin_frac)).astype(np.int32)
dosage = np.zeros((a.P, T))
bptr = np.zeros(a.P * n_thin + 1, dtype=np.int32)
cap = a.P * n_thin * 64
bidx = np.zeros(cap, dtype=np.int32)
bval = np.zeros(cap)


def sum_order_batched():
    """Old and new form of the reference-order kernels in turn, same process, same inputs, outputs compared."""
    import json
    dev.set_dosage_precision(64)
    dev.set_sum_order(1)
    rows = []
    for n in a.sets:
        for what, flag in (("ranking", 0), ("dosage", 1)):
            wd = np.full(n, flag, dtype=np.int32)
            row = dict(K=panel.K, nGrids=G, passes=n, flags=what)
            outs = {}
            for r in range(a.reps):
                for form, on in (("validation", 0), ("batched", 1)):
                    check(lib().qa_panel_set_sum_order_batched(dev.handle, C.c_int32(on)))
                    t0 = time.time()
                    check(lib().qa_fullpass_batch(dev.handle, C.c_int32(n), ptr(gl), ptr(wd), ptr(cols), C.c_int32(a.ktop),
                                                  ptr(dosage), ptr(bptr), ptr(bidx), ptr(bval), C.c_int64(cap)))
                    wall = time.time() - t0
                    tm = last_fullpass_timing_ms()
                    outs[form] = (dosage[:n].copy() if flag else None, bptr[:n * n_thin + 1].copy(), bidx[:bptr[n * n_thin]].copy(),
                                  bval[:bptr[n * n_thin]].copy())
                    best = row.get(form + "_wall_s")
                    if best is None or wall < best:
                        row[form + "_wall_s"] = wall
                        row[form + "_passes_per_s"] = n / wall
                        row[form + "_last_launch_set_fwd_bwd_ms"] = [tm["forward"], tm["backward"]]
                    print(f"P={n} {what} rep {r} {form}: wall {wall:.3f}s = {n / wall:.1f} passes/s  (last launch set: forward "
                          f"{tm['forward']:.1f} ms, backward {tm['backward']:.1f} ms)", flush=True)
            row["outputs_identical"] = all(x is None or np.array_equal(x, y) for x, y in zip(outs["validation"], outs["batched"]))
            row["speedup"] = row["validation_wall_s"] / row["batched_wall_s"]
            rows.append(row)
            print(row, flush=True)
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(dict(what="reference-order full-panel passes: validation kernels (fullpass_ref.hip) against the batched form "
                            "(fullpass_ord.hip), qa_fullpass_batch wall time, best of reps, same process and inputs",
                       reps=a.reps, rows=rows), f, indent=1)
        f.write("\n")


def validation_large_k():
    """Production mode, validation mode and validation mode's batched form in turn, same process, same inputs; the two validation
    forms' outputs compared.  A record, not a bar."""
    import json
    dev.set_dosage_precision(64)
    forms = (("production", 0, 0), ("validation", 1, 0), ("validation_batched", 1, 1))
    rows = []
    for n in a.sets:
        for what, flag in (("ranking", 0), ("dosage", 1)):
            wd = np.full(n, flag, dtype=np.int32)
            row = dict(K=panel.K, nGrids=G, passes=n, flags=what)
            outs = {}
            for r in range(a.reps):
                for form, order, on in forms:
                    dev.set_sum_order(order)
                    check(lib().qa_panel_set_sum_order_batched(dev.handle, C.c_int32(on)))
                    t0 = time.time()
                    check(lib().qa_fullpass_batch(dev.handle, C.c_int32(n), ptr(gl), ptr(wd), ptr(cols), C.c_int32(a.ktop),
                                                  ptr(dosage), ptr(bptr), ptr(bidx), ptr(bval), C.c_int64(cap)))
                    wall = time.time() - t0
                    tm = last_fullpass_timing_ms()
                    outs[form] = (dosage[:n].copy() if flag else None, bptr[:n * n_thin + 1].copy(), bidx[:bptr[n * n_thin]].copy(),
                                  bval[:bptr[n * n_thin]].copy())
                    best = row.get(form + "_wall_s")
                    if best is None or wall < best:
                        row[form + "_wall_s"] = wall
                        row[form + "_passes_per_s"] = n / wall
                        row[form + "_last_launch_set_fwd_bwd_ms"] = [tm["forward"], tm["backward"]]
                    print(f"P={n} {what} rep {r} {form}: wall {wall:.3f}s = {n / wall:.1f} passes/s  (last launch set: forward "
                          f"{tm['forward']:.1f} ms, backward {tm['backward']:.1f} ms)", flush=True)
            row["outputs_identical"] = all(x is None or np.array_equal(x, y)
                                           for x, y in zip(outs["validation"], outs["validation_batched"]))
            row["production_over_validation"] = row["validation_wall_s"] / row["production_wall_s"]
            if flag:
                row["production_dosage_max_abs_diff"] = float(np.abs(outs["production"][0] - outs["validation"][0]).max())
            rows.append(row)
            print(row, flush=True)
    check(lib().qa_panel_set_sum_order_batched(dev.handle, C.c_int32(0)))
    os.makedirs(os.path.dirname(a.json), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(dict(what="full-panel passes beyond 57 344 haplotypes: production mode (fp64 dosage and ranking kernels), "
                            "validation mode (fullpass_ref.hip) and its batched form (fullpass_ord.hip), qa_fullpass_batch wall time, "
                            "best of reps, same process and inputs; outputs_identical: the two validation forms",
                       reps=a.reps, rows=rows), f, indent=1)
        f.write("\n")


if a.sum_order_batched:
    sum_order_batched()
    sys.exit(0)
if a.validation_large_k:
    validation_large_k()
    sys.exit(0)
NAMES = [lib().qa_profile_name(C.c_int32(k)).decode() for k in range(lib().qa_profile_count())]
for r in range(a.reps):
    t0 = time.time()
    lib().qa_profile_reset()
    check(lib().qa_fullpass_batch(dev.handle, C.c_int32(a.P), ptr(gl), ptr(want), ptr(cols), C.c_int32(a.ktop),
                                  ptr(dosage), ptr(bptr), ptr(bidx), ptr(bval), C.c_int64(cap)))
    wall = time.time() - t0
    tm = last_fullpass_timing_ms()
    nd = int(want.sum()); nt = a.P - nd
    alg = (nd * 10.0 + nt * 2.8) * panel.K * G
    line = []
    for k, nm in enumerate(NAMES):
        ms, n, b = C.c_double(), C.c_int64(), C.c_double()
        lib().qa_profile_get(C.c_int32(k), C.byref(ms), C.byref(n), C.byref(b))
        if n.value:
            line.append(f"{nm} {ms.value:.1f} ms ({b.value / 1e6 / max(ms.value, 1e-9):.0f} GB/s)")
    print(f"rep {r}: wall {wall:.3f}s  " + "  ".join(line), flush=True)
print("dosage range", dosage[want == 1].min() if want.any() else None, dosage.max())
