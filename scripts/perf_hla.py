"""Developer aid: what hla_run costs the range call.  An HLA-shaped run -- K = 5 008 haplotypes (1000 Genomes-like), a few hundred
grids, 1x short reads, 128 samples -- through qa_impute_samples and qa_impute_samples_hla alternately in one process, same inputs;
prints one JSON line (and writes it to the path given as the first argument, if any)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from quilt_amd.driver import DriverParams, HlaDriverParams  # noqa: E402
from quilt_amd.impute import impute_samples  # noqa: E402
from quilt_amd.native import DevicePanel  # noqa: E402
from quilt_amd.synth import make_1000g_like_panel, make_synthetic_sample  # noqa: E402

N_SAMPLES, N_SNPS, REPS = 128, 9600, 3
panel = make_1000g_like_panel(K=5008, nSNPs=N_SNPS)
samples = [make_synthetic_sample(panel, seed=7000 + i) for i in range(N_SAMPLES)]
grid = int(np.round(panel.nGrids / 2)) - 1            # iGrid = round(nGrids / 2): gamma_physically_closest_to = NA
common = dict(seed=5)
dev = DevicePanel(panel)
dev.set_dosage_precision(64)
impute_samples([dev], samples[:4], DriverParams(**common))   # warm-up: kernels loaded, buffers grown
times = {"plain": [], "hla": []}
same = True
for rep in range(REPS):
    for name in ("plain", "hla"):
        prm = DriverParams(**common) if name == "plain" else HlaDriverParams(**common, hla_grid=grid)
        t0 = time.perf_counter()
        out = impute_samples([dev], samples, prm)
        times[name].append(time.perf_counter() - t0)
        if name == "plain":
            ref = [r.dosage.copy() for r in out]
        else:
            same = same and all(np.array_equal(a.dosage, b) for a, b in zip(out, ref))
dev.close()
best = {k: min(v) for k, v in times.items()}
line = dict(what="HLA-shaped run: qa_impute_samples vs qa_impute_samples_hla, alternated", K=panel.K, nGrids=panel.nGrids,
            nSNPs=N_SNPS, samples=N_SAMPLES, reads_per_sample=int(np.mean([s.nReads for s in samples])), grid=grid,
            seconds_plain=[round(x, 3) for x in times["plain"]], seconds_hla=[round(x, 3) for x in times["hla"]],
            samples_per_s_plain=round(N_SAMPLES / best["plain"], 2), samples_per_s_hla=round(N_SAMPLES / best["hla"], 2),
            hla_overhead_fraction=round(best["hla"] / best["plain"] - 1, 4), dosages_identical=bool(same))
print(json.dumps(line), flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(line) + "\n")
