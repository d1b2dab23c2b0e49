"""Developer aid: what hla_run costs the range call.  An HLA-shaped run -- K = 5 008 haplotypes (1000 Genomes-like), a few hundred
grids, 1x short reads, 128 samples -- through qa_impute_samples and qa_impute_samples_hla alternately in one process, same inputs;
prints one JSON line (and writes it to the path given as the first argument, if any).

    python scripts/perf_hla.py --from-bam [OUT.json]
the same shape FROM BAM FILES: the compute-only leg (qa_impute_samples_hla on reads already in memory -- the files' own reads, loaded
beforehand) alternated in one process with qa_impute_bam_range_ex(hla_grid) on the files (native loader beside the imputation,
columns and counts formatted).  Default output: profiles/hla_from_bam.json."""
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


def from_bam(out_path):
    import tempfile
    from quilt_amd.impute import impute_bam_range
    from quilt_amd.io import loadBamAndConvert
    from quilt_amd.synth import synthetic_alleles, write_synthetic_bam
    ref, alt = synthetic_alleles(panel.nSNPs, 1)
    d = tempfile.mkdtemp(prefix="qa_hla_")
    files = []
    for i in range(N_SAMPLES):
        files.append(os.path.join(d, f"s{i}.bam"))
        write_synthetic_bam(files[-1], make_synthetic_sample(panel, seed=7000 + i), panel.L, ref, alt, seed=i)
    opts = dict(downsampleToCov=0, bqFilter=1)
    grid_of = panel.grid if panel.grid is not None else np.arange(panel.nSNPs, dtype=np.int32) // 32
    loaded = [loadBamAndConvert(f, "chr20", panel.L, ref, alt, grid_of, **opts) for f in files]
    grid = int(np.round(panel.nGrids / 2)) - 1
    prm = HlaDriverParams(seed=5, hla_grid=grid)
    dev = DevicePanel(panel)
    dev.set_dosage_precision(64)
    impute_samples([dev], loaded[:4], prm)   # warm-up
    times = {"compute_only": [], "from_bam": []}
    same = True
    for rep in range(REPS):
        t0 = time.perf_counter()
        mem = impute_samples([dev], loaded, prm)
        times["compute_only"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        rng = impute_bam_range([dev], files, "chr20", ref, alt, DriverParams(seed=5), hla_grid=grid, discard_sample_arrays=True, **opts)
        times["from_bam"].append(time.perf_counter() - t0)
        same = same and all(rng["imputed"]) and all(np.array_equal(rng["results"][i].gamma_total, mem[i].gamma_total) and
                                                    np.array_equal(rng["results"][i].gamma1, mem[i].gamma1) for i in range(N_SAMPLES))
    dev.close()
    best = {k: min(v) for k, v in times.items()}
    line = dict(what="HLA-shaped run from BAM files: qa_impute_samples_hla on reads in memory vs qa_impute_bam_range_ex(hla_grid) on "
                     "the files, alternated in one process (wall time of the Python call, copies of the results included)",
                K=panel.K, nGrids=panel.nGrids, nSNPs=N_SNPS, samples=N_SAMPLES, reads_per_sample=int(np.mean([s.nReads for s in loaded])),
                grid=grid, seconds_compute_only=[round(x, 3) for x in times["compute_only"]],
                seconds_from_bam=[round(x, 3) for x in times["from_bam"]],
                samples_per_s_compute_only=round(N_SAMPLES / best["compute_only"], 2),
                samples_per_s_from_bam=round(N_SAMPLES / best["from_bam"], 2),
                from_bam_over_compute_only=round(best["compute_only"] / best["from_bam"], 4), gammas_identical=bool(same),
                cpus=os.cpu_count())
    print(json.dumps(line), flush=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(line) + "\n")


if len(sys.argv) > 1 and sys.argv[1] == "--from-bam":
    from_bam(sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                                "hla_from_bam.json"))
    sys.exit(0)
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
