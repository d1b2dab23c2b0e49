"""The native BAM loader's host time.

Default: how it scales with host threads on the GPU box -- qa_impute_bam_range with a minimum read count nobody meets runs its
load phase only.
    python scripts/perf_bam_load.py [--use-bx-tag]

--alternate PARENT_LIB: no device.  The per-file time of qa_bam_load_sample_reads on untagged files of the headline shape (20 000
reads per file), three ways ALTERNATED in one process: (a) a build of an earlier commit's loader (PARENT_LIB: any shared object
that exports qa_bam_load_sample_reads, e.g. that commit's libquilt_amd.so), (b) this tree's loader with the BX rule off, (c) with
it on (--use-bx-tag; what a QUILT run with default arguments now asks for; a PARENT_LIB that has the rule is timed with it on as
well).  Each round times every file once per way, one
thread; the result (medians over the rounds, and the spread between rounds) goes to --out as JSON.
    python scripts/perf_bam_load.py --alternate /path/to/parent/libquilt_amd.so --use-bx-tag --out profiles/bx_loader.json

--names: no device.  The same files through this tree's loader with read names kept (qa_bam_load_sample_reads_named, what
output_read_label_prob asks for) and without, ALTERNATED file by file, one thread; names exported in the timed region.
    python scripts/perf_bam_load.py --names --out profiles/read_label_names.json
"""
import argparse, ctypes as C, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multiprocessing as mp
import numpy as np
from quilt_amd.synth import make_synthetic_panel, make_synthetic_sample, synthetic_alleles, write_synthetic_bam

ap = argparse.ArgumentParser()
ap.add_argument("--use-bx-tag", action="store_true", help="load with use_bx_tag = TRUE (bxTagUpperLimit 50000)")
ap.add_argument("--alternate", metavar="PARENT_LIB", help="compare with an earlier build's loader, alternated; no device")
ap.add_argument("--names", action="store_true", help="names on / off, alternated; no device")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

N = int(os.environ.get("N_FILES", "16" if (args.alternate or args.names) else "512"))
panel = make_synthetic_panel(K=2000, nSNPs=64000, seed=4916)
ref, alt = synthetic_alleles(panel.nSNPs, 1)
d = tempfile.mkdtemp(prefix="qa_load_")


def mk(i):
    s = make_synthetic_sample(panel, seed=i, n_reads=20000)
    write_synthetic_bam(os.path.join(d, f"s{i}.bam"), s, panel.L, ref, alt, seed=i)
    return i


with mp.get_context("fork").Pool(min(32, N, os.cpu_count() or 1)) as pool:
    pool.map(mk, range(N), chunksize=4)
files = [os.path.join(d, f"s{i}.bam") for i in range(N)]
print("files", N, "bytes each", os.path.getsize(files[0]))

if args.names:
    from quilt_amd.io import loadBamAndConvert
    grid = np.arange(panel.nSNPs, dtype=np.int32) // 32
    ways = [("names_off", False), ("names_on", True)]

    def load(path, names):
        t = time.perf_counter()
        r = loadBamAndConvert(path, "chr20", panel.L, ref, alt, grid, bqFilter=1, downsampleToCov=0, use_bx_tag=args.use_bx_tag,
                              return_names=names)
        t = time.perf_counter() - t
        s_, nm = r if names else (r, None)
        assert nm is None or len(nm) == s_.nReads
        return t, s_.nReads

    for _, nm in ways:
        load(files[0], nm)
    per_round = {w: [] for w, _ in ways}
    for r in range(args.rounds):
        tot = {w: 0.0 for w, _ in ways}
        for f in files:
            counts = set()
            for w, nm in ways:
                t, n = load(f, nm)
                tot[w] += t
                counts.add(n)
            assert len(counts) == 1
        for w in tot:
            per_round[w].append(1e3 * tot[w] / N)
        print("round", r, {w: round(v[-1], 3) for w, v in per_round.items()})
    med = {w: float(np.median(v)) for w, v in per_round.items()}
    res = dict(what="loadBamAndConvert per file with and without read names (qa_bam_load_sample_reads_named), one thread, files of "
                    "20 000 reads over 64 000 SNPs, export included; ms", n_files=N, rounds=args.rounds, use_bx_tag=bool(args.use_bx_tag),
               bytes_per_file=os.path.getsize(files[0]), ms_per_file_by_round=per_round, ms_per_file_median=med,
               spread_between_rounds={w: float((max(v) - min(v)) / np.median(v)) for w, v in per_round.items()},
               names_on_over_off=med["names_on"] / med["names_off"], cpus=os.cpu_count())
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)

if args.alternate:
    from quilt_amd.io import BamOpts
    from quilt_amd.native import lib, ptr
    here, parent = lib(), C.CDLL(os.path.abspath(args.alternate))
    Lc = np.ascontiguousarray(panel.L, dtype=np.int32)
    grid = np.ascontiguousarray(np.arange(panel.nSNPs) // 32, dtype=np.int32)
    o = BamOpts(1, 1000000, 0, 0, 0, 0, 1, 1)   # (bqFilter 1, no cap: the options of the headline's load)

    def load(L_, path, bx):
        h = C.c_void_p()
        a = (path.encode(), b"chr20", C.c_int32(panel.nSNPs), ptr(Lc), ref.encode(), alt.encode(), ptr(grid), C.byref(o))
        t = time.perf_counter()
        st = L_.qa_bam_load_sample_reads(*a, C.byref(h)) if bx is None else \
            L_.qa_bam_load_sample_reads_bx(*a, C.c_int32(bx), C.c_int32(50000), C.byref(h))
        t = time.perf_counter() - t
        assert st == 0
        n = L_.qa_sample_reads_n_reads(h)
        L_.qa_sample_reads_destroy(h)
        return t, n

    ways = [("parent", parent, None), ("tag_off", here, 0)] + ([("tag_on", here, 1)] if args.use_bx_tag else [])
    if args.use_bx_tag and hasattr(parent, "qa_bam_load_sample_reads_bx"):   # (a parent that has the rule: its own time with the tag on)
        ways.insert(1, ("parent_tag_on", parent, 1))
    for _, L_, bx in ways:   # (warm-up: page cache, allocator)
        load(L_, files[0], bx)
    per_round = {w: [] for w, _, _ in ways}
    for r in range(args.rounds):
        tot, reads = {w: 0.0 for w, _, _ in ways}, {}
        for f in files:   # alternated file by file: every way sees the machine in the same state
            for w, L_, bx in ways:
                t, n = load(L_, f, bx)
                tot[w] += t
                reads.setdefault(f, set()).add(n)
        assert all(len(v) == 1 for v in reads.values()), "the ways disagree on a file's read count"
        for w in tot:
            per_round[w].append(1e3 * tot[w] / N)
        print("round", r, {w: round(v[-1], 3) for w, v in per_round.items()})
    med = {w: float(np.median(v)) for w, v in per_round.items()}
    res = dict(what="qa_bam_load_sample_reads per file, one thread, untagged files of 20 000 reads over 64 000 SNPs; ms",
               n_files=N, rounds=args.rounds, bytes_per_file=os.path.getsize(files[0]), ms_per_file_by_round=per_round,
               ms_per_file_median=med,
               spread_between_rounds={w: float((max(v) - min(v)) / np.median(v)) for w, v in per_round.items()},
               tag_off_over_parent=med["tag_off"] / med["parent"],
               tag_on_over_parent=(med["tag_on"] / med["parent"]) if "tag_on" in med else None,
               tag_on_over_parent_tag_on=(med["tag_on"] / med["parent_tag_on"]) if "parent_tag_on" in med else None, cpus=os.cpu_count())
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)

from quilt_amd.driver import DriverParams
from quilt_amd.impute import impute_bam_range
from quilt_amd.native import DevicePanel
dev = DevicePanel(panel)
for nt in (1, 8, 16, 32, 64, 128):
    t = time.perf_counter()
    r = impute_bam_range([dev], files, "chr20", ref, alt, DriverParams(), minimum_number_of_sample_reads=10 ** 9, n_io_threads=nt,
                         downsampleToCov=0, bqFilter=1, use_bx_tag=args.use_bx_tag)
    w = time.perf_counter() - t
    print(f"{nt:4d} threads: load {r['seconds']['load']:.3f} s  ({1e3 * r['seconds']['load'] * nt / N:.1f} thread-ms per file), call {w:.3f} s")
dev.close()
