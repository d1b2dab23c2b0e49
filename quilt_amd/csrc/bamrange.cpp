// bamrange.cpp -- qa_impute_bam_range (include/quilt_amd_io.h): a core's sample range from BAM paths to VCF columns in ONE
// native call.  (The product's three entry points over this code are in csrc/bamrange_entry.cpp; this file names no device entry
// point, so tests/c can link it with the loop and the loader alone.)
//
// What it replaces: per sample of the range, get_and_impute_one_sample's own I/O either side of the imputation
// (QUILT/R/functions.R:243-298: STITCH::loadBamAndConvert + load() of the per-sample RData temp file +
// snap_sampleReads_to_grid; :1380-1463: allele counts from the pile-up, eij / fij / max_gen, rcpp_make_column_of_vcf and the
// paste0 assembly of the column) and the range's part of the loop body around it (quilt.R:955-961: the four count arrays
// summed over the samples of the core).  In R these run one sample after the other on the worker that owns the GPU: about a
// sample per second, against the ~40 samples per second the device imputes -- the R loader, not the device, would set the
// throughput a QUILT2.R user sees.  Here
//   1. the BAM files are read by qa_bam_load_sample_reads on n_io_threads host threads (17 ms per 1x sample and thread), in file
//      order and BESIDE the imputation: the first launch set starts as soon as its own files are read;
//   2. the kept samples go through ONE qa_impute_samples call (csrc/impute.cpp) that is handed each sample when the launch set
//      holding it is taken (params->sample_source) -- params->sample_index names every kept sample's GLOBAL index, so a sample
//      dropped for too few reads does not shift the streams of the samples behind it;
//   3. the columns of every finished launch set are formatted by qa_vcf_column_diploid / _nipt on host threads while later sets
//      are on the device (params->on_samples_done), and the four count arrays are summed over the imputed samples in sample
//      order (the order of the reference's loop: floating-point sums).
// Host code only: no HIP here (the device work is inside qa_impute_samples).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <sys/mman.h>
#include <unistd.h>

#include "../../include/quilt_amd.h"
#include "../../include/quilt_amd_io.h"
#include "impute_testhook.h"   // (qa_impute_bam_range_backend: the same host code over a checker's entry points, for tests/)

#include "bamrange_impl.hpp"

namespace qa { void set_error(const char *fmt, ...); }

// The imputation's result arrays: 48 bytes per sample and SNP (7.9 GB at 2 560 samples x 64 000 SNPs).  qa_impute_samples does not
// ask for them zeroed (it zeroes a launch set's rows itself, on the thread that takes the set), so they are allocated WITHOUT a
// fill: std::vector's zero fill touched every page on the calling thread before the first launch -- 2.4 s of the 70 s job.
struct RawDoubles {
    std::unique_ptr<double[]> p;
    void alloc(size_t n) { p.reset(new double[std::max<size_t>(n, 1)]); }
    double *data() const { return p.get(); }
};

struct qa_bam_range_result {
    int n = 0, n_kept = 0, T_out = 0, nL = 2;
    bool nipt = false, discarded = false;
    std::vector<uint8_t> imputed;        // per file
    std::vector<int32_t> n_reads;        // per file: reads the loader returned (before the minimum test)
    std::vector<int32_t> slot;           // per file: index among the kept samples, or -1
    std::vector<int32_t> kept;           // per kept sample: its file
    std::vector<std::vector<int32_t>> labels_of;   // per kept sample: its reads' consensus labels
    std::vector<int32_t> nDosage;
    RawDoubles dosage, gp_t, haps, fet_dosage, fet_gp_t;            // kept-major, the layouts of qa_impute_samples
    std::vector<std::vector<char>> col_buf;
    std::vector<std::vector<int64_t>> col_off;
    std::vector<double> infoCount, afCount, hweCount, alleleCount;
    double seconds[4] = {0, 0, 0, 0};    // load, impute (the columns of finished launch sets are formatted beside it), what is left of formatting + counts, whole call
    double format_busy_s = 0;            // thread-seconds spent formatting (most of them inside seconds[1])
    int64_t stats[11] = {0};
    int64_t load_stats[8] = {0};         // the loader's counters summed over the files (qa_sample_reads_stats)
    int64_t bx_stats[4] = {0};           // the BX rule's counters summed over the files (qa_sample_reads_bx_stats)
    // output_read_label_prob: per kept sample its reads' names (NUL-terminated, back to back, n + 1 offsets) and label confidences
    bool with_prob = false;
    std::vector<std::vector<char>> names_buf;
    std::vector<std::vector<int64_t>> names_off;
    std::vector<std::vector<double>> prob_of;
    // hla_grid >= 0: kept-major gamma1 / gamma2 / gamma_total (K per sample) and list_of_gammas (nG x 2 x K per sample)
    bool with_hla = false;
    int K = 0, nG = 0;
    RawDoubles gamma1, gamma2, gamma_total, list_of_gammas;
};

namespace {

using Clock = std::chrono::steady_clock;
double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// The entry's arguments and, once check_range_request has passed them, what they resolve to (resolve()).  Read-only from then on:
// every part below holds a reference to it, on whatever thread.
struct RangeCall {
    const qa_impute_params_t *params; const qa_bam_range_io_t *io; const qa_bam_range_extras_t *ex;
    int32_t K, G, n_sample;   // K, G: the panel's haplotypes and grids (read with ex->hla_grid >= 0 only)
    const char *const *bam_paths; const int64_t *sample_index; const double *ff;
    bool rare = false, nipt = false, want_prob = false, want_hla = false;
    int T = 0, T_out = 0, nL = 2, min_reads = 1, n_io = 1;
    void resolve() {
        rare = params->rare_common != nullptr; nipt = params->nipt != nullptr;
        want_prob = ex->output_read_label_prob != 0; want_hla = ex->hla_grid >= 0;
        T = io->nSNPs; T_out = rare ? io->nSNPs_all : T; nL = nipt ? 3 : 2;
        min_reads = io->minimum_number_of_sample_reads > 0 ? io->minimum_number_of_sample_reads : 1;   // (an empty sample cannot be imputed)
        // host threads of the loading and of the formatting (each): 16 by default.  Measured at 2 560 files on a 128-core host, both ends
        // beside the imputation: 16 / 32 / 64 threads -> the last file is in after 3.1 / 2.9 / 3.0 s either way (the loading does not
        // scale past 16), the formatters' busy time is 11.5 / 14.6 / 30.3 thread-seconds (they get in each other's way), and the
        // imputation itself takes 61.4 / 61.8 / 63.2 s (they get in ITS host threads' way): 40.3 / 40.0 / 39.2 samples/s.
        n_io = io->n_io_threads > 0 ? io->n_io_threads : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    }
};

template <class... A> int invalid(const char *fmt, A... a) { qa::set_error(fmt, a...); return (int)QA_ERR_INVALID; }

// Every refusal of the call, the first that applies: before any file is opened, any memory taken or any thread started.
int check_range_request(const RangeCall &c, bool has_out) {
    const auto *params = c.params; const auto *io = c.io; const auto *ex = c.ex;
    if (!ex) return invalid("qa_impute_bam_range_ex: ex is NULL");
    if (ex->hla_grid < -1) return invalid("qa_impute_bam_range_ex: hla_grid = %d (-1 is off, a grid is 0-based)", (int)ex->hla_grid);
    if (ex->bxTagUpperLimit < 0) return invalid("qa_impute_bam_range: bxTagUpperLimit = %d is negative", (int)ex->bxTagUpperLimit);
    if (!params || !io || c.n_sample < 0 || (c.n_sample > 0 && (!c.bam_paths || !c.sample_index)) || !has_out ||
        !io->chr || io->nSNPs < 1 || !io->L || !io->ref || !io->alt || !io->grid)
        return invalid("qa_impute_bam_range: missing argument");
    const bool rare = params->rare_common != nullptr, nipt = params->nipt != nullptr;
    if (rare && (io->nSNPs_all < io->nSNPs || !io->L_all || !io->ref_all || !io->alt_all || !io->grid_all ||
                 params->rare_common->nSNPs_all != io->nSNPs_all))
        return invalid("qa_impute_bam_range: impute_rare_common needs the all-SNP sites (L_all, ref_all, alt_all, grid_all; nSNPs_all as in "
                       "params->rare_common)");
    if (nipt && c.n_sample > 0 && !c.ff) return invalid("qa_impute_bam_range: method = \"nipt\" needs one fetal fraction per file");
    for (int i = 0; i < c.n_sample; i++)
        if (!c.bam_paths[i]) return invalid("qa_impute_bam_range: bam_paths[%d] is null", i);
    if (ex->hla_grid >= 0) {   // hla_run: qa_impute_samples_hla's refusals, here, before any file is opened
        int n_seek = params->n_seek_its, n_burn = params->n_burn_in_seek_its < 0 ? params->n_seek_its - 1 : params->n_burn_in_seek_its;
        if (c.K < params->Ksubset) { n_seek = 1; n_burn = 0; }   // (quilt.R:453-471, as the loop resets them)
        const char *why = params->use_mspbwt ? "use_mspbwt = TRUE is not covered (the gamma columns come from the full-panel passes)"
                          : nipt ? "method = \"nipt\" is not covered (diploid only)"
                          : rare ? "impute_rare_common = TRUE is not covered"
                          : ex->hla_grid >= c.G ? "grid outside [0, nGrids)"
                          : n_burn >= n_seek ? "the last seek iteration is not a dosage pass (n_burn_in_seek_its >= n_seek_its)"
                          : params->nGibbsSamples < 1 ? "nGibbsSamples < 1"
                          : nullptr;
        if (why) return invalid("qa_impute_bam_range_ex: hla_grid = %d (nGrids = %d): %s", (int)ex->hla_grid, (int)c.G, why);
    }
    return QA_OK;
}

// The result with every array the call will fill, taken before the first thread exists (a failure here leaves nothing to join).
// The per-sample arrays are sized for every file -- an upper bound of the kept samples; untouched pages of rows that no kept sample
// takes cost nothing.
std::unique_ptr<qa_bam_range_result> allocate_result(const RangeCall &c) {
    const size_t n = (size_t)c.n_sample, T_out = (size_t)c.T_out;
    std::unique_ptr<qa_bam_range_result> R(new qa_bam_range_result);
    R->n = c.n_sample; R->T_out = c.T_out; R->nL = c.nL; R->nipt = c.nipt;
    R->imputed.assign(n, 0); R->n_reads.assign(n, 0); R->slot.assign(n, -1);
    R->infoCount.assign(T_out * 2, 0.0); R->afCount.assign(T_out, 0.0); R->hweCount.assign(T_out * 3, 0.0); R->alleleCount.assign(T_out * 2, 0.0);
    R->with_prob = c.want_prob;
    if (c.want_prob) { R->names_buf.resize(n); R->names_off.resize(n); R->prob_of.resize(n); }
    R->kept.assign(n, -1);   // (entry j is written before kept sample j is handed to anyone; cut to n_kept at the end)
    R->labels_of.resize(n);
    if (c.want_hla) {
        R->with_hla = true; R->K = c.K; R->nG = c.params->nGibbsSamples;
        R->gamma1.alloc(n * c.K); R->gamma2.alloc(n * c.K); R->gamma_total.alloc(n * c.K);
        R->list_of_gammas.alloc(n * R->nG * 2 * c.K);
    }
    R->dosage.alloc(n * T_out); R->gp_t.alloc(n * 3 * T_out); R->haps.alloc(n * c.nL * T_out);
    R->nDosage.assign(std::max<size_t>(n, 1), 0);
    if (c.nipt) { R->fet_dosage.alloc(n * T_out); R->fet_gp_t.alloc(n * 3 * T_out); }
    R->col_buf.resize(n); R->col_off.resize(n);
    R->discarded = c.io->discard_sample_arrays != 0;
    return R;
}

struct Loaded {
    std::vector<int32_t> read_ptr, u, bq, wif;
    int32_t R = 0;
    std::vector<char> names;          // (keep_names only)
    std::vector<int64_t> names_off;
    int64_t stats[8] = {0}, bx_stats[4] = {0};   // the loader's counters for this file
};

// The sites a file is piled up against: the common SNPs, and with impute_rare_common all SNPs.
struct Sites { int32_t T; const int32_t *L; const char *ref, *alt; const int32_t *grid; };

// ---- 1. the reads of every file (functions.R:251-298; with impute_rare_common also over all SNPs, :132-172), on host threads
// BESIDE the imputation, which is handed each sample when the launch set holding it is taken (qa_sample_source_t) -- as the
// reference's loop reads a sample's BAM at the top of its own iteration.  Whether a file is imputed (functions.R:274-287) is known
// once it is loaded; the kept samples are numbered in file order as the files before them are settled.
//
// Threads: body() runs on the loader's own threads (started by start(), joined by stop_and_join() and by the destructor);
// acquire() and prob_dest() are called by qa_impute_samples' host threads; the calling thread makes the object, starts and joins it,
// and reads status / err / n_kept / done_s after the join.  pileup() and release() are the formatters', for a sample that was acquired.
// mu guards loaded, settled, n_kept, status, err, done_s and whatever settle_in_order() writes -- index, ffk and the result's
// n_reads / load_stats / bx_stats / slot / imputed / kept / labels_of / names / prob_of.  Kept sample j's entries are written before
// n_kept passes j; acquire(j) reads n_kept under mu, so whoever is handed sample j sees them.  common[f] / all_snps[f]
// are written by the one thread that loads file f, before it marks f loaded under mu.
struct FileLoader {
    const RangeCall &c;
    qa_bam_range_result &R;
    const Clock::time_point t0;
    const Sites sites, sites_all;
    std::vector<Loaded> common, all_snps;
    std::vector<int64_t> index;   // per kept sample: its global index (params->sample_index of the imputation)
    std::vector<double> ffk;      // per kept sample: its fetal fraction
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint8_t> loaded;
    int settled = 0;              // files [0, settled) are loaded and sorted into kept / dropped
    int n_kept = 0;
    int status = QA_OK;
    std::string err;
    double done_s = 0;            // when the last file was settled, from t0
    std::atomic<int> next{0};
    std::atomic<bool> stop{false};
    std::vector<std::thread> threads;

    FileLoader(const RangeCall &c_, qa_bam_range_result &R_, Clock::time_point t0_)
        : c(c_), R(R_), t0(t0_), sites{c_.io->nSNPs, c_.io->L, c_.io->ref, c_.io->alt, c_.io->grid},
          sites_all{c_.io->nSNPs_all, c_.io->L_all, c_.io->ref_all, c_.io->alt_all, c_.io->grid_all},
          common((size_t)c_.n_sample), all_snps(c_.rare ? (size_t)c_.n_sample : 0),
          index((size_t)std::max(c_.n_sample, 1)), ffk((size_t)std::max(c_.n_sample, 1)), loaded((size_t)c_.n_sample, 0) {}
    ~FileLoader() { stop_and_join(); }

    void start() {
        const int W = std::max(1, std::min(c.n_io, c.n_sample));
        threads.reserve((size_t)W);
        for (int w = 0; w < W; w++) threads.emplace_back(&FileLoader::body, this);
    }
    void stop_and_join() {   // (files being read are finished and settled; no other is begun)
        stop.store(true);
        for (auto &t : threads) t.join();
        threads.clear();
    }

    int load_one(const char *path, const Sites &s, bool keep_names, Loaded &out, std::string &e) const {
        qa_sample_reads_t *h = nullptr;
        const int st = qa_bam_load_sample_reads_named(path, c.io->chr, s.T, s.L, s.ref, s.alt, s.grid, &c.io->bam, c.ex->use_bx_tag,
                                                      c.ex->bxTagUpperLimit, keep_names ? 1 : 0, &h);
        if (st != QA_OK) { e = std::string("cannot load ") + path + ": " + qa_last_error(); return st; }
        out.R = qa_sample_reads_n_reads(h);
        const int64_t nb = qa_sample_reads_n_bases(h);
        out.read_ptr.assign((size_t)out.R + 1, 0); out.u.resize((size_t)nb); out.bq.resize((size_t)nb); out.wif.resize((size_t)out.R);
        int32_t dummy = 0;   // (export wants non-null pointers only for what it writes; empty vectors have a null data())
        const int st2 = qa_sample_reads_export(h, out.read_ptr.data(), nb ? out.u.data() : &dummy, nb ? out.bq.data() : &dummy,
                                               out.R ? out.wif.data() : &dummy, nullptr);
        int st3 = QA_OK;
        if (keep_names) {
            out.names.resize((size_t)std::max<int64_t>(qa_sample_reads_names_bytes(h), 0));
            out.names_off.assign((size_t)out.R + 1, 0);
            st3 = qa_sample_reads_export_names(h, out.names.data(), out.names_off.data());
        }
        qa_sample_reads_stats(h, out.stats);
        qa_sample_reads_bx_stats(h, out.bx_stats);
        qa_sample_reads_destroy(h);
        if (st3 != QA_OK) { e = std::string("cannot export the read names of ") + path; return st3; }
        if (st2 != QA_OK) e = std::string("cannot export the reads of ") + path;
        return st2;
    }

    void body() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= c.n_sample || stop.load()) return;
            std::string e;
            int s1;
            try {
                s1 = load_one(c.bam_paths[i], sites, c.want_prob, common[(size_t)i], e);
                // (the all-SNP pile-up only for samples that will be imputed: the minimum test is on the common-SNP reads, functions.R:274)
                if (s1 == QA_OK && c.rare && common[(size_t)i].R >= c.min_reads)
                    s1 = load_one(c.bam_paths[i], sites_all, false, all_snps[(size_t)i], e);
            } catch (const std::exception &ex) {
                s1 = QA_ERR_INVALID;
                e = ex.what();
            }
            std::lock_guard<std::mutex> g(mu);
            if (s1 != QA_OK) {   // the first failure is the call's; no further file is begun
                if (status == QA_OK) { status = s1; err = e; }
                stop.store(true);
                cv.notify_all();
                return;
            }
            loaded[(size_t)i] = 1;
            settle_in_order();
            cv.notify_all();
        }
    }

    // (mu held) every file whose predecessors are all loaded: counters summed in file order, kept or dropped, a kept sample's slot
    void settle_in_order() {
        while (settled < c.n_sample && loaded[(size_t)settled]) {
            const int f = settled;
            Loaded &got = common[(size_t)f];
            R.n_reads[(size_t)f] = got.R;
            for (int q = 0; q < 8; q++) R.load_stats[q] += got.stats[q];
            for (int q = 0; q < 4; q++) R.bx_stats[q] += got.bx_stats[q];
            bool keep = got.R >= c.min_reads;
            if (keep && c.rare && all_snps[(size_t)f].R < 1) keep = false;   // (cannot happen: every common SNP is among the all-SNP sites)
            if (keep) {
                const size_t j = (size_t)n_kept;
                index[j] = c.sample_index[f];
                if (c.nipt) ffk[j] = c.ff[f];
                R.labels_of[j].assign((size_t)got.R, 0);
                if (c.want_prob) {   // (the names leave the loaded reads here: those are released when the column is formatted)
                    R.names_buf[j] = std::move(got.names);
                    R.names_off[j] = std::move(got.names_off);
                    R.prob_of[j].assign((size_t)got.R, 0.0);
                }
                R.slot[(size_t)f] = (int32_t)j;
                R.imputed[(size_t)f] = 1;
                R.kept[j] = f;
                n_kept++;
            }
            settled++;
        }
        if (settled == c.n_sample) done_s = since(t0);
    }

    // qa_sample_source_t: kept sample s, once the files before it are settled; the end of the range; or the loaders' failure
    static int acquire(void *ctx, int32_t s, qa_sample_view_t *v) {
        FileLoader &F = *static_cast<FileLoader *>(ctx);
        int f;
        {
            std::unique_lock<std::mutex> lk(F.mu);
            F.cv.wait(lk, [&F, s] { return F.n_kept > s || F.settled == F.c.n_sample || F.status != QA_OK; });
            if (F.status != QA_OK) { qa::set_error("%s", F.err.c_str()); return F.status; }
            if (F.n_kept <= s) return QA_END_OF_SAMPLES;
            f = F.R.kept[(size_t)s];
        }
        const Loaded &c = F.common[(size_t)f];
        static const int32_t none = 0;   // (a read-less base array is never dereferenced; the pointers must not be null)
        v->n_reads = c.R; v->read_ptr = c.read_ptr.data(); v->u = c.u.empty() ? &none : c.u.data(); v->bq = c.bq.empty() ? &none : c.bq.data();
        v->wif = c.wif.data();
        v->read_labels = F.R.labels_of[(size_t)s].data();
        if (F.c.rare) {
            const Loaded &a = F.all_snps[(size_t)f];
            v->n_reads_all = a.R; v->read_ptr_all = a.read_ptr.data(); v->u_all = a.u.empty() ? &none : a.u.data();
            v->bq_all = a.bq.empty() ? &none : a.bq.data(); v->wif_all = a.wif.data();
        }
        return QA_OK;
    }
    // qa_impute_reads_out_t.dest: asked after acquire(s) returned, so kept sample s is settled
    static int prob_dest(void *ctx, int32_t s, double **dst) {
        *dst = static_cast<FileLoader *>(ctx)->R.prob_of[(size_t)s].data();
        return QA_OK;
    }

    // the reads a kept sample's allele counts are taken from (a file that was settled and acquired), and their release
    const Loaded &pileup(int file) const { return c.rare ? all_snps[(size_t)file] : common[(size_t)file]; }
    void release(int file) {
        common[(size_t)file] = Loaded();
        if (c.rare) all_snps[(size_t)file] = Loaded();
    }
};

// The range's sums, per SNP over the samples IN SAMPLE ORDER, as the reference's loop adds them (quilt.R:955-961: floating-point
// sums, so the order is part of the result).  Launch sets finish nearly in order: whichever formatter completes the next sample
// in line adds it -- and every formatted sample behind it -- to the sums and releases its per-SNP vectors, beside the device
// work; nothing is left to sum, and 2 MB per sample less to hand back, when the call ends.
//
// Threads: the formatters.  terms[j] is written by the one formatter of sample j, which then calls add(j).  mu guards formatted, next,
// the result's four count arrays and the reading and release of terms[]; the calling thread reads next after the formatters' join.
struct OrderedSums {
    struct Terms {   // one sample's: eij, fij, the pile-up's allele counts (2 x T_out), max_gen
        std::vector<double> eij, fij, ac;
        std::vector<uint8_t> maxg;
    };
    qa_bam_range_result &R;
    const int n, T_out;
    std::vector<Terms> terms;
    std::mutex mu;
    std::vector<uint8_t> formatted;
    int next = 0;

    OrderedSums(qa_bam_range_result &R_, int n_) : R(R_), n(n_), T_out(R_.T_out), terms((size_t)n_), formatted((size_t)n_, 0) {}

    void add(int j_done) {
        std::lock_guard<std::mutex> g(mu);
        formatted[(size_t)j_done] = 1;
        double *i0 = R.infoCount.data(), *i1 = i0 + T_out, *af = R.afCount.data(), *hw = R.hweCount.data();
        double *a0 = R.alleleCount.data(), *a1 = a0 + T_out;
        while (next < n && formatted[(size_t)next]) {
            Terms &s = terms[(size_t)next++];
            const double *E = s.eij.data(), *F = s.fij.data(), *c1 = s.ac.data(), *c2 = c1 + T_out;
            const uint8_t *M = s.maxg.data();
            for (int t = 0; t < T_out; t++) {
                i0[t] += E[t];
                i1[t] += F[t] - E[t] * E[t];
                af[t] += E[t] / 2;
                hw[(size_t)M[t] * T_out + t] += 1;
                a0[t] += c2[t];              // per_sample_alleleCount = cbind(c2, c1 + c2) (functions.R:1398)
                a1[t] += c1[t] + c2[t];
            }
            s = Terms();
        }
    }
};

// [3][T] rows -> 3 x T column-major, as the column writers take it
void rows_to_columns(const double *rows, int T, std::vector<double> &cols) {
    cols.resize((size_t)3 * T);
    for (int t = 0; t < T; t++)
        for (int g = 0; g < 3; g++) cols[(size_t)3 * t + g] = rows[(size_t)g * T + t];
}

// the whole pages inside [p, p + n): their memory goes back to the system now (the addresses stay valid and read as zeros)
void give_back(double *p, size_t n) {
    static const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE);
    const uintptr_t lo = ((uintptr_t)p + page - 1) / page * page, hi = ((uintptr_t)(p + n)) / page * page;
    if (hi > lo) madvise(reinterpret_cast<void *>(lo), hi - lo, MADV_DONTNEED);
}

// ---- 3. (beside 2.) per kept sample: its VCF column (functions.R:1408-1463), eij / fij / max_gen and the pile-up's allele counts
// (:1380-1418).
//
// Threads: the formatters; sample j is formatted once, by one of them, after qa_impute_samples reported it final.  No mutex: it reads
// the result's rows of sample j and the sample's loaded reads, and writes col_buf[j] / col_off[j] and sums.terms[j] -- all sample j's alone.
struct ColumnFormatter {
    const RangeCall &c;
    qa_bam_range_result &R;
    FileLoader &files;
    OrderedSums &sums;

    int format_one(int j, std::string &e) const {
        const int T_out = c.T_out;
        const size_t row = (size_t)j * T_out;
        const double *gp = R.gp_t.data() + 3 * row;          // [3][T_out]
        const double *hd = R.haps.data() + c.nL * row;       // [nL][T_out] == T_out x nL column-major
        std::vector<double> gpc, fgc;
        rows_to_columns(gp, T_out, gpc);
        if (c.nipt) rows_to_columns(R.fet_gp_t.data() + 3 * row, T_out, fgc);
        auto &buf = R.col_buf[(size_t)j];
        auto &off = R.col_off[(size_t)j];
        off.assign((size_t)T_out + 1, 0);
        int64_t need = 0, cap = (int64_t)48 * T_out + 64;
        for (int pass = 0; pass < 2; pass++) {
            buf.assign((size_t)cap, 0);
            const int s1 = c.nipt ? qa_vcf_column_nipt(T_out, gpc.data(), fgc.data(), hd, R.dosage.data() + row, R.fet_dosage.data() + row,
                                                       buf.data(), cap, off.data(), &need)
                                  : qa_vcf_column_diploid(T_out, gpc.data(), hd, c.io->output_gt_phased_genotypes, buf.data(), cap, off.data(), &need);
            if (s1 == QA_ERR_CAPACITY && pass == 0) { cap = need; continue; }
            if (s1 != QA_OK) { e = std::string("VCF column of a sample could not be formatted: ") + qa_last_error(); return s1; }
            break;
        }
        buf.resize((size_t)off[(size_t)T_out]);
        buf.shrink_to_fit();
        // eij, fij (functions.R:1399-1400: round(x, 3)), max_gen (STITCH::get_max_gen_rapid: the first maximum), the pile-up's
        // allele counts (increment2N over STITCH::convertScaledBQtoProbs of the reads as loaded, :1382-1398)
        OrderedSums::Terms &S = sums.terms[(size_t)j];
        S.eij.resize((size_t)T_out); S.fij.resize((size_t)T_out); S.maxg.resize((size_t)T_out); S.ac.assign((size_t)2 * T_out, 0.0);
        for (int t = 0; t < T_out; t++) {
            const double g0 = gp[t], g1 = gp[(size_t)T_out + t], g2 = gp[(size_t)2 * T_out + t];
            S.eij[(size_t)t] = std::nearbyint((g1 + 2 * g2) * 1000.0) / 1000.0;
            S.fij[(size_t)t] = std::nearbyint((g1 + 4 * g2) * 1000.0) / 1000.0;
            S.maxg[(size_t)t] = (uint8_t)((g1 > g0) ? ((g2 > g1) ? 2 : 1) : ((g2 > g0) ? 2 : 0));
        }
        const int file = R.kept[(size_t)j];   // (settled before the sample was handed to the imputation)
        const Loaded &s = files.pileup(file);
        double *c1 = S.ac.data(), *c2 = S.ac.data() + T_out;   // sums of P(ref), P(alt) per site, bases in the order they were loaded
        for (size_t b = 0; b < s.u.size(); b++) {
            const int q = s.bq[b];
            const double eps = std::pow(10.0, -std::fabs((double)q) / 10.0);
            c1[s.u[b]] += q < 0 ? 1 - eps : eps / 3;
            c2[s.u[b]] += q < 0 ? eps / 3 : 1 - eps;
        }
        // the sample is final: its reads are not needed again (released here, on this thread, not in one sweep at the end)
        if (R.discarded) {   // nor are its result rows, for a caller that asked for columns, labels and counts only
            give_back(R.dosage.data() + row, (size_t)T_out);
            give_back(R.gp_t.data() + 3 * row, (size_t)3 * T_out);
            give_back(R.haps.data() + c.nL * row, (size_t)c.nL * T_out);
            if (c.nipt) {
                give_back(R.fet_dosage.data() + row, (size_t)T_out);
                give_back(R.fet_gp_t.data() + 3 * row, (size_t)3 * T_out);
            }
        }
        files.release(file);
        return (int)QA_OK;
    }
};

// qa_impute_samples reports every launch set whose samples are final (params->on_samples_done); this pool of host threads formats
// those samples, and adds them to the range's sums, while later launch sets are still on the device.
//
// Threads: on_samples_done() is called by qa_impute_samples' host threads; body() runs on the pool's own threads (started by start(),
// joined by close_and_join() and by the destructor, after the queue is drained); the calling thread reads status / err / busy_s /
// queue after the join.  mu guards queue, head, closed, status, err and busy_s.
struct FormatPool {
    const ColumnFormatter &columns;
    OrderedSums &sums;
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> queue;
    size_t head = 0;
    bool closed = false;
    int status = QA_OK;
    std::string err;
    double busy_s = 0;
    std::vector<std::thread> threads;

    FormatPool(const ColumnFormatter &columns_, OrderedSums &sums_) : columns(columns_), sums(sums_) {}
    ~FormatPool() { close_and_join(); }

    void start(int W) {
        threads.reserve((size_t)W);
        for (int w = 0; w < W; w++) threads.emplace_back(&FormatPool::body, this);
    }
    void close_and_join() {   // (what is queued is still formatted)
        { std::lock_guard<std::mutex> g(mu); closed = true; }
        cv.notify_all();
        for (auto &t : threads) t.join();
        threads.clear();
    }
    static void on_samples_done(void *ctx, int32_t lo, int32_t hi) {
        FormatPool *p = static_cast<FormatPool *>(ctx);
        {
            std::lock_guard<std::mutex> g(p->mu);
            for (int j = lo; j < hi; j++) p->queue.push_back(j);
        }
        p->cv.notify_all();
    }
    void body() {
        for (;;) {
            int j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [this] { return head < queue.size() || closed; });
                if (head >= queue.size()) return;
                j = queue[head++];
            }
            const auto tj = Clock::now();
            std::string e;
            int s1;
            try { s1 = columns.format_one(j, e); } catch (const std::exception &ex) { s1 = QA_ERR_INVALID; e = ex.what(); }
            if (s1 == QA_OK) sums.add(j);
            std::lock_guard<std::mutex> g(mu);
            busy_s += since(tj);
            if (s1 != QA_OK && status == QA_OK) { status = s1; err = e; }
        }
    }
};

// ---- 2. the ONE call for every chain of every kept sample: the caller's parameters with the range's own sample source, kept-sample
// indices, result rows and hook in place of the caller's (the structs the copy points to live here, so this is not copied).
struct ImputeArgs {
    qa_impute_params_t P;
    qa_impute_rare_common_t rcq;
    qa_impute_nipt_t nq;
    qa_impute_hla_t hla{};
    const qa_sample_source_t source;
    const qa_impute_reads_out_t reads_out;

    ImputeArgs(const RangeCall &c, qa_bam_range_result &R, FileLoader &files, FormatPool &pool)
        : P(*c.params), source{&FileLoader::acquire, &files}, reads_out{nullptr, &FileLoader::prob_dest, &files} {
        P.sample_index = files.index.data();
        P.sample_source = &source;
        P.on_samples_done = &FormatPool::on_samples_done;
        P.on_samples_done_ctx = &pool;
        if (c.rare) {
            rcq = *c.params->rare_common;
            rcq.read_off = rcq.read_ptr = rcq.u = rcq.bq = rcq.wif = nullptr;
            P.rare_common = &rcq;
        }
        if (c.nipt) {
            nq = *c.params->nipt;
            nq.ff = files.ffk.data();
            nq.fet_dosage = R.fet_dosage.data();
            nq.fet_gp_t = R.fet_gp_t.data();
            P.nipt = &nq;
        }
        if (c.want_hla) {
            hla.grid = c.ex->hla_grid;
            hla.gamma1 = R.gamma1.data(); hla.gamma2 = R.gamma2.data(); hla.gamma_total = R.gamma_total.data();
            hla.list_of_gammas = R.list_of_gammas.data();
        }
    }
    ImputeArgs(const ImputeArgs &) = delete;
};

}  // namespace

// The call: refusals, the result's memory, then the parts above -- the two thread owners last, so that whichever way this function is
// left (a return or an exception) their destructors join the formatters and then the loaders before anything they use is released.
// A loader's failure wins over the imputation's status, which wins over a formatter's.
int qa::bam_range_impl(const qa::BamRangeImputeFn &impute, const qa_impute_params_t *params, const qa_bam_range_io_t *io,
                       const qa_bam_range_extras_t *ex, int32_t K, int32_t G, int32_t n_sample, const char *const *bam_paths,
                       const int64_t *sample_index, const double *ff, qa_bam_range_result_t **out) {
    if (out) *out = nullptr;
    RangeCall c{params, io, ex, K, G, n_sample, bam_paths, sample_index, ff};
    if (const int st = check_range_request(c, out != nullptr)) return st;
    const auto t_all = Clock::now();
    c.resolve();
    const bool trace = std::getenv("QA_BAM_RANGE_TRACE") != nullptr;   // (phase times on stderr)
    auto t0 = Clock::now();
    std::unique_ptr<qa_bam_range_result> R = allocate_result(c);
    OrderedSums sums(*R, n_sample);
    FileLoader files(c, *R, t0);
    const ColumnFormatter columns{c, *R, files, sums};
    FormatPool pool(columns, sums);
    ImputeArgs a(c, *R, files, pool);
    files.start();   // (from here on there are threads: nothing below allocates for the result)
    pool.start(std::max(1, std::min(c.n_io, n_sample)));
    const double tr_setup = since(t0);
    int st = QA_OK;   // (n_sample = the files: an upper bound, the source ends the range)
    if (n_sample > 0)
        st = impute(&a.P, n_sample, nullptr, nullptr, nullptr, nullptr, nullptr, R->dosage.data(), R->gp_t.data(), R->haps.data(), nullptr,
                    R->nDosage.data(), R->stats, c.want_hla ? &a.hla : nullptr, c.want_prob ? &a.reads_out : nullptr);
    files.stop_and_join();
    if (files.status != QA_OK) { pool.close_and_join(); qa::set_error("qa_impute_bam_range: %s", files.err.c_str()); return files.status; }
    if (st != QA_OK) { pool.close_and_join(); return st; }   // (qa_last_error holds qa_impute_samples' text)
    const int nk = R->n_kept = files.n_kept;
    R->kept.resize((size_t)nk);
    R->seconds[0] = files.done_s;
    R->seconds[1] = since(t0);
    const double tr_call = R->seconds[1] - tr_setup;
    t0 = Clock::now();
    pool.close_and_join();   // (what is still queued when the device work ends: the last launch sets' samples)
    const double tr_drain = since(t0);
    if (pool.status != QA_OK) { qa::set_error("qa_impute_bam_range: %s", pool.err.c_str()); return pool.status; }
    if ((int)pool.queue.size() != nk) { qa::set_error("qa_impute_bam_range: %d of %d samples were reported final", (int)pool.queue.size(), nk); return QA_ERR_INVALID; }
    if (sums.next != nk) { qa::set_error("qa_impute_bam_range: %d of %d samples were added to the range's sums", sums.next, nk); return QA_ERR_INVALID; }
    R->format_busy_s = pool.busy_s;
    R->seconds[2] = since(t0);
    R->seconds[3] = since(t_all);
    if (trace)
        std::fprintf(stderr, "qa_impute_bam_range: %d files (%d kept), %d host threads: last file loaded at %.3f s (beside the imputation), setup %.3f, "
                     "qa_impute_samples %.3f, formatters' drain %.3f (busy %.3f thread-s), sums %.3f, whole call %.3f\n", n_sample, nk, c.n_io,
                     R->seconds[0], tr_setup, tr_call, tr_drain, pool.busy_s, R->seconds[2] - tr_drain, R->seconds[3]);
    *out = R.release();
    return QA_OK;
}

extern "C" {

// test hook (impute_testhook.h): the same host code -- loader, kept-sample bookkeeping, formatting, counts -- with the imputation
// running over a checker's entry points instead of the device
int qa_impute_bam_range_backend(const qa_impute_backend_t *backend, void *const *handles, int32_t n_handles, int32_t K, int32_t nGrids,
                                const qa_impute_params_t *params, const qa_bam_range_io_t *io, int32_t n_sample, const char *const *bam_paths,
                                const int64_t *sample_index, const double *ff, qa_bam_range_result_t **out) {
    const qa_bam_range_extras_t ex{0, 0, 0, -1};
    return qa_impute_bam_range_backend_ex(backend, nullptr, handles, n_handles, K, nGrids, params, io, &ex, n_sample, bam_paths, sample_index,
                                          ff, out);
}

int qa_impute_bam_range_backend_bx(const qa_impute_backend_t *backend, void *const *handles, int32_t n_handles, int32_t K, int32_t nGrids,
                                   const qa_impute_params_t *params, const qa_bam_range_io_t *io, int32_t use_bx_tag,
                                   int32_t bxTagUpperLimit, int32_t n_sample, const char *const *bam_paths, const int64_t *sample_index,
                                   const double *ff, qa_bam_range_result_t **out) {
    const qa_bam_range_extras_t ex{use_bx_tag, bxTagUpperLimit, 0, -1};
    return qa_impute_bam_range_backend_ex(backend, nullptr, handles, n_handles, K, nGrids, params, io, &ex, n_sample, bam_paths, sample_index,
                                          ff, out);
}

int qa_impute_bam_range_backend_ex(const qa_impute_backend_t *backend, qa_fullpass_select_gamma_fn select_gamma, void *const *handles,
                                   int32_t n_handles, int32_t K, int32_t nGrids, const qa_impute_params_t *params,
                                   const qa_bam_range_io_t *io, const qa_bam_range_extras_t *ex, int32_t n_sample,
                                   const char *const *bam_paths, const int64_t *sample_index, const double *ff,
                                   qa_bam_range_result_t **out) {
    if (!backend || !handles || !io || (ex && ex->hla_grid >= 0 && !select_gamma)) {
        if (out) *out = nullptr;
        qa::set_error("qa_impute_bam_range_backend: missing argument");
        return QA_ERR_INVALID;
    }
    const int32_t T = io->nSNPs;
    return qa::bam_range_impl(
        [=](const qa_impute_params_t *P, int32_t n, const int32_t *ro, const int32_t *rp, const int32_t *u, const int32_t *bq, const int32_t *wif,
            double *dosage, double *gp_t, double *haps, int32_t *labels, int32_t *nDosage, int64_t *stats, const qa_impute_hla_t *hla,
            const qa_impute_reads_out_t *reads_out) {
            if (!hla && !reads_out)
                return qa_impute_samples_backend(backend, handles, n_handles, K, nGrids, T, P, n, 0, ro, rp, u, bq, wif, dosage, gp_t, haps,
                                                 labels, nDosage, stats);
            return qa_impute_samples_backend_reads(backend, select_gamma, handles, n_handles, K, nGrids, T, P, n, 0, ro, rp, u, bq, wif, dosage,
                                                   gp_t, haps, labels, nDosage, stats, hla, reads_out);
        },
        params, io, ex, K, nGrids, n_sample, bam_paths, sample_index, ff, out);
}

int32_t qa_bam_range_n_samples(const qa_bam_range_result_t *r) { return r ? r->n : 0; }
int32_t qa_bam_range_n_snps(const qa_bam_range_result_t *r) { return r ? r->T_out : 0; }
int32_t qa_bam_range_imputed(const qa_bam_range_result_t *r, int32_t i) { return (r && i >= 0 && i < r->n) ? r->imputed[(size_t)i] : 0; }
int32_t qa_bam_range_n_reads(const qa_bam_range_result_t *r, int32_t i) { return (r && i >= 0 && i < r->n) ? r->n_reads[(size_t)i] : 0; }

int qa_bam_range_column(const qa_bam_range_result_t *r, int32_t i, const char **buf, const int64_t **off) {
    if (!r || i < 0 || i >= r->n || !buf || !off) return QA_ERR_INVALID;
    const int j = r->slot[(size_t)i];
    *buf = j < 0 ? nullptr : r->col_buf[(size_t)j].data();
    *off = j < 0 ? nullptr : r->col_off[(size_t)j].data();
    return QA_OK;
}

int qa_bam_range_sample(const qa_bam_range_result_t *r, int32_t i, const double **dosage, const double **gp_t, const double **phasing_haps,
                        const double **fet_dosage, const double **fet_gp_t, const int32_t **read_labels, int32_t *n_labels, int32_t *nDosage) {
    if (!r || i < 0 || i >= r->n) return QA_ERR_INVALID;
    const int j = r->slot[(size_t)i];
    const size_t T = (size_t)r->T_out;
    if (dosage) *dosage = (j < 0 || r->discarded) ? nullptr : r->dosage.data() + (size_t)j * T;
    if (gp_t) *gp_t = (j < 0 || r->discarded) ? nullptr : r->gp_t.data() + (size_t)j * 3 * T;
    if (phasing_haps) *phasing_haps = (j < 0 || r->discarded) ? nullptr : r->haps.data() + (size_t)j * r->nL * T;
    if (fet_dosage) *fet_dosage = (j < 0 || !r->nipt || r->discarded) ? nullptr : r->fet_dosage.data() + (size_t)j * T;
    if (fet_gp_t) *fet_gp_t = (j < 0 || !r->nipt || r->discarded) ? nullptr : r->fet_gp_t.data() + (size_t)j * 3 * T;
    if (read_labels) *read_labels = j < 0 ? nullptr : r->labels_of[(size_t)j].data();
    if (n_labels) *n_labels = j < 0 ? 0 : (int32_t)r->labels_of[(size_t)j].size();
    if (nDosage) *nDosage = j < 0 ? 0 : r->nDosage[(size_t)j];
    return QA_OK;
}

int qa_bam_range_counts(const qa_bam_range_result_t *r, double *infoCount, double *afCount, double *hweCount, double *alleleCount) {
    if (!r) return QA_ERR_INVALID;
    const size_t T = (size_t)r->T_out;
    if (infoCount) std::memcpy(infoCount, r->infoCount.data(), sizeof(double) * 2 * T);
    if (afCount) std::memcpy(afCount, r->afCount.data(), sizeof(double) * T);
    if (hweCount) std::memcpy(hweCount, r->hweCount.data(), sizeof(double) * 3 * T);
    if (alleleCount) std::memcpy(alleleCount, r->alleleCount.data(), sizeof(double) * 2 * T);
    return QA_OK;
}

void qa_bam_range_timings(const qa_bam_range_result_t *r, double seconds[4], int64_t impute_stats[11], int64_t load_stats[8]) {
    if (!r) return;
    if (seconds) std::memcpy(seconds, r->seconds, sizeof r->seconds);
    if (impute_stats) std::memcpy(impute_stats, r->stats, sizeof r->stats);
    if (load_stats) std::memcpy(load_stats, r->load_stats, sizeof r->load_stats);
}

int qa_bam_range_read_label_prob(const qa_bam_range_result_t *r, int32_t i, const char **names, const int64_t **names_off,
                                 const double **prob, int32_t *n) {
    if (!r || i < 0 || i >= r->n) return QA_ERR_INVALID;
    const int j = r->with_prob ? r->slot[(size_t)i] : -1;
    if (names) *names = j < 0 ? nullptr : r->names_buf[(size_t)j].data();
    if (names_off) *names_off = j < 0 ? nullptr : r->names_off[(size_t)j].data();
    if (prob) *prob = j < 0 ? nullptr : r->prob_of[(size_t)j].data();
    if (n) *n = j < 0 ? 0 : (int32_t)r->prob_of[(size_t)j].size();
    return QA_OK;
}

int qa_bam_range_hla(const qa_bam_range_result_t *r, int32_t i, const double **gamma1, const double **gamma2, const double **gamma_total,
                     const double **list_of_gammas, int32_t *K, int32_t *nGibbsSamples) {
    if (!r || i < 0 || i >= r->n) return QA_ERR_INVALID;
    const int j = r->with_hla ? r->slot[(size_t)i] : -1;
    const size_t Kk = (size_t)r->K;
    if (gamma1) *gamma1 = j < 0 ? nullptr : r->gamma1.data() + (size_t)j * Kk;
    if (gamma2) *gamma2 = j < 0 ? nullptr : r->gamma2.data() + (size_t)j * Kk;
    if (gamma_total) *gamma_total = j < 0 ? nullptr : r->gamma_total.data() + (size_t)j * Kk;
    if (list_of_gammas) *list_of_gammas = j < 0 ? nullptr : r->list_of_gammas.data() + (size_t)j * r->nG * 2 * Kk;
    if (K) *K = j < 0 ? 0 : r->K;
    if (nGibbsSamples) *nGibbsSamples = j < 0 ? 0 : r->nG;
    return QA_OK;
}

void qa_bam_range_bx_stats(const qa_bam_range_result_t *r, int64_t out[4]) {
    if (r && out) std::memcpy(out, r->bx_stats, sizeof r->bx_stats);
}

void qa_bam_range_destroy(qa_bam_range_result_t *r) { delete r; }

}  // extern "C"
