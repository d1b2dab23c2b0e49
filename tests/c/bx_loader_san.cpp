// bx_loader_san.cpp -- the BAM loader (csrc/hostio.cpp, linked alone with bx_loader_stubs.cpp) as a stand-alone program for
// g++ -fsanitize=address,undefined (tests/test_bx_loader_cpu.py): every file named in a list is loaded with the BX rule off and
// on, with and without a coverage cap, and its reads exported.  The files include records cut at every byte of their auxiliary
// data: a file may load or be refused, but nothing may be read outside a record.
//   bx_loader_san <sites.bin> <list.txt>     sites.bin: int32 T, int32 L[T], char ref[T], char alt[T], int32 grid[T]
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/quilt_amd.h"
#include "../../include/quilt_amd_io.h"

namespace qa { extern char g_last_error[1024]; }

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: bx_loader_san sites.bin list.txt\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    int32_t T = 0;
    if (!f || std::fread(&T, 4, 1, f) != 1 || T < 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<int32_t> L((size_t)T), grid((size_t)T);
    std::vector<char> ref((size_t)T), alt((size_t)T);
    const bool ok = std::fread(L.data(), 4, (size_t)T, f) == (size_t)T && std::fread(ref.data(), 1, (size_t)T, f) == (size_t)T &&
                    std::fread(alt.data(), 1, (size_t)T, f) == (size_t)T && std::fread(grid.data(), 4, (size_t)T, f) == (size_t)T;
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "%s is cut short\n", argv[1]); return 2; }
    std::ifstream list(argv[2]);
    std::string path;
    int n_files = 0, n_loaded = 0;
    int64_t n_reads = 0, tagged = 0;
    while (std::getline(list, path)) {
        if (path.empty()) continue;
        n_files++;
        for (int use_bx = 0; use_bx < 2; use_bx++)
            for (int cap = 0; cap < 3; cap += 2)
                for (int32_t limit : {1000, 50000}) {
                    if (!use_bx && limit != 1000) continue;   // (without the tag the limit is not looked at)
                    qa_bam_opts_t o;
                    qa_bam_opts_default(&o);
                    o.downsampleToCov = cap;
                    qa_sample_reads_t *h = nullptr;
                    const int st = qa_bam_load_sample_reads_bx(path.c_str(), "1", T, L.data(), ref.data(), alt.data(), grid.data(), &o, use_bx,
                                                               limit, &h);
                    if (st != QA_OK) {
                        if (h) { std::fprintf(stderr, "%s: a handle came back with status %d\n", path.c_str(), st); return 1; }
                        continue;
                    }
                    const int32_t R = qa_sample_reads_n_reads(h);
                    const int64_t nb = qa_sample_reads_n_bases(h);
                    std::vector<int32_t> rp((size_t)R + 1), u((size_t)nb + 1), bq((size_t)nb + 1), wif((size_t)R + 1), cen((size_t)R + 1);
                    if (qa_sample_reads_export(h, rp.data(), u.data(), bq.data(), wif.data(), cen.data()) != QA_OK) return 1;
                    if (rp[(size_t)R] != nb) { std::fprintf(stderr, "%s: read_ptr does not end at the bases\n", path.c_str()); return 1; }
                    for (int64_t b = 0; b < nb; b++)
                        if (u[(size_t)b] < 0 || u[(size_t)b] >= T) { std::fprintf(stderr, "%s: a site outside the panel\n", path.c_str()); return 1; }
                    int64_t s8[8], s4[4];
                    qa_sample_reads_stats(h, s8);
                    qa_sample_reads_bx_stats(h, s4);
                    if (!use_bx && (s4[0] | s4[1] | s4[2] | s4[3])) { std::fprintf(stderr, "%s: BX counters without the tag\n", path.c_str()); return 1; }
                    n_reads += R;
                    tagged += s4[0];
                    n_loaded++;
                    qa_sample_reads_destroy(h);
                }
    }
    // a negative limit is refused before the file is opened
    qa_sample_reads_t *h = nullptr;
    if (qa_bam_load_sample_reads_bx("/nonexistent", "1", T, L.data(), ref.data(), alt.data(), grid.data(), nullptr, 1, -1, &h) != QA_ERR_INVALID || h)
        return 1;
    if (n_loaded == 0 || tagged == 0) { std::fprintf(stderr, "nothing was loaded (%s)\n", qa::g_last_error); return 1; }
    std::printf("bx loader: ok, %d files, %d loads, %lld reads\n", n_files, n_loaded, (long long)n_reads);
    return 0;
}
