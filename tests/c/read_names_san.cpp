// read_names_san.cpp -- the BAM loader with read names (qa_bam_load_sample_reads_named, csrc/hostio.cpp linked alone with
// bx_loader_stubs.cpp) as a stand-alone program for g++ -fsanitize=address,undefined (tests/test_read_label_prob_cpu.py): the file
// is loaded with names requested -- BX rule off and on, with and without the coverage cap --, the names are exported and walked
// through their offsets, and the last combination's names are printed one per line for the test to compare.
//   read_names_san <sites.bin> <file.bam> <bxTagUpperLimit> <downsampleToCov>
//   sites.bin: int32 T, int32 L[T], char ref[T], char alt[T], int32 grid[T]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/quilt_amd.h"
#include "../../include/quilt_amd_io.h"

namespace qa { extern char g_last_error[1024]; }

int main(int argc, char **argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: read_names_san sites.bin file.bam limit cap\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    int32_t T = 0;
    if (!f || std::fread(&T, 4, 1, f) != 1 || T < 1) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<int32_t> L((size_t)T), grid((size_t)T);
    std::vector<char> ref((size_t)T), alt((size_t)T);
    const bool ok = std::fread(L.data(), 4, (size_t)T, f) == (size_t)T && std::fread(ref.data(), 1, (size_t)T, f) == (size_t)T &&
                    std::fread(alt.data(), 1, (size_t)T, f) == (size_t)T && std::fread(grid.data(), 4, (size_t)T, f) == (size_t)T;
    std::fclose(f);
    if (!ok) { std::fprintf(stderr, "%s is cut short\n", argv[1]); return 2; }
    const int32_t limit = (int32_t)std::atoi(argv[3]), cap_arg = (int32_t)std::atoi(argv[4]);
    std::vector<char> last_names;
    std::vector<int64_t> last_off;
    for (int use_bx = 0; use_bx < 2; use_bx++)
        for (int32_t cap : {0, cap_arg}) {
            qa_bam_opts_t o;
            qa_bam_opts_default(&o);
            o.downsampleToCov = cap;
            qa_sample_reads_t *h = nullptr, *plain = nullptr;
            if (qa_bam_load_sample_reads_named(argv[2], "1", T, L.data(), ref.data(), alt.data(), grid.data(), &o, use_bx, limit, 1, &h) != QA_OK ||
                qa_bam_load_sample_reads_named(argv[2], "1", T, L.data(), ref.data(), alt.data(), grid.data(), &o, use_bx, limit, 0, &plain) != QA_OK) {
                std::fprintf(stderr, "cannot load %s: %s\n", argv[2], qa::g_last_error);
                return 1;
            }
            const int32_t R = qa_sample_reads_n_reads(h);
            const int64_t nb = qa_sample_reads_n_bases(h), bytes = qa_sample_reads_names_bytes(h);
            // without the request: no names, and the same read arrays
            if (qa_sample_reads_names_bytes(plain) != -1 || qa_sample_reads_export_names(plain, nullptr, nullptr) != QA_ERR_INVALID) return 1;
            if (qa_sample_reads_n_reads(plain) != R || qa_sample_reads_n_bases(plain) != nb) return 1;
            std::vector<int32_t> a((size_t)R + 1 + 2 * (size_t)nb + (size_t)R + 2), b(a.size());
            qa_sample_reads_export(h, a.data(), a.data() + R + 1, a.data() + R + 1 + nb, a.data() + R + 1 + 2 * nb, nullptr);
            qa_sample_reads_export(plain, b.data(), b.data() + R + 1, b.data() + R + 1 + nb, b.data() + R + 1 + 2 * nb, nullptr);
            if (std::memcmp(a.data(), b.data(), 4 * a.size()) != 0) { std::fprintf(stderr, "the names request changed the reads\n"); return 1; }
            if (bytes < R) { std::fprintf(stderr, "names_bytes = %lld for %d reads\n", (long long)bytes, (int)R); return 1; }
            // exactly-sized buffers: one byte past either is the sanitizer's to find
            std::vector<char> names((size_t)bytes);
            std::vector<int64_t> off((size_t)R + 1);
            if (qa_sample_reads_export_names(h, names.data(), off.data()) != QA_OK) return 1;
            if (off[0] != 0 || off[(size_t)R] != bytes) { std::fprintf(stderr, "the offsets do not span the names\n"); return 1; }
            for (int32_t r = 0; r < R; r++) {
                if (off[(size_t)r + 1] <= off[(size_t)r] || names[(size_t)off[(size_t)r + 1] - 1] != 0) { std::fprintf(stderr, "name %d is not terminated\n", (int)r); return 1; }
                if ((int64_t)std::strlen(names.data() + off[(size_t)r]) != off[(size_t)r + 1] - off[(size_t)r] - 1) { std::fprintf(stderr, "name %d holds a NUL\n", (int)r); return 1; }
            }
            // either pointer may be NULL
            if (qa_sample_reads_export_names(h, nullptr, off.data()) != QA_OK || qa_sample_reads_export_names(h, names.data(), nullptr) != QA_OK) return 1;
            last_names = names;
            last_off = off;
            qa_sample_reads_destroy(h);
            qa_sample_reads_destroy(plain);
        }
    for (size_t r = 0; r + 1 < last_off.size(); r++) std::printf("%s\n", last_names.data() + last_off[r]);
    std::printf("read names: ok\n");
    return 0;
}
