// align.cpp -- global alignment from the command line (nw_align of libnwhip.so):
//   nw_align A.bdna B.bdna [OUT1 OUT2] [--scheme m,mm,g] [--mem BYTES] [--block-rows K] [--score-only]
//   A = s1 "across the top", B = s2 "down the side", as in driver.cpp
//   stdout: "<align ms>\nScore: <t[n2][n1]>\n" (the reference driver's format,
//   src/common/driver.cpp:32-35); the time covers fill, traceback and transfers.
//   OUT1 / OUT2: the two gapped rows as .bdna files, byte 0 = gap, equal length.
//   --mem BYTES / --block-rows K: align in linear memory (nw_align_ckpt) within BYTES
//   of device memory / in blocks of K rows (a multiple of 64); the output is the same.
//   --score-only: no alignment, the score from the table-free sweep (nw_score).
// Argument and missing-file errors are nw_driver's (exit 1); a device failure is
// reported on stderr and exits 2.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "nw_hip.h"

static bool write_file(const char *path, const std::vector<int8_t> &row) {
    FILE *f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = row.empty() || std::fwrite(row.data(), 1, row.size(), f) == row.size();
    return std::fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    nw_params p;
    nw_params_default(&p);
    std::vector<const char *> pos;
    nw_ckpt_opts co;
    std::memset(&co, 0, sizeof co);
    bool ckpt = false, score_only = false;
    for (int a = 1; a < argc; ++a) {
        if (std::strcmp(argv[a], "--scheme") == 0) {
            int m, mm, g;
            if (a + 1 >= argc || std::sscanf(argv[a + 1], "%d,%d,%d", &m, &mm, &g) != 3) {
                std::cout << "error: --scheme expects match,mismatch,gap" << std::endl;
                return 1;
            }
            p.match = m;
            p.mismatch = mm;
            p.gap = g;
            ++a;
        } else if (std::strcmp(argv[a], "--mem") == 0 || std::strcmp(argv[a], "--block-rows") == 0) {
            long long v = 0;
            if (a + 1 >= argc || std::sscanf(argv[a + 1], "%lld", &v) != 1 || v <= 0) {
                std::cout << "error: " << argv[a] << " expects a positive number" << std::endl;
                return 1;
            }
            (std::strcmp(argv[a], "--mem") == 0 ? co.mem_bytes : co.block_rows) = v;
            ckpt = true;
            ++a;
        } else if (std::strcmp(argv[a], "--score-only") == 0) {
            score_only = true;
        } else {
            pos.push_back(argv[a]);
        }
    }
    if (pos.size() != 2 && pos.size() != 4) {
        std::cout << "error: incorrect number of arguments (expected 2 or 4, got " << pos.size() << ")" << std::endl;
        return 1;
    }
    int8_t *s1 = nullptr, *s2 = nullptr;
    int64_t n1 = 0, n2 = 0;
    if (nw_read_bdna(pos[0], &s1, &n1) != NW_OK) {
        std::cout << "ERROR: no such file " << pos[0] << std::endl;
        return 1;
    }
    if (nw_read_bdna(pos[1], &s2, &n2) != NW_OK) {
        std::cout << "ERROR: no such file " << pos[1] << std::endl;
        return 1;
    }
    std::vector<uint8_t> ops((size_t)(n1 + n2) + 1);
    nw_alignment al;

    auto wallStart = std::chrono::system_clock::now();
    int st;
    if (score_only) {
        nw_result r;
        st = nw_score(s1, n1, s2, n2, &p, &r);
        al.score = r.score;
    } else if (ckpt) {
        st = nw_align_ckpt(s1, n1, s2, n2, &p, &co, nullptr, ops.data(), n1 + n2, &al, nullptr);
    } else {
        st = nw_align(s1, n1, s2, n2, &p, nullptr, ops.data(), n1 + n2, &al, nullptr);
    }
    auto wallDiff = std::chrono::system_clock::now() - wallStart;
    if (st != NW_OK) {
        std::fprintf(stderr, "nw_align (libnwhip): %s\n", nw_strerror(st));
        return 2;
    }
    int wallMsec = std::chrono::duration_cast<std::chrono::milliseconds>(wallDiff).count();
    std::cout << wallMsec;
    std::cout << "\nScore: " << al.score << std::endl;

    if (pos.size() == 4 && !score_only) {
        std::vector<int8_t> row1((size_t)al.n_ops), row2((size_t)al.n_ops);
        if (nw_ops_expand(s1, n1, s2, n2, al.begin_i, al.begin_j, ops.data(), al.n_ops, row1.data(), row2.data()) !=
            NW_OK) {
            std::fprintf(stderr, "nw_align (libnwhip): inconsistent ops\n");
            return 2;
        }
        if (!write_file(pos[2], row1) || !write_file(pos[3], row2)) {
            std::cout << "ERROR: cannot write " << pos[2] << " / " << pos[3] << std::endl;
            return 1;
        }
    }
    nw_free(s1);
    nw_free(s2);
    return 0;
}
