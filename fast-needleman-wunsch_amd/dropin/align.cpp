// align.cpp -- global alignment from the command line (nw_align of libnwhip.so):
//   nw_align A.bdna B.bdna [OUT1 OUT2] [--scheme m,mm,g] [--mem BYTES] [--block-rows K] [--score-only]
//   A = s1 "across the top", B = s2 "down the side", as in driver.cpp
//   stdout: "<align ms>\nScore: <t[n2][n1]>\n" (the reference driver's format,
//   src/common/driver.cpp:32-35); the time covers fill, traceback and transfers.
//   OUT1 / OUT2: the two gapped rows as .bdna files, byte 0 = gap, equal length.
//   --mem BYTES / --block-rows K: align in linear memory (nw_align_ckpt) within BYTES
//   of device memory / in blocks of K rows (a multiple of 64); the output is the same.
//   --score-only: no alignment, the score from the table-free sweep (nw_score).
//   nw_align --batch LIST [--scheme m,mm,g] [--mem BYTES] [--score-only] [--gap-open G] [--matrix FILE] [--local | --ends N | --band W | --gap2 O2,E2 [--gap2-band W]]
//   LIST: a text file, one pair "A.bdna B.bdna" per line (paths relative to the
//   list's directory unless absolute); all pairs are aligned in ONE call
//   (nw_align_batch; --score-only: nw_score_batch).  stdout: "<ms>\n", then one
//   "Score: <t[n2][n1]>" line per pair, in the list's order.
//   --gap-open G (G <= 0, with --batch only): affine gap cost, a gap of length L costs
//   G + L * g (nw_align_batch_affine / nw_score_batch_affine).
//   --matrix FILE (with --batch only): substitution by matrix (nw_align_batch_matrix /
//   nw_score_batch_matrix); --scheme's third number is the gap extension, --gap-open the
//   opening (default 0).  FILE is the usual NCBI text layout: '#' comment lines, a header
//   row of letters, one row per letter (the letter, then one integer in -128..127 per
//   header letter); the entry of row r, column c scores an A letter r against a B letter
//   c.  A letter is one character or 0xHH (a byte value); a lower-case byte maps like its
//   upper-case letter; with a '*' among the letters every unlisted byte maps to it,
//   without one an unlisted byte in a sequence is an error.
//   --local (with --batch only): local alignment, Smith-Waterman under the same gap cost
//   (nw_align_batch_local / nw_score_batch_local): the best-scoring pair of substrings
//   of every pair.  Without --matrix the substitution is --scheme's match / mismatch over
//   A, C, G, T (either case); every other byte is one more letter that mismatches
//   everything, itself included.  Per pair one line
//     "Score: <max H> begin (<i>, <j>) end (<i>, <j>)"     (cells of the table: i counts B)
//   and, unless --score-only (which prints no begin cell), the two gapped rows of the
//   aligned segment alone, "A: ..." and "B: ..." ('-' = gap, a non-printing byte as '?').
//   --ends N (with --batch only, not with --local; N = 0 .. 15, the sum of 1: a skipped
//   prefix of A is free, 2: a skipped suffix of A, 4: a prefix of B, 8: a suffix of B):
//   semi-global alignment (nw_align_batch_semi / nw_score_batch_semi), e.g. 3: all of B
//   inside A, 12: all of A inside B, 15: overlap.  Substitution and output are --local's:
//   the score (it may be negative), begin and end cell and the gapped rows of the aligned
//   part; the skipped ends are not printed.
//   --band W (with --batch only, not with --local or --ends; W >= 0): banded global
//   alignment (nw_align_batch_banded / nw_score_batch_banded): only paths that stay within
//   W diagonals of the pair's own (of 0 .. |B| - |A|) count.  Substitution as --local's
//   (--matrix, or --scheme's match / mismatch over A, C, G, T); one "Score:" line per pair.
//   --gap2 O2,E2 (with --batch only, not with --local, --ends or --band; O2 <= 0): a second
//   piece of the gap cost (nw_align_batch_dual / nw_score_batch_dual): a gap of length L
//   costs max(G + L * g, O2 + L * E2), G from --gap-open (default 0) and g from --scheme --
//   short gaps by the steep piece, long ones by the flat piece (minimap2's -O4,24 -E2,1 is
//   --scheme 2,-4,-2 --gap-open -4 --gap2 -24,-1).  Substitution as --band's; one "Score:"
//   line per pair.
//   --gap2-band W (with --gap2 only, not with --band, --local or --ends; W >= 0): the two-piece
//   gap cost inside a band (nw_align_batch_dual_banded / nw_score_batch_dual_banded): only
//   paths that stay within W diagonals of the pair's own count, and a long gap in them is
//   still priced by the flat piece.  (--gap2 with --band stays an error: --band is the
//   one-piece entry's option.)
// Argument and missing-file errors are nw_driver's (exit 1); a device failure is
// reported on stderr and exits 2.
#include <chrono>
#include <cstdint>
#include <fstream>
#include <sstream>
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

// a letter of a matrix file: one character, or 0xHH
static int letter_byte(const std::string &t) {
    if (t.size() == 1) return (unsigned char)t[0];
    if (t.size() == 4 && t[0] == '0' && (t[1] == 'x' || t[1] == 'X')) {
        char *end = nullptr;
        const long v = std::strtol(t.c_str() + 2, &end, 16);
        if (*end == 0 && v >= 0 && v <= 255) return (int)v;
    }
    return -1;
}

// --matrix FILE into *m; listed[b]: byte b is a letter (or the lower case of one).  The
// format is nwhip.SubMatrix.from_text's.
static bool read_matrix(const char *path, nw_submat *m, bool *listed, std::string *err) {
    std::ifstream in(path);
    if (!in) {
        *err = std::string("ERROR: no such file ") + path;
        return false;
    }
    std::memset(m, 0, sizeof *m);
    std::vector<int> letters;
    int pos[256];
    bool have_row[NW_SUBMAT_MAX] = {false};
    for (int b = 0; b < 256; ++b) pos[b] = -1;
    std::string line;
    size_t rows = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::vector<std::string> tok;
        for (std::string t; ls >> t;) tok.push_back(t);
        if (tok.empty() || tok[0][0] == '#') continue;
        if (letters.empty()) {
            for (const std::string &t : tok) {
                const int b = letter_byte(t);
                if (b < 0 || pos[b] >= 0 || letters.size() >= (size_t)NW_SUBMAT_MAX) {
                    *err = "error: --matrix: the header must be 1..32 distinct letters (one character or 0xHH)";
                    return false;
                }
                pos[b] = (int)letters.size();
                letters.push_back(b);
            }
            continue;
        }
        const int r = letter_byte(tok[0]);
        if (r < 0 || pos[r] < 0 || have_row[pos[r]] || tok.size() != letters.size() + 1) {
            *err = "error: --matrix: row '" + line + "': a letter of the header and one number per letter expected";
            return false;
        }
        for (size_t c = 0; c < letters.size(); ++c) {
            char *end = nullptr;
            const long v = std::strtol(tok[c + 1].c_str(), &end, 10);
            if (*end != 0 || end == tok[c + 1].c_str() || v < -128 || v > 127) {
                *err = "error: --matrix: row '" + line + "': integers in -128..127 expected";
                return false;
            }
            m->score[pos[r] * NW_SUBMAT_MAX + (int)c] = (int8_t)v;
        }
        have_row[pos[r]] = true;
        ++rows;
    }
    if (letters.empty() || rows != letters.size()) {
        *err = "error: --matrix: a header row and one row per letter expected";
        return false;
    }
    m->n = (int32_t)letters.size();
    const int other = pos[(unsigned char)'*'];
    for (int b = 0; b < 256; ++b) {
        int k = pos[b];
        if (k < 0 && b >= 'a' && b <= 'z') k = pos[b - 32];
        listed[b] = k >= 0 || other >= 0;
        m->index[b] = (uint8_t)(k >= 0 ? k : other >= 0 ? other : 0);
    }
    return true;
}

// --local without --matrix: match / mismatch over A, C, G, T (either case) and one more
// letter for every other byte, which mismatches everything, itself included
static void uniform_dna(const nw_params &p, nw_submat *m, bool *listed) {
    std::memset(m, 0, sizeof *m);
    m->n = 5;
    for (int x = 0; x < 5; ++x)
        for (int y = 0; y < 5; ++y)
            m->score[x * NW_SUBMAT_MAX + y] = (int8_t)(x == y && x < 4 ? p.match : p.mismatch);
    for (int b = 0; b < 256; ++b) {
        listed[b] = true;
        m->index[b] = 4;
    }
    const char *acgt = "ACGT";
    for (int k = 0; k < 4; ++k) m->index[(unsigned char)acgt[k]] = m->index[(unsigned char)acgt[k] + 32] = (uint8_t)k;
}

static std::string row_text(const std::vector<int8_t> &row) {
    std::string t(row.size(), '?');
    for (size_t k = 0; k < row.size(); ++k)
        if (row[k] == 0)
            t[k] = '-';
        else if (row[k] > 32 && row[k] < 127)
            t[k] = (char)row[k];
    return t;
}

// --batch LIST: every pair of the list in one call
static int run_batch(const char *list, const nw_params &p, int64_t mem_bytes, bool score_only, const int32_t *gap_open,
                     const char *matrix, bool local, int ends, int64_t band, const int32_t *gap2,
                     int64_t gap2_band) {
    nw_submat mat;
    bool listed[256];
    const bool semi = ends >= 0;
    const bool banded = band >= 0;
    const bool hit_lines = local || semi;  // a result is an nw_local_hit
    const bool dual = gap2 != nullptr;  // gap2[0] the opening, gap2[1] the extension of piece 2
    if ((hit_lines || banded || dual) && matrix == nullptr) {
        if (p.match < -128 || p.match > 127 || p.mismatch < -128 || p.mismatch > 127) {
            std::cout << "error: " << (local ? "--local" : semi ? "--ends" : banded ? "--band" : "--gap2")
                      << " without --matrix needs match and mismatch in -128..127" << std::endl;
            return 1;
        }
        uniform_dna(p, &mat, listed);
    }
    if (matrix != nullptr) {
        std::string err;
        if (!read_matrix(matrix, &mat, listed, &err)) {
            std::cout << err << std::endl;
            return 1;
        }
    }
    std::ifstream in(list);
    if (!in) {
        std::cout << "ERROR: no such file " << list << std::endl;
        return 1;
    }
    std::string dir(list);
    const size_t slash = dir.find_last_of('/');
    dir = slash == std::string::npos ? std::string() : dir.substr(0, slash + 1);
    std::vector<int8_t> s1cat, s2cat;
    std::vector<int64_t> off1(1, 0), off2(1, 0);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string fa, fb;
        if (!(ls >> fa)) continue;  // blank line
        if (!(ls >> fb)) {
            std::cout << "error: --batch expects two files per line" << std::endl;
            return 1;
        }
        const std::string *names[2] = {&fa, &fb};
        for (int k = 0; k < 2; ++k) {
            const std::string path = (*names[k])[0] == '/' ? *names[k] : dir + *names[k];
            int8_t *s = nullptr;
            int64_t n = 0;
            if (nw_read_bdna(path.c_str(), &s, &n) != NW_OK) {
                std::cout << "ERROR: no such file " << path << std::endl;
                return 1;
            }
            if (matrix != nullptr || hit_lines || banded || dual)
                for (int64_t x = 0; x < n; ++x)
                    if (!listed[(unsigned char)s[x]]) {
                        std::cout << "ERROR: byte " << (int)(unsigned char)s[x] << " of " << path
                                  << " is not a letter of the matrix (list a '*' letter for such bytes)" << std::endl;
                        return 1;
                    }
            std::vector<int8_t> &cat = k == 0 ? s1cat : s2cat;
            cat.insert(cat.end(), s, s + n);
            (k == 0 ? off1 : off2).push_back((int64_t)cat.size());
            nw_free(s);
        }
    }
    const int64_t npairs = (int64_t)off1.size() - 1;
    std::vector<int32_t> scores((size_t)npairs + 1);
    std::vector<int64_t> ops_off((size_t)npairs + 1), n_ops((size_t)npairs + 1);
    for (int64_t i = 0; i <= npairs; ++i) ops_off[(size_t)i] = off1[(size_t)i] + off2[(size_t)i];
    std::vector<uint8_t> ops((size_t)ops_off[(size_t)npairs] + 1);
    nw_batch_opts bo;
    std::memset(&bo, 0, sizeof bo);
    bo.mem_bytes = mem_bytes;
    auto wallStart = std::chrono::system_clock::now();
    int st;
    std::vector<nw_local_hit> hits((size_t)npairs + 1);
    if (local)
        st = score_only ? nw_score_batch_local(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                               gap_open ? *gap_open : 0, hits.data(), nullptr)
                        : nw_align_batch_local(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                               gap_open ? *gap_open : 0, &bo, hits.data(), ops.data(), ops_off.data(),
                                               n_ops.data(), nullptr);
    else if (semi)
        st = score_only ? nw_score_batch_semi(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                              gap_open ? *gap_open : 0, ends, hits.data(), nullptr)
                        : nw_align_batch_semi(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                              gap_open ? *gap_open : 0, ends, &bo, hits.data(), ops.data(),
                                              ops_off.data(), n_ops.data(), nullptr);
    else if (banded)
        st = score_only ? nw_score_batch_banded(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                                gap_open ? *gap_open : 0, (int32_t)band, scores.data(), nullptr)
                        : nw_align_batch_banded(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                                gap_open ? *gap_open : 0, (int32_t)band, &bo, scores.data(),
                                                ops.data(), ops_off.data(), n_ops.data(), nullptr);
    else if (dual && gap2_band >= 0)
        st = score_only
                 ? nw_score_batch_dual_banded(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                              gap_open ? *gap_open : 0, gap2[0], gap2[1], (int32_t)gap2_band,
                                              scores.data(), nullptr)
                 : nw_align_batch_dual_banded(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                              gap_open ? *gap_open : 0, gap2[0], gap2[1], (int32_t)gap2_band, &bo,
                                              scores.data(), ops.data(), ops_off.data(), n_ops.data(), nullptr);
    else if (dual)
        st = score_only ? nw_score_batch_dual(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                              gap_open ? *gap_open : 0, gap2[0], gap2[1], scores.data(), nullptr)
                        : nw_align_batch_dual(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                              gap_open ? *gap_open : 0, gap2[0], gap2[1], &bo, scores.data(),
                                              ops.data(), ops_off.data(), n_ops.data(), nullptr);
    else if (matrix != nullptr)
        st = score_only ? nw_score_batch_matrix(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                                gap_open ? *gap_open : 0, scores.data(), nullptr)
                        : nw_align_batch_matrix(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &mat,
                                                gap_open ? *gap_open : 0, &bo, scores.data(), ops.data(),
                                                ops_off.data(), n_ops.data(), nullptr);
    else if (gap_open != nullptr)
        st = score_only ? nw_score_batch_affine(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p,
                                                *gap_open, scores.data(), nullptr)
                        : nw_align_batch_affine(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p,
                                                *gap_open, &bo, scores.data(), ops.data(), ops_off.data(),
                                                n_ops.data(), nullptr);
    else
        st = score_only ? nw_score_batch(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p,
                                         scores.data(), nullptr)
                        : nw_align_batch(s1cat.data(), off1.data(), s2cat.data(), off2.data(), npairs, &p, &bo,
                                         scores.data(), ops.data(), ops_off.data(), n_ops.data(), nullptr);
    auto wallDiff = std::chrono::system_clock::now() - wallStart;
    if (st != NW_OK) {
        std::fprintf(stderr, "nw_align (libnwhip): %s\n", nw_strerror(st));
        return 2;
    }
    std::cout << std::chrono::duration_cast<std::chrono::milliseconds>(wallDiff).count() << "\n";
    for (int64_t i = 0; i < npairs && !hit_lines; ++i) std::cout << "Score: " << scores[(size_t)i] << "\n";
    for (int64_t i = 0; i < npairs && hit_lines; ++i) {
        const nw_local_hit &h = hits[(size_t)i];
        std::cout << "Score: " << h.score;
        if (!score_only) std::cout << " begin (" << h.begin_i << ", " << h.begin_j << ")";
        std::cout << " end (" << h.end_i << ", " << h.end_j << ")\n";
        if (score_only) continue;
        const int64_t n = n_ops[(size_t)i], n1 = off1[(size_t)i + 1] - off1[(size_t)i],
                      n2 = off2[(size_t)i + 1] - off2[(size_t)i];
        std::vector<int8_t> row1((size_t)n + 1), row2((size_t)n + 1);
        if (nw_ops_expand(s1cat.data() + off1[(size_t)i], n1, s2cat.data() + off2[(size_t)i], n2, h.begin_i, h.begin_j,
                          ops.data() + ops_off[(size_t)i], n, row1.data(), row2.data()) != NW_OK) {
            std::fprintf(stderr, "nw_align (libnwhip): inconsistent ops\n");
            return 2;
        }
        row1.resize((size_t)n);
        row2.resize((size_t)n);
        std::cout << "A: " << row_text(row1) << "\nB: " << row_text(row2) << "\n";
    }
    std::cout.flush();
    return 0;
}

int main(int argc, char **argv) {
    nw_params p;
    nw_params_default(&p);
    std::vector<const char *> pos;
    nw_ckpt_opts co;
    std::memset(&co, 0, sizeof co);
    bool ckpt = false, score_only = false;
    const char *batch = nullptr, *matrix = nullptr;
    int32_t gap_open = 0;
    bool affine = false, local = false;
    int ends = -1;  // --ends N: semi-global
    long long band = -1;  // --band W: banded global
    int32_t gap2[2] = {0, 0};  // --gap2 O2,E2: the second piece of the gap cost
    bool dual = false;
    long long gap2_band = -1;  // --gap2-band W: the two-piece cost inside a band
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
        } else if (std::strcmp(argv[a], "--gap-open") == 0) {
            int g = 0;
            if (a + 1 >= argc || std::sscanf(argv[a + 1], "%d", &g) != 1 || g > 0) {
                std::cout << "error: --gap-open expects a number <= 0" << std::endl;
                return 1;
            }
            gap_open = g;
            affine = true;
            ++a;
        } else if (std::strcmp(argv[a], "--matrix") == 0) {
            if (a + 1 >= argc) {
                std::cout << "error: --matrix expects a matrix file" << std::endl;
                return 1;
            }
            matrix = argv[++a];
        } else if (std::strcmp(argv[a], "--local") == 0) {
            local = true;
        } else if (std::strcmp(argv[a], "--ends") == 0) {
            int v = 0;
            char tail = 0;
            if (a + 1 >= argc || std::sscanf(argv[a + 1], "%d%c", &v, &tail) != 1 || v < 0 || v > NW_ENDS_OVERLAP) {
                std::cout << "error: --ends expects a number in 0..15" << std::endl;
                return 1;
            }
            ends = v;
            ++a;
        } else if (std::strcmp(argv[a], "--band") == 0) {
            long long v = 0;
            char tail = 0;
            if (a + 1 >= argc || std::sscanf(argv[a + 1], "%lld%c", &v, &tail) != 1 || v < 0 || v > INT32_MAX) {
                std::cout << "error: --band expects a number >= 0 (below 2^31)" << std::endl;
                return 1;
            }
            band = v;
            ++a;
        } else if (std::strcmp(argv[a], "--gap2-band") == 0) {
            long long v = 0;
            char tail = 0;
            if (a + 1 >= argc || std::sscanf(argv[a + 1], "%lld%c", &v, &tail) != 1 || v < 0 || v > INT32_MAX) {
                std::cout << "error: --gap2-band expects a number >= 0 (below 2^31)" << std::endl;
                return 1;
            }
            gap2_band = v;
            ++a;
        } else if (std::strcmp(argv[a], "--gap2") == 0) {
            int o2 = 0, e2 = 0;
            char tail = 0;
            if (a + 1 >= argc || std::sscanf(argv[a + 1], "%d,%d%c", &o2, &e2, &tail) != 2 || o2 > 0) {
                std::cout << "error: --gap2 expects open,extend with open <= 0" << std::endl;
                return 1;
            }
            gap2[0] = o2;
            gap2[1] = e2;
            dual = true;
            ++a;
        } else if (std::strcmp(argv[a], "--score-only") == 0) {
            score_only = true;
        } else if (std::strcmp(argv[a], "--batch") == 0) {
            if (a + 1 >= argc) {
                std::cout << "error: --batch expects a list file" << std::endl;
                return 1;
            }
            batch = argv[++a];
        } else {
            pos.push_back(argv[a]);
        }
    }
    if (batch != nullptr) {
        if (!pos.empty() || co.block_rows != 0) {
            std::cout << "error: --batch takes the list alone (and --scheme, --mem, --score-only, --gap-open, "
                         "--matrix, --local, --ends, --band, --gap2, --gap2-band)"
                      << std::endl;
            return 1;
        }
        if (local && ends >= 0) {
            std::cout << "error: --ends cannot be combined with --local (choose one)" << std::endl;
            return 1;
        }
        if (band >= 0 && (local || ends >= 0)) {
            std::cout << "error: --band cannot be combined with " << (local ? "--local" : "--ends")
                      << " (the band is built for the global alignment only)" << std::endl;
            return 1;
        }
        if (gap2_band >= 0 && (band >= 0 || local || ends >= 0)) {
            std::cout << "error: --gap2-band cannot be combined with "
                      << (band >= 0 ? "--band" : local ? "--local" : "--ends")
                      << " (it is the band of the two-piece global alignment)" << std::endl;
            return 1;
        }
        if (gap2_band >= 0 && !dual) {
            std::cout << "error: --gap2-band needs --gap2 (the one-piece band is --band)" << std::endl;
            return 1;
        }
        if (dual && (local || ends >= 0 || band >= 0)) {
            std::cout << "error: --gap2 cannot be combined with " << (local ? "--local" : ends >= 0 ? "--ends" : "--band")
                      << " (the two-piece gap cost is built for the global alignment only)" << std::endl;
            return 1;
        }
        if (local) {
            if (p.gap > 0) {
                std::cout << "error: --local needs a gap of at most 0 (--scheme's third number)" << std::endl;
                return 1;
            }
            p.mode = NW_MODE_SW;
        }
        return run_batch(batch, p, co.mem_bytes, score_only, affine ? &gap_open : nullptr, matrix, local, ends, band,
                         dual ? gap2 : nullptr, gap2_band);
    }
    if (gap2_band >= 0) {
        std::cout << "error: --gap2-band needs --batch (the band is built for the batched alignment only)"
                  << std::endl;
        return 1;
    }
    if (dual) {
        std::cout << "error: --gap2 needs --batch (the two-piece gap cost is built for the batched alignment only)"
                  << std::endl;
        return 1;
    }
    if (band >= 0) {
        std::cout << "error: --band needs --batch (the band is built for the batched alignment only)" << std::endl;
        return 1;
    }
    if (ends >= 0) {
        std::cout << "error: --ends needs --batch (semi-global alignment is built for the batched alignment only)"
                  << std::endl;
        return 1;
    }
    if (local) {
        std::cout << "error: --local needs --batch (the one-pair local alignment is nw_sw_align's)" << std::endl;
        return 1;
    }
    if (matrix != nullptr) {
        std::cout << "error: --matrix needs --batch (substitution matrices are built for the batched alignment only)"
                  << std::endl;
        return 1;
    }
    if (affine) {
        std::cout << "error: --gap-open needs --batch (affine gaps are built for the batched alignment only)"
                  << std::endl;
        return 1;
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
