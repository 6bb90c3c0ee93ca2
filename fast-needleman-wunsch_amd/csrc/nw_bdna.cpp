// nw_bdna.cpp -- host helpers of libnwhip.so: .bdna I/O and the seeded
// synthetic-sequence generator (declared in include/nw_hip.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "nw_hip.h"

extern "C" {

// readSequence semantics (src/common/helper.cpp:3-25): the whole file, byte by
// byte, no newline stripping; an unopenable file is an error (the reference
// throws std::string(fileName), helper.cpp:5).
int nw_read_bdna(const char *path, int8_t **out, int64_t *n) {
    if (!path || !out || !n) return NW_ERR_ARG;
    *out = nullptr;
    *n = 0;
    FILE *f = std::fopen(path, "rb");
    if (!f) return NW_ERR_ARG;
    int64_t cap = 1 << 16, len = 0;
    int8_t *buf = (int8_t *)std::malloc((size_t)cap);
    if (!buf) {
        std::fclose(f);
        return NW_ERR_OOM;
    }
    for (;;) {
        if (len == cap) {
            cap *= 2;
            int8_t *nb = (int8_t *)std::realloc(buf, (size_t)cap);
            if (!nb) {
                std::free(buf);
                std::fclose(f);
                return NW_ERR_OOM;
            }
            buf = nb;
        }
        size_t got = std::fread(buf + len, 1, (size_t)(cap - len), f);
        len += (int64_t)got;
        if (got == 0) break;
    }
    std::fclose(f);
    *out = buf;
    *n = len;
    return NW_OK;
}

void nw_free(void *p) { std::free(p); }

// i.i.d. uniform bytes in {1,2,3,4} (the .bdna alphabet, README.md:8) from a
// SplitMix64 stream; SURVEY.md 8(d) fixes seeds 1 (s1) and 2 (s2).
void nw_synth_bdna(uint64_t seed, int64_t n, int8_t *out) {
    uint64_t x = seed;
    for (int64_t i = 0; i < n; ++i) {
        x += 0x9E3779B97F4A7C15ull;
        uint64_t z = x;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        out[i] = (int8_t)(1 + (z >> 62));
    }
}

}  // extern "C"

// Walk alignment ops from (begin_i, begin_j); f(k, op, i, j) sees the cell BEFORE
// the move, i.e. the characters s2[i] / s1[j] that the move consumes.
template <typename F>
static int walk_ops(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t i, int64_t j,
                    const uint8_t *ops, int64_t n_ops, F &&f) {
    if (n1 < 0 || n2 < 0 || n_ops < 0 || i < 0 || j < 0 || i > n2 || j > n1) return NW_ERR_ARG;
    if ((n_ops > 0 && !ops) || (n1 > 0 && !s1) || (n2 > 0 && !s2)) return NW_ERR_ARG;
    for (int64_t k = 0; k < n_ops; ++k) {
        const uint8_t op = ops[k];
        if (op > 2) return NW_ERR_ARG;
        if ((op != 2 && i >= n2) || (op != 1 && j >= n1)) return NW_ERR_ARG;
        f(k, op, i, j);
        i += op != 2;
        j += op != 1;
    }
    return NW_OK;
}

extern "C" {

int nw_ops_expand(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i, int64_t begin_j,
                  const uint8_t *ops, int64_t n_ops, int8_t *row1, int8_t *row2) {
    if (n_ops > 0 && (!row1 || !row2)) return NW_ERR_ARG;
    return walk_ops(s1, n1, s2, n2, begin_i, begin_j, ops, n_ops, [&](int64_t k, uint8_t op, int64_t i, int64_t j) {
        row1[k] = op != 1 ? s1[j] : 0;
        row2[k] = op != 2 ? s2[i] : 0;
    });
}

int nw_ops_score(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i, int64_t begin_j,
                 const uint8_t *ops, int64_t n_ops, const nw_params *p, int64_t *score) {
    if (!p || !score) return NW_ERR_ARG;
    int64_t sum = 0;
    const int st = walk_ops(s1, n1, s2, n2, begin_i, begin_j, ops, n_ops, [&](int64_t, uint8_t op, int64_t i, int64_t j) {
        sum += op != 0 ? p->gap : s1[j] == s2[i] ? p->match : p->mismatch;
    });
    if (st == NW_OK) *score = sum;
    return st;
}

int nw_ops_score_affine(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i, int64_t begin_j,
                        const uint8_t *ops, int64_t n_ops, const nw_params *p, int32_t gap_open, int64_t *score) {
    if (!p || !score) return NW_ERR_ARG;
    int64_t sum = 0;
    uint8_t prev = 0;  // (a diag: the first gap op opens a run)
    const int st = walk_ops(s1, n1, s2, n2, begin_i, begin_j, ops, n_ops, [&](int64_t, uint8_t op, int64_t i, int64_t j) {
        if (op != 0)
            sum += p->gap + (op != prev ? gap_open : 0);
        else
            sum += s1[j] == s2[i] ? p->match : p->mismatch;
        prev = op;
    });
    if (st == NW_OK) *score = sum;
    return st;
}

int nw_ops_score_matrix(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i, int64_t begin_j,
                        const uint8_t *ops, int64_t n_ops, const nw_params *p, const nw_submat *m, int32_t gap_open,
                        int64_t *score) {
    if (!p || !score || !m || m->n < 1 || m->n > NW_SUBMAT_MAX) return NW_ERR_ARG;
    if (m->reserved[0] != 0 || m->reserved[1] != 0 || m->reserved[2] != 0) return NW_ERR_ARG;
    for (int b = 0; b < 256; ++b)
        if (m->index[b] >= m->n) return NW_ERR_ARG;
    int64_t sum = 0;
    uint8_t prev = 0;  // (a diag: the first gap op opens a run)
    const int st = walk_ops(s1, n1, s2, n2, begin_i, begin_j, ops, n_ops, [&](int64_t, uint8_t op, int64_t i, int64_t j) {
        if (op != 0)
            sum += p->gap + (op != prev ? gap_open : 0);
        else
            sum += m->score[m->index[(uint8_t)s1[j]] * NW_SUBMAT_MAX + m->index[(uint8_t)s2[i]]];
        prev = op;
    });
    if (st == NW_OK) *score = sum;
    return st;
}

int nw_ops_score_dual(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i, int64_t begin_j,
                      const uint8_t *ops, int64_t n_ops, const nw_params *p, const nw_submat *m, int32_t gap_open,
                      int32_t gap_open2, int32_t gap2, int64_t *score) {
    if (!p || !score || !m || m->n < 1 || m->n > NW_SUBMAT_MAX) return NW_ERR_ARG;
    if (m->reserved[0] != 0 || m->reserved[1] != 0 || m->reserved[2] != 0) return NW_ERR_ARG;
    for (int b = 0; b < 256; ++b)
        if (m->index[b] >= m->n) return NW_ERR_ARG;
    int64_t sum = 0, run = 0;  // run: ops of the maximal run of ups or of lefts that is open
    uint8_t prev = 0;          // (a diag: the first gap op opens a run)
    auto close = [&]() {       // the run, priced whole by its better piece
        if (run > 0) sum += std::max((int64_t)gap_open + run * p->gap, (int64_t)gap_open2 + run * gap2);
        run = 0;
    };
    const int st = walk_ops(s1, n1, s2, n2, begin_i, begin_j, ops, n_ops, [&](int64_t, uint8_t op, int64_t i, int64_t j) {
        if (op != prev) close();
        if (op != 0)
            run += 1;
        else
            sum += m->score[m->index[(uint8_t)s1[j]] * NW_SUBMAT_MAX + m->index[(uint8_t)s2[i]]];
        prev = op;
    });
    close();
    if (st == NW_OK) *score = sum;
    return st;
}

}  // extern "C"
