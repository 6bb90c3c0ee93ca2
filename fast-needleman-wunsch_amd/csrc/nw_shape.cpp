// nw_shape.cpp -- every decision of libnwhip.so that needs no device: kernel
// family and strip / panel shape of a fill, the band layouts, and which
// parameters a launch or a traceback accepts.
#include <algorithm>

#include "nw_host_int.h"
#include "nw_tuned.h"

namespace nwh {
namespace {

constexpr int kLdsPerCU = 160 * 1024;

// Strip shape for nw_params.substrips = strip_waves = 0: the measured table of
// tools/tune.py (csrc/nw_tuned.h, by table size), else (2, 2).  The table is
// measured on squares.  A table at least 4x wider than tall is bound by the
// chain of strip-to-strip hand-offs (strips x hop latency) rather than by its
// stores, and wants the shape with the shortest hop: measured with
// tools/rect_time.py, 524288 x 8191 fills in 15.5 ms with (4,1) against 19.9
// (2,2) and 29.7 (1,4); 524288 x 65535 in 33.0 ms with (2,2), 33.7 (4,1), 37.4 (1,4).
void tuned_shape(int64_t n1, int64_t n2, int32_t *c, int32_t *nc, int32_t *kernel = nullptr, int cus = 0) {
    const double cells = (double)(n1 + 1) * (double)(n2 + 1);
    *c = 2;
    *nc = 2;
    if (kernel) *kernel = NW_KERNEL_STRIPS;
    if (n1 + 1 >= 4 * (n2 + 1) && n1 >= 65536) {
        *c = n2 + 1 <= 32768 ? 4 : 2;
        *nc = n2 + 1 <= 32768 ? 1 : 2;
        return;
    }
    // a panel entry applies only when every CU gets a panel in one pass (the
    // table is measured on squares; a tall narrow table with as many cells would
    // leave CUs idle) -- otherwise the last strip entry that applies stands
    for (const auto &e : nw::kTuned) {
        if (cells < e.min_cells) continue;
        if (e.kernel == NW_KERNEL_PANELS) {
            if (!kernel || !nw::panel_shape_ok(e.c, e.nc) || n1 + 1 < (int64_t)cus * nw::kWave * e.c * e.nc) continue;
            *kernel = NW_KERNEL_PANELS;
        } else {
            if (!nw::shape_ok(e.c, e.nc)) continue;
            if (kernel) *kernel = NW_KERNEL_STRIPS;
        }
        *c = e.c;
        *nc = e.nc;
    }
}

// Panel shape for nw_params.kernel = PANELS with substrips = strip_waves = 0:
// the widest panel that still gives every CU a panel (a panel is one CU's
// work; the 256k square has 262144 / 1024 = 256 of (4,4)).
void panel_auto(int64_t n1, int cus, int32_t *c, int32_t *nw) {
    const int64_t cols = n1 + 1;
    if (cols >= (int64_t)cus * 1024) {
        *c = 4;
        *nw = 4;
    } else if (cols >= (int64_t)cus * 512) {
        *c = 2;
        *nw = 4;
    } else {
        *c = 4;
        *nw = 1;
    }
}

}  // namespace

// col0: first swept column (1 when the table's column 1 starts a 256-byte line)
Shape make_shape(int64_t n1, int64_t n2, int32_t waves_req, int32_t sub_req, int32_t nc_req, int cus,
                 int64_t col0, bool sw, int32_t kernel_req) {
    Shape s;
    s.kernel = kernel_req == NW_KERNEL_PANELS ? NW_KERNEL_PANELS : NW_KERNEL_STRIPS;
    if (kernel_req == NW_KERNEL_AUTO && sub_req <= 0 && nc_req <= 0 && !sw) {
        // the measured choice of kernel family and shape (csrc/nw_tuned.h)
        tuned_shape(n1, n2, &s.K, &s.NC, &s.kernel, cus);
    } else if (s.kernel == NW_KERNEL_PANELS) {
        if (sub_req <= 0 && nc_req <= 0) {
            panel_auto(n1, cus, &s.K, &s.NC);
        } else {
            s.K = sub_req > 0 ? sub_req : 4;
            s.NC = nc_req > 0 ? nc_req : 4;
        }
    } else if (sub_req <= 0 && nc_req <= 0 && sw) {
        // Smith-Waterman cells cost 4 VALU instead of 2, which moves the balance
        // toward more compute waves: 65536^2 (tools/sw_shapes.py) (2,2) 7.15 ms,
        // (4,1) 7.57, (2,1) 7.95, (1,4) 8.64
        s.K = 2;
        s.NC = 2;
    } else if (sub_req <= 0 && nc_req <= 0) {
        tuned_shape(n1, n2, &s.K, &s.NC);
    } else {
        s.K = sub_req > 0 ? sub_req : 2;
        s.NC = nc_req > 0 ? nc_req : (s.K == 1 ? 4 : s.K == 2 ? 2 : 1);
    }
    s.nRows = n2 + 1;
    s.nCols = n1 + 1;
    const int64_t width = (int64_t)nw::kWave * s.K * s.NC;
    s.nstrips = std::max<int64_t>(1, (s.nCols - col0 + width - 1) / width);
    s.nblocks = (s.nRows + nw::kWave - 1) / nw::kWave;
    // one strip workgroup per LDS ring set; as many as fit in a CU's LDS (a
    // panel workgroup is 2 * NW waves: at most 32 waves per CU)
    const int lds = s.kernel == NW_KERNEL_PANELS ? nw::panel_lds_bytes(s.K, s.NC) : nw::lds_bytes(s.K, s.NC);
    int64_t per_cu = std::max(1, kLdsPerCU / std::max(lds, 1));
    // a panel workgroup (NW compute, 2-3 store waves per compute wave, 2 feeder
    // waves, ~88 VGPRs each) fills a CU's wave slots on its own
    if (s.kernel == NW_KERNEL_PANELS) per_cu = 1;
    int64_t w = waves_req > 0 ? waves_req : per_cu * cus;
    s.waves_max = std::max<int64_t>(1, w);
    s.waves = std::max<int64_t>(1, std::min<int64_t>(w, s.nstrips));
    // Strip p publishes into slot p % M.  When strip p is claimed, every strip
    // <= p - waves has finished, so M = waves + 1 slots never alias a live one.
    s.M = std::min<int64_t>(s.nstrips, s.waves + 1);
    s.gstride = s.nblocks * nw::kWave;
    return s;
}

// Row / column band fills: AUTO means the strips (the tuned table is measured
// on whole square tables, and a band's geometry is set by its caller).
int32_t band_kernel(int32_t k) { return k == NW_KERNEL_AUTO ? NW_KERNEL_STRIPS : k; }

bool shape_valid(const Shape &s) {
    return s.kernel == NW_KERNEL_PANELS ? nw::panel_shape_ok(s.K, s.NC) : nw::shape_ok(s.K, s.NC);
}

// the range of nw_params.gap (and of the two-piece entries' gap2)
bool valid_gap(int32_t gap) { return std::abs(gap) < (1 << 12); }

bool valid_params(const nw_params *p) {
    if (!p) return false;
    if (p->mode != NW_MODE_NW && p->mode != NW_MODE_SW) return false;
    if (p->mode == NW_MODE_SW && p->gap > 0) return false;  // local alignment needs a penalty
    if (p->substrips != 0 && p->substrips != 1 && p->substrips != 2 && p->substrips != 4) return false;
    if (p->strip_waves != 0 && p->strip_waves != 1 && p->strip_waves != 2 && p->strip_waves != 4 &&
        p->strip_waves != 8)
        return false;
    if (p->kernel != NW_KERNEL_AUTO && p->kernel != NW_KERNEL_STRIPS && p->kernel != NW_KERNEL_PANELS) return false;
    if (p->timeout_ms < 0) return false;
    // known flag bits only; the debug probes leave the table unwritten, so only with TIMING_ONLY
    const int32_t dbg = NW_FLAG_DEBUG_DRAIN | NW_FLAG_DEBUG_NO_STORE;
    if ((p->flags & ~(NW_FLAG_TIMING_ONLY | NW_FLAG_NO_PROFILE | NW_FLAG_NO_FINISH | NW_FLAG_DEBUG_NO_CHAIN |
                      NW_FLAG_DEBUG_STAGGER | dbg)) != 0)
        return false;
    if ((p->flags & NW_FLAG_DEBUG_STAGGER) && !(p->flags & NW_FLAG_DEBUG_NO_CHAIN)) return false;
    if ((p->flags & dbg) != 0 && (p->flags & NW_FLAG_TIMING_ONLY) == 0) return false;
    // keep every intermediate far from int32 overflow (|score| < 2^29)
    const int32_t lim = 1 << 12;
    return std::abs(p->match) < lim && std::abs(p->mismatch) < lim && valid_gap(p->gap);
}

// Arguments of nw_traceback / nw_align that need no device to judge; on NW_OK the
// window geometry (defaults applied) and the aim.
int tb_args(int64_t n1, int64_t n2, const nw_params *p, const nw_tb_opts *o, const uint8_t *ops, int64_t ops_cap,
            const nw_alignment *out, int32_t *band, int32_t *maxwin, int32_t *aim) {
    if (!out || n1 < 0 || n2 < 0 || n1 >= INT32_MAX || n2 >= INT32_MAX) return NW_ERR_ARG;
    if (!valid_params(p) || p->mode != NW_MODE_NW) return NW_ERR_ARG;
    // the table must hold a fill: no scratch-tile stores, no probes
    if ((p->flags & (NW_FLAG_TIMING_ONLY | NW_FLAG_DEBUG_DRAIN | NW_FLAG_DEBUG_NO_STORE | NW_FLAG_DEBUG_NO_CHAIN |
                     NW_FLAG_DEBUG_STAGGER)) != 0)
        return NW_ERR_ARG;
    if (ops_cap < n1 + n2 || (n1 + n2 > 0 && !ops)) return NW_ERR_ARG;
    *band = nw::kTbBandDefault;
    *maxwin = nw::kTbMaxWinDefault;
    *aim = 1;
    if (o) {
        if (o->band < 0 || o->band > 256 || o->max_windows < 0 || (o->flags & ~NW_TB_NO_AIM) != 0 || o->reserved != 0)
            return NW_ERR_ARG;
        if (o->band > 0) *band = o->band;
        if (o->max_windows > 0) *maxwin = o->max_windows;
        *aim = (o->flags & NW_TB_NO_AIM) ? 0 : 1;
    }
    return NW_OK;
}

// Column band r of nbands (nw_colband_layout): strips [sf, sf + sc) of the whole
// table's sweep (col0 = 1), local column 0 = global column start = sf * W.
int colband_layout(int64_t n1, int64_t n2, int32_t nb, int32_t r, const nw_params *p, int cus, int64_t *sf,
                   int64_t *sc, int64_t *start, int64_t *ncols) {
    if (!p || n1 < 1 || n2 < 0 || nb < 1 || r < 0 || r >= nb) return NW_ERR_ARG;
    const Shape s = make_shape(n1, n2, 0, p->substrips, p->strip_waves, cus, 1, false, band_kernel(p->kernel));
    if (!shape_valid(s) || nb > s.nstrips) return NW_ERR_ARG;
    const int64_t W = (int64_t)nw::kWave * s.K * s.NC;
    const int64_t base = s.nstrips / nb, extra = s.nstrips % nb;
    *sf = r * base + std::min<int64_t>(r, extra);
    *sc = base + (r < extra ? 1 : 0);
    *start = *sf * W;
    *ncols = std::min(*sc * W, n1 - *start) + 1;  // + the left column (band r-1's last)
    return NW_OK;
}

}  // namespace nwh

using namespace nwh;

extern "C" {

void nw_band_layout(int64_t n2, int32_t nbands, int32_t r, int64_t *n_rows, int64_t *start) {
    // mpi-horz-driver.cpp:31-32 / mpi-horz.cpp:16: base = (n2+1)/P rows per band; bands
    // after the first carry one extra (halo) row; the last band takes the remainder.
    int64_t rows = 0, st = 0;
    if (nbands > 0 && r >= 0 && r < nbands) {
        const int64_t total = n2 + 1, base = total / nbands;
        rows = base + (r > 0 ? 1 : 0) + (r == nbands - 1 ? total % nbands : 0);
        st = base * r - (r > 0 ? 1 : 0);
    }
    if (n_rows) *n_rows = rows;
    if (start) *start = st;
}

int nw_colband_layout(int64_t n1, int64_t n2, int32_t nbands, int32_t r, const nw_params *p,
                      int64_t *strip_first, int64_t *strip_count, int64_t *start, int64_t *n_cols) {
    int64_t sf = 0, sc = 0, st = 0, nc = 0;
    const int rc = colband_layout(n1, n2, nbands, r, p, 256, &sf, &sc, &st, &nc);
    if (strip_first) *strip_first = sf;
    if (strip_count) *strip_count = sc;
    if (start) *start = st;
    if (n_cols) *n_cols = nc;
    return rc;
}

void nw_tuned_shape(int64_t n1, int64_t n2, int32_t *substrips, int32_t *strip_waves) {
    int32_t c = 2, nc = 2;
    if (n1 >= 0 && n2 >= 0) tuned_shape(n1, n2, &c, &nc);
    if (substrips) *substrips = c;
    if (strip_waves) *strip_waves = nc;
}

void nw_auto_shape(int64_t n1, int64_t n2, int32_t cus, int32_t *kernel, int32_t *substrips, int32_t *strip_waves) {
    int32_t k = NW_KERNEL_STRIPS, c = 2, nc = 2;
    if (n1 >= 0 && n2 >= 0) tuned_shape(n1, n2, &c, &nc, &k, std::max(cus, 1));
    if (kernel) *kernel = k;
    if (substrips) *substrips = c;
    if (strip_waves) *strip_waves = nc;
}

}  // extern "C"
