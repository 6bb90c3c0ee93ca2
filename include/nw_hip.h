/*
 * nw_hip.h -- C ABI of libnwhip.so, the MI355X (gfx950) Needleman-Wunsch fill.
 *
 * This is the drop-in boundary for the reference's fill plugins.  The reference
 * selects a fill at link time: every fill TU defines
 *
 *     void needlemanWunsch(dnaArray s1, dnaArray s2, int* t);
 *       src/serial/serial.cpp:4          (serial -- the oracle)
 *       src/sentinel/sentinel-mt.cpp:4   (sentinel-mt)
 *       src/idxarray/idxarray-mt.cpp:4   (idxarray-mt)
 *
 * and textually includes src/common/driver.cpp (its main(), :1-40).  The
 * MI355X drop-in TU (fast-needleman-wunsch_amd/dropin/needleman-wunsch-hip.cpp)
 * defines that same C++ symbol and forwards to nw_fill() below.  Everything in
 * this header is plain C: pointers, sizes, PODs -- no HIP or torch types.
 *
 * Table layout (reference contract, serial.cpp:6-7,21-31): nRows = n2 + 1
 * (s2 "down the side"), nCols = n1 + 1 (s1 "across the top"), cell (i, j) at
 * t[i * nCols + j], int32.  On the device the library may use a row pitch
 * >= nCols (see nw_table_pitch); host copies always use the reference layout.
 */
#ifndef NW_HIP_H
#define NW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes (the reference's fill is void and cannot fail; the C ABI reports
 * what the device path can: bad arguments, HIP errors, OOM, a watchdog trip) */
enum {
    NW_OK = 0,
    NW_ERR_ARG = 1,       /* invalid argument (sizes, pitch, alignment, mode)   */
    NW_ERR_HIP = 2,       /* a HIP runtime call failed                         */
    NW_ERR_OOM = 3,       /* device allocation failed / table does not fit     */
    NW_ERR_TIMEOUT = 4,   /* a bounded in-kernel wait expired (never expected) */
    NW_ERR_NODEVICE = 5,  /* no gfx950 device visible                          */
    NW_ERR_UNSUPPORTED = 6
};
enum { NW_ERR_TABLE = 7 };  /* traceback: a cell no move reproduces -- not a table of these params */

/* nw_params.mode: global alignment (the reference fills) or Smith-Waterman local
 * alignment (BASELINE config 5; no reference counterpart -- conventions in
 * nw_sw_align below) */
enum { NW_MODE_NW = 0, NW_MODE_SW = 1 };

/* nw_params.flags (0 = normal fill) */
enum {
    NW_FLAG_TIMING_ONLY = 1, /* table stores go to a scratch tile (kernel timing only) */
    NW_FLAG_NO_PROFILE = 2,  /* substitution by byte compares instead of the per-lane
                                v_perm score tables */
    NW_FLAG_NO_FINISH = 4,   /* nw_fill_tband_async: sweep every row in strips, also a
                                last strip that runs alone as one more pass (default:
                                such rows go to the row-scan finisher) */
    /* debug probes of the compute pace: only together with NW_FLAG_TIMING_ONLY
       (refused otherwise -- the table is not written) */
    NW_FLAG_DEBUG_DRAIN = 0x100,    /* store waves drain the LDS ring without reading it */
    NW_FLAG_DEBUG_NO_STORE = 0x200, /* no store waves at all */
    /* store-pattern probe (strip kernel, no halo / feed): every strip takes the
       boundary column instead of its left neighbour's and publishes nothing, so the
       strips run unchained; the table IS written to HBM but holds no fill (refused
       on bands and in NW_MODE_SW, whose best cell would be meaningless) */
    NW_FLAG_DEBUG_NO_CHAIN = 0x400,
    /* with NO_CHAIN: strip p of a one-pass launch starts p * 11.5 us after it is
       claimed -- the chained sweep's diagonal, without its hand-offs */
    NW_FLAG_DEBUG_STAGGER = 0x800
};

/* nw_params.kernel: which gfx950 kernel family fills the table.  Both compute
 * the same cells (serial.cpp:21-33); they differ in how the wavefront maps onto
 * a wave:
 *   STRIPS: a wave holds an ANTI-DIAGONAL of a 64*C-column strip (lane = row
 *           offset; DPP carries the left neighbour), rows leave through a
 *           128-slot LDS ring.  Shapes (substrips C, strip_waves NC): (4,1)
 *           (2,1) (1,1) (2,2) (1,2) (1,4); and (2,4), Smith-Waterman only: 512-
 *           column strips on half-word rings, refused (NW_ERR_UNSUPPORTED) when
 *           more than 64 cells could reach 2^16 (max(match, mismatch) * min(i, j)
 *           >= 65536), which are then recomputed exactly after the fill.
 *   PANELS: a wave holds a ROW of 64*C columns, computed as a prefix maximum
 *           (lane-local prefix + a 64-lane DPP max-scan) in the w form; rows
 *           leave through a 32-row ring.  Shapes (C, NW compute waves per
 *           panel): (4,4) (4,2) (2,4) (4,1) (2,2) (1,4).
 *   AUTO:   with substrips = strip_waves = 0, the measured family and shape
 *           for the table size (nw_auto_shape); with an explicit shape, STRIPS.
 *           Smith-Waterman, row-band and column-band AUTO fills use the strips. */
enum { NW_KERNEL_AUTO = 0, NW_KERNEL_STRIPS = 1, NW_KERNEL_PANELS = 2 };

/* Runtime replacement for the compile-time constants of
 * src/common/needleman-wunsch.hpp:11-13 (MATCH 1, MISMATCH 0, GAP -1). */
typedef struct nw_params {
    int32_t match;     /* default  1 */
    int32_t mismatch;  /* default  0 */
    int32_t gap;       /* default -1 */
    int32_t mode;      /* NW_MODE_NW */
    int32_t waves;     /* persistent strip workers (waves; 0 = auto)     */
    int32_t device;    /* HIP device ordinal, -1 = current device         */
    int32_t flags;     /* NW_FLAG_* bits, 0 for a normal fill            */
    int32_t substrips; /* columns per lane C of a compute wave (1, 2 or 4); 0 = auto */
    int32_t strip_waves; /* chained compute waves per strip NC (1, 2 or 4); 0 = auto.
                            A strip is NC * 64 * C columns; supported (C, NC):
                            (4,1) (2,1) (1,1) (2,2) (1,2) (1,4), SW also (2,4)
                            (see NW_KERNEL_AUTO); auto = the tuned
                            shape for the size (nw_tuned_shape) */
    int32_t timeout_ms;  /* bound of every in-kernel wait (hand-off, halo, ring);
                            0 = 20000.  A wait that expires makes the fill return
                            NW_ERR_TIMEOUT instead of hanging the device. */
    int32_t kernel;      /* NW_KERNEL_*; 0 = auto.  With PANELS, substrips /
                            strip_waves are the panel's (C, NW): a panel is
                            NW * 64 * C columns */
} nw_params;

typedef struct nw_result {
    int32_t score;          /* t[n2][n1] -- what driver.cpp:35 prints     */
    int32_t status;         /* NW_OK or an error code                     */
    int64_t cells;          /* n1 * n2 inner cells (GCUPS numerator)      */
    double kernel_ms;       /* device time of the fill (HIP events)       */
    double table_bytes;     /* bytes of table stored: 4 * nRows * nCols   */
    int32_t strips;         /* strips swept (64 * substrips * strip_waves columns each) */
    int32_t waves;          /* persistent workers launched                */
    int32_t substrips;      /* columns per lane of a compute wave         */
    int32_t strip_waves;    /* compute waves per strip                    */
    int64_t end_i, end_j;   /* cell `score` was read from: (n2, n1) for NW; for SW
                               the best cell, first in row-major order     */
    int32_t kernel;         /* NW_KERNEL_STRIPS or NW_KERNEL_PANELS (what ran) */
    int32_t reserved;
} nw_result;

/* An alignment: Smith-Waterman (nw_sw_align / nw_sw_traceback) or global (nw_align /
 * nw_traceback: begin = (0, 0), end = (n2, n1), score = t[n2][n1]). */
typedef struct nw_alignment {
    int32_t score;           /* t[end_i][end_j], the table maximum            */
    int32_t status;
    int64_t begin_i, begin_j; /* cell where the traceback reached t == 0      */
    int64_t end_i, end_j;    /* best cell (first row-major maximum)          */
    int64_t n_ops;           /* ops written, path order begin -> end          */
    double fill_ms, traceback_ms;
} nw_alignment;

/* Fill `p` with the reference defaults (1, 0, -1). */
void nw_params_default(nw_params *p);

/* Human-readable text for a status code. */
const char *nw_strerror(int status);

/* Library / kernel build identification (gfx target, kernel variant). */
const char *nw_version(void);

/*
 * One-shot fill from host buffers (the drop-in path).  Copies s1/s2 to the
 * device, fills the whole table in HBM, and -- when host_t != NULL -- copies
 * the table back in the reference layout (nCols-pitched, (n2+1)*(n1+1) ints).
 * With host_t == NULL only the score is returned.  Returns NW_OK or an error.
 * Replaces needlemanWunsch() of serial.cpp:4 / sentinel-mt.cpp:4 /
 * idxarray-mt.cpp:4 (called from driver.cpp:28).
 */
int nw_fill(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2,
            const nw_params *p, int32_t *host_t, nw_result *out);

/*
 * nw_fill, nw_fill_emb and nw_sw_align keep per-device state between calls: a
 * context, the device table (kept when at most 16 GiB) and sequence buffers,
 * and three pinned staging chunks (up to 256 MiB each) through which the
 * table is copied back (DMA of the next chunks overlapping the threaded copy of
 * one into host_t; NW_COPY_THREADS sets the copy threads, default min(8, cores):
 * it is read on every call and clamped to 1..64 -- 0, a negative or a
 * non-numeric value is 1, anything above 64 is 64; a chunk below 8 MiB is one
 * memcpy whatever the count).  The chunks only grow, so how a table is cut
 * depends on the largest table since the last nw_host_release.
 * nw_host_warmup(device) creates it ahead of the first call (context, copy
 * stream, staging; not the table, whose size is not known yet; -1: the current
 * device); nw_host_release(device) frees it (-1: every device).
 * NW_HOST_TIMING=1 prints nw_fill's phases (prepare, fill, copy back) to stderr.
 */
int nw_host_warmup(int device);
void nw_host_release(int device);

/*
 * The same fill into the "emb" table layout of the reference's second driver
 * (src/common/driver2.cpp:20-22 allocates (s1.size+2) * (s2.size+1) ints;
 * src/idxarray/idxarray-emb-mt.cpp:4-65 fills it): rows of n1+2 ints, column 0
 * = each row's progress counter at its final value n1+2, columns 1 .. n1+1 = the
 * serial table.  host_t is required.
 */
int nw_fill_emb(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2,
                const nw_params *p, int32_t *host_t, nw_result *out);

/*
 * Smith-Waterman local alignment with on-device traceback (BASELINE config 5).
 * Table: t[i][0] = t[0][j] = 0, t[i][j] = max(0, t[i-1][j-1] + s, t[i-1][j] + GAP,
 * t[i][j-1] + GAP) (gap <= 0).  Best cell: the maximum, first in row-major
 * order.  Traceback from it while t > 0, preferring diag > up > left (the order
 * of serial.cpp:24-30's max).  ops[k] (path order, begin -> end): 0 = diagonal
 * (s1[j-1] against s2[i-1]), 1 = up (s2[i-1] against a gap), 2 = left (s1[j-1]
 * against a gap); ops_cap >= n1 + n2 always suffices.  p->mode must be
 * NW_MODE_SW.  The reference has no local alignment: parity is against the
 * build's CPU restatement (oracle/nw_oracle.c), not the reference.
 */
int nw_sw_align(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
                uint8_t *ops, int64_t ops_cap, nw_alignment *out);

/* Device-resident API ------------------------------------------------------ */
typedef struct nw_ctx nw_ctx;

/*
 * Global alignment with on-device traceback: the path of the Needleman-Wunsch
 * table from (n2, n1) back to (0, 0), taking at every cell the first move that
 * reproduces t, diag > up > left (the order of serial.cpp:24-30's max); along
 * row 0 the moves are left, along column 0 up.  ops as in nw_sw_align (path order
 * begin -> end: 0 diagonal, 1 up, 2 left); a global path has between max(n1, n2)
 * and n1 + n2 ops, and ops_cap >= n1 + n2 is required up front.
 * out->begin_* = (0, 0), out->end_* = (n2, n1), out->score = t[n2][n1].
 */
enum { NW_TB_NO_AIM = 1 };    /* nw_tb_opts.flags */
typedef struct nw_tb_opts {   /* NULL = defaults */
    int32_t band;             /* window half-width B, 1..256; 0 = 256 */
    int32_t max_windows;      /* windows (of 64 rows) per round, >= 1; 0 = 512 */
    int32_t flags;            /* NW_TB_NO_AIM: rounds on the slope-1 diagonal instead of
                                 aimed at (0, 0) (A/B and tests); other bits refused */
    int32_t reserved;         /* must be 0 */
} nw_tb_opts;

typedef struct nw_tb_stats {
    int32_t rounds, windows;  /* rounds run (one stream synchronisation each), windows launched */
    int32_t band, max_windows; /* the geometry used */
    int64_t tail_ops;         /* ops of the forced run along row 0 / column 0 (one memset) */
} nw_tb_stats;

/* Traceback of a device-resident table filled in NW_MODE_NW by nw_fill_device /
 * nw_fill_device_async.  Stream-ordered after the fill on `stream` (a
 * hipStream_t, NULL = default stream); synchronises that stream only.  `stats`
 * may be NULL.  Refused with NW_ERR_ARG before any device work: p->mode other than
 * NW_MODE_NW, p->flags with NW_FLAG_TIMING_ONLY or a debug bit (the table would
 * not hold a fill), ops_cap < n1 + n2, ops == NULL with n1 + n2 > 0, band outside
 * 0..256, max_windows < 0, unknown opts flags, reserved != 0.  NW_ERR_TABLE: the
 * walk met a cell that no move reproduces (the table is not a fill of these
 * sequences and parameters); reported at the end of that round. */
int nw_traceback(nw_ctx *ctx, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2,
                 const nw_params *p, const int32_t *d_t, int64_t pitch, const nw_tb_opts *o,
                 void *stream, uint8_t *ops, int64_t ops_cap, nw_alignment *out, nw_tb_stats *stats);

/* Strip shape (columns per lane C, chained compute waves NC) that a fill with
 * nw_params.substrips = strip_waves = 0 uses for an n1 x n2 table: the table
 * measured by tools/tune.py (the analogue of the reference's block tuner,
 * src/common/block-tuner.cpp:26-34, src/block-tune.sh). */
void nw_tuned_shape(int64_t n1, int64_t n2, int32_t *substrips, int32_t *strip_waves);

/* Kernel family and shape a global-alignment fill with kernel = substrips =
 * strip_waves = 0 uses for an n1 x n2 table on a device with `cus` compute units
 * (hipDeviceProp_t.multiProcessorCount): the same measured table, whose panel
 * entries apply only when every CU gets a panel (n1 + 1 >= cus * 64 * C * NW). */
void nw_auto_shape(int64_t n1, int64_t n2, int32_t cus, int32_t *kernel, int32_t *substrips,
                   int32_t *strip_waves);

/* Row pitch (in int32 elements) the library allocates for nCols = n1+1: a
 * multiple of 64 (256-byte rows) with at least 3 columns of slack after column
 * n1, which the strips need to start at column 1 (nw_table_offset).  Any
 * multiple of 64 >= n1 + 1 is accepted; a tighter one sweeps from column 0. */
int64_t nw_table_pitch(int64_t n1);

/* Bytes of device memory a table of (n2+1) rows at nw_table_pitch(n1) takes. */
int64_t nw_table_bytes(int64_t n1, int64_t n2);

/* Preferred element offset of the table base from a 256-byte aligned
 * allocation (of nw_table_bytes + 256 bytes): 63, which puts column 1 of every
 * row on a 256-byte line.  The fill then sweeps columns 1..n1 only -- an
 * N x N table is exactly N / 256 strips -- and stores the boundary column 0
 * separately.  A 256-byte aligned base (offset 0) is accepted too. */
int64_t nw_table_offset(void);

/* LDS bytes of one strip workgroup of shape (C = substrips, NC = strip_waves),
 * -1 for an unsupported shape.  A CU holds floor(160 KiB / this) of them; a
 * caller co-scheduling several fills on one device (LocalBands) sizes their
 * `waves` from it so that all of them stay resident. */
int64_t nw_strip_lds_bytes(int32_t substrips, int32_t strip_waves);
/* LDS bytes of one PANEL workgroup (NW_KERNEL_PANELS) of shape (C, NW); -1 if
 * unsupported. */
int64_t nw_panel_lds_bytes(int32_t substrips, int32_t strip_waves);

/* Create / destroy a context bound to `device` (-1 = current).  The context
 * owns the hand-off workspace and the strip ticket counter. */
int nw_ctx_create(int device, nw_ctx **out);
void nw_ctx_destroy(nw_ctx *ctx);

/* Workspace bytes the context will allocate for this shape (advisory). */
int64_t nw_ctx_workspace_bytes(int64_t n1, int64_t n2, int32_t waves);

/*
 * Fill a device-resident table.  d_s1/d_s2: device int8 sequences; d_t: device
 * table with row pitch `pitch` (a multiple of 64 >= n1 + 1; nw_table_pitch
 * preferred), base 256-byte aligned or -- preferred -- 4 bytes short of it
 * (nw_table_offset; used when pitch >= n1 + 4).
 * `stream` is a hipStream_t (NULL = default stream).
 * Asynchronous with respect to the host unless out != NULL, in which case the
 * call synchronises the stream and fills `out` (score read back from HBM).
 */
int nw_fill_device(nw_ctx *ctx, const int8_t *d_s1, int64_t n1,
                   const int8_t *d_s2, int64_t n2, const nw_params *p,
                   int32_t *d_t, int64_t pitch, void *stream, nw_result *out);

/* Traceback of a device-resident SW table filled by nw_fill_device /
 * nw_fill_device_async (mode SW) from (end_i, end_j) (nw_result.end_i/end_j);
 * ops copied to the host as in nw_sw_align.  Synchronous: it first waits for
 * all work on the device (the fill may be on any stream).  `p` must be a valid
 * SW parameter set (mode NW_MODE_SW), else NW_ERR_ARG. */
int nw_sw_traceback(nw_ctx *ctx, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2,
                    const nw_params *p, const int32_t *d_t, int64_t pitch, int64_t end_i, int64_t end_j,
                    uint8_t *ops, int64_t ops_cap, nw_alignment *out);

/* One-shot global alignment from host buffers (the counterpart of nw_sw_align):
 * copies s1 / s2 to the device, fills the table in HBM, walks it there
 * (nw_traceback) and returns the ops.  p == NULL: the reference defaults.
 * n1 == 0 or n2 == 0 needs no table: the ops are all ups / all lefts and the
 * score is gap * max(n1, n2).  The refusals of nw_traceback apply, all checked
 * before any HIP call; a host without a device answers NW_ERR_NODEVICE. */
int nw_align(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
             const nw_tb_opts *o, uint8_t *ops, int64_t ops_cap, nw_alignment *out, nw_tb_stats *stats);

/* Checkpointed (linear-memory) global alignment ------------------------------
 * For tables that do not fit in HBM.  A forward SWEEP computes the whole table and
 * stores only every K-th row (the checkpoints) and the score; then the K-row
 * blocks are re-filled one at a time from the last to the first, each from its
 * checkpoint (nw_fill_band_async into one block table), and walked with
 * nw_traceback_block from the column where the path left the block below.
 * Device memory: O(K * n1) for the block table + O(n1 * n2 / K) for the
 * checkpoints; nothing proportional to n1 * n2. */
typedef struct nw_ckpt_opts {   /* NULL = defaults */
    int64_t block_rows;         /* K, a multiple of 64; 0 = planned (nw_ckpt_plan)           */
    int64_t mem_bytes;          /* device budget; 0 = 80 % of the free HBM at the call       */
    int32_t reserved[4];        /* must be 0 */
} nw_ckpt_opts;

typedef struct nw_ckpt_stats {
    int64_t block_rows, blocks;  /* K, ceil(n2 / K)                                         */
    int64_t ckpt_bytes;          /* checkpoint rows (nw_ckpt_bytes)                         */
    int64_t block_bytes;         /* the block table                                         */
    int64_t peak_bytes;          /* everything the call holds on the device at once         */
    int64_t refill_cells;        /* cells computed by the re-fills (the sweep's n1 * n2 not counted) */
    int32_t rounds, windows;     /* traceback rounds / windows over all blocks              */
    double sweep_ms, refill_ms, traceback_ms;
} nw_ckpt_stats;

/* The plan for an n1 x n2 pair within mem_bytes of device memory: the largest K (a
 * multiple of 64, at most n2 rounded up to 64) whose peak_bytes -- block table,
 * checkpoints, hand-off workspace, sequences, row packs, ops and traceback scratch,
 * as the allocations round them -- is <= mem_bytes; blocks = 1 when the whole table
 * fits.  Host only (no HIP call; the hand-off workspace is sized for 256 CUs).
 * NW_ERR_OOM when K = 64 does not fit, NW_ERR_ARG for negative sizes. */
int nw_ckpt_plan(int64_t n1, int64_t n2, int64_t mem_bytes, nw_ckpt_stats *plan);

/* peak_bytes of block height K (a multiple of 64), as nw_ckpt_plan counts it: what a
 * caller that sets nw_ckpt_opts.block_rows itself should have free; -1 for refused
 * arguments. */
int64_t nw_ckpt_peak_bytes(int64_t n1, int64_t n2, int64_t K);

/* Bytes of the checkpoint rows of an n1 x n2 sweep with block height K: nck = ceil(n2
 * / K) - 1 rows (table rows K, 2K, .. nck * K) of n1 + 1 granules {tag:32 | t:32},
 * row r at d_ckpt + r * (n1 + 1) granules -- each what nw_fill_band_async takes as
 * halo_in with nw_band.tag = NW_CKPT_TAG. */
#define NW_CKPT_TAG 1u
int64_t nw_ckpt_bytes(int64_t n1, int64_t n2, int64_t K);

/* The sweep on device buffers, asynchronous on `stream`: fills d_ckpt (may be NULL
 * when K >= n2: no checkpoint rows) and *d_score = t[n2][n1]; n1, n2 >= 1.  It stores
 * no table.  Strips of 256 columns, nw_params.waves persistent one-wave workers (0:
 * four per CU); substrips / strip_waves are not used.  Refused before any launch
 * with NW_ERR_ARG: invalid parameters or sizes beyond the int32 range of the w form,
 * mode other than NW_MODE_NW, any flag but NW_FLAG_NO_PROFILE, K <= 0 or not a
 * multiple of 64; with NW_ERR_UNSUPPORTED: kernel = NW_KERNEL_PANELS.  A wait that
 * expires (nw_params.timeout_ms) is reported by nw_ctx_status. */
int nw_ckpt_sweep_async(nw_ctx *ctx, const int8_t *d_s1, int64_t n1, const int8_t *d_s2, int64_t n2,
                        const nw_params *p, int64_t K, void *d_ckpt, int32_t *d_score, void *stream);

/* Score only, from host buffers: the sweep with no checkpoints.  out->score, cells,
 * kernel_ms (the sweep), end_i / end_j, strips, waves; table_bytes = 0 -- no table is
 * stored, so n1 x n2 is bounded by the int32 range alone.  n1 = 0 or n2 = 0 is
 * answered without a launch.  The sweep's refusals, before any HIP call; a host
 * without a device answers NW_ERR_NODEVICE. */
int nw_score(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p, nw_result *out);

/* Traceback of one row block: d_t holds global rows row0 .. row0 + rows of the table
 * over columns 0..n1 (local row 0 = the checkpoint row, as nw_fill_band_async writes
 * it from halo_in), d_s2_block the block's `rows` side characters.  Walks from local
 * (rows, n1) to local row 0: out->begin_i = row0, out->begin_j = the column where the
 * path arrived there, out->end_* = (row0 + rows, n1), ops in begin -> end order.  A
 * walk that meets column 0 first runs up it (one memset, stats->tail_ops) and
 * begin_j = 0.  With row0 = 0 it is nw_traceback (row 0 walked left to (0, 0)).
 * Aimed rounds follow the line from the global cell to the global (0, 0).
 * Refusals and NW_ERR_TABLE as nw_traceback (ops_cap >= n1 + rows). */
int nw_traceback_block(nw_ctx *ctx, const int8_t *d_s1, int64_t n1, const int8_t *d_s2_block, int64_t rows,
                       int64_t row0, const nw_params *p, const int32_t *d_t, int64_t pitch, const nw_tb_opts *o,
                       void *stream, uint8_t *ops, int64_t ops_cap, nw_alignment *out, nw_tb_stats *stats);

/* One-shot global alignment in linear memory, from host buffers.  blocks = 1 (the
 * table fits the budget): nw_align's path.  Otherwise one sweep, then per block, last
 * to first, a re-fill of its rows over columns 0..cj and its traceback (cj: where
 * the path left the block below; once cj = 0 the rest is one run of ups).  The ops
 * are byte-identical to nw_align's and `out` is filled as by nw_align (fill_ms =
 * sweep_ms + refill_ms).  NW_ERR_TABLE when the last block does not reproduce the
 * sweep's score.  nw_align's and the sweep's refusals, and block_rows < 0 or not a
 * multiple of 64, mem_bytes < 0, reserved != 0 (NW_ERR_ARG), before any HIP call;
 * NW_ERR_OOM when no K fits mem_bytes; NW_ERR_NODEVICE without a device.  `stats`
 * may be NULL. */
int nw_align_ckpt(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, const nw_params *p,
                  const nw_ckpt_opts *co, const nw_tb_opts *o, uint8_t *ops, int64_t ops_cap, nw_alignment *out,
                  nw_ckpt_stats *stats);

/* Batched pairwise global alignment ------------------------------------------
 * Many small pairs in one call.  Pairs are given CSR-style: pair i is s1cat[off1[i] ..
 * off1[i+1]) against s2cat[off2[i] .. off2[i+1]); the offsets are int64, non-
 * decreasing, off[0] = 0, npairs + 1 of them.  A persistent grid of one-wave workers
 * (nw_params.waves; 0 = four per CU, at most one per pair) claims pairs from a
 * ticket, longest first, and each worker computes its pair's whole table alone in
 * 256-column strips, the cells exactly the sweep's (csrc/nw_batch.hip).  Per batch:
 * one copy of each concatenation, one alphabet decision (v_perm tables when the
 * concatenated s1 holds at most 7 distinct characters, else byte compares) and a
 * constant number of launches; nothing per pair.  Results land at the pair's index.
 * Refused with NW_ERR_ARG before any HIP call: invalid parameters, mode other than
 * NW_MODE_NW, any flag but NW_FLAG_NO_PROFILE, npairs < 0, NULL arrays with npairs >
 * 0, offsets that do not start at 0 or decrease, a pair beyond the int32 range of
 * the w form; then kernel = NW_KERNEL_PANELS with NW_ERR_UNSUPPORTED; then a host
 * without a device answers NW_ERR_NODEVICE.  npairs = 0 is NW_OK.  A pair with n1 = 0
 * or n2 = 0 has no cells: score gap * max(n1, n2), ops all ups / all lefts. */
typedef struct nw_batch_opts {   /* NULL = defaults */
    int64_t mem_bytes;           /* device budget of nw_align_batch; 0 = 80 % of the free HBM */
    int32_t reserved[6];         /* must be 0 */
} nw_batch_opts;

typedef struct nw_batch_stats {
    int64_t pairs, cells;        /* npairs, the sum of n1 * n2                              */
    int64_t chunks;              /* launches of the batch kernel (nw_score_batch: 1)        */
    int64_t dir_bytes;           /* direction bytes of all pairs (nw_batch_dir_bytes)       */
    int64_t peak_bytes;          /* everything the call holds on the device at once         */
    int32_t waves, reserved;     /* workers launched                                        */
    double fill_ms, walk_ms;     /* device time of the batch kernel / of the walks          */
} nw_batch_stats;

/* Direction bytes of one pair in nw_align_batch: 2 bits per cell, padded to whole
 * 64-step iterations of whole 256-column strips -- ceil(n1 / 256) * (n2 / 64 + 2) *
 * 4096 (4096 x 4096: 1.03 x n1 * n2 / 4).  0 when a side is empty, -1 for a negative
 * size.  Host only. */
int64_t nw_batch_dir_bytes(int64_t n1, int64_t n2);

/* Scores of a batch on device buffers, asynchronous on `stream`: d_scores[i] = t[n2_i]
 * [n1_i].  The lengths are on the device, so the caller states total1 = off1[npairs],
 * total2 = off2[npairs] and max_n2 >= every n2_i (the workers' column scratch is sized
 * by it; a pair with more rows gets INT32_MIN and is not computed), pairs are claimed
 * in index order -- submit them longest first -- and the w-form range is checked for
 * max_n2 alone: every pair must satisfy what nw_score_batch checks.  Empty pairs are
 * answered by the kernel.  The refusals above but for the offsets' contents; also
 * NW_ERR_ARG: p == NULL, a negative total or max_n2, max_n2 > total2, ctx == NULL. */
int nw_score_batch_async(nw_ctx *ctx, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                         const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2, int64_t max_n2,
                         const nw_params *p, int32_t *d_scores, void *stream);

/* Scores of a batch from host buffers: scores[i] for every pair.  p == NULL: the
 * reference defaults; `stats` may be NULL. */
int nw_score_batch(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                   int64_t npairs, const nw_params *p, int32_t *scores, nw_batch_stats *stats);

/* Scores and alignments of a batch from host buffers.  ops_off (npairs + 1, non-
 * decreasing) gives pair i the slot ops[ops_off[i] .. ops_off[i+1]) of at least n1_i +
 * n2_i bytes; its n_ops[i] ops (0 diag, 1 up, 2 left) start the slot, in path order
 * (0, 0) -> (n2, n1), byte-identical to nw_align's.  The kernel keeps 2 direction bits
 * per cell (nw_batch_dir_bytes) and one thread per pair walks them back; the longest-
 * first order is processed in chunks whose direction bytes and ops, with everything
 * else the call holds, fit mem_bytes (stats: chunks, peak_bytes).  Also NW_ERR_ARG:
 * a slot shorter than n1 + n2, NULL ops / ops_off / n_ops, mem_bytes < 0, reserved !=
 * 0.  NW_ERR_OOM when one pair alone does not fit: that pair is nw_align_ckpt's. */
int nw_align_batch(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                   int64_t npairs, const nw_params *p, const nw_batch_opts *o, int32_t *scores, uint8_t *ops,
                   const int64_t *ops_off, int64_t *n_ops, nw_batch_stats *stats);

/* Batched global alignment under affine gap cost (Gotoh) ------------------------
 * A run of L consecutive ups, or of L consecutive lefts, costs gap_open + L *
 * gap_extend; an up-run directly followed by a left-run is two gaps.  gap_extend is
 * nw_params.gap, gap_open the extra argument (gap_open = 0 is the linear cost, and
 * then scores and ops are those of the linear entries).
 *   E[i][j] = max(E[i][j-1] + ge, H[i][j-1] + go + ge)      (a left run ends at (i, j))
 *   F[i][j] = max(F[i-1][j] + ge, H[i-1][j] + go + ge)      (an up run ends at (i, j))
 *   H[i][j] = max(H[i-1][j-1] + s(s1[j-1], s2[i-1]), F[i][j], E[i][j])
 *   H[0][0] = 0, H[0][j] = go + j*ge, H[i][0] = go + i*ge, E[i][0] = F[0][j] = -inf
 * score = H[n2][n1].  The ops are the walk of a machine of three states from (n2, n1)
 * to (0, 0): in H on row 0 / column 0 it goes left / up; in H at an inner cell it
 * takes the first of diag, F, E that equals H (diag: op 0; F, E: change state, no op);
 * in F it emits op 1, moves up and returns to H when F[i][j] == H[i-1][j] + go + ge
 * (opening wins a tie over extending), else stays; E likewise with op 2 and a move
 * left.  Contracts, CSR layout, options, statistics, slot sizes (n1 + n2), chunking
 * and the order of the refusals are those of the linear entries above (the kernels:
 * csrc/nw_batch_affine.hip; a worker keeps two columns between strips, the
 * directions are 4 bits per cell).  Also refused with NW_ERR_ARG: gap_open > 0 (the
 * machine would open a new gap at every step and the ops would no longer determine
 * the score), and a pair beyond the int32 range of the kernel's form -- it holds H, E
 * and F minus ge*(i+j) next to a "minus infinity" of -2^29, and
 *   3*|gap_open| + (max(|match|, |mismatch|, |gap|) + |gap|) * (n1 + n2 + 2) < 2^28
 * keeps every one of them above -2^28 (the _async form checks it for n1 = 0, n2 =
 * max_n2).  A pair with an empty side scores gap_open + gap * max(n1, n2) (0 for 0 x
 * 0), ops all ups / all lefts. */

/* Direction bytes of one pair in nw_align_batch_affine: 4 bits per cell, 2 *
 * nw_batch_dir_bytes(n1, n2).  0 when a side is empty, -1 for a negative size.  Host
 * only. */
int64_t nw_batch_affine_dir_bytes(int64_t n1, int64_t n2);

int nw_score_batch_affine_async(nw_ctx *ctx, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                                const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                                int64_t max_n2, const nw_params *p, int32_t gap_open, int32_t *d_scores,
                                void *stream);

int nw_score_batch_affine(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, int32_t gap_open, int32_t *scores,
                          nw_batch_stats *stats);

int nw_align_batch_affine(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, int32_t gap_open, const nw_batch_opts *o,
                          int32_t *scores, uint8_t *ops, const int64_t *ops_off, int64_t *n_ops,
                          nw_batch_stats *stats);

/* Batched global alignment with a substitution matrix ---------------------------
 * The affine entries above with s(s1[j-1], s2[i-1]) = score[index[s1[j-1]]][index[s2[i-
 * 1]]] in the place of match / mismatch: BLOSUM / PAM for proteins, transition /
 * transversion and IUPAC matrices for nucleotides.  At most NW_SUBMAT_MAX letters;
 * EVERY byte value maps to a letter -- a caller who wants "unknown" points those bytes
 * at its own wildcard letter (X, N, *); there is no separate unknown-character path and
 * the sequences are never scanned on the host.  The matrix may be asymmetric: the first
 * index is always the s1 (column) letter.  Entries at or beyond n are ignored.
 * nw_params.gap is the extension and gap_open the opening, as above (gap_open = 0: the
 * linear cost with a matrix); match and mismatch are not used but must be valid.  The
 * recurrence, the boundaries, the three-state walk and its tie-breaks are word for word
 * those of the affine entries, and so are the CSR layout, options, statistics, slot
 * sizes, chunking, nw_batch_affine_dir_bytes, the empty-side pairs and the INT32_MIN of
 * a pair longer than max_n2 in the _async form (kernels: csrc/nw_batch_matrix.hip; the
 * matrix travels in the kernel arguments, a worker keeps a profile of its four columns
 * in 8 KiB of LDS).  The refusals and their order are the affine entries'; also
 * NW_ERR_ARG, after the parameter checks: m == NULL, n outside 1 .. NW_SUBMAT_MAX, a
 * reserved word != 0, an index entry >= n; and a pair beyond
 *   3*|gap_open| + (M + |gap|) * (n1 + n2 + 2) < 2^28,  M = max(|gap|, max |score[x][y]|
 *   over x, y < n)
 * -- the affine range with the matrix's largest entry in the place of match / mismatch.
 * Exact for every int8 matrix and every gap that bound admits. */
enum { NW_SUBMAT_MAX = 32 };
typedef struct nw_submat {
    int32_t n;              /* letters, 1..NW_SUBMAT_MAX */
    int32_t reserved[3];    /* must be 0 */
    uint8_t index[256];     /* byte (as unsigned) -> letter 0..n-1; every entry < n */
    int8_t  score[NW_SUBMAT_MAX * NW_SUBMAT_MAX];
                            /* score[x * NW_SUBMAT_MAX + y] = s(s1 letter x, s2 letter y) */
} nw_submat;

int nw_score_batch_matrix_async(nw_ctx *ctx, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                                const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                                int64_t max_n2, const nw_params *p, const nw_submat *m, int32_t gap_open,
                                int32_t *d_scores, void *stream);

int nw_score_batch_matrix(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t *scores,
                          nw_batch_stats *stats);

int nw_align_batch_matrix(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                          const nw_batch_opts *o, int32_t *scores, uint8_t *ops, const int64_t *ops_off,
                          int64_t *n_ops, nw_batch_stats *stats);

/* Batched LOCAL alignment (Smith-Waterman) with affine gaps and a matrix ---------
 * The best-scoring pair of substrings of every pair of a batch: a read against a
 * reference window, a protein against a database hit.  Substitution, the nw_submat and
 * its validity rules, gap_open (<= 0) and nw_params.gap as the extension ge are exactly
 * those of the matrix entries above.  The recurrence is Gotoh's with a floor of zero
 * and free ends:
 *   E[i][j] = max(E[i][j-1] + ge, H[i][j-1] + go + ge)
 *   F[i][j] = max(F[i-1][j] + ge, H[i-1][j] + go + ge)
 *   H[i][j] = max(0, H[i-1][j-1] + s(s1[j-1], s2[i-1]), F[i][j], E[i][j])
 *   H[0][j] = H[i][0] = 0,   E[i][0] = F[0][j] = -inf
 * score = the maximum of H over the whole table; the end cell is the maximising cell
 * with the smallest i and among those the smallest j (first in row-major order, as
 * nw_sw_align).  When the maximum is 0, end = begin = (0, 0) and n_ops = 0; a pair
 * with an empty side gives the same.  The ops are the walk of the affine entries'
 * machine of three states, started at the end cell in state H, with one more rule that
 * is checked first: in state H at a cell with H == 0 (every cell of row 0 and column 0
 * is one) the walk stops, and that cell is the begin cell.  Otherwise the first of
 * diag, F, E that equals H is taken; in F and E opening wins a tie over extending.  Ops
 * are 0 diag / 1 up / 2 left in path order begin -> end, n_ops <= n1 + n2, and
 * nw_ops_score_matrix(..., begin_i, begin_j, ...) of them equals the score.  With
 * gap_open = 0 and a match / mismatch matrix the score, both cells and the ops are
 * nw_sw_align's (tie order diag > up > left).
 * CSR layout, options, statistics, slot sizes (n1 + n2 bytes), longest-first tickets,
 * chunking by mem_bytes, nw_batch_affine_dir_bytes and NW_ERR_OOM for a pair that does
 * not fit alone are the matrix entries'.  So are the refusals and their order, with the
 * hits in the place of the scores and p->mode required to be NW_MODE_SW (which refuses
 * gap > 0; p == NULL: the defaults with mode NW_MODE_SW), and the range:
 *   3*|gap_open| + (M + |gap|) * (n1 + n2 + 2) < 2^28
 * unchanged, conservative for a local table.  In the _async form a pair longer than
 * max_n2 gets score INT32_MIN and -1 in the four coordinates; empty pairs are answered
 * by the kernel.  The score entries find no begin cell (that needs a reverse sweep)
 * and write -1.  Nothing per pair crosses to the host between the sweep and the walk:
 * the sweep writes the hit, the walk reads its start from it on the device (kernels:
 * csrc/nw_batch_local.hip). */
typedef struct nw_local_hit {      /* 32 bytes */
    int32_t score;                 /* max H, >= 0 (semi-global entries: may be < 0)  */
    int32_t end_i, end_j;          /* first row-major maximum; (0,0) when score == 0 */
    int32_t begin_i, begin_j;      /* align entry: where the walk stopped; score entries: -1 */
    int32_t reserved[3];           /* written as 0 */
} nw_local_hit;

int nw_score_batch_local_async(nw_ctx *ctx, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                               const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                               int64_t max_n2, const nw_params *p, const nw_submat *m, int32_t gap_open,
                               nw_local_hit *d_hits, void *stream);

int nw_score_batch_local(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                         int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                         nw_local_hit *hits, nw_batch_stats *stats);

int nw_align_batch_local(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                         int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                         const nw_batch_opts *o, nw_local_hit *hits, uint8_t *ops, const int64_t *ops_off,
                         int64_t *n_ops, nw_batch_stats *stats);

/* Batched SEMI-GLOBAL alignment: free end gaps per side ---------------------------
 * Between the matrix entries (both sequences end to end) and the local ones (the best
 * pair of substrings): a read that must align over its whole length somewhere inside a
 * reference window ("fit"), a primer inside a read, two reads that dovetail.  `ends` is
 * a set of four bits; s1 runs along the columns and s2 along the rows, as everywhere:
 *   NW_ENDS_S1_BEGIN (1)  a skipped prefix of s1 costs nothing: H[0][j] = 0
 *   NW_ENDS_S1_END   (2)  a skipped suffix of s1 costs nothing: the end cell may be any (n2, j)
 *   NW_ENDS_S2_BEGIN (4)  H[i][0] = 0
 *   NW_ENDS_S2_END   (8)  the end cell may be any (i, n1)
 * NW_ENDS_GLOBAL = 0, NW_ENDS_S2_IN_S1 = 3 (all of s2 inside s1), NW_ENDS_S1_IN_S2 = 12,
 * NW_ENDS_OVERLAP = 15; the dovetails are 9 (a suffix of s1 against a prefix of s2) and 6.
 * A path runs from a begin cell -- (0, 0), or any (0, j) with bit 1, or any (i, 0) with
 * bit 4 -- to an end cell -- (n2, n1), or any (n2, j), 0 <= j <= n1, with bit 2, or any
 * (i, n1), 0 <= i <= n2, with bit 8 --, and the score is the best Gotoh score of such a
 * path; it may be negative.  As a table: the matrix entries' recurrence, no floor,
 *   E, F and H of inner cells as there;  E[i][0] = F[0][j] = -inf;  H[0][0] = 0;
 *   a boundary that is not free holds go + k * ge, a free one 0.
 * The table is the definition.  With gap <= 0 it is the best score over those paths.  With
 * gap > 0 a run along a free boundary from (0, 0) would be PAID go + k * ge > 0, and a free
 * boundary holds 0 all the same: a skipped end is not priced, also where pricing it would
 * gain, so the score may then be below the best path's (with ends = 0 nothing is free and the
 * two agree for every gap).
 * End cell: among the admissible end cells of maximal H the first in row-major order
 * (smallest i, then smallest j), the local entries' rule; (n2, 0) and (0, n1) are
 * candidates where their side is free, so with ends = 15 the score is >= 0.
 * Walk: the affine entries' machine of three states, started at the end cell in state H.
 * At (0, 0) it stops; on row 0 it stops if bit 1 is set, else it goes left to (0, 0)
 * emitting lefts; on column 0 it stops if bit 4 is set, else it goes up emitting ups; the
 * cell where it stops is the begin cell.  Tie-breaks are the affine entries': diag, then
 * F, then E; opening wins over extending.  Ops run begin -> end, n_ops <= n1 + n2, and
 * nw_ops_score_matrix(..., begin_i, begin_j, ...) of them equals the score; the skipped
 * prefix and suffix emit nothing.
 * The result is an nw_local_hit whose score may be negative here.  The score entries
 * write -1 into the begin cell.  In the _async form a pair longer than max_n2 gets
 * INT32_MIN and -1 in the four coordinates, and the kernel answers pairs with an empty
 * side; in the host forms the host answers them without a launch, ops included (a table
 * with an empty side follows the same definition: one boundary, no special rule).
 * ends = 0: score, ops and n_ops are byte for byte nw_*_batch_matrix's, end (n2, n1),
 * begin (0, 0).  Parameters, refusals and their order are the matrix entries'
 * (NW_MODE_NW, gap_open <= 0, the matrix checks); then ends outside 0 .. 15 is
 * NW_ERR_ARG, before the range bound, which is the matrix entries' unchanged:
 *   3*|gap_open| + (M + |gap|) * (n1 + n2 + 2) < 2^28
 * Direction bytes (nw_batch_affine_dir_bytes), chunking by mem_bytes, NW_ERR_OOM, slot
 * sizes, longest-first tickets and the statistics are the matrix entries' too (kernels:
 * csrc/nw_batch_semi.hip). */
enum {
    NW_ENDS_S1_BEGIN = 1,
    NW_ENDS_S1_END = 2,
    NW_ENDS_S2_BEGIN = 4,
    NW_ENDS_S2_END = 8,
    NW_ENDS_GLOBAL = 0,
    NW_ENDS_S2_IN_S1 = 3,
    NW_ENDS_S1_IN_S2 = 12,
    NW_ENDS_OVERLAP = 15
};

int nw_score_batch_semi_async(nw_ctx *ctx, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                              const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2, int64_t max_n2,
                              const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t ends,
                              nw_local_hit *d_hits, void *stream);

int nw_score_batch_semi(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                        int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t ends,
                        nw_local_hit *hits, nw_batch_stats *stats);

int nw_align_batch_semi(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                        int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t ends,
                        const nw_batch_opts *o, nw_local_hit *hits, uint8_t *ops, const int64_t *ops_off,
                        int64_t *n_ops, nw_batch_stats *stats);

/* Batched BANDED global alignment: the matrix entries inside a band of diagonals ----
 * For pairs whose path stays near the diagonal (reads against a window, amplicons,
 * homologous proteins, overlaps verified after seeding): the sweep visits the band's
 * neighbourhood only and keeps direction bits for it only.  The entries are the matrix
 * entries' with `int32_t band` after gap_open.
 * Definition.  band = w >= 0, one value per call.  For a pair with n1 columns (s1) and n2
 * rows (s2) let delta = n2 - n1, dlo = min(0, delta) - w and dhi = max(0, delta) + w.
 *   Cell (i, j), 0 <= i <= n2, 0 <= j <= n1, is IN THE BAND iff dlo <= i - j <= dhi;
 *   boundary cells are included in this rule.
 *   H, E and F of a cell outside the band are -inf.
 *   Inside the band the recurrence, the boundaries (go + k * ge, H[0][0] = 0, E[i][0] =
 *   F[0][j] = -inf), the three-state walk and its tie-breaks are the matrix entries', word
 *   for word.
 *   score = H[n2][n1].
 * Equivalently: the score is the best Gotoh score over the paths (0, 0) -> (n2, n1) all of
 * whose vertices are in the band.  Three consequences:
 *   Every in-band inner cell has a finite H: its diagonal predecessor lies on the same
 *   diagonal, and the path "diagonal, then one run" is always inside the band.  So the
 *   score is always a real score; there is no sentinel.
 *   When dlo <= -n1 and dhi >= n2 the band is the whole table -- any w >= max(n1, n2)
 *   guarantees it -- and scores, ops and n_ops are byte for byte nw_*_batch_matrix's.
 *   The walk never leaves the band: the predecessor it picks equals a finite H.
 * Results are int32 scores.  The CSR layout, options, statistics, slot sizes (n1 + n2),
 * longest-first tickets, empty-side pairs and the INT32_MIN of a pair over max_n2 in the
 * _async form are the matrix entries'; an empty-side pair follows the definition: its one
 * boundary is inside the band because the band widens by |delta|.  Refusals and their
 * order are the matrix entries'; after the matrix checks and before the range bound, band
 * < 0 is NW_ERR_ARG.  The range bound is the matrix entries' unchanged,
 *   3*|gap_open| + (M + |gap|) * (n1 + n2 + 2) < 2^28
 * and still holds with cells forced to -inf: its lower bound on H is the score of a path
 * with one run up and one run left, and for an in-band cell the path "diagonal, then one
 * run" is such a path inside the band; its upper bound does not depend on the path.  A
 * forced -2^29 is copied, never accumulated: what is added to it (go, s - 2 ge) is added
 * once, and the sum is dropped by the next maximum or forced again (kernels:
 * csrc/nw_batch_banded.hip).
 *
 * nw_batch_banded_dir_bytes: direction bytes of one pair in nw_align_batch_banded, the
 * number the chunking uses.  0 when a side is empty, -1 for a negative size or a negative
 * band.  Host only.  A strip of 256 columns keeps only the 64-step iterations that can
 * touch an in-band row of its columns:
 *   ceil(n1 / 256) * min(n2 / 64 + 2, ceil((dhi' - dlo' + 319) / 64) + 2) * 8192
 * with dlo' = max(dlo, -n1 - 1024), dhi' = min(dhi, n2 + 1024).  It equals
 * nw_batch_affine_dir_bytes(n1, n2) when the band covers the table, is never above it,
 * does not decrease when w grows, and is at most
 *   ceil(n1 / 256) * (ceil((2 * band + |n2 - n1| + 319) / 64) + 3) * 8192
 * (a strip's 256 columns need 256 + dhi - dlo rows; the lane skew adds 63 steps; a step
 * range touches one more 64-step iteration than its length; the right column's last
 * block is stored one iteration later; one row of slack covers the feed). */
int64_t nw_batch_banded_dir_bytes(int64_t n1, int64_t n2, int32_t band);

int nw_score_batch_banded_async(nw_ctx *ctx, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                                const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2,
                                int64_t max_n2, const nw_params *p, const nw_submat *m, int32_t gap_open,
                                int32_t band, int32_t *d_scores, void *stream);

int nw_score_batch_banded(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t band,
                          int32_t *scores, nw_batch_stats *stats);

int nw_align_batch_banded(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                          int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t band,
                          const nw_batch_opts *o, int32_t *scores, uint8_t *ops, const int64_t *ops_off,
                          int64_t *n_ops, nw_batch_stats *stats);

/* Batched global alignment under a TWO-PIECE affine gap cost ----------------------
 * For long reads and genome-to-genome pairs: a run of k consecutive ups, or of k
 * consecutive lefts, costs
 *   g(k) = max(go1 + k*ge1, go2 + k*ge2)
 * -- a short indel is priced by the steep piece, a long deletion or an intron by the flat
 * one (minimap2's -O4,24 -E2,1 is go = -4, -24 and ge = -2, -1).  The entries are the matrix
 * entries' with `int32_t gap_open2, int32_t gap2` after gap_open: piece 1 is (gap_open,
 * nw_params.gap) = (go1, ge1), piece 2 is (gap_open2, gap2) = (go2, ge2), s comes from the
 * nw_submat exactly as in the matrix entries.
 *   E_t[i][j] = max(E_t[i][j-1] + ge_t, H[i][j-1] + go_t + ge_t)      t = 1, 2
 *   F_t[i][j] = max(F_t[i-1][j] + ge_t, H[i-1][j] + go_t + ge_t)
 *   H[i][j]   = max(H[i-1][j-1] + s, F_1[i][j], E_1[i][j], F_2[i][j], E_2[i][j])
 *   H[0][0] = 0, H[0][j] = g(j), H[i][0] = g(i), E_t[i][0] = F_t[0][j] = -inf
 * score = H[n2][n1].  It equals the maximum over all global paths of the sum of s over the
 * diagonal steps plus g(k) for every maximal run of ups and every maximal run of lefts; an
 * up-run directly followed by a left-run is two gaps.  With go1, go2 <= 0 splitting one run
 * into two gaps (which the recurrence can do: a run of one piece may open from an H that a
 * run of the other piece made) never beats pricing it whole by one piece: g is convex in k
 * and max(go1, go2), its value at 0, is <= 0, so g(a) + g(b) <= g(a + b).  So the ops alone
 * determine the score: nw_ops_score_dual computes exactly that sum, with the max per run.
 * The ops are the walk of a machine of five states from (n2, n1) to (0, 0): in H on row 0
 * it goes left, on column 0 up; in H at an inner cell it takes the first of diag, F_1, E_1,
 * F_2, E_2 that equals H (diag: op 0; the others: change state, no op); in F_t it emits op
 * 1, moves up and returns to H when F_t[i][j] == H[i-1][j] + go_t + ge_t (opening wins a tie
 * over extending), else stays; E_t likewise with op 2 and a move left.  Ops are 0 / 1 / 2 as
 * everywhere; they do not say which piece priced a run.
 * Reductions, byte for byte in scores, ops and n_ops: equal pieces give the matrix
 * entries' results; so does a piece 2 that is nowhere above piece 1 (go2 <= go1 and ge2 <=
 * ge1: F_2 <= F_1 and E_2 <= E_1 everywhere, and the order diag, F_1, E_1, F_2, E_2 never
 * reaches them); a piece 1 strictly below piece 2 (go1 + ge1 < go2 + ge2 and ge1 <= ge2)
 * gives the matrix entries' results under piece 2.
 * The CSR layout, options, statistics, slot sizes (n1 + n2), chunking under mem_bytes,
 * longest-first tickets and the INT32_MIN of a pair longer than max_n2 in the _async form
 * are the matrix entries'; a pair with an empty side scores g(max(n1, n2)) (0 for 0 x 0),
 * ops all ups / all lefts.  Refusals and their order are the matrix entries'; then
 * NW_ERR_ARG for gap_open2 > 0, for gap2 outside nw_params.gap's range (|gap2| < 4096;
 * positive extensions are legal as there), and for a pair beyond the int32 range of the
 * kernel's form: it holds H, E_t and F_t minus ge1*(i+j) next to a "minus infinity" of
 * -2^29 (piece 1 extends for free, piece 2 for one add of ge2 - ge1), and with G =
 * max(|go1|, |go2|), A = max(|ge1|, |ge2|), M = max(A, max |score[x][y]| over x, y < n)
 *   3*G + (M + A) * (n1 + n2 + 2) < 2^28
 * keeps every one of them above -2^28: a value is a path sum of at most i + j steps of at
 * most M each and at most three openings, and the subtracted ge1*(i+j) is at most A*(i+j)
 * -- which also covers the piece-2 values' drift of ge2 - ge1 per step (the _async form
 * checks it for n1 = 0, n2 = max_n2).  Kernels: csrc/nw_batch_dual.hip; a worker keeps
 * three columns between strips, the directions are one byte per cell.
 *
 * nw_batch_dual_dir_bytes: direction bytes of one pair in nw_align_batch_dual, 2 *
 * nw_batch_affine_dir_bytes(n1, n2).  0 when a side is empty, -1 for a negative size.
 * Host only. */
int64_t nw_batch_dual_dir_bytes(int64_t n1, int64_t n2);

int nw_score_batch_dual_async(nw_ctx *ctx, const int8_t *d_s1cat, const int64_t *d_off1, const int8_t *d_s2cat,
                              const int64_t *d_off2, int64_t npairs, int64_t total1, int64_t total2, int64_t max_n2,
                              const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t gap_open2,
                              int32_t gap2, int32_t *d_scores, void *stream);

int nw_score_batch_dual(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                        int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t gap_open2,
                        int32_t gap2, int32_t *scores, nw_batch_stats *stats);

int nw_align_batch_dual(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                        int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open, int32_t gap_open2,
                        int32_t gap2, const nw_batch_opts *o, int32_t *scores, uint8_t *ops, const int64_t *ops_off,
                        int64_t *n_ops, nw_batch_stats *stats);

/* The two-piece gap cost inside a band ----------------------------------------------
 * The aligner for long reads: global, banded, concave gap cost, many pairs per call.  The
 * entries are the two-piece entries' with `int32_t band` after gap2.  The definition is the
 * conjunction of the two above and nothing else:
 *   - the recurrence, the boundaries, the walk of five states and its tie-breaks are the
 *     two-piece entries' (nw_*_batch_dual), word for word;
 *   - the band is the banded entries' (nw_*_batch_banded): with w = band, dlo = min(0, n2 -
 *     n1) - w and dhi = max(0, n2 - n1) + w, cell (i, j), 0 <= i <= n2, 0 <= j <= n1, counts iff
 *     dlo <= i - j <= dhi, boundary cells included; H, E_1, E_2, F_1 and F_2 of a cell outside
 *     the band are -inf.  score = H[n2][n1].
 * Equivalently the score is the best two-piece score (the sum of s over the diagonal steps
 * plus g(k) per maximal run) over the global paths all of whose vertices lie in the band.
 * Both corners are in the band for every w >= 0, and so is the path "diagonal, then one
 * run" to any in-band cell: every in-band inner cell is finite.  The walk never leaves the
 * band: a source or a run is chosen only where its value equals a finite H, and a value that
 * came from outside the band is -inf.  One long deletion -- what piece 2 exists to price --
 * lies inside a narrow band, because the band is defined between the table's two corners.
 * Reductions, byte for byte in scores, ops and n_ops: a covering band (w >= max(n1, n2))
 * gives nw_*_batch_dual's results; equal pieces, or a piece 2 that is nowhere above piece 1
 * (go2 <= go1 and ge2 <= ge1), give nw_*_batch_banded's.  The score does not decrease in w.
 * A pair with an empty side follows the two-piece entries: g(max(n1, n2)) (0 for 0 x 0), ops
 * all ups or all lefts, whatever the band.  Refusals and their order are the two-piece
 * entries'; after them NW_ERR_ARG for band < 0; then, per pair, the two-piece entries' range
 * bound 3*G + (M + A) * (n1 + n2 + 2) < 2^28.  It still holds with cells forced to -inf: its
 * lower bound on H needs one path with at most two openings that the recurrence can take,
 * and "diagonal, then one run" is such a path inside the band; the bounds on E_t and F_t are
 * per step; a forced cell holds no real value, and the kernel adds to its -2^29 at most once
 * (csrc/nw_batch_dual_banded.hip's header has the argument for piece 2's drift).  The ops are
 * scored by nw_ops_score_dual.
 *
 * nw_batch_dual_banded_dir_bytes: direction bytes of one pair in nw_align_batch_dual_banded,
 * 2 * nw_batch_banded_dir_bytes(n1, n2, band): a byte per cell for the iterations of each
 * strip's range alone.  0 when a side is empty, -1 for a negative size or band; equal to
 * nw_batch_dual_dir_bytes under a covering band, never above it, not decreasing in band.  The
 * chunking under mem_bytes uses it.  Host only. */
int64_t nw_batch_dual_banded_dir_bytes(int64_t n1, int64_t n2, int32_t band);

int nw_score_batch_dual_banded_async(nw_ctx *ctx, const int8_t *d_s1cat, const int64_t *d_off1,
                                     const int8_t *d_s2cat, const int64_t *d_off2, int64_t npairs, int64_t total1,
                                     int64_t total2, int64_t max_n2, const nw_params *p, const nw_submat *m,
                                     int32_t gap_open, int32_t gap_open2, int32_t gap2, int32_t band,
                                     int32_t *d_scores, void *stream);

int nw_score_batch_dual_banded(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                               int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                               int32_t gap_open2, int32_t gap2, int32_t band, int32_t *scores,
                               nw_batch_stats *stats);

int nw_align_batch_dual_banded(const int8_t *s1cat, const int64_t *off1, const int8_t *s2cat, const int64_t *off2,
                               int64_t npairs, const nw_params *p, const nw_submat *m, int32_t gap_open,
                               int32_t gap_open2, int32_t gap2, int32_t band, const nw_batch_opts *o,
                               int32_t *scores, uint8_t *ops, const int64_t *ops_off, int64_t *n_ops,
                               nw_batch_stats *stats);

/* Launch-only variant for timing loops: no synchronisation, no readback. */
int nw_fill_device_async(nw_ctx *ctx, const int8_t *d_s1, int64_t n1,
                         const int8_t *d_s2, int64_t n2, const nw_params *p,
                         int32_t *d_t, int64_t pitch, void *stream);

/* Row bands (multi-GPU) ---------------------------------------------------
 * The reference's 8-GPU twin is src/mpi/mpi-horz.cpp:4-99 (+ mpi-horz-driver.cpp):
 * rank r fills a contiguous band of rows whose row 0 is rank r-1's last row (the
 * halo), received in chunks while r-1 is still filling.  Here band r's kernel
 * takes that row from `halo_in` -- granules {tag:32 | value:32}, one per column
 * 0..n1 -- as each strip (64 * substrips * strip_waves columns) starts, and
 * publishes its own last row into
 * `halo_out` (the next band's halo_in, usually peer memory on the next GPU
 * mapped with nw_ipc_open_handle) as each strip finishes: a pipelined halo with
 * no host round trip.  `tag` identifies the launch (> 0, the same value on both
 * sides of a halo, new for every launch); halo buffers must start zeroed. */
typedef struct nw_band {
    const uint64_t *halo_in;  /* NULL: row 0 is the boundary j*gap (first band)  */
    uint64_t *halo_out;       /* NULL: last band                                  */
    uint32_t tag;
    uint32_t row0;            /* global row index of the band's row 0 (nw_band_layout
                                 `start`): bounds the cell values for the range check */
} nw_band;

/* Band layout of mpi-horz-driver.cpp:31-32: rows of band r (including its halo
 * row) and the global index of its row 0, for a table of n2+1 rows in nbands. */
void nw_band_layout(int64_t n2, int32_t nbands, int32_t r, int64_t *n_rows, int64_t *start);

/* Bytes of one halo granule buffer for n1 (+1) columns. */
int64_t nw_halo_bytes(int64_t n1);

/* A zeroed halo granule buffer of its own hipMalloc (so that nw_ipc_get_handle
 * exports exactly it); device -1 = current. */
int nw_halo_alloc(int device, int64_t n1, uint64_t **d_halo);
int nw_halo_free(uint64_t *d_halo);

/* Fill one band: d_t holds n2_band+1 rows (row 0 = the halo row, written by
 * the kernel from halo_in), d_s2_band = the band's side characters
 * (s2 + start of the band: local row i >= 1 uses d_s2_band[i-1]).  Async. */
int nw_fill_band_async(nw_ctx *ctx, const int8_t *d_s1, int64_t n1, const int8_t *d_s2_band,
                       int64_t n2_band, const nw_params *p, const nw_band *band, int32_t *d_t,
                       int64_t pitch, void *stream);

/* Block-cyclic row bands (the config-4 row-band case, pipelined) --------------
 * Same contract as nw_fill_band_async (mpi-horz.cpp:4-99: a block's row 0 is the
 * previous block's last row, streamed strip by strip), but the table's rows are
 * cut into P * nblk blocks of n2_blk rows dealt round robin to the P ranks --
 * global block g = k * P + r is rank r's block k -- so that every rank is busy
 * after P blocks instead of waiting for P - 1 whole bands.  One launch fills all
 * of a rank's blocks, strips claimed in (block, strip) order:
 *   * block k's table is d_t + k * t_stride (each laid out like a band: n2_blk + 1
 *     rows, row 0 = the halo row), its side characters d_s2_blocks + k * n2_blk;
 *   * its halo row comes from region k of halo_in (regions of nw_halo_bytes(n1),
 *     nw_halo_alloc_regions) -- block 0 only if hin_first (rank 0: block 0's
 *     row 0 is the boundary);
 *   * its last row goes to region k + hout_shift of halo_out (the next rank's
 *     halo_in; hout_shift = 1 on the last rank, whose block k feeds rank 0's
 *     block k + 1; regions >= nblk are not written).  With P = 1, halo_out =
 *     halo_in and hout_shift = 1 chain a rank's blocks through its own buffer.
 * Strip kernel only (NW_ERR_UNSUPPORTED for panels). */
typedef struct nw_band_cycle {
    const uint64_t *halo_in;
    uint64_t *halo_out;
    int32_t nblk;
    int32_t hin_first;
    int32_t hout_shift;
    uint32_t tag;             /* as nw_band.tag                                       */
    int64_t row0_max;         /* global row of the last block's row 0 (range check)   */
    int64_t t_stride;         /* int32 elements between blocks' tables (>= (n2_blk+1) * pitch,
                                 a multiple of 64)                                     */
} nw_band_cycle;

int nw_halo_alloc_regions(int device, int64_t n1, int32_t nregions, uint64_t **d_halo);
int nw_fill_band_cycle_async(nw_ctx *ctx, const int8_t *d_s1, int64_t n1, const int8_t *d_s2_blocks,
                             int64_t n2_blk, const nw_params *p, const nw_band_cycle *cy, int32_t *d_t,
                             int64_t pitch, void *stream);

/* Column bands (multi-GPU, n1 >> n2) ------------------------------------------
 * The reference's twin is src/mpi/mpi-vert.cpp:4-109 (+ mpi-vert-driver.cpp:35-38):
 * rank r fills a contiguous band of columns whose column 0 is rank r-1's last
 * column, received in COMMBUF_SIZE-row chunks while r-1 is still filling.  Here
 * the bands are whole strips of the global table's sweep (strips of
 * W = 64 * substrips * strip_waves columns starting at column 1): band r owns
 * strips [strip_first, strip_first + strip_count) and its local table holds
 * global columns [start, start + n_cols), start = strip_first * W, so local
 * column 0 is band r-1's last column as in mpi-vert.  The first strip of band
 * r > 0 takes that column from `feed_in` as band r-1's last strip produces it
 * (granules {tag:32 | value:32}, one per row, nw_feed_bytes), and band r's last
 * strip publishes its right column into `feed_out` (band r+1's feed_in, usually
 * peer memory mapped with nw_ipc_open_handle) row block by row block.  After
 * the fill, local column 0 of band r > 0 is written from feed_in.  Every band
 * must use the same n1, n2 and strip shape (explicit substrips / strip_waves, or
 * 0/0 = the tuned shape of the whole n1 x n2 table); NW mode only. */
typedef struct nw_colband {
    const uint64_t *feed_in;  /* NULL: first band (column 0 = the boundary i*gap) */
    uint64_t *feed_out;       /* NULL: last band                                  */
    uint32_t tag;             /* launch tag (> 0, the same on both sides of a feed,
                                 new for every launch; not the value of any other
                                 launch's tag on these buffers)                    */
    int32_t nbands;           /* bands of the table                               */
    int32_t r;                /* this band                                        */
    int32_t reserved;
} nw_colband;

/* Layout of band r of nbands over an n1 x n2 table with the strip shape of `p`:
 * its strips and the global column range of its local table (local column 0 =
 * global column start).  Returns NW_ERR_ARG when nbands exceeds the strips. */
int nw_colband_layout(int64_t n1, int64_t n2, int32_t nbands, int32_t r, const nw_params *p,
                      int64_t *strip_first, int64_t *strip_count, int64_t *start, int64_t *n_cols);

/* Bytes of one feed granule buffer for n2 (+1) rows, and a zeroed one of its own
 * hipMalloc (exportable by nw_ipc_get_handle); free with nw_halo_free. */
int64_t nw_feed_bytes(int64_t n2);
int nw_feed_alloc(int device, int64_t n2, uint64_t **d_feed);

/* Fill column band band->r: d_s1 / d_s2 the WHOLE sequences (n1 / n2); d_t the
 * band's local table laid out like nw_table_offset's (n_cols - 1 = its "n1"),
 * pitch >= nw_table_pitch(n_cols - 1).  Asynchronous on `stream`. */
int nw_fill_colband_async(nw_ctx *ctx, const int8_t *d_s1, int64_t n1, const int8_t *d_s2,
                          int64_t n2, const nw_params *p, const nw_colband *band, int32_t *d_t,
                          int64_t pitch, void *stream);

/* Row bands in HORIZONTAL strips (the config-4 row-band case, short chain) ----
 * The same contract and partition as nw_fill_band_async (src/mpi/mpi-horz.cpp:4-99,
 * nw_band_layout: band r's row 0 is band r-1's last row) and the same row-major
 * band table, but the band is swept the other way round: its rows are cut into
 * strips of 256 rows that run left to right along the columns, one step per
 * column (the (4, 1) strip kernel on the transposed band, whose store waves
 * write the row-major table in 128-byte row pieces).  Band r's first strip takes
 * row 0 from `feed_in` column by column as band r-1's last strip produces it
 * (granules {tag:32 | w:32}, one per column 0..n1: nw_feed_alloc(device, n1)), and
 * band r's last strip publishes its last row into `feed_out`.  Band r+1 therefore
 * starts 256 rows (a strip's 64-column hop) after band r instead of after band
 * r's whole height -- the reference streams its halo in 1280-column chunks for
 * the same reason (mpi-horz.cpp:28-40).  After the fill, row 0 is written from
 * feed_in (the boundary j*gap for band 0) and column 0 is the boundary i*gap.
 * d_t: (n2_band + 1) rows laid out like nw_table_offset's (column 1 starts a
 * 256-byte line), pitch >= nw_table_pitch(n1); d_s2_band: the band's n2_band side
 * characters (global rows row0 + 1 ..).  NW mode, strip shapes (4, 1) (the default,
 * nw_params.substrips = strip_waves = 0) and (2, 2) -- 256 rows either way
 * (NW_ERR_UNSUPPORTED otherwise).  Asynchronous on `stream`. */
/* nw_tband.flags */
enum {
    /* the band's waiting strips poll their feed with s_sleep 1 instead of s_sleep 64
       between polls (and the chain's leader is not throttled): a shorter strip-to-strip
       lag (10.0 vs 12.2-12.5 us) at a slower leading strip (28.0-28.5 vs 26.8-27.2 ms) --
       the better choice for chains of more than ~520 strips (2+ bands of 65536 rows;
       DESIGN.md section 5) */
    NW_TBAND_DENSE_POLLS = 1
};
typedef struct nw_tband {
    const uint64_t *feed_in;  /* NULL: first band (row 0 = the boundary j*gap)     */
    uint64_t *feed_out;       /* NULL: last band                                    */
    uint32_t tag;             /* launch tag, as nw_colband.tag                      */
    uint32_t flags;           /* NW_TBAND_* (0: sparse polls); unknown bits refused */
    int64_t row0;             /* global row of the band's row 0 (nw_band_layout start;
                                 0 exactly when feed_in is NULL)                    */
} nw_tband;

int nw_fill_tband_async(nw_ctx *ctx, const int8_t *d_s1, int64_t n1, const int8_t *d_s2_band,
                        int64_t n2_band, const nw_params *p, const nw_tband *band, int32_t *d_t,
                        int64_t pitch, void *stream);

/* Cross-process device pointers (one process per GPU): export a device
 * allocation, open a peer's export.  Handles are NW_IPC_HANDLE_BYTES bytes. */
#define NW_IPC_HANDLE_BYTES 64
int nw_ipc_get_handle(const void *d_ptr, void *handle);
int nw_ipc_open_handle(const void *handle, void **d_ptr);
int nw_ipc_close_handle(void *d_ptr);

/* Launch-to-launch flow control between neighbouring bands -------------------
 * A band sweep that enqueues K fills back to back (no host round trip between
 * them) alternates two halo / feed buffers by launch parity, so the producer's
 * launch k + 2 must not start before the consumer's launch k has read buffer
 * k % 2.  The consumer signals "done with launch k" into a LINK word that lives
 * in the producer's memory (a peer store over xGMI), the producer's stream waits
 * on it.  (The reference's blocking MPI_Send / MPI_Recv pairs,
 * src/mpi/mpi-horz.cpp:41-42,53-54, give the same ordering per chunk.)
 * nw_link_alloc: a zeroed 256-byte fine-grained word pair of its own allocation
 *   (exportable by nw_ipc_get_handle; free with nw_halo_free).
 * nw_link_wait_async: stream-ordered wait until word[0] >= value (wrapping
 *   compare); after timeout_ms (0 = 20000) it gives up and records value in
 *   word[1].
 * nw_link_wait_ctx_async: the same, and a wait that gives up also records the
 *   failure in ctx (code 4): ctx's next fill then gives up at once, without
 *   publishing into the buffer its consumer has not released, and nw_ctx_status
 *   reports NW_ERR_TIMEOUT.
 * nw_link_signal_async: stream-ordered word[0] = value (word may be peer memory).
 * nw_link_status: word[1] (0 = no wait gave up), read synchronously. */
int nw_link_alloc(int device, uint32_t **d_word);
int nw_link_wait_async(uint32_t *d_word, uint32_t value, int32_t timeout_ms, void *stream);
int nw_link_wait_ctx_async(nw_ctx *ctx, uint32_t *d_word, uint32_t value, int32_t timeout_ms, void *stream);
int nw_link_signal_async(uint32_t *d_word, uint32_t value, void *stream);
int nw_link_status(const uint32_t *d_word, uint32_t *out);

/* NW_ERR_TIMEOUT if ANY launch on ctx since the previous call gave up (an
 * in-kernel watchdog, or a nw_link_wait_ctx_async that expired), else NW_OK;
 * syncs the stream and clears the record.  Until it is read, a recorded failure
 * makes every later launch on ctx give up at once (a back-to-back sweep stops
 * at its first failure instead of waiting out one watchdog per launch). */
int nw_ctx_status(nw_ctx *ctx, void *stream);

/* Debug hooks (diagnosis, not needed for fills).
 * nw_debug_ctrl: the 8 control words of the context's last launch: [0] strip
 *   ticket, [1] error code (0 ok; 1 hand-off granule wait -- strips, panels, the
 *   finisher's look-back (site 30) --, 2 halo wait, 3 LDS counter wait expired), [2] site << 24 | wave << 16 | address bits, [3] the
 *   value the wait needed, [4] the value it last saw.  Syncs the device.  (A
 *   launch that a recorded failure made give up carries that failure's words.)
 * nw_debug_failure: the first failure recorded on ctx -- code (1 granule wait,
 *   2 halo wait, 3 LDS counter, 4 link wait), site word, need, seen, and the
 *   number of failed launches (the failing one and every launch it poisoned) -- pending, or as the last nw_ctx_status cleared it.
 * nw_debug_set_trace: per-strip timeline buffer (device memory of at least
 *   strips * nw_debug_trace_words() uint64), NULL = off. */
int nw_debug_ctrl(nw_ctx *ctx, uint32_t *out8);
int nw_debug_failure(nw_ctx *ctx, uint32_t *out5);
int nw_debug_set_trace(nw_ctx *ctx, void *d_trace);
int32_t nw_debug_trace_words(void);
/* nw_debug_tb_shift: the cumulative column shift of window k of a traceback round
 *   from local (is, js) with band half-width `band`, in a table whose row 0 is global
 *   row row0 (0: a whole table; host arithmetic, no device). */
int64_t nw_debug_tb_shift(int64_t k, int64_t is, int64_t js, int32_t band, int32_t aim, int64_t row0);

/* Host helpers ------------------------------------------------------------- */

/* readSequence semantics (src/common/helper.cpp:3-25): every byte of the file,
 * no stripping.  *out is malloc'ed; free with nw_free().  Returns NW_OK or
 * NW_ERR_ARG if the file cannot be opened. */
int nw_read_bdna(const char *path, int8_t **out, int64_t *n);
void nw_free(void *p);

/* Seeded synthetic sequence: i.i.d. uniform bytes in {1,2,3,4} (SplitMix64). */
void nw_synth_bdna(uint64_t seed, int64_t n, int8_t *out);

/* Alignment ops (nw_align, nw_traceback, nw_sw_align, nw_sw_traceback) on the
 * host, no device.  The path starts at cell (begin_i, begin_j) -- (0, 0) for a
 * global alignment, nw_alignment.begin_* for a local one -- and op k moves to the
 * next cell: 0 pairs s1[j] with s2[i], 1 pairs s2[i] with a gap, 2 pairs s1[j]
 * with a gap (i, j the cell before the move).  Both return NW_ERR_ARG for an op
 * above 2 and for ops that run past either sequence.
 * nw_ops_expand: the two gapped rows, n_ops bytes each (0 = gap, the .bdna
 *   convention): row1 from s1, row2 from s2.
 * nw_ops_score: the sum of match / mismatch / gap along the ops.
 * nw_ops_score_affine: the same sum under affine gap cost -- match / mismatch per op
 *   0, gap per op 1 or 2, plus gap_open whenever an op 1 or 2 differs from the op
 *   before it (the first op has none before it: a gap there opens a run). */
int nw_ops_expand(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i,
                  int64_t begin_j, const uint8_t *ops, int64_t n_ops, int8_t *row1, int8_t *row2);
int nw_ops_score(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i,
                 int64_t begin_j, const uint8_t *ops, int64_t n_ops, const nw_params *p, int64_t *score);
int nw_ops_score_affine(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i,
                        int64_t begin_j, const uint8_t *ops, int64_t n_ops, const nw_params *p, int32_t gap_open,
                        int64_t *score);
/* nw_ops_score_matrix: nw_ops_score_affine with score[index[s1[j]]][index[s2[i]]] per op 0;
 *   also NW_ERR_ARG for m == NULL, n outside 1 .. NW_SUBMAT_MAX, a reserved word != 0, an
 *   index entry >= n. */
int nw_ops_score_matrix(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i,
                        int64_t begin_j, const uint8_t *ops, int64_t n_ops, const nw_params *p, const nw_submat *m,
                        int32_t gap_open, int64_t *score);
/* nw_ops_score_dual: nw_ops_score_matrix under the two-piece gap cost of the nw_*_batch_dual
 *   entries: every maximal run of k ops 1, or of k ops 2, adds max(gap_open + k * gap,
 *   gap_open2 + k * gap2); an up-run directly followed by a left-run is two runs. */
int nw_ops_score_dual(const int8_t *s1, int64_t n1, const int8_t *s2, int64_t n2, int64_t begin_i,
                      int64_t begin_j, const uint8_t *ops, int64_t n_ops, const nw_params *p, const nw_submat *m,
                      int32_t gap_open, int32_t gap_open2, int32_t gap2, int64_t *score);

#ifdef __cplusplus
}
#endif
#endif /* NW_HIP_H */
