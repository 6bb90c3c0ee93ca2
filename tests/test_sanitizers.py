"""Host-side sanitizer runs (CPU only; GPU sanitizers are not available on the pool).

* oracle/san_check.c under AddressSanitizer + UndefinedBehaviorSanitizer: every
  entry point of the C restatement on small ragged shapes (empty included),
  cross-checked against each other (serial fill, score-only rows/checksums, row
  and column bands, SW fill / best cell / traceback replay).
* the idxarray-mt restatement (nw_oracle.c, idxarray-mt.cpp:4-70 semantics) under
  ThreadSanitizer, built with LLVM's libomp + Archer so that OpenMP's own
  synchronisation is visible to TSan (libgomp is not instrumented: its barriers
  show up as false races).
* the product's .bdna reader / synthetic generator (csrc/nw_bdna.cpp, host
  code of the drop-in helper.cpp:3-25) under ASan + UBSan on every fixture, an
  empty file and a missing file.
* the device-free half of nw_fill's copy-back (csrc/nw_hostcopy.h: the threaded
  memcpy, the copy-thread rule, the chunk plan) from a stand-alone program:
  par_memcpy under ASan + UBSan over the sizes at which the span arithmetic can
  leave bytes uncopied or run past the block, once under TSan, and the plan and
  the thread rule against tests/nw_hostcopy.py's restatement.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
LLVM = "/opt/rocm/lib/llvm"
BDNA_DIR = os.path.join(ROOT, "tests", "golden", "bdna")


def _run(cmd, env=None, timeout=120):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)


def _need(tool):
    if shutil.which(tool) is None and not os.path.exists(tool):
        pytest.skip(f"{tool} not available")


def test_oracle_asan_ubsan(tmp_path):
    _need("gcc")
    exe = str(tmp_path / "asan")
    r = _run(["gcc", "-std=c11", "-O1", "-g", "-fopenmp", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=all", "-o", exe,
              os.path.join(ORACLE, "san_check.c"), os.path.join(ORACLE, "nw_oracle.c")])
    assert r.returncode == 0, r.stderr
    r = _run([exe, "all"])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr, r.stderr


def test_oracle_idxarray_tsan(tmp_path):
    clang = os.path.join(LLVM, "bin", "clang")
    _need(clang)
    if not os.path.exists(os.path.join(LLVM, "lib", "libarcher.so")):
        pytest.skip("LLVM OpenMP Archer not available")
    exe = str(tmp_path / "tsan")
    r = _run([clang, "-std=c11", "-O1", "-g", "-fopenmp", "-fsanitize=thread", "-o", exe,
              os.path.join(ORACLE, "san_check.c"), os.path.join(ORACLE, "nw_oracle.c"),
              "-L" + os.path.join(LLVM, "lib"), "-Wl,-rpath," + os.path.join(LLVM, "lib")])
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, TSAN_OPTIONS="ignore_noninstrumented_modules=1 halt_on_error=1",
               OMP_NUM_THREADS="4")
    r = _run([exe, "threads"], env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stderr, r.stderr


BDNA_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "nw_hip.h"
int main(int argc, char **argv) {
    // argv[1..]: paths; prints "<n> <sum>" or "err <code>" per path
    for (int a = 1; a < argc; ++a) {
        int8_t *p = nullptr; int64_t n = -1;
        int rc = nw_read_bdna(argv[a], &p, &n);
        if (rc != 0) { std::printf("err %d\n", rc); continue; }
        long long s = 0;
        for (int64_t i = 0; i < n; ++i) s += p[i];
        std::printf("%lld %lld\n", (long long)n, s);
        nw_free(p);
    }
    int8_t buf[1000];
    nw_synth_bdna(7, 1000, buf);
    for (int i = 0; i < 1000; ++i) if (buf[i] < 1 || buf[i] > 4) return 3;
    return 0;
}
"""


def test_bdna_reader_asan(tmp_path):
    _need("g++")
    src = tmp_path / "bdna_main.cpp"
    src.write_text(BDNA_MAIN)
    exe = str(tmp_path / "bdna_asan")
    r = _run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
              "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src),
              os.path.join(ROOT, "fast-needleman-wunsch_amd", "csrc", "nw_bdna.cpp")])
    assert r.returncode == 0, r.stderr
    fixtures = sorted(os.path.join(BDNA_DIR, f) for f in os.listdir(BDNA_DIR) if f.endswith(".bdna"))
    assert fixtures
    empty = tmp_path / "empty.bdna"
    empty.write_bytes(b"")
    paths = fixtures + [str(empty), str(tmp_path / "missing.bdna")]
    r = _run([exe] + paths)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(paths)
    for path, line in zip(fixtures, lines):
        data = open(path, "rb").read()
        n, s = map(int, line.split())
        assert n == len(data) and s == sum(int.from_bytes(bytes([b]), "little", signed=True) for b in data)
    assert lines[-2].split()[0] in ("0", "err")
    assert lines[-1].startswith("err")


# ---------------------------------------------------------------- nw_fill's copy-back, device-free
CSRC = os.path.join(ROOT, "fast-needleman-wunsch_amd", "csrc")

HOSTCOPY_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "nw_hostcopy.h"
// copy T,T,... B B ...   par_memcpy of B bytes with T threads, every pair: source and
//                        destination in heap blocks of exactly B bytes, the destination
//                        poisoned; prints "FAIL bytes B threads T uncopied U" per miss
// plan FILE              per line "table_bytes row_bytes rows stage_cap": prints
//                        "stage_cap rpc nch direct rows_covered in_order max_chunk_rows"
// threads CORES E E ...  copy_threads_of per E ("--unset": no variable), one per line
int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "copy" && argc > 3) {
        std::vector<int> threads;
        for (char *t = std::strtok(argv[2], ","); t; t = std::strtok(nullptr, ",")) threads.push_back(std::atoi(t));
        int bad = 0;
        for (int a = 3; a < argc; ++a) {
            const size_t n = (size_t)std::strtoull(argv[a], nullptr, 10);
            char *src = (char *)std::malloc(n), *dst = (char *)std::malloc(n);
            if (!src || !dst) return 2;
            for (size_t i = 0; i < n; ++i) src[i] = (char)(1 + (i * 2654435761u >> 13) % 200);  // never 0xA5
            for (int t : threads) {
                std::memset(dst, 0xA5, n);
                nwh::par_memcpy(dst, src, n, t);
                if (std::memcmp(dst, src, n) != 0) {
                    size_t u = 0;
                    for (size_t i = 0; i < n; ++i) u += dst[i] != src[i];
                    std::printf("FAIL bytes %zu threads %d uncopied %zu\n", n, t, u);
                    ++bad;
                }
            }
            std::free(src);
            std::free(dst);
        }
        std::printf(bad ? "failed\n" : "ok\n");
        return bad ? 1 : 0;
    }
    if (mode == "plan" && argc > 2) {
        std::FILE *f = std::fopen(argv[2], "r");
        if (!f) return 2;
        unsigned long long tb, rb, cap;
        long long rows;
        while (std::fscanf(f, "%llu %llu %lld %llu", &tb, &rb, &rows, &cap) == 4) {
            const nwh::CopyPlan p = nwh::copy_plan((size_t)tb, (size_t)rb, rows, (size_t)cap);
            long long covered = 0, biggest = 0;
            bool in_order = true;
            for (int64_t ch = 0; ch < p.nch; ++ch) {
                in_order = in_order && p.first_row(ch) == covered && p.rows_of(ch, rows) >= 1;
                covered += p.rows_of(ch, rows);
                biggest = std::max<long long>(biggest, p.rows_of(ch, rows));
            }
            std::printf("%zu %lld %lld %d %lld %d %lld\n", p.stage_cap, (long long)p.rpc, (long long)p.nch,
                        (int)p.direct, covered, (int)in_order, biggest);
        }
        std::fclose(f);
        return 0;
    }
    if (mode == "threads" && argc > 2) {
        for (int a = 3; a < argc; ++a)
            std::printf("%d\n", nwh::copy_threads_of(std::strcmp(argv[a], "--unset") ? argv[a] : nullptr,
                                                     (unsigned)std::atoi(argv[2])));
        return 0;
    }
    return 2;
}
"""

MIB = 1 << 20
# The sizes at which par_memcpy's span (bytes / threads, rounded up to 4096) is on an
# edge: the 8 MiB threshold below which the copy is one memcpy; 32768 k + 4, where
# the floor quotient by 8 is a multiple of 4096 and 8 does not divide (k = 256 is 8
# MiB + 4, the (5418, 386) table); the same for 3 threads, 12288 k + 4 and + 8 (k =
# 683, the first above 8 MiB); one byte under and over a whole span.
COPY_BYTES = [8 * MIB - 4, 8 * MIB, 8 * MIB + 4, 32768 * 257 + 4, 32768 * 300 + 4, 32768 * 512 + 4,
              12288 * 683 + 4, 12288 * 683 + 8, 8 * MIB + 4095, 8 * MIB + 4097]
COPY_THREADS = list(range(1, 18)) + [63, 64]


def _hostcopy_exe(tmp_path, name, san):
    _need("g++")
    src = tmp_path / "hostcopy_main.cpp"
    src.write_text(HOSTCOPY_MAIN)
    exe = str(tmp_path / name)
    r = _run(["g++", "-std=c++17", "-O1", "-g", "-pthread", *san, "-I", CSRC, "-o", exe, str(src)])
    assert r.returncode == 0, r.stderr
    return exe


def test_par_memcpy_asan_ubsan(tmp_path):
    """Every byte copied, none written or read beyond the exactly sized blocks, for
    every (bytes, threads).  (Before the span was taken from the ceiling of bytes /
    threads, this reported 4 uncopied bytes at 8 MiB + 4 with 8 threads.)"""
    import nw_hostcopy as hc
    # the restatement of the span before the fix loses bytes on this grid, the fixed one none
    lost = [(b, t) for b in COPY_BYTES for t in COPY_THREADS if hc.uncopied(b, t, fixed=False)]
    assert (8 * MIB + 4, 8) in lost and (32768 * 300 + 4, 5) in lost and len(lost) >= 10
    assert not [(b, t) for b in COPY_BYTES for t in COPY_THREADS if hc.uncopied(b, t)]
    exe = _hostcopy_exe(tmp_path, "hostcopy_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = _run([exe, "copy", ",".join(map(str, COPY_THREADS))] + [str(b) for b in COPY_BYTES], timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr


def test_par_memcpy_tsan(tmp_path):
    """The spans of the copy threads are disjoint: no two threads write one byte."""
    exe = _hostcopy_exe(tmp_path, "hostcopy_tsan", ["-fsanitize=thread"])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = _run([exe, "copy", "2,3,8,17,64", str(8 * MIB + 4), str(12288 * 683 + 8), str(8 * MIB + 4097)],
             env=env, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stderr, r.stderr


def _plan_grid():
    """(n1, n2, stage_cap): the GPU module's shapes and their neighbours, rows as
    wide as a chunk to the byte, tables at the 16 MiB floor, the 2 MiB rounding and
    the 256 MiB cap, under every stage_cap an earlier call can have left."""
    shapes = [(0, 0), (1, 1), (1500, 1100), (5418, 386), (386, 5418), (4194304, 3), (12, 1049204),
              (1048575, 13), (13, 1048575), (3000000, 4), (2359295, 6), (4400000, 1), (20000, 14000),
              (1051306, 9), (355234, 33), (1500000, 14), (100000, 100000), (2**31, 2), (0, 5 * 10**7)]
    for w in (16 * MIB, 18 * MIB, 256 * MIB):  # a row of exactly / just under / just over a chunk
        shapes += [(w // 4 - 1 + d, r) for d in (-1, 0, 1) for r in (0, 1, 2, 3, 7)]
    for t in (48 * MIB, 54 * MIB, 768 * MIB):  # table bytes at the floor / a rounding step / the cap
        shapes += [(999, (t + d) // 4000 - 1) for d in (-4000, 0, 4000)]
    caps = [0, 16 * MIB, 18 * MIB, 20 * MIB, 22 * MIB, 30 * MIB, 256 * MIB]
    return [(n1, n2, c) for (n1, n2) in shapes for c in caps]


def test_copy_plan_vs_restatement(tmp_path):
    """csrc/nw_hostcopy.h copy_plan on a grid of (n1, n2, stage_cap): the chunks tile
    rows 0..n2 once and in order, no chunk is larger than the chunk size, direct
    holds iff one row is; tests/nw_hostcopy.py gives the same plan; the plans the GPU
    module relies on are pinned."""
    import nw_hostcopy as hc
    exe = _hostcopy_exe(tmp_path, "hostcopy_plan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    grid = _plan_grid()
    f = tmp_path / "grid.txt"
    f.write_text("".join(f"{4 * (n1 + 1) * (n2 + 1)} {4 * (n1 + 1)} {n2 + 1} {c}\n" for n1, n2, c in grid))
    r = _run([exe, "plan", str(f)])
    assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(grid)
    n_direct = 0
    for (n1, n2, c), line in zip(grid, lines):
        cap, rpc, nch, direct, covered, in_order, biggest = map(int, line.split())
        w, rows = 4 * (n1 + 1), n2 + 1
        assert (cap, rpc, nch, bool(direct)) == tuple(hc.plan(n1, n2, c)), (n1, n2, c)
        assert covered == rows and in_order == 1, (n1, n2, c)
        assert cap >= c and cap >= hc.STAGE_MIN and (cap <= hc.STAGE_MAX or cap == c)
        assert bool(direct) == (w > cap), (n1, n2, c)
        assert direct or biggest * w <= cap, (n1, n2, c)
        assert sum(nr for _, nr in hc.chunks(hc.plan(n1, n2, c), rows)) == rows
        n_direct += direct
    assert 10 <= n_direct <= len(grid) - 100
    P = hc.Plan
    pins = {(5418, 386, 0): P(16 * MIB, 773, 1, False), (386, 5418, 0): P(16 * MIB, 10837, 1, False),
            (4194304, 3, 0): P(22 * MIB, 1, 4, False), (12, 1049204, 0): P(18 * MIB, 362968, 3, False),
            (1048575, 13, 0): P(20 * MIB, 5, 3, False), (13, 1048575, 0): P(20 * MIB, 374491, 3, False),
            (3000000, 4, 0): P(20 * MIB, 1, 5, False), (2359295, 6, 0): P(22 * MIB, 2, 4, False),
            (4400000, 1, 0): P(16 * MIB, 1, 2, True), (20000, 14000, 0): P(256 * MIB, 3355, 5, False),
            (1051306, 9, 0): P(16 * MIB, 3, 4, False), (355234, 33, 0): P(16 * MIB, 11, 4, False),
            (1500000, 14, 0): P(30 * MIB, 5, 3, False), (13, 1048575, 30 * MIB): P(30 * MIB, 561737, 2, False),
            (1048575, 13, 256 * MIB): P(256 * MIB, 64, 1, False), (1500, 1100, 20 * MIB): P(20 * MIB, 3492, 1, False)}
    for (n1, n2, c), want in pins.items():
        assert hc.plan(n1, n2, c) == want, (n1, n2, c)
    assert hc.chunks(hc.plan(12, 1049204), 1049205)[-1] == (725936, 323269)
    assert [nr for _, nr in hc.chunks(hc.plan(1048575, 13), 14)] == [5, 5, 4]
    assert hc.warm_cap() == 256 * MIB
    # the cells the span before the fix left unwritten, with the default 8 threads
    assert hc.holes(5418, 386) == [(0, 386, 5418)] and hc.holes(386, 5418) == [(0, 5418, 386)]
    assert hc.holes(4194304, 3) == [(ch, ch, 4194304) for ch in range(4)]
    assert hc.holes(12, 1049204) == [(2, 1049204, 12)]
    assert hc.holes(1051306, 9) == [(0, 2, 1051306), (1, 5, 1051306), (2, 8, 1051306)]
    assert hc.holes(355234, 33) == [(0, 10, 355234), (1, 21, 355234), (2, 32, 355234)]
    assert not hc.holes(5418, 386, fixed=True) and not hc.holes(4400000, 1)


def test_copy_threads_rule(tmp_path):
    """NW_COPY_THREADS: clamped to 1..64; 0, negative and non-numeric are 1; unset is
    min(8, cores).  The header and the restatement agree."""
    import nw_hostcopy as hc
    exe = _hostcopy_exe(tmp_path, "hostcopy_thr", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    envs = ["--unset", "1", "2", "3", "5", "7", "8", "16", "64", "65", "1000", "0", "-3", "x", "", " 12", "4x",
            "99999999999999999999", "-99999999999999999999"]
    want = [8, 1, 2, 3, 5, 7, 8, 16, 64, 64, 64, 1, 1, 1, 1, 12, 4, 64, 1]
    for cores, unset in ((256, 8), (4, 4), (0, 1)):
        r = _run([exe, "threads", str(cores)] + envs)
        assert r.returncode == 0 and "runtime error" not in r.stderr, r.stdout + r.stderr
        got = list(map(int, r.stdout.split()))
        assert got == [unset] + want[1:]
        assert got == [hc.threads_of(None if e == "--unset" else e, cores) for e in envs]
