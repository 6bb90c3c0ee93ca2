"""GPU: the host table of nw_fill / nw_fill_emb against the oracle, on the tables at
which the copy-back (csrc/nw_hostpath.cpp host_copy_back, csrc/nw_hostcopy.h) takes
each of its paths: several staging chunks and the reuse of the three-slot ring, a
short last chunk, the threaded memcpy at the sizes where its spans meet the end of
a chunk, the strided (emb) copy over several chunks, a row wider than a chunk
(direct hipMemcpy2D), the 256 MiB cap, a ring grown by earlier calls, the device
table reused at another pitch, nw_host_warmup / nw_host_release, NW_COPY_THREADS.

Every call goes through ctypes into a table pre-filled with a value no cell can
hold (the range bound keeps |t| < 2^28), so a cell that is not copied is seen, not
left to whatever the allocator returned.  Every comparison is exact.  The path a
call took is read from the library's own NW_HOST_TIMING line ("copy back: N chunks
of M MiB, T threads"; none on the direct branch) and asserted, together with what
tests/nw_hostcopy.py's restatement says about the shape, before the table is
looked at.
"""
import ctypes
import functools
import os
import re
import threading

import numpy as np
import pytest

import nw_hostcopy as hc
import nwhip
import oracle

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
SCHEME = (1, -1, -1)
MIB = hc.MIB
COPY_LINE = re.compile(r"copy back: (\d+) chunks of (\d+) MiB, (\d+) threads")
FILL_LINE = re.compile(r"nw_fill: prepare .* copy back [0-9.]+ ms \(([0-9.]+) GB/s\)")
I8P, I32P = ctypes.POINTER(ctypes.c_int8), ctypes.POINTER(ctypes.c_int32)
CORES = len(os.sched_getaffinity(0))  # what std::thread::hardware_concurrency() reports


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    return _t


@pytest.fixture(autouse=True)
def fresh_host_path(torch, monkeypatch):
    """Every test starts and ends with nothing held: stage_cap only grows, so the plan
    of a table depends on the calls before it."""
    monkeypatch.setenv("NW_HOST_TIMING", "1")
    monkeypatch.delenv("NW_COPY_THREADS", raising=False)
    nwhip.host_release()
    yield
    nwhip.host_release()


def seqs(n1, n2):
    rng = np.random.default_rng(n1 * 31 + n2)
    return rng.integers(1, 5, n1).astype(np.int8), rng.integers(1, 5, n2).astype(np.int8)


def _readonly(t):
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def want(n1, n2):
    """oracle.fill of the shape's pair, computed once and shared (read-only)."""
    return _readonly(oracle.fill(*seqs(n1, n2), SCHEME))


@functools.lru_cache(maxsize=None)
def want_emb(n1, n2):
    return _readonly(oracle.fill_emb(*seqs(n1, n2), SCHEME))


def call_fill(n1, n2, emb=False, table=True):
    """lib().nw_fill / nw_fill_emb into a poisoned host table: (table or None, NwResult)."""
    s1, s2 = seqs(n1, n2)
    t = np.full((n2 + 1, n1 + 1 + emb), POISON, dtype=np.int32) if table else None
    r, p = nwhip.NwResult(), nwhip.params(SCHEME, device=0)
    L = nwhip.lib()
    st = (L.nw_fill_emb if emb else L.nw_fill)(s1.ctypes.data_as(I8P), n1, s2.ctypes.data_as(I8P), n2, ctypes.byref(p),
                                             t.ctypes.data_as(I32P) if table else None, ctypes.byref(r))
    assert st == nwhip.NW_OK and r.status == nwhip.NW_OK, (n1, n2, st)
    return t, r


def copy_lines(capfd):
    """[(chunks, MiB a chunk, threads)] of the copy-back lines printed since the last read."""
    err = capfd.readouterr().err
    return [tuple(map(int, m.groups())) for m in COPY_LINE.finditer(err)], err


def assert_same(t, w, what):
    assert t.shape == w.shape, what
    bad = np.flatnonzero(t.reshape(-1) != w.reshape(-1))
    if bad.size:
        i, j = divmod(int(bad[0]), t.shape[1])
        raise AssertionError(f"{what}: {bad.size} cells differ ({int((t == POISON).sum())} never written), first at "
                             f"({i}, {j}): got {t[i, j]}, want {w[i, j]}")


def check_fill(capfd, n1, n2, line, what=None):
    """One nw_fill whose copy-back must print exactly `line` ((N, M, T), or None: the
    direct branch); then the table against the oracle."""
    capfd.readouterr()
    t, r = call_fill(n1, n2)
    lines, err = copy_lines(capfd)
    assert lines == ([line] if line else []), (n1, n2, err)
    assert len(FILL_LINE.findall(err)) == 1, err
    w = want(n1, n2)
    assert_same(t, w, what or str((n1, n2)))
    assert r.score == w[-1, -1]
    return t


# (n1, n2): (chunks, MiB a chunk) after a release (None: direct), rows of the chunks,
# and the cells the threaded copy left unwritten before its span was fixed, as
# (chunk, row, column), with 8 threads -- all asserted from the restatement
SHAPES = {
    # 8 MiB + 4 B in one chunk: the one hole is the last cell, the score the reference driver prints
    (5418, 386): ((1, 16), [387], [(0, 386, 5418)]),
    (386, 5418): ((1, 16), [5419], [(0, 5418, 386)]),
    # 16 MiB + 4 B a row, a row a chunk: the last cell of every row; slot 0 used twice
    (4194304, 3): ((4, 22), [1, 1, 1, 1], [(0, 0, 4194304), (1, 1, 4194304), (2, 2, 4194304), (3, 3, 4194304)]),
    # tall; the short last chunk is 32768 * 513 + 4 bytes
    (12, 1049204): ((3, 18), [362968, 362968, 323269], [(2, 1049204, 12)]),
    # the ring filled once, no slot used twice, wide and tall
    (1048575, 13): ((3, 20), [5, 5, 4], []),
    (13, 1048575): ((3, 20), [374491, 374491, 299594], []),
    # slots 0 and 1 used twice
    (3000000, 4): ((5, 20), [1] * 5, []),
    # a last chunk of one row after chunks of two
    (2359295, 6): ((4, 22), [2, 2, 2, 1], []),
    # a 16.8 MiB row is wider than the 16 MiB chunk: direct, no staging
    (4400000, 1): (None, [1, 1], []),
    # three whole chunks of 32768 k + 4 bytes and a short one: holes in chunks 1 and 2, neither first nor last
    (1051306, 9): ((4, 16), [3, 3, 3, 1], [(0, 2, 1051306), (1, 5, 1051306), (2, 8, 1051306)]),
    (355234, 33): ((4, 16), [11, 11, 11, 1], [(0, 10, 355234), (1, 21, 355234), (2, 32, 355234)]),
}


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_tables_vs_oracle(capfd, monkeypatch, shape):
    """nw_fill's host table after a release, with 8 copy threads set (the count the
    holes are worked out for; test_copy_threads runs the default)."""
    n1, n2 = shape
    line, rows, holes = SHAPES[shape]
    p = hc.plan(n1, n2)
    assert [nr for _, nr in hc.chunks(p, n2 + 1)] == rows
    assert (None if p.direct else (p.nch, p.stage_cap // MIB)) == line and p.stage_cap % MIB == 0
    assert hc.holes(n1, n2, threads=8) == holes and not hc.holes(n1, n2, threads=8, fixed=True)
    monkeypatch.setenv("NW_COPY_THREADS", "8")
    check_fill(capfd, n1, n2, line + (8,) if line else None)


def test_table_at_the_chunk_cap(capfd):
    """1068 MiB: five chunks at the 256 MiB cap (a third of the table would be 356),
    slots 0 and 1 used twice, the default thread count."""
    n1, n2 = 20000, 14000
    p = hc.plan(n1, n2)
    assert p == hc.Plan(hc.STAGE_MAX, 3355, 5, False) and hc.stage_want(4 * (n1 + 1) * (n2 + 1)) == hc.STAGE_MAX
    assert 4 * (n1 + 1) * (n2 + 1) // 3 > hc.STAGE_MAX
    capfd.readouterr()
    t, r = call_fill(n1, n2)
    lines, err = copy_lines(capfd)
    assert lines == [(5, 256, min(8, CORES))], err
    w = oracle.fill(*seqs(n1, n2), SCHEME)
    assert_same(t, w, "20000 x 14000")
    assert r.score == w[-1, -1]


@pytest.mark.parametrize("shape", [(1048575, 13), (13, 1048575)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_emb_over_three_chunks(capfd, shape):
    """nw_fill_emb: rows of n1 + 1 cells copied one by one out of three chunks into
    rows of n1 + 2; column 0 is n1 + 2 in every row and nothing is left unwritten."""
    n1, n2 = shape
    assert hc.plan(n1, n2)[1:] == (SHAPES[shape][1][0], 3, False)
    capfd.readouterr()
    t, r = call_fill(n1, n2, emb=True)
    lines, err = copy_lines(capfd)
    assert lines == [(3, 20, min(8, CORES))], err
    assert (t[:, 0] == n1 + 2).all()
    assert not (t == POISON).any()
    assert_same(t, want_emb(n1, n2), f"emb {shape}")
    assert_same(t[:, 1:], want(n1, n2), f"emb {shape} columns 1..")
    assert r.score == want(n1, n2)[-1, -1]


# one chunk whose bytes / threads is a whole multiple of 4096 (the span needs no
# rounding).  5 and 7 threads: floor(bytes / threads), with a remainder of 4 bytes that
# the span before the fix lost.  3 threads: no such size exists for int32 cells
# (3 * 4096 k + r is a multiple of 4 only for r = 0), so the exact quotient.
EXACT_SPAN = {"3": (1023, 2048), "5": (1428, 1468), "7": (1024, 2048)}


@pytest.mark.parametrize("value", [None, "1", "2", "3", "5", "7", "8", "16", "64", "1000", "0", "-3", "x"],
                         ids=lambda v: "unset" if v is None else v)
def test_copy_threads(capfd, monkeypatch, value):
    """NW_COPY_THREADS is read on every call; the line reports the documented count
    (unset: min(8, cores); above 64: 64; 0, negative, not a number: 1) and the table
    is the oracle's under every count."""
    if value is None:
        monkeypatch.delenv("NW_COPY_THREADS", raising=False)
    else:
        monkeypatch.setenv("NW_COPY_THREADS", value)
    T = hc.threads_of(value, CORES)
    assert T == {None: min(8, CORES), "1000": 64, "0": 1, "-3": 1, "x": 1}.get(value) or T == int(value)
    check_fill(capfd, 5418, 386, (1, 16, T))
    check_fill(capfd, 1048575, 13, (3, 20, T))
    if value in EXACT_SPAN:
        n1, n2 = EXACT_SPAN[value]
        nbytes = 4 * (n1 + 1) * (n2 + 1)
        assert hc.plan(n1, n2, 20 * MIB).nch == 1 and nbytes >= hc.PAR_MIN and (nbytes // T) % 4096 == 0
        assert [c for _, *c in hc.holes(n1, n2, threads=T, stage_cap=20 * MIB)] == ([] if T == 3 else [[n2, n1]])
        check_fill(capfd, n1, n2, (1, 20, T))


def test_carried_state(capfd):
    """What one call leaves for the next: the ring's chunk size (grow-only), the device
    table at another pitch, the context shared with nw_sw_align and nw_align, and
    nw_host_warmup / nw_host_release around them.  Every result against the oracle."""
    L = nwhip.lib()
    T = min(8, CORES)
    tall, wide, small, bigger = (13, 1048575), (1048575, 13), (1500, 1100), (1500000, 14)
    assert hc.plan(*tall) == hc.Plan(20 * MIB, 374491, 3, False)
    check_fill(capfd, *tall, (3, 20, T), "tall after a release")
    assert hc.plan(*small, 20 * MIB) == hc.Plan(20 * MIB, 3492, 1, False)
    check_fill(capfd, *small, (1, 20, T), "small in the kept ring")
    # score only: no copy-back, the device table of the call before is reused
    capfd.readouterr()
    _, r = call_fill(2000, 900, table=False)
    lines, err = copy_lines(capfd)
    assert lines == [] and r.score == oracle.score(*seqs(2000, 900), SCHEME), err
    # the alignments run through the same per-device state (host_run)
    s1, s2 = seqs(300, 200)
    al, ops = nwhip.sw_align(s1, s2, SCHEME, device=0)
    sc, ei, ej = oracle.sw_best(s1, s2, SCHEME)
    wops, bi, bj = oracle.sw_traceback(s1, s2, oracle.sw_fill(s1, s2, SCHEME), (ei, ej), SCHEME)
    assert (al.score, al.end_i, al.end_j, al.begin_i, al.begin_j) == (sc, ei, ej, bi, bj)
    np.testing.assert_array_equal(ops, wops)
    check_fill(capfd, *small, (1, 20, T), "small after sw_align")
    al, ops, _ = nwhip.align(s1, s2, SCHEME, device=0)
    assert al.score == oracle.fill(s1, s2, SCHEME)[-1, -1] == nwhip.ops_score(s1, s2, ops, SCHEME)
    assert (al.end_i, al.end_j, al.n_ops) == (200, 300, ops.size)
    # a larger table grows the ring to 30 MiB ...
    assert hc.plan(*bigger, 20 * MIB) == hc.Plan(30 * MIB, 5, 3, False)
    check_fill(capfd, *bigger, (3, 30, T), "86 MiB, wide")
    # ... under which the tall table is two chunks, not three, in the wide one's device
    # buffer at a pitch of 64 cells instead of 1.5 million
    assert hc.plan(*tall, 30 * MIB) == hc.Plan(30 * MIB, 561737, 2, False)
    assert nwhip.table_pitch(tall[0]) != nwhip.table_pitch(bigger[0])
    check_fill(capfd, *tall, (2, 30, T), "tall in the grown ring")
    assert hc.plan(*wide, 30 * MIB) == hc.Plan(30 * MIB, 7, 2, False)
    check_fill(capfd, *wide, (2, 30, T), "wide after tall")
    # warmup takes the ring to the cap: one chunk
    assert L.nw_host_warmup(0) == nwhip.NW_OK
    assert hc.plan(*wide, hc.warm_cap()) == hc.Plan(256 * MIB, 64, 1, False)
    check_fill(capfd, *wide, (1, 256, T), "wide after warmup")
    check_fill(capfd, *tall, (1, 256, T), "tall after warmup")
    # release twice, release of one device with nothing held, then from nothing again
    nwhip.host_release()
    nwhip.host_release()
    nwhip.host_release(0)
    check_fill(capfd, *tall, (3, 20, T), "tall after the releases")
    assert L.nw_host_warmup(0) == nwhip.NW_OK  # warmup right after a fill: the ring is replaced
    check_fill(capfd, *small, (1, 256, T), "small after the second warmup")


def test_two_python_threads(capfd):
    """Two threads call nw_fill on device 0 at once (ctypes drops the GIL; the
    per-device mutex serialises them): both tables are right.  Whichever call comes
    second sees the ring the first one left."""
    a, b = (1048575, 13), (5418, 386)
    T = min(8, CORES)
    want(*a), want(*b)
    out, errs = {}, []
    gate = threading.Barrier(2)

    def work(shape):
        try:
            gate.wait(timeout=60)
            out[shape] = call_fill(*shape)
        except BaseException as e:  # noqa: BLE001 -- reported by the main thread
            errs.append(e)

    capfd.readouterr()
    ts = [threading.Thread(target=work, args=(s,)) for s in (a, b)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    lines, err = copy_lines(capfd)
    # (b first: 16 MiB, then grown to 20 for a; a first: b finds 20)
    assert sorted(lines) in ([(1, 16, T), (3, 20, T)], [(1, 20, T), (3, 20, T)]), err
    for s in (a, b):
        t, r = out[s]
        assert_same(t, want(*s), f"thread {s}")
        assert r.score == want(*s)[-1, -1]
