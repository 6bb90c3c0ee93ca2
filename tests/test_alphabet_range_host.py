"""CPU: the alphabets, the generator and the batch cases of tests/test_alphabet_range.py,
and the conditions under which they can tell a wrong v_perm score table from a right one.

Seven kernel families (strip fill NW / SW, panel fill NW / SW, checkpointed sweep, linear
batch, affine batch) build per-lane score tables when s1 holds at most 7 distinct bytes:
nw_charmap gives a byte its index among them in increasing unsigned order, indices 0..3
go to a lane's low table, 4..6 to its high table, and the row side maps s2 with
min(charmap[b], 7): selector 7 is "in no column" and reads a mismatch byte.  Every other
test of those kernels draws from the bytes 1..4 (index 3 is the highest that matches), from
9 or 20 letters or from all 256 bytes (compares).  Here the alphabets have 4, 5, 7 and 8
letters and sit at both ends of the signed and of the unsigned byte range.

Everything below is judged from the checkers alone (oracle.score, oracle.sw_best,
tests/nw_gotoh.py), so that a failure on the device points at a kernel:
  1. the high table decides: with every s2 letter of index >= 4 replaced by a byte no
     alphabet holds, the score changes;
  2. selector 7 decides: with every such foreign byte of s2 replaced by the alphabet's
     last letter, the score changes;
  3. the -1 byte decides: v_perm answers a selector of 0xFF (charmap's "absent", should
     the min(.., 7) go missing) with the byte 0xFF = -1; no scheme here has a mismatch
     table byte of -1;
  4. the batch cases hold the letters they claim, pair by pair and over the s1 sides.
A case that fails a condition gets another seed (SEEDS); none is dropped.
"""
import functools

import numpy as np
import pytest

import nw_gotoh
import nwhip
import oracle
from nw_walk import path_score, walk
from test_batch_host import VALID
from test_batch_matrix_host import random_matrix
from test_scheme_range_host import status_of


def _bytes(*v):
    a = np.array(v, np.uint8).view(np.int8)
    a.setflags(write=False)
    return a


A4 = _bytes(0x00, 0x7F, 0x80, 0xFF)
A5 = _bytes(0x00, 0x7F, 0x80, 0xC8, 0xFF)
A7 = _bytes(0x00, 0x01, 0x7F, 0x80, 0xC8, 0xFE, 0xFF)
A8 = _bytes(0x00, 0x01, 0x41, 0x7F, 0x80, 0xC8, 0xFE, 0xFF)  # A7 + 41: eight letters, compares
OUT = _bytes(0x02, 0x42, 0x81, 0xFD)                          # in no alphabet
ALPHABETS = {4: A4, 5: A5, 7: A7, 8: A8}
NDS = [4, 5, 7, 8]
MAX_PERM = 7  # csrc/nw_internal.h kMaxPerm, restated

# the unit kind; generic; sign decides values; a table byte of -128
UNIT, GENERIC, SIGNED, DEEP = (1, 0, -1), (2, -1, -2), (7, -5, 3), (1, -130, -1)
SCHEMES = [UNIT, GENERIC, SIGNED]
SW_SCHEMES = [UNIT, GENERIC, (1, -1, -1), DEEP]  # local alignment refuses a positive gap
OPENS = [-3, -11]
# Under (7, -5, 3) with gap_open -11 the two boundary runs win every cell (3 a step against 7 a
# diagonal less 11 a turn) and no substitution decides anything: that scheme runs with -3 only.
AFFINE = [(s, go) for s in (UNIT, GENERIC, DEEP) for go in OPENS] + [(SIGNED, -3)]

STRIP, PANEL, CKPT, TB = (600, 200), (1100, 130), (300, 150), (300, 200)  # (n1, n2)
BATCH_SIZES = [(300, 150), (257, 65), (5, 130), (1, 1)]
THIN = (5, 130)
# seeds that differ from the default (1000 nd + n1 + 7 n2), and what the default failed: the
# one row letter of a 1 x 1 pair fell to a substitution or to OUT; the thin pairs' ops stayed
# the same under condition 2 with (1, 0, -1), or no column matched under gap_open -11
SEEDS = {(4, 1, 1): 4008, (7, 1, 1): 7009, (5, 5, 130): 1, (7, 5, 130): 1, (8, 5, 130): 1}


def u8(s):
    return np.asarray(s, np.int8).view(np.uint8)


def charmap_of(s1):
    """nw_charmap restated: byte -> index among s1's distinct bytes in unsigned order, 255 = absent."""
    cm = np.full(256, 255, np.int64)
    cm[np.unique(u8(s1))] = np.arange(np.unique(u8(s1)).size)
    return cm


def weights(nd):
    """Letters of index >= 4 carry 60 % together (nd > 4), the rest is uniform."""
    if nd <= 4:
        return np.full(nd, 1.0 / nd)
    w = np.empty(nd)
    w[:4], w[4:] = 0.4 / 4, 0.6 / (nd - 4)
    return w


def mutated_window(rng, s1, n2, alpha):
    """n2 letters: a window of s1 (s1 repeated where it is the shorter) with about 5 % deletions
    and 5 % substitutions from `alpha`, then about 20 % of the positions overwritten from OUT."""
    m = n2 + n2 // 4 + 8
    if s1.size >= m:
        start = int(rng.integers(0, s1.size - m + 1))
        src = s1[start:start + m]
    else:
        src = np.resize(np.roll(s1, -int(rng.integers(0, s1.size))), m)
    s2 = src[rng.random(m) >= 0.05][:n2].copy()
    assert s2.size == n2
    sub = rng.random(n2) < 0.05
    s2[sub] = rng.choice(alpha, int(sub.sum()))
    out = rng.random(n2) < 0.20
    s2[out] = rng.choice(OUT, int(out.sum()))
    return s2


@functools.lru_cache(maxsize=None)
def pair(nd, n1, n2, seed):
    """(s1, s2): s1 from ALPHABETS[nd] by weights(nd), its first nd positions holding every letter
    once (a shorter s1: the last n1 letters, the high ones); s2 = mutated_window of it."""
    alpha = ALPHABETS[nd]
    rng = np.random.default_rng(seed)
    s1 = rng.choice(alpha, n1, p=weights(nd))
    k = min(nd, n1)
    s1[:k] = alpha[nd - k:]
    s2 = mutated_window(rng, s1, n2, alpha)
    for a in (s1, s2):
        a.setflags(write=False)
    return s1, s2


def case(nd, shape):
    """The pair of alphabet nd at this size, with its seed."""
    n1, n2 = shape
    return pair(nd, n1, n2, SEEDS.get((nd, n1, n2), 1000 * nd + n1 + 7 * n2))


@functools.lru_cache(maxsize=None)
def batch(nd):
    return tuple(case(nd, sh) for sh in BATCH_SIZES)


def high_dead(nd, s2):
    """s2 with every letter of index >= 4 replaced by a byte from OUT: what a high table that
    never matches computes."""
    out = np.array(s2, np.int8)
    hit = np.isin(u8(out), u8(ALPHABETS[nd][4:]))
    out[hit] = np.resize(OUT, int(hit.sum()))
    return out


def out_collides(nd, s2, letter=None):
    """s2 with every OUT byte replaced by the alphabet's last letter (or by `letter`): what
    selector 7 computes when it reads the table byte of a letter."""
    out = np.array(s2, np.int8)
    out[np.isin(u8(out), u8(OUT))] = ALPHABETS[nd][-1] if letter is None else letter
    return out


# ------------------------------------------------------------------ the batch-wide decision
LOW, HIGH, MID = (0, 1, 2), (4, 5, 6), (3, 4)  # the indices of A7 that P, Q and R draw s1 from
S2_ONLY = _bytes(0x41, 0x03, 0xC9)             # case (c): three more letters, on s2 sides only


def _sub_pair(rng, idx, n1, n2):
    """s1 over the letters A7[idx], every one present; s2 = mutated_window with a further 10 %
    of its positions drawn from all of A7 (the other pairs' letters)."""
    letters = A7[list(idx)]
    s1 = rng.choice(letters, n1)
    s1[:letters.size] = letters
    s2 = mutated_window(rng, s1, n2, letters)
    other = rng.random(n2) < 0.10
    s2[other] = rng.choice(A7, int(other.sum()))
    return s1, s2


@functools.lru_cache(maxsize=None)
def decision_case(name):
    """(a): P, Q, R over indices {0,1,2}, {4,5,6}, {3,4} of A7 -- no pair holds more than three
    letters in s1, the union over the s1 sides is A7.  (b): (a) plus a pair whose s1 holds 41:
    union 8, compares.  (c): (a) with S2_ONLY over a further 8 % of every s2: the union over
    the s1 sides stays 7."""
    rng = np.random.default_rng(71)
    pairs = [_sub_pair(rng, LOW, 257, 65), _sub_pair(rng, HIGH, 300, 150), _sub_pair(rng, MID, 70, 130)]
    if name == "b":
        s1 = rng.choice(_bytes(0x41, 0x01, 0xFF), 65)
        s1[:3] = _bytes(0x41, 0x01, 0xFF)
        pairs.append((s1, mutated_window(rng, s1, 40, A8)))
    if name == "c":
        for _, b in pairs:
            more = rng.random(b.size) < 0.08
            b[more] = np.resize(S2_ONLY, int(more.sum()))
    for a, b in pairs:
        a.setflags(write=False)
        b.setflags(write=False)
    return tuple(pairs)


# ------------------------------------------------------------------ one context, changing alphabets
SUB3 = _bytes(0x01, 0xC8, 0xFF)  # indices 1, 4, 6 of A7 become 0, 1, 2


def context_sequence(shape):
    """A7, A8, a 3-letter subset, A7 again (other sequences than the first): what a context sees
    in this order; a charmap[], nprof or present[] left from the launch before shows here."""
    n1, n2 = shape
    rng = np.random.default_rng(n1 + n2)
    s1 = rng.choice(SUB3, n1)
    s1[:3] = SUB3
    sub = (s1, mutated_window(rng, s1, n2, A7))
    return [("A7", *pair(7, n1, n2, 1)), ("A8", *pair(8, n1, n2, 2)), ("SUB3", *sub), ("A7 again", *pair(7, n1, n2, 3))]


# ------------------------------------------------------------------ the matrix of item 11
@functools.lru_cache(maxsize=None)
def matrix7():
    """Seeded, asymmetric, entries -8..12 over the A7 bytes; every other byte (OUT) scores as 7F."""
    m = random_matrix(np.random.default_rng(507), 7, letters=u8(A7).tolist(), other=0x7F)
    assert (m.scores != m.scores.T).any()
    return m


# ------------------------------------------------------------------ references, computed once
@functools.lru_cache(maxsize=None)
def nw_table(nd, shape, scheme):
    t = oracle.fill(*case(nd, shape), scheme)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def nw_ops(nd, shape, scheme):
    ops = walk(*case(nd, shape), nw_table(nd, shape, scheme), scheme)
    ops.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=None)
def sw_table(nd, shape, scheme):
    t = oracle.sw_fill(*case(nd, shape), scheme)
    t.setflags(write=False)
    return t


# ================================================================== tests
def test_alphabets_are_what_they_say():
    for nd, a in ALPHABETS.items():
        assert a.dtype == np.int8 and a.size == nd and (np.diff(u8(a).astype(int)) > 0).all()
        assert not np.isin(u8(OUT), u8(a)).any()
    assert not np.isin(u8(S2_ONLY), u8(A7)).any()
    assert set(u8(A8)) == set(u8(A7)) | {0x41} and set(u8(A4)) < set(u8(A5)) < set(u8(A7))
    # both ends of the signed and of the unsigned order, so a signed sort or compare shows
    for a in ALPHABETS.values():
        assert {0x00, 0x7F, 0x80, 0xFF} <= set(u8(a)) and a.min() == -128 and a.max() == 127
    assert not np.isin(u8(S2_ONLY), u8(OUT)).any() and set(u8(SUB3)) < set(u8(A7))
    # letters of index >= 4 exist from 5 letters on, and A8's index 7 is FF
    assert [int(charmap_of(ALPHABETS[nd])[0xFF]) for nd in NDS] == [3, 4, 6, 7]
    assert charmap_of(SUB3)[u8(SUB3)].tolist() == [0, 1, 2] and charmap_of(A7)[u8(SUB3)].tolist() == [1, 4, 6]


def test_seq_and_csr_keep_every_byte():
    every = np.arange(256, dtype=np.uint8).view(np.int8)
    np.testing.assert_array_equal(nwhip._seq(every), every)
    np.testing.assert_array_equal(u8(nwhip._seq(bytes(range(256)))), np.arange(256))
    np.testing.assert_array_equal(nwhip._seq(u8(A8)), A8)  # a uint8 array wraps to the same bytes
    s1, off1, s2, off2 = nwhip.batch_csr(batch(8))
    np.testing.assert_array_equal(s1, np.concatenate([a for a, _ in batch(8)]))
    np.testing.assert_array_equal(s2, np.concatenate([b for _, b in batch(8)]))
    assert s1.dtype == s2.dtype == np.int8 and off1.tolist() == [0, 300, 557, 562, 563]


def test_no_entry_refuses_a_byte():
    """Every wrapper the device module calls takes all these bytes: valid arguments reach the
    device (or its absence), none is refused by contract."""
    a, b = case(8, (5, 130))
    b = np.concatenate([b, OUT, S2_ONLY, A8])
    pairs, mat = [(a, b), (A7, OUT)], matrix7()
    calls = [lambda: nwhip.fill(a, b, GENERIC), lambda: nwhip.fill(a, b, GENERIC, kernel=nwhip.KERNEL_PANELS),
             lambda: nwhip.score_sweep(a, b, GENERIC), lambda: nwhip.align(a, b, GENERIC),
             lambda: nwhip.sw_align(a, b, GENERIC), lambda: nwhip.align_ckpt(a, b, GENERIC, block_rows=64),
             lambda: nwhip.score_batch(pairs, GENERIC), lambda: nwhip.align_batch(pairs, GENERIC),
             lambda: nwhip.score_batch_affine(pairs, GENERIC, -3), lambda: nwhip.align_batch_affine(pairs, GENERIC, -3),
             lambda: nwhip.score_batch_matrix(pairs, mat, -1, -3), lambda: nwhip.align_batch_matrix(pairs, mat, -1, -3),
             lambda: nwhip.score_batch_local(pairs, mat, -1, -3), lambda: nwhip.align_batch_local(pairs, mat, -1, -3)]
    for f in calls:
        assert status_of(f) in VALID
    # the matrix routes every unlisted byte to 7F's letter and keeps the listed ones apart
    assert mat.index[u8(A7)].tolist() == list(range(7)) and (mat.index[u8(OUT)] == 2).all()
    assert mat.index[0x41] == mat.index[0x61] == 2


@pytest.mark.parametrize("scheme", SCHEMES + [DEEP])
def test_ops_score_counts_these_bytes_as_the_walk_does(scheme):
    """nw_ops_score and nw_ops_score_affine run on the host: the checkers' direct sums."""
    a, b = case(7, (5, 130))
    a, b = np.concatenate([a, A7]), b[:40]
    ops = walk(a, b, None, scheme)
    assert nwhip.ops_score(a, b, ops, scheme) == path_score(a, b, ops, scheme) == oracle.score(a, b, scheme)
    ops = nw_gotoh.walk(a, b, scheme, -3)
    assert nwhip.ops_score_affine(a, b, ops, scheme, -3) == nw_gotoh.path_score_affine(a, b, ops, scheme, -3) \
        == nw_gotoh.score(a, b, scheme, -3)


def test_the_minus_one_byte_decides():
    """Condition 3.  mismatch - 2 gap is the table byte a foreign row letter must read; 0xFF is
    what it would read without the min(.., 7).  (The SW panels' bytes are s - gap.)"""
    for m, mm, g in SCHEMES + [DEEP]:
        assert mm - 2 * g != -1 and -128 <= mm - 2 * g <= 127 and -128 <= m - 2 * g <= 127
    for m, mm, g in SW_SCHEMES:
        assert mm - 2 * g != -1 and mm - g != -1
    assert DEEP[1] - 2 * DEEP[2] == -128


def _linear(a, b, s, ops):
    t = oracle.fill(a, b, s)
    return (int(t[-1, -1]), walk(a, b, t, s).tobytes()) if ops else int(t[-1, -1])


def _affine(a, b, s, go, ops):
    tables = nw_gotoh.fill(a, b, s, go)
    return (int(tables[0][-1, -1]), nw_gotoh.walk(a, b, s, go, tables).tobytes()) if ops else int(tables[0][-1, -1])


def _scorers(shape):
    """What the entries run on a pair of this size compute, as (name, function of (s1, s2)): the
    score.  With five columns against 130 rows every column finds its letter whatever s2 holds
    more of, so a score cannot rise with more matching rows: for the thin pair the walked ops
    are part of what must change (they are what align_batch returns for it)."""
    thin = shape == THIN
    out = [(f"nw {s}", functools.partial(_linear, s=s, ops=thin)) for s in SCHEMES + [DEEP]]
    if shape in (STRIP, PANEL, TB):
        out += [(f"sw {s}", lambda a, b, s=s: oracle.sw_best(a, b, s)[0]) for s in SW_SCHEMES]
    if shape in BATCH_SIZES:
        out += [(f"affine {s} {go}", functools.partial(_affine, s=s, go=go, ops=thin)) for s, go in AFFINE]
    return out


ALL_CASES = [(nd, sh) for nd in NDS for sh in [STRIP, PANEL, CKPT, TB] + BATCH_SIZES[1:]]


@pytest.mark.parametrize("nd,shape", ALL_CASES)
def test_high_table_and_selector_7_decide(nd, shape):
    """Conditions 1 and 2 for every generated pair under everything it is used with.  A 1 x 1
    pair has one row letter: it is the s1 letter (the alphabet's last, of the high table from 5
    letters on) and condition 2 has nothing to replace."""
    s1, s2 = case(nd, shape)
    alpha = ALPHABETS[nd]
    assert set(u8(s1)) <= set(u8(alpha)) and (shape[0] < nd or set(u8(s1)) == set(u8(alpha)))
    assert (charmap_of(s1)[u8(s1)].max() == nd - 1) == (shape[0] >= nd)
    foreign = np.isin(u8(s2), u8(OUT))
    if shape == (1, 1):
        assert s2[0] == s1[0] == alpha[-1]
    else:
        assert 0.1 < foreign.mean() < 0.3 and set(u8(s2)[~foreign]) <= set(u8(alpha))
        if nd > 4 and shape[0] >= 65:
            assert 0.5 < np.isin(u8(s1), u8(alpha[4:])).mean() < 0.7
    for name, f in _scorers(shape):
        true = f(s1, s2)
        if nd >= 5:
            assert f(s1, high_dead(nd, s2)) != true, f"condition 1, {name}"
        if shape != (1, 1):
            assert f(s1, out_collides(nd, s2)) != true, f"condition 2, {name}"


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_batch_wide_decision_cases(name):
    """Condition 4, and conditions 1 and 2 pair by pair: Q matches through high tables only."""
    pairs = decision_case(name)
    idx = [sorted(set(charmap_of(A8 if name == "b" else A7)[u8(a)].tolist())) for a, _ in pairs]
    if name == "b":
        assert idx == [[0, 1, 3], [5, 6, 7], [4, 5], [1, 2, 7]]  # A8's indices: 41 is 2
    else:
        assert idx == [list(LOW), list(HIGH), list(MID)]
    union = np.unique(np.concatenate([u8(a) for a, _ in pairs]))
    assert union.size == (8 if name == "b" else 7) and all(np.unique(u8(a)).size <= 3 for a, _ in pairs)
    assert (union.size <= MAX_PERM) == (name != "b")
    rows = np.unique(np.concatenate([u8(b) for _, b in pairs]))
    if name != "b":
        assert np.isin(u8(S2_ONLY), rows).sum() == (3 if name == "c" else 0)
    assert np.isin(u8(S2_ONLY), union).sum() == (1 if name == "b" else 0)
    for k, (a, b) in enumerate(pairs[:3]):
        assert np.isin(u8(b), u8(OUT)).any() and np.isin(u8(b), np.setdiff1d(u8(A7), u8(a))).any()
        top = a[np.argmax(u8(a))]  # a selector that lands on a letter of this pair's columns
        for f in [functools.partial(oracle.score, scheme=s) for s in SCHEMES] + \
                 [lambda a, b, s=s, go=go: nw_gotoh.score(a, b, s, go) for s, go in AFFINE]:
            if k:  # Q and R hold letters of index >= 4 of the batch-wide map
                assert f(a, high_dead(7, b)) != f(a, b)
            assert f(a, out_collides(7, b, top)) != f(a, b)


def test_context_sequence_changes_the_map():
    for shape in (STRIP, PANEL, CKPT):
        seq = context_sequence(shape)
        assert [np.unique(u8(a)).size for _, a, _ in seq] == [7, 8, 3, 7]
        # SUB3's letters sit at other indices than under A7, and its s2 holds A7 letters SUB3 lacks
        _, a, b = seq[2]
        assert np.isin(u8(b), np.setdiff1d(u8(A7), u8(SUB3))).any() and np.isin(u8(b), u8(OUT)).any()
        assert not np.array_equal(seq[0][1], seq[3][1])
