"""GPU: every kernel family that builds v_perm score tables, over alphabets of 4, 5, 7 and 8
letters at both ends of the byte range (tests/test_alphabet_range_host.py: the alphabets, the
generator, the batch cases and the conditions that make a wrong table visible).

The strip fill (NW and SW kinds), the panel fill (NW and SW), the checkpointed sweep, the
linear and the affine batch each build their own tables; every other test of them draws
from the bytes 1..4, where index 3 is the highest that ever matches, or from 9 letters and
more, which run on compares.  Here indices 4..6 (the high table) carry most of the matches,
a fifth of every s2 is bytes no column holds (selector 7), the eighth letter tips the
launch -- or the whole batch -- to compares, and one context sees the alphabets change.
Every comparison is exact: oracle.fill / oracle.score / oracle.sw_*, tests/nw_walk.py,
tests/nw_gotoh.py, tests/nw_gotoh_matrix.py, tests/nw_local.py.
"""
import numpy as np
import pytest

import nw_gotoh
import nw_gotoh_matrix as gm
import nwhip
import oracle
import test_batch as tb
import test_batch_affine as tba
import test_batch_local as tbl
import test_batch_matrix as tbm
import test_ckpt as tc
from test_alphabet_range_host import (AFFINE, CKPT, DEEP, NDS, PANEL, SCHEMES, STRIP, SW_SCHEMES, TB, batch, case,
                                      context_sequence, decision_case, matrix7, nw_ops, nw_table, sw_table)
from test_gpu_parity import STRIP_SHAPES
from test_panels import PANEL_SHAPES
from test_scheme_range import same_ops
from test_sw import SW_SHAPES

pytestmark = pytest.mark.gpu

FORMS = [0, nwhip.FLAG_NO_PROFILE]  # tables (compares from 8 letters on); compares
NW_SCHEMES = SCHEMES + [DEEP]
S, P = nwhip.KERNEL_STRIPS, nwhip.KERNEL_PANELS


@pytest.fixture(scope="module")
def torch():
    import torch as _t
    if not _t.cuda.is_available():
        pytest.skip("no GPU")
    return _t


@pytest.fixture(scope="module")
def ctx(torch):
    c = nwhip.Context(0)
    yield c
    c.close()


def check_sw(torch, ctx, s1, s2, want, scheme, shape, kernel, flags):
    """Table, best cell and the traceback from it, as test_sw_table_and_best_vs_oracle."""
    n1, n2 = s1.size, s2.size
    d1, d2 = tc.dev(torch, s1), tc.dev(torch, s2)
    tab = nwhip.Context.alloc_table(n1, n2)
    r = ctx.fill(d1, d2, tab, scheme, substrips=shape[0], strip_waves=shape[1], mode=nwhip.MODE_SW, kernel=kernel,
                 flags=flags)
    what = str((scheme, shape, flags))
    assert r.status == 0 and (r.substrips, r.strip_waves, r.kernel) == (shape[0], shape[1], kernel)
    np.testing.assert_array_equal(tab[:n2 + 1, :n1 + 1].cpu().numpy(), want, err_msg=what)
    assert (r.score, r.end_i, r.end_j) == oracle.sw_best(s1, s2, scheme), what
    al, ops = ctx.sw_traceback(d1, d2, tab, (r.end_i, r.end_j), scheme)
    wops, bi, bj = oracle.sw_traceback(s1, s2, want, (r.end_i, r.end_j), scheme)
    np.testing.assert_array_equal(ops, wops, err_msg=what)
    assert (al.begin_i, al.begin_j, al.score) == (bi, bj, r.score)


# ------------------------------------------------------------------ 1. strip fill, NW kinds
@pytest.mark.parametrize("strip", STRIP_SHAPES)
@pytest.mark.parametrize("nd", NDS)
def test_strip_fill_nw(nd, strip):
    """600 x 200: three strips of 256 columns (ten of 64) and four row blocks."""
    s1, s2 = case(nd, STRIP)
    for scheme in NW_SCHEMES:
        for flags in FORMS:
            t, r = nwhip.fill(s1, s2, scheme, substrips=strip[0], strip_waves=strip[1], flags=flags, kernel=S)
            assert (r.substrips, r.strip_waves, r.kernel) == (strip[0], strip[1], S)
            np.testing.assert_array_equal(t, nw_table(nd, STRIP, scheme), err_msg=str((scheme, strip, flags)))


# ------------------------------------------------------------------ 2. strip fill, SW kind
@pytest.mark.parametrize("strip", SW_SHAPES)
@pytest.mark.parametrize("nd", NDS)
def test_strip_fill_sw(torch, ctx, nd, strip):
    """600 x 200: two strips at (2, 4), 512 columns."""
    s1, s2 = case(nd, STRIP)
    for scheme in SW_SCHEMES:
        for flags in FORMS:
            check_sw(torch, ctx, s1, s2, sw_table(nd, STRIP, scheme), scheme, strip, S, flags)


# ------------------------------------------------------------------ 3. panel fill, NW and SW
@pytest.mark.parametrize("panel", PANEL_SHAPES)
@pytest.mark.parametrize("nd", NDS)
def test_panel_fill_nw(nd, panel):
    """1100 x 130: two panels at (4, 4), 1024 columns; the prefix tables ttlo / tthi."""
    s1, s2 = case(nd, PANEL)
    for scheme in NW_SCHEMES:
        for flags in FORMS:
            t, r = nwhip.fill(s1, s2, scheme, substrips=panel[0], strip_waves=panel[1], flags=flags, kernel=P)
            assert (r.substrips, r.strip_waves, r.kernel) == (panel[0], panel[1], P)
            np.testing.assert_array_equal(t, nw_table(nd, PANEL, scheme), err_msg=str((scheme, panel, flags)))


@pytest.mark.parametrize("panel", PANEL_SHAPES)
@pytest.mark.parametrize("nd", NDS)
def test_panel_fill_sw(torch, ctx, nd, panel):
    """The SW panels' table bytes are s - gap: (1, -130, -1) leaves int8 there and runs on compares."""
    s1, s2 = case(nd, PANEL)
    for scheme in SW_SCHEMES:
        for flags in FORMS:
            check_sw(torch, ctx, s1, s2, sw_table(nd, PANEL, scheme), scheme, panel, P, flags)


# ------------------------------------------------------------------ 4. checkpointed sweep
@pytest.mark.parametrize("nd", NDS)
def test_checkpointed(torch, ctx, nd):
    """300 x 150 with K = 64: the sweep's rows 64 and 128, nw_score, and nw_align_ckpt over
    three blocks."""
    s1, s2 = case(nd, CKPT)
    for scheme in NW_SCHEMES:
        t, want = nw_table(nd, CKPT, scheme), nw_ops(nd, CKPT, scheme)
        for flags in FORMS:
            tc.check_sweep(torch, ctx, s1, s2, t, 64, scheme, flags=flags)
            assert nwhip.score_sweep(s1, s2, scheme, flags=flags).score == t[-1, -1]
            stats = tc.check_align(s1, s2, scheme, want, int(t[-1, -1]), 64, flags=flags)
            assert stats.blocks == 3


# ------------------------------------------------------------------ 5. linear batch
_WANT = {}  # the checkers' scores, once per (batch, cost); the batches are the host module's cached tuples


def linear_want(pairs, scheme):
    key = (id(pairs), scheme)
    if key not in _WANT:
        _WANT[key] = (pairs, [oracle.score(a, b, scheme) for a, b in pairs])
    return _WANT[key][1]


def check_linear(pairs, schemes=NW_SCHEMES):
    for scheme in schemes:
        want = linear_want(pairs, scheme)
        for waves in (0, 1):
            for flags in FORMS:
                what = str((scheme, waves, flags))
                assert nwhip.score_batch(pairs, scheme, waves=waves, flags=flags).tolist() == want, what
            sc, ops, st = nwhip.align_batch(pairs, scheme, waves=waves)
            assert waves == 0 or st.waves == 1
            if waves == 0:
                tb.check_alignments(pairs, scheme, sc, ops)
                sc0, ops0 = sc, ops
            else:
                assert sc.tolist() == sc0.tolist()
                same_ops(ops, ops0)
        sc, ops, _ = nwhip.align_batch(pairs, scheme, flags=nwhip.FLAG_NO_PROFILE)
        assert sc.tolist() == want
        same_ops(ops, ops0)


@pytest.mark.parametrize("nd", NDS)
def test_linear_batch(nd):
    """300 x 150, 257 x 65, 5 x 130 and 1 x 1 of one alphabet; one worker takes them in turn."""
    check_linear(batch(nd))


# ------------------------------------------------------------------ 6. affine batch
def affine_want(pairs, scheme, go):
    key = (id(pairs), scheme, go)
    if key not in _WANT:
        _WANT[key] = (pairs, [nw_gotoh.score(a, b, scheme, go) for a, b in pairs])
    return _WANT[key][1]


def check_affine(pairs, costs=AFFINE):
    for scheme, go in costs:
        want = affine_want(pairs, scheme, go)
        for waves in (0, 1):
            for flags in FORMS:
                got = nwhip.score_batch_affine(pairs, scheme, go, waves=waves, flags=flags)
                assert got.tolist() == want, str((scheme, go, waves, flags))
            sc, ops, _ = nwhip.align_batch_affine(pairs, scheme, go, waves=waves)
            if waves == 0:
                tba.check_alignments(pairs, scheme, go, sc, ops)
                sc0, ops0 = sc, ops
            else:
                assert sc.tolist() == sc0.tolist()
                same_ops(ops, ops0)
        sc, ops, _ = nwhip.align_batch_affine(pairs, scheme, go, flags=nwhip.FLAG_NO_PROFILE)
        assert sc.tolist() == want
        same_ops(ops, ops0)


@pytest.mark.parametrize("nd", NDS)
def test_affine_batch(nd):
    check_affine(batch(nd))


# ------------------------------------------------------------------ 7. the batch-wide decision
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_batch_wide_decision_linear(name):
    """No pair's s1 holds more than three letters, the batch's s1 sides hold seven (a, c: tables
    over the batch-wide map, Q's matches all from high tables) or eight (b: compares)."""
    check_linear(decision_case(name))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_batch_wide_decision_affine(name):
    check_affine(decision_case(name))


# ------------------------------------------------------------------ 8. async device entries
def device_batch(torch, pairs):
    d = [tc.dev(torch, x) for x in nwhip.batch_csr(pairs)]
    return d, max(b.size for _, b in pairs)


def test_context_score_batch_on_a_stream(torch, ctx):
    pairs = batch(7)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d, max_n2 = device_batch(torch, pairs)
        got = [ctx.score_batch(*d, max_n2, s, stream=stream) for s in SCHEMES]
        got += [ctx.score_batch_affine(*d, max_n2, s, go, stream=stream) for s, go in AFFINE]
    stream.synchronize()
    assert ctx.status(stream) == nwhip.NW_OK
    want = [linear_want(pairs, s) for s in SCHEMES] + [affine_want(pairs, s, go) for s, go in AFFINE]
    for g, w in zip(got, want):
        assert g.cpu().numpy().tolist() == w


# ------------------------------------------------------------------ 9. one context, changing alphabets
@pytest.mark.parametrize("entry", ["strips", "panels", "ckpt_sweep", "score_batch"])
def test_one_context_changing_alphabets(torch, entry):
    """A7, A8, three letters of A7, A7 again on one context: every launch builds charmap[], nprof
    and present[] anew."""
    c = nwhip.Context(0)
    scheme = (2, -1, -2)
    try:
        for name, s1, s2 in context_sequence({"strips": STRIP, "panels": PANEL}.get(entry, CKPT)):
            d1, d2 = tc.dev(torch, s1), tc.dev(torch, s2)
            want = oracle.fill(s1, s2, scheme)
            if entry in ("strips", "panels"):
                tab = nwhip.Context.alloc_table(s1.size, s2.size)
                r = c.fill(d1, d2, tab, scheme, kernel=S if entry == "strips" else P)
                assert r.status == 0 and r.score == want[-1, -1], name
                np.testing.assert_array_equal(tab[:s2.size + 1, :s1.size + 1].cpu().numpy(), want, err_msg=name)
            elif entry == "ckpt_sweep":
                tc.check_sweep(torch, c, s1, s2, want, 64, scheme)
            else:
                pairs = [(s1, s2), (s1[:70], s2[:40])]
                d, max_n2 = device_batch(torch, pairs)
                got = c.score_batch(*d, max_n2, scheme)
                torch.cuda.synchronize()
                assert c.status() == nwhip.NW_OK
                assert got.cpu().numpy().tolist() == [int(want[-1, -1]), oracle.score(*pairs[1], scheme)], name
    finally:
        c.close()


# ------------------------------------------------------------------ 10. tracebacks over high bytes
@pytest.mark.parametrize("nd", [7, 8])
def test_global_traceback(nd):
    s1, s2 = case(nd, TB)
    for scheme in NW_SCHEMES:
        t, want = nw_table(nd, TB, scheme), nw_ops(nd, TB, scheme)
        al, ops, _ = nwhip.align(s1, s2, scheme)
        np.testing.assert_array_equal(ops, want, err_msg=str(scheme))
        assert al.score == t[-1, -1] == nwhip.ops_score(s1, s2, ops, scheme)
        assert (al.begin_i, al.begin_j, al.end_i, al.end_j, al.n_ops) == (0, 0, s2.size, s1.size, want.size)


@pytest.mark.parametrize("nd", [7, 8])
def test_local_traceback(nd):
    s1, s2 = case(nd, TB)
    for scheme in SW_SCHEMES:
        t = sw_table(nd, TB, scheme)
        best = oracle.sw_best(s1, s2, scheme)
        want, bi, bj = oracle.sw_traceback(s1, s2, t, best[1:], scheme)
        al, ops = nwhip.sw_align(s1, s2, scheme)
        np.testing.assert_array_equal(ops, want, err_msg=str(scheme))
        assert (al.score, al.end_i, al.end_j) == best and (al.begin_i, al.begin_j, al.n_ops) == (bi, bj, want.size)
        assert nwhip.ops_score(s1, s2, ops, scheme, begin=(bi, bj)) == best[0] > 0


# ------------------------------------------------------------------ 11. matrix and local batch
@pytest.mark.parametrize("ge,go", [(-1, -11), (-2, -3)])
@pytest.mark.parametrize("nd", [7, 8])
def test_matrix_and_local_batch(nd, ge, go):
    """index[256] in the place of the charmap: the A7 bytes as letters, everything else (OUT,
    and 41 of A8) scored as 7F."""
    pairs, mat = batch(nd), matrix7()
    want = [gm.score(a, b, mat.scores, mat.index, ge, go) for a, b in pairs]
    hits = np.array([tbl.want_hit(a, b, mat.scores, mat.index, ge, go) for a, b in pairs])
    for waves in (0, 1):
        assert nwhip.score_batch_matrix(pairs, mat, ge, go, waves=waves).tolist() == want
        np.testing.assert_array_equal(tbl.hit_rows(nwhip.score_batch_local(pairs, mat, ge, go, waves=waves)), hits)
        sc, ops, _ = nwhip.align_batch_matrix(pairs, mat, ge, go, waves=waves)
        tbm.check_alignments(pairs, mat, ge, go, sc, ops)
        lh, lops, _ = nwhip.align_batch_local(pairs, mat, ge, go, waves=waves)
        tbl.check_alignments(pairs, mat, ge, go, lh, lops)
