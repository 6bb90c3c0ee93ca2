"""CPU: the Python wrappers of the batch entries (nwhip.score_batch* / align_batch* and the
Context.score_batch* methods) share their bodies; this pins what a caller sees of each.  The
parameter names and defaults against a literal table; for every module wrapper, that a cost its
C entry refuses before it looks for a device comes back as an NwError naming that wrapper's own
entry with NW_ERR_ARG -- once per argument the wrapper passes between the params and the results,
each time with every other argument valid, so that a wrapper on another entry or with its
arguments in another order shows; and for the Context methods that take a matrix, the ValueError
of a matrix without other=, which they raise before they touch the context.  No device is used.
"""
import inspect

import numpy as np
import pytest

import nwhip

_S = ("scheme", (1, 0, -1))
_TAIL_SCORE = [("waves", 0), ("device", -1), ("return_stats", False)]
_TAIL_ALIGN = [("mem_bytes", 0), ("waves", 0), ("device", -1)]
_MAT = [("pairs",), ("mat",), ("gap", -1), ("gap_open", 0)]
_DUAL = [("pairs",), ("mat",), ("gap", -2), ("gap_open", -4), ("gap2", -1), ("gap_open2", -24)]

MODULE = {
    "score_batch": [("pairs",), _S, ("waves", 0), ("device", -1), ("flags", 0), ("return_stats", False)],
    "align_batch": [("pairs",), _S, ("mem_bytes", 0), ("waves", 0), ("device", -1), ("flags", 0)],
    "score_batch_affine": [("pairs",), _S, ("gap_open", 0), ("waves", 0), ("device", -1), ("flags", 0),
                           ("return_stats", False)],
    "align_batch_affine": [("pairs",), _S, ("gap_open", 0), ("mem_bytes", 0), ("waves", 0), ("device", -1),
                           ("flags", 0)],
    "score_batch_matrix": _MAT + _TAIL_SCORE,
    "align_batch_matrix": _MAT + _TAIL_ALIGN,
    "score_batch_local": _MAT + _TAIL_SCORE,
    "align_batch_local": _MAT + _TAIL_ALIGN,
    "score_batch_semi": _MAT + [("ends", 3)] + _TAIL_SCORE,
    "align_batch_semi": _MAT + [("ends", 3)] + _TAIL_ALIGN,
    "score_batch_banded": _MAT + [("band", 0)] + _TAIL_SCORE,
    "align_batch_banded": _MAT + [("band", 0)] + _TAIL_ALIGN,
    "score_batch_dual": _DUAL + _TAIL_SCORE,
    "align_batch_dual": _DUAL + _TAIL_ALIGN,
    "score_batch_dual_banded": _DUAL + [("band", 0)] + _TAIL_SCORE,
    "align_batch_dual_banded": _DUAL + [("band", 0)] + _TAIL_ALIGN,
}

_DEV = [("self",), ("d_s1cat",), ("d_off1",), ("d_s2cat",), ("d_off2",), ("max_n2",)]
_DEV_TAIL = [("stream", None), ("waves", 0)]
_DEV_MAT = _DEV + [("mat",), ("gap", -1), ("gap_open", 0)]
_DEV_DUAL = _DEV + [("mat",), ("gap", -2), ("gap_open", -4), ("gap2", -1), ("gap_open2", -24)]

CONTEXT = {
    "score_batch": _DEV + [_S, ("stream", None), ("waves", 0), ("flags", 0), ("gap_open", None), ("mat", None),
                           ("band", None), ("piece2", None)],
    "score_batch_affine": _DEV + [_S, ("gap_open", 0), ("stream", None), ("waves", 0), ("flags", 0)],
    "score_batch_matrix": _DEV_MAT + _DEV_TAIL,
    "score_batch_banded": _DEV_MAT + [("band", 0)] + _DEV_TAIL,
    "score_batch_dual": _DEV_DUAL + _DEV_TAIL,
    "score_batch_dual_banded": _DEV_DUAL + [("band", 0)] + _DEV_TAIL,
    "score_batch_local": _DEV_MAT + _DEV_TAIL,
    "score_batch_semi": _DEV_MAT + [("ends", 3)] + _DEV_TAIL,
}


def _signature(f):
    return [(p.name,) if p.default is inspect.Parameter.empty else (p.name, p.default)
            for p in inspect.signature(f).parameters.values()]


def test_the_tables_name_every_wrapper():
    assert nwhip.ENDS_S2_IN_S1 == 3
    kinds = ["", "_affine", "_matrix", "_local", "_semi", "_banded", "_dual", "_dual_banded"]
    assert sorted(MODULE) == sorted(w + k for w in ("score_batch", "align_batch") for k in kinds)
    assert sorted(CONTEXT) == sorted(n for n in vars(nwhip.Context) if n.startswith("score_batch"))


@pytest.mark.parametrize("name", sorted(MODULE))
def test_module_wrapper_signature(name):
    assert _signature(getattr(nwhip, name)) == MODULE[name]


@pytest.mark.parametrize("name", sorted(CONTEXT))
def test_context_method_signature(name):
    assert _signature(getattr(nwhip.Context, name)) == CONTEXT[name]


# One refused value per argument a wrapper hands its entry besides the params' own fields: a gap
# cost of a run must not be positive, `ends` has four bits, a band is not negative.
REFUSED = {"gap_open": 1, "gap_open2": 1, "ends": 16, "band": -1}
PAIRS = [(np.array([1, 2, 3, 4, 1], np.int8), np.array([2, 3, 1], np.int8))]


def _refusals(name):
    args = [a[0] for a in MODULE[name]]
    if "mat" not in args and "gap_open" not in args:
        return [{"scheme": (1, 0, -(1 << 20))}]   # the linear entries: a gap beyond the range bound
    return [{a: REFUSED[a]} for a in args if a in REFUSED]


@pytest.mark.parametrize("name", sorted(MODULE))
def test_module_wrapper_reports_its_own_entry(name):
    mat = nwhip.SubMatrix([1, 2, 3, 4], 3 * np.eye(4, dtype=np.int64) - 1)
    lead = (PAIRS, mat) if "mat" in [a[0] for a in MODULE[name]] else (PAIRS,)
    cases = _refusals(name)
    assert cases
    for kw in cases:
        with pytest.raises(nwhip.NwError) as e:
            getattr(nwhip, name)(*lead, **kw)
        assert e.value.status == nwhip.NW_ERR_ARG, (name, kw)
        assert str(e.value).startswith("libnwhip nw_%s: " % name), (name, kw, str(e.value))


@pytest.mark.parametrize("name", sorted(n for n in CONTEXT if ("mat",) in CONTEXT[n]))
def test_context_method_needs_a_matrix_with_other(name):
    mat = nwhip.SubMatrix([1, 2, 3, 4], np.eye(4, dtype=np.int64))
    assert mat.other is None and not mat.listed.all()
    with pytest.raises(ValueError) as e:
        getattr(nwhip.Context, name)(None, None, None, None, None, 8, mat)
    assert str(e.value) == "Context.%s needs a matrix with other= (it cannot check the sequences)" % name
