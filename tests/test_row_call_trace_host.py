"""The ctypes calls behind the row functions of ``gmath`` and the methods of ``PoincareBall``, on the host: which entry point is called,
with which sizes, flags and curvature, and which of its pointers are NULL -- compared with a recorded trace
(tests/golden/row_call_trace.json).  The autograd functions of hyperspace/gmath.py decide nothing else about a call, so a change that only
moves them about leaves the trace as it is.

``_C.lib`` is replaced by a recorder: the ``*_workspace_bytes`` functions go through to the library, every other entry point is written
down and answers 0.  ``_C.require_cuda`` lets host tensors through and ``_C.stream`` gives the NULL stream, so no call needs a device.
A record is the entry's name, then its arguments in order: a number as it is, a pointer as "ptr" or "NULL".

Every function runs forward and then ``backward`` of its summed result on fp32 operands of shape (7, 5) (the hyperboloid side: (7, 6))
that all require grad; then t and r as a number, as one element and per row; expmap, dist and lambda_x over no rows; and each function of
several operands with only its first operand requiring grad, which pins the NULL pattern of the gradients.

``python tests/test_row_call_trace_host.py --write`` records the trace anew.
"""
import ctypes
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "row_call_trace.json")
ROWS, D = 7, 5
# function: its row operands, "p" a point or tangent (ROWS, D), "h" a hyperboloid point (ROWS, D + 1)
GMATH_AND_BALL = {
    "expmap": "pp", "logmap": "pp", "gyration": "ppp", "parallel_transport": "ppp", "parallel_transport0": "pp", "parallel_transport0back": "pp",
    "mobius_sub": "pp", "mobius_coadd": "pp", "mobius_cosub": "pp", "egrad2rgrad": "pp", "lambda_x": "p", "inner": "ppp", "norm": "pp",
    "dist": "pp", "dist0": "p", "sproj": "h", "inv_sproj": "p",
}
BALL_ONLY = {"project": "p", "expmap0": "p", "logmap0": "p", "mobius_add": "pp", "mobius_pointwise_mul": "pp"}
TIMED = {"geodesic": "pp", "geodesic_unit": "pp"}                 # t, then the rows
TIMED_BALL_ONLY = {"mobius_scalar_mul": "p"}
NO_ROWS = ("expmap", "dist", "lambda_x")


class Recorder:
    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return getattr(self.real, name)

        def entry(*args):
            self.calls.append([name] + [_written(a) for a in args])
            return 0
        return entry


def _written(a):
    if a is None:
        return "NULL"
    if isinstance(a, ctypes.c_void_p):
        return "ptr" if a.value else "NULL"
    assert isinstance(a, (int, float)), a
    return a


def _leaf(seed, *shape, grad=True):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.1).requires_grad_(grad)


def _operands(kinds, rows=ROWS, only=None):
    """Leaves for the operand kinds; ``only``: the index of the one that requires grad (None: all of them)."""
    return [_leaf(i, rows, D + (k == "h"), grad=only in (None, i)) for i, k in enumerate(kinds)]


def record(setattr_):
    """The trace: [{"case": label, "calls": [[entry, argument, ...], ...]}, ...] in the order of the calls below."""
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    rec = Recorder(_C.lib)
    setattr_(_C, "lib", rec)
    setattr_(_C, "require_cuda", lambda t, *a, **kw: t)
    setattr_(_C, "stream", lambda: None)
    trace = []

    def run(label, fn):
        start = len(rec.calls)
        out = fn()
        if out.requires_grad:
            out.sum().backward()
        trace.append({"case": label, "calls": rec.calls[start:]})

    apis = [("gmath", lambda name: (lambda *a, **kw: getattr(gmath, name)(*a, k=-1.0, **kw)), GMATH_AND_BALL, TIMED)]
    for c in (1.0, 0.5):
        apis.append((f"ball({c:g})", lambda name, _b=PoincareBall(c): getattr(_b, name), {**GMATH_AND_BALL, **BALL_ONLY}, {**TIMED, **TIMED_BALL_ONLY}))
    for api, get, plain, timed in apis:
        for name, kinds in plain.items():
            run(f"{api}.{name}", lambda: get(name)(*_operands(kinds)))
            if len(kinds) > 1:
                run(f"{api}.{name} grad[0]", lambda: get(name)(*_operands(kinds, only=0)))
        for name, kinds in timed.items():
            run(f"{api}.{name} t per row", lambda: get(name)(_leaf(9, ROWS, 1), *_operands(kinds)))
            run(f"{api}.{name} t one element", lambda: get(name)(_leaf(9, 1), *_operands(kinds)))
            run(f"{api}.{name} t a number", lambda: get(name)(0.25, *_operands(kinds)))
            run(f"{api}.{name} grad[t]", lambda: get(name)(_leaf(9, ROWS, 1), *_operands(kinds, only=-1)))
            run(f"{api}.{name} grad[0]", lambda: get(name)(_leaf(9, ROWS, 1, grad=False), *_operands(kinds, only=0)))
        for name in NO_ROWS:
            run(f"{api}.{name} no rows", lambda: get(name)(*_operands(plain[name], rows=0)))
        if api == "gmath":
            continue
        run(f"{api}.antipode", lambda: get("antipode")(_leaf(0, ROWS, D)))
        run(f"{api}.dist_matmul", lambda: get("dist_matmul")(_leaf(0, ROWS, D), _leaf(1, D, ROWS)))
        run(f"{api}.weighted_midpoint", lambda: get("weighted_midpoint")(_leaf(0, ROWS, D), _leaf(1, ROWS)))
        run(f"{api}.weighted_midpoint_bmm", lambda: get("weighted_midpoint_bmm")(_leaf(0, ROWS, D), _leaf(1, 3, ROWS)))
        run(f"{api}.hyperbolic_attention", lambda: get("hyperbolic_attention")(_leaf(0, 3, D), _leaf(1, ROWS, D), _leaf(2, ROWS, D), beta=0.5))
    return trace


def test_the_calls_are_the_recorded_ones(monkeypatch):
    trace = record(monkeypatch.setattr)
    with open(FIXTURE) as f:
        want = json.load(f)
    assert [t["case"] for t in trace] == [t["case"] for t in want]
    for got, exp in zip(trace, want):
        assert got["calls"] == exp["calls"], got["case"]


def test_the_trace_holds_the_cases_it_names():
    with open(FIXTURE) as f:
        want = {t["case"]: t["calls"] for t in json.load(f)}
    entries = {c[0] for calls in want.values() for c in calls}
    for name in list(GMATH_AND_BALL) + list(TIMED):
        assert {f"hypad_{name}_fwd", f"hypad_{name}_bwd", f"hypad_ball_{name}_fwd", f"hypad_ball_{name}_bwd"} <= entries, name
    for name in list(BALL_ONLY) + list(TIMED_BALL_ONLY):
        assert {f"hypad_ball_{name}_fwd", f"hypad_ball_{name}_bwd"} <= entries, name
    assert want["ball(0.5).antipode"] == [] and "hypad_column_sum" in entries
    # no rows: the pointers are NULL and the entry points are called all the same
    assert want["gmath.dist no rows"][0] == ["hypad_dist_fwd", "NULL", "NULL", "NULL", 0, D, "NULL"]
    assert want["ball(0.5).expmap no rows"][0] == ["hypad_ball_expmap_fwd", "NULL", "NULL", "NULL", 0, D, 0.5, "NULL"]
    # one operand requires grad: the others' gradients are NULL
    assert want["gmath.gyration grad[0]"][1] == ["hypad_gyration_bwd", "ptr", "ptr", "ptr", "ptr", "ptr", "NULL", "NULL", ROWS, D, "NULL"]
    assert want["ball(0.5).geodesic grad[t]"][1] == ["hypad_ball_geodesic_bwd"] + ["ptr"] * 5 + ["NULL", "NULL", ROWS, D, ROWS, 0.5, "NULL"]
    # a t shared by the rows: its per-row gradients are summed by hypad_column_sum
    assert [c[0] for c in want["gmath.geodesic t one element"]] == ["hypad_geodesic_fwd", "hypad_geodesic_bwd", "hypad_column_sum"]
    assert want["ball(0.5).mobius_scalar_mul t one element"][2] == ["hypad_column_sum", "ptr", "ptr", ROWS, 1, "NULL"]
    # the projections take the ball's width
    assert want["gmath.sproj"][0][3:5] == [ROWS, D] and want["ball(0.5).inv_sproj"][0][3:5] == [ROWS, D]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_row_call_trace_host.py --write")
    sys.path.insert(0, ROOT)
    with pytest.MonkeyPatch.context() as mp:
        trace = record(mp.setattr)
    with open(FIXTURE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(t) for t in trace) + "\n]\n")
    print(f"{FIXTURE}: {len(trace)} cases, {sum(len(t['calls']) for t in trace)} calls")
