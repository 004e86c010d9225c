"""What the first-generation layer functions accept and refuse, on host tensors (the table: tests/layer_call_forms_cases.py; the pattern
of tests/test_layer_operand_shapes.py): a refused call raises ``NotImplementedError`` before any device tensor is asked for, and the same
call with acceptable arguments gets as far as "must live on the GPU".  No device call can happen.

The registry check at the end keeps the table complete: every public function and ``nn.Module`` of hyperspace/gmath.py,
hyperspace/hyrnn_nets.py, hyperspace/poincare_distance.py and hypad_amd/autograd.py is an entry of the table or is named in
``COVERED_ELSEWHERE`` with a test of its own that exists.
"""
import inspect
import os
import re

import numpy
import pytest
import torch

import layer_call_forms_cases as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ENTRIES = {}


def _entry(name):
    if not _ENTRIES:
        _ENTRIES.update({e.name: e for e in cf.entries()})
    return _ENTRIES[name]


def _passes(call):
    from hypad_amd import _C
    with pytest.raises(_C.HypadError, match="must live on the GPU"):
        call()


def test_the_table_is_the_one_named_here():
    es = cf.entries()
    assert [e.name for e in es] == cf.NAMES
    assert [e.name for e in es if e.dim_call] == cf.WITH_DIM
    assert [e.name for e in es if e.k_call] == cf.WITH_K


@pytest.mark.parametrize("name", cf.WITH_DIM)
def test_a_dim_that_is_not_the_last_is_refused_not_ignored(name):
    e = _entry(name)
    for dim in (-1, 2):                                     # the row operand of every dim_call is 3-D
        _passes(lambda: e.dim_call(dim))
    for dim in (0, -2):
        with pytest.raises(NotImplementedError, match="supported:"):
            e.dim_call(dim)


@pytest.mark.parametrize("name", cf.WITH_K)
def test_only_curvature_minus_one_is_taken(name):
    e = _entry(name)
    for k in ([None] if e.k_none else []) + [-1, -1.0, torch.tensor(-1.0), numpy.float32(-1)]:
        _passes(lambda: e.k_call(k))
    for k in (-0.5, 0.0, 1.0):
        with pytest.raises(NotImplementedError):
            e.k_call(k)


def test_mobius_add_broadcasts_leading_dimensions_and_refuses_what_does_not_broadcast():
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    Z = torch.zeros
    for xs, ys in (((2, 4, 8), (4, 8)), ((1, 8), (4, 8)), ((2, 1, 8), (4, 8)), ((4, 8), (8,)), ((8,), (8,))):
        _passes(lambda: gmath.mobius_add(Z(*xs), Z(*ys)))
    for xs, ys in (((2, 4, 8), (3, 8)), ((4, 8), (4, 7)), ((2, 4, 8), (2, 3, 8))):
        with pytest.raises((_C.HypadError, NotImplementedError)) as info:
            gmath.mobius_add(Z(*xs), Z(*ys))
        assert str(xs) in str(info.value) and str(ys) in str(info.value), info.value


def test_poincare_distance_refuses_an_operand_that_requires_grad_before_any_device_tensor():
    from hypad_amd import _C
    from hypad_amd.hyperspace.poincare_distance import poincare_distance
    a, b = torch.zeros(4, 8), torch.zeros(5, 8)
    for pred, gt in ((a.clone().requires_grad_(True), b), (a, b.clone().requires_grad_(True))):
        with pytest.raises(_C.HypadError, match=r"gmath\.dist_matmul"):
            poincare_distance(pred, gt)
        with torch.no_grad():
            _passes(lambda: poincare_distance(pred, gt))
    _passes(lambda: poincare_distance(a, b))
    with pytest.raises(_C.HypadError, match=r"\(4, 8\).*\(5, 7\)"):
        poincare_distance(a, torch.zeros(5, 7))


# ------------------------------------------------------------------------------------------------ the registry
def _public():
    """{"gmath.expmap0": object, ...}: the functions and nn.Modules defined in the four files, by their public names."""
    from hypad_amd import autograd
    from hypad_amd.hyperspace import gmath, hyrnn_nets, poincare_distance
    out = {}
    for short, mod in (("gmath", gmath), ("hyrnn_nets", hyrnn_nets), ("poincare_distance", poincare_distance), ("autograd", autograd)):
        for name, obj in vars(mod).items():
            own = getattr(obj, "__module__", None) == mod.__name__
            if not name.startswith("_") and own and (inspect.isfunction(obj) or (inspect.isclass(obj) and issubclass(obj, torch.nn.Module))):
                out[f"{short}.{name}"] = obj
    return out


def test_every_public_function_is_in_the_table_or_covered_elsewhere():
    public = _public()
    assert {"gmath.expmap0", "hyrnn_nets.MobiusLinear", "poincare_distance.poincare_distance", "autograd.lstm_seq"} <= set(public)
    in_table = {c for e in cf.entries() for c in e.covers}
    assert in_table <= set(public), sorted(in_table - set(public))
    assert not in_table & set(cf.COVERED_ELSEWHERE), sorted(in_table & set(cf.COVERED_ELSEWHERE))
    missing = sorted(set(public) - in_table - set(cf.COVERED_ELSEWHERE))
    assert not missing, (f"{missing}: neither an entry of tests/layer_call_forms_cases.py nor a key of COVERED_ELSEWHERE -- a public layer "
                         "function ships with its calling forms tested")
    stale = sorted(set(cf.COVERED_ELSEWHERE) - set(public))
    assert not stale, f"COVERED_ELSEWHERE names {stale}, which the package does not define"


def test_every_test_named_in_covered_elsewhere_exists():
    texts = {}
    for name, where in cf.COVERED_ELSEWHERE.items():
        m = re.fullmatch(r"(tests/\w+\.py)::(test_\w+)", where)
        assert m, (name, where)
        path = os.path.join(ROOT, m.group(1))
        assert os.path.isfile(path), f"{name}: {m.group(1)} does not exist"
        if path not in texts:
            with open(path) as f:
                texts[path] = f.read()
        assert re.search(rf"^def {m.group(2)}\(", texts[path], re.M), f"{name}: {m.group(1)} has no {m.group(2)}"
