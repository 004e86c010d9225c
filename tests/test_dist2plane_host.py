"""dist2plane / MobiusDist2Hyperplane on the host: the plain-torch restatement of tests/dist2plane_ref.py against
tests/golden/mobius_dist2plane.npz -- the outputs and gradients of the reference's own ``dist2plane`` at k = -1 in fp32
(tests/golden/gen_mobius_dist2plane.py) -- which it meets in fp64 and in fp32 at 1e-6 (error relative to max(1, max|recorded|), as
sweep_common.rel_err); the C ABI's three new entry points; the refusals of gmath.dist2plane, of the module and of RiemannianAdam,
which raise before anything touches a device; the module's keys, shapes and initial invariants.
"""
import os
import re

import numpy as np
import pytest
import torch

import sweep_common as sc
from dist2plane_ref import dist2plane_ref, layer_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mobius_dist2plane.npz")
FLAGS = [(False, False), (False, True), (True, False), (True, True)]          # (signed, scaled)
NEW_ENTRY_POINTS = ("hypad_dist2plane_workspace_bytes", "hypad_dist2plane_fwd", "hypad_dist2plane_bwd")


def case_name(signed, scaled):
    return f"signed{int(signed)}_scaled{int(scaled)}"


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _meets(what, got, recorded, failures, tol=1e-6):
    err, i = sc.rel_err(got, recorded)
    if not err <= tol:
        failures.append(f"{what}: {err:.3e} > {tol:g} at flat index {i}")


def test_fixture_holds_every_case():
    fx = load_fixture()
    assert fx["x"].shape == (9, 7) and fx["p"].shape == (5, 7) and fx["a"].shape == (5, 7) and fx["scale"].shape == (5,)
    norms = np.linalg.norm(fx["x"].astype(np.float64), axis=1)
    assert (fx["x"][3] == 0).all() and abs(norms[5] - 0.9) < 1e-6 and (fx["x"][7] == fx["p"][2]).all() and norms.max() < 0.91
    assert np.linalg.norm(fx["p"].astype(np.float64), axis=1).max() < 0.9                  # points of the ball, as the layer draws them
    assert np.allclose(np.linalg.norm(fx["a"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    names = [case_name(s, c) for s, c in FLAGS] + ["layer"]
    for n in names:
        for part, shape in (("out", (9, 5)), ("grad_x", (9, 7)), ("grad_p", (5, 7)), ("grad_a", (5, 7))):
            assert fx[f"{n}.{part}"].shape == shape and fx[f"{n}.{part}"].dtype == np.float32 and np.isfinite(fx[f"{n}.{part}"]).all()
    assert fx["layer.grad_scale"].shape == (5,)
    assert len(fx) == 5 + 4 * 5 + 1
    # signed and unsigned differ only in sign; the row on a plane's own point has distance zero to that plane
    assert np.allclose(np.abs(fx["signed1_scaled0.out"]), fx["signed0_scaled0.out"], rtol=0, atol=1e-6)
    assert (fx["signed1_scaled0.out"] < 0).any() and (fx["signed0_scaled0.out"] >= 0).all()
    assert abs(fx["signed1_scaled0.out"][7, 2]) < 1e-6


@pytest.mark.parametrize("signed,scaled", FLAGS)
def test_restatement_meets_the_reference(signed, scaled):
    fx, name, failures = load_fixture(), case_name(signed, scaled), []
    for dt in (torch.float64, torch.float32):
        x, p, a = (torch.from_numpy(fx[k]).to(dt).requires_grad_(True) for k in ("x", "p", "a"))
        out = dist2plane_ref(x, p, a, signed, scaled)
        grads = torch.autograd.grad(out, [x, p, a], torch.from_numpy(fx["grad_output"]).to(dt))
        tag = "fp64" if dt == torch.float64 else "fp32"
        _meets(f"{tag} out", out, fx[f"{name}.out"], failures)
        for part, g in zip(("grad_x", "grad_p", "grad_a"), grads):
            g, rec = g.numpy(), fx[f"{name}.{part}"]
            if not signed:
                # |s| at s = rounding noise: row 7 lies ON plane 2, where the unsigned distance has its kink and the sign of s -- hence
                # of that pair's whole contribution -- is decided by the last bit of whichever arithmetic evaluates it
                g, rec = _without_the_kink(part, g, rec, fx, dt)
            _meets(f"{tag} {part}", g, rec, failures)
    assert not failures, name + ": " + "; ".join(failures)


def _without_the_kink(part, g, rec, fx, dt):
    """The unsigned gradients without what the pair (row 7, plane 2) feeds: row 7 of grad_x, plane 2 of grad_p / grad_a (the fp32
    restatement draws the other sign there and sits 3.8e-3 from the record).  The signed forms and the layer form are compared whole."""
    if part == "grad_x":
        return np.delete(g, 7, axis=0), np.delete(rec, 7, axis=0)
    return np.delete(g, 2, axis=0), np.delete(rec, 2, axis=0)


def test_layer_form_meets_the_reference():
    fx, failures = load_fixture(), []
    for dt in (torch.float64, torch.float32):
        x, p, a, s = (torch.from_numpy(fx[k]).to(dt).requires_grad_(True) for k in ("x", "p", "a", "scale"))
        out = layer_ref(x, p, a, s)
        grads = torch.autograd.grad(out, [x, p, a, s], torch.from_numpy(fx["grad_output"]).to(dt))
        tag = "fp64" if dt == torch.float64 else "fp32"
        _meets(f"{tag} out", out, fx["layer.out"], failures)
        for part, g in zip(("grad_x", "grad_p", "grad_a", "grad_scale"), grads):
            _meets(f"{tag} {part}", g, fx[f"layer.{part}"], failures)
    assert not failures, "; ".join(failures)


def test_header_and_binding_declare_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "hypad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(hypad_[a-z0-9_]+)\s*\(", body))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
    assert "#define HYPAD_ABI_VERSION 7" in header
    for const in ("HYPAD_D2P_SIGNED = 1", "HYPAD_D2P_SCALED = 2"):
        assert const in body, const
    assert "global: hypad_*;" in open(os.path.join(ROOT, "hypad_amd", "csrc", "exports.map")).read()
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7
    for name in NEW_ENTRY_POINTS:
        assert name in _C.EXPORTS and hasattr(_C.lib, name), name
    assert (_C.D2P_SIGNED, _C.D2P_SCALED) == (1, 2)
    # every entry point the header declares is bound, and nothing is bound that it does not declare
    assert declared == set(_C.EXPORTS)
    from hypad_amd import build
    assert "dist2plane.hip" in build.SOURCES


def test_workspace_size_is_a_function_of_the_shape_alone():
    from hypad_amd import _C
    K, N = 100, 200
    for rows, slices in ((130, 1), (4099, 17), (200000, 64), (0, 1)):      # the C^T x products: slices of >= 256 rows, at most 64
        tiles = (rows + 63) // 64
        want = 4 * ((1 + slices) * 2 * N * K + 2 * rows * N + rows + 4 * tiles * N)
        assert _C.lib.hypad_dist2plane_workspace_bytes(rows, K, N) == want, rows
    assert _C.lib.hypad_dist2plane_workspace_bytes(-1, K, N) == 0


def test_refusals_raise_before_touching_a_device():
    from hypad_amd import optim
    from hypad_amd.hyperspace import gmath, hyrnn_nets
    x, p, a = torch.zeros(4, 1, 8), torch.zeros(5, 8), torch.zeros(5, 8)                  # host tensors: a device call would raise HypadError
    for call in (lambda: gmath.dist2plane(x, p, a, k=1.0),
                 lambda: gmath.dist2plane(x, p, a, k=-0.5, signed=True),
                 lambda: gmath.dist2plane(x, p, a, dim=0),
                 lambda: gmath.dist2plane(x.squeeze(1), p, a),                           # (rows, K) against (N, K): element-wise in geoopt
                 lambda: gmath.dist2plane(x, p.unsqueeze(0), a.unsqueeze(0)),
                 lambda: gmath.dist2plane(x, p, a[:4]),
                 lambda: gmath.dist2plane(torch.zeros(4, 1, 257), torch.zeros(5, 257), torch.zeros(5, 257)),
                 lambda: hyrnn_nets.MobiusDist2Hyperplane(8, 5, fp64_hyper=True),
                 lambda: hyrnn_nets.MobiusDist2Hyperplane(8, 5, k=1.0)):
        with pytest.raises(NotImplementedError, match="supported"):
            call()
    layer = hyrnn_nets.MobiusDist2Hyperplane(8, 5)
    for prm in (layer.point, layer.tangent):
        prm.grad = torch.zeros_like(prm)
        before = prm.detach().clone()
        with pytest.raises(NotImplementedError, match="Euclidean optimiser"):
            optim.RiemannianAdam([prm], lr=0.1).step()
        assert torch.equal(prm.detach(), before)
    # what every existing caller passes -- a 1-D ball vector, or an untagged parameter -- gets past the check (and then needs a device)
    bias = hyrnn_nets.MobiusLinear(8, 5, fp64_hyper=False).bias
    assert bias.dim() == 1 and isinstance(bias.manifold, hyrnn_nets.PoincareBall)
    optim._check_ball_vector(bias)
    optim._check_ball_vector(layer.scale)
    optim._check_ball_vector(torch.nn.Parameter(torch.zeros(3, 4)))


def test_module_keys_shapes_and_initial_invariants():
    from hypad_amd.hyperspace import hyrnn_nets
    torch.manual_seed(5)
    layer = hyrnn_nets.MobiusDist2Hyperplane(33, 17)
    assert list(layer.state_dict()) == ["scale", "point", "tangent"]
    assert layer.scale.shape == (17,) and layer.point.shape == (17, 33) and layer.tangent.shape == (17, 33)
    assert bool((layer.scale == 0).all()) and type(layer.scale) is torch.nn.Parameter
    assert isinstance(layer.point, hyrnn_nets.ManifoldParameter) and isinstance(layer.point.manifold, hyrnn_nets.PoincareBall)
    assert isinstance(layer.tangent, hyrnn_nets.ManifoldParameter) and isinstance(layer.tangent.manifold, hyrnn_nets.Sphere)
    assert float(layer.point.manifold.k) == -1.0
    pn = layer.point.detach().double().norm(dim=1)
    assert bool((pn < 1).all()) and bool((pn > 0).all())
    assert bool(((layer.tangent.detach().double().norm(dim=1) - 1).abs() < 1e-6).all())
    assert all(p.requires_grad and p.dtype == torch.float32 for p in layer.parameters())
    assert "in_features=33, out_features=17" in repr(layer)
    # the state dict round-trips, manifolds included, through a second instance
    other = hyrnn_nets.MobiusDist2Hyperplane(33, 17)
    other.load_state_dict(layer.state_dict())
    assert torch.equal(other.point, layer.point) and isinstance(other.tangent.manifold, hyrnn_nets.Sphere)
