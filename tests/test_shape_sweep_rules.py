"""CPU side of the shape sweep (tests/sweep_common.py): the comparison rule catches what it is meant to catch, passes what it must
pass, and the grid is what it claims to be -- runtime shapes only (plus the two tagged anchors), none of them ill-conditioned."""
import numpy as np
import pytest
import torch

import sweep_common as sc


def _anchor_refs(hyper):
    S, L, B = sc.ANCHOR
    sd = sc.init_state(S, L, hyper)
    data = sc.iteration_data(S, L, B)
    return sc.iterations(sc.cast(sd, torch.float64), *data, hyper), sc.iterations(sd, *data, hyper)


def test_rule_catches_a_planted_tail_column_error():
    r64, r32 = _anchor_refs(True)
    name = "dec.dense2.weight"
    g64, g32 = r64["dec"][2][name], r32["dec"][2][name]
    allow = sc.grad_allowance(g64, g32)
    bad = g32.clone()
    bad[7, -1] += 10 * allow
    ck = sc.Checker("planted")
    ck.cmp(name, bad, g64, g32)
    with pytest.raises(AssertionError) as e:
        ck.done()
    msg = str(e.value)
    assert name in msg and f"row 7, col {g64.shape[1] - 1}" in msg and "err32" in msg


def test_rule_passes_the_fp32_oracle_itself():
    for hyper in (True, False):
        r64, r32 = _anchor_refs(hyper)
        ck = sc.Checker(f"fp32 oracle hyper={hyper}")
        for kind in ("cx", "cz", "dec"):
            ck.cmp(kind + " loss", r32[kind][0], r64[kind][0], r32[kind][0])
            for k, g in r64[kind][-1].items():
                ck.cmp(k, r32[kind][-1][k], g, r32[kind][-1][k])
        ck.cmp("aux", r32["dec"][1], r64["dec"][1], r32["dec"][1])
        ck.done()


def test_resolvable_mask_excludes_rounding_level_gradients():
    g64 = torch.tensor([[1e-3, -2e-4, 1e-12, 0.0]], dtype=torch.float64)
    g32 = (g64 + 1e-9).float()
    ok = sc.resolvable(g64, g32)
    assert ok.tolist() == [[True, True, False, False]]


@pytest.mark.parametrize("case", sc.grid(), ids=sc.grid_id)
def test_grid_shapes_are_well_conditioned(case):
    """fp32 against fp64 on the losses and the aux term: below 1e-5 at every grid shape (else its data scale, not the rule, changes)."""
    S, L, B, hyper, _ = case
    sd = sc.init_state(S, L, hyper)
    data = sc.iteration_data(S, L, B)
    r64, r32 = sc.iterations(sc.cast(sd, torch.float64), *data, hyper), sc.iterations(sd, *data, hyper)
    for kind in ("cx", "cz", "dec"):
        e, _ = sc.rel_err(r32[kind][0], r64[kind][0])
        assert e < 1e-5, (case, kind, e)
    e, _ = sc.rel_err(r32["dec"][1], r64["dec"][1])
    assert e < 1e-5, (case, "aux", e)
    if hyper:        # the ball bias really is off the origin's conformal factor
        b = sd["dec.hyperbolic_linear.bias"].double()
        assert 2 / (1 - float(b @ b)) > 2.01


def test_grid_is_runtime_shapes_plus_tagged_anchors():
    import ctypes
    from hypad_amd import _C
    cases = sc.grid()
    anchors = [c for c in cases if c[4] == "anchor"]
    assert sorted(c[3] for c in anchors) == [False, True] and all(c[:3] == sc.ANCHOR for c in anchors)
    for S, L, B, hyper, tag in cases:
        if tag != "anchor":
            assert (S, L, B) not in sc.SHIPPED, (S, L, B)
        assert B % 16 == 0 and 1 <= L <= 32 and 1 <= S <= 256
    hyp = [c for c in cases if c[3] and c[4] == "runtime"]
    # both edges of every epl16_dispatch row-layout class
    widths = {c[0] for c in hyp}
    for edge in (8, 64, 65, 112, 113, 128, 129, 256):
        assert edge in widths, edge
    assert {c[1] for c in hyp} >= {1, 32} and {c[2] for c in hyp} >= {32, 256}
    assert any(c[0] % 4 for c in hyp) and any(c[0] % 16 for c in hyp)
    ms, ml = ctypes.c_int(), ctypes.c_int()
    _C.lib.hypad_limits(ctypes.byref(ms), ctypes.byref(ml))
    assert max(widths) == ms.value and max(c[1] for c in cases) == ml.value      # the widest window and latent the library takes


def test_training_workspace_refuses_only_what_the_critic_launches_cannot_hold():
    """hypad_train_workspace_bytes (host only) is 0 exactly where the stand-alone critic launches need more than 160 KiB of LDS:
    latent 29..32 with windows above 240, the grid's REFUSED shape among them; every grid shape is accepted."""
    import ctypes
    from hypad_amd import _C
    ws = lambda S, L, B=32, h=1: _C.lib.hypad_train_workspace_bytes(ctypes.byref(_C.Dims(S, L, B, h, 1, 0)))
    assert ws(*sc.REFUSED) == 0
    for S, L, B, hyper, _ in sc.grid():
        assert ws(S, L, B, int(hyper)) > 0, (S, L, B, hyper)
    for L in range(1, 33):
        for S in (1, 100, 240, 241, 256):
            assert (ws(S, L) == 0) == (L >= 29 and S > 240), (S, L)


def test_oracle_runs_at_the_grid_extremes_in_both_dtypes():
    """The fp64 oracle is the yardstick: it must accept every grid shape and agree with its own fp32 run to fp32 rounding."""
    for S, L, B in ((8, 20, 16), (256, 32, 16)):
        sd = sc.init_state(S, L, True)
        data = sc.iteration_data(S, L, B)
        r64 = sc.iterations(sc.cast(sd, torch.float64), *data, True)
        r32 = sc.iterations(sd, *data, True)
        for k, g in r64["dec"][2].items():
            assert g.dtype == torch.float64 and torch.isfinite(g).all(), k
            e, _ = sc.rel_err(r32["dec"][2][k], g)
            assert e < 1e-4, (S, L, k, e)
        assert np.isfinite(float(r64["dec"][0]))
