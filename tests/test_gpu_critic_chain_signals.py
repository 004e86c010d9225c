"""The segmented critic-score chain of a signal group (hypad_quantiles_signals, hypad_critic_chain_signals,
utils.anomaly_detection_utils.final_critic_scores_signals) against the per-segment paths it replaces: np.quantile and hypad_quantiles
per segment, hypad_kde_mode_signals + hypad_critic_score_signals, final_critic_scores per signal -- equal fp64 bit patterns, NaNs
included -- and the reference's own final_critic_scores numbers (fixture score.npz)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from helpers import load, same_bits

pytestmark = pytest.mark.gpu
_same_bits = functools.partial(same_bits, dtype=torch.float64)       # (every score compared here is fp64)


def _toff(row_off, w):
    return [int(r) + s * (w - 1) for s, r in enumerate(row_off)]


# ------------------------------------------------------------------------------------------------ quantiles
def _keys(x):
    """The 64-bit keys of the radix selection (unsigned order = numeric order of the doubles)."""
    b = x.view(np.uint64)
    return np.where(b >> np.uint64(63), ~b, b ^ np.uint64(1 << 63))


def _special_segments(rng):
    """(name, values) -- the segments the selection's special paths need."""
    band = 1.5 * (1.0 + rng.random(6_500) * 2.0 ** -23)                     # all within a relative band of 2^-23 < 2^-22, not equal
    assert len(np.unique(band)) > 4_096 and band.max() / band.min() - 1.0 < 2.0 ** -22
    prefix, count = np.unique(_keys(band) >> np.uint64(31), return_counts=True)
    assert count.max() > 4_096, count.max()                                  # > QS_CAND keys share one 33-bit prefix: the fallback over the input
    mixed = np.concatenate([-rng.random(300), np.zeros(40), -np.zeros(7), rng.random(300) * 5e-324 * 1000, [5e-324, -5e-324, 2.2e-308, -1e-310],
                            rng.standard_normal(200) * 1e-300, rng.standard_normal(100)])
    rng.shuffle(mixed)
    with_nan = rng.standard_normal(3_000)
    with_nan[1_234] = np.nan
    first = [("one", rng.standard_normal(1)), ("two", rng.standard_normal(2)), ("99", rng.standard_normal(99)),
             ("1024", rng.standard_normal(1_024)), ("1025", rng.standard_normal(1_025)), ("20000", 3.0 + 0.02 * rng.standard_normal(20_000)),
             ("ties", rng.integers(0, 5, 4_000).astype(np.float64)), ("mixed", mixed)]
    last = [("constant", np.full(2_500, 0.731)), ("band", band), ("nan", with_nan), ("after_nan", rng.standard_normal(777))]
    return first, last


def _quantiles_signals(flat, row_off, w, q):
    from hypad_amd import _C
    k = len(row_off) - 1
    qa = (ctypes.c_double * len(q))(*q)
    out = torch.full((k, len(q)), -7.0, dtype=torch.float64, device="cuda")
    nbytes = _C.lib.hypad_quantiles_signals_workspace_bytes(k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")                # exactly what the function asks for
    _C.check(_C.lib.hypad_quantiles_signals(_C.ptr(flat), k, _C.int64s(row_off), w, qa, len(q), _C.ptr(out), ws.data_ptr(), nbytes, _C.stream()),
             "quantiles_signals")
    return out


def _check_quantile_group(segments, w):
    """segments: (name, values of length n_s + w - 1); laid out in timestep layout with window w."""
    from hypad_amd.utils import anomaly_detection_utils as adu
    counts = [len(v) - (w - 1) for _, v in segments]
    assert min(counts) >= 1
    row_off = [int(v) for v in np.cumsum([0] + counts)]
    t_off = _toff(row_off, w)
    host = np.concatenate([v for _, v in segments]).astype(np.float64)
    assert len(host) == t_off[-1]
    flat = torch.from_numpy(host).cuda()
    for q in ((0.25, 0.75), (0.5,), (0.0, 1.0), (1.0 / 3.0, 0.999), (0.75, 0.25)):
        got = _quantiles_signals(flat, row_off, w, q).cpu()
        for s, (name, v) in enumerate(segments):
            ref = np.quantile(v, q)
            mine = got[s].numpy()
            if np.isnan(v).any():
                assert np.isnan(ref).all() and np.isnan(mine).all(), (name, q, mine)
                continue
            assert not np.isnan(mine).any(), (name, s, q, mine)
            assert mine.tobytes() == np.asarray(ref, dtype=np.float64).tobytes(), (name, s, q, mine, ref)
            single = adu.quantiles(flat[t_off[s]: t_off[s + 1]], q)
            _same_bits(got[s], single, (name, s, q))


def test_quantiles_of_every_segment_equal_numpy_and_the_single_signal_call():
    rng = np.random.default_rng(21)
    first, last = _special_segments(rng)
    # one group with every special segment, window 1 (a segment of the layout is exactly its n_s values: lengths 1 and 2 exist)
    _check_quantile_group(first + last, 1)
    # 70 segments in one call: the specials on both sides of the 64-segment chunk boundary (NaN segment at index 68, a neighbour on each side)
    fill = [("fill%d" % i, rng.standard_normal(int(n))) for i, n in enumerate(rng.integers(1, 3_000, size=70 - len(first) - len(last)))]
    group = first + fill + last
    assert len(group) == 70 and group[68][0] == "nan"
    _check_quantile_group(group, 1)
    # the timestep layout of a real window (segments n_s + 99 long, s * 99 entries between the row offsets and the segments)
    _check_quantile_group([(n, v) for n, v in first + last if len(v) >= 100], 100)


# ------------------------------------------------------------------------------------------------ the chain
def _old_chain(critic, row_off, w):
    """hypad_kde_mode_signals + hypad_critic_score_signals: the per-segment launches."""
    from hypad_amd import _C
    k = len(row_off) - 1
    offs = _C.int64s(row_off)
    modes = torch.empty(row_off[-1] + k * (w - 1), device="cuda", dtype=torch.float64)
    _C.check(_C.lib.hypad_kde_mode_signals(_C.ptr(critic), _C.ptr(modes), k, offs, w, _C.stream()), "kde_mode_signals")
    out = torch.empty_like(modes)
    nbytes = _C.lib.hypad_critic_score_signals_workspace_bytes(k, offs, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _C.check(_C.lib.hypad_critic_score_signals(_C.ptr(modes), _C.ptr(out), k, offs, w, ws.data_ptr(), nbytes, _C.stream()), "critic_score_signals")
    return modes, out


def _new_chain(critic, row_off, w, with_modes=True):
    from hypad_amd import _C
    k = len(row_off) - 1
    offs = _C.int64s(row_off)
    out = torch.full((row_off[-1] + k * (w - 1),), -7.0, device="cuda", dtype=torch.float64)
    modes = torch.full_like(out, -7.0) if with_modes else None
    nbytes = _C.lib.hypad_critic_chain_signals_workspace_bytes(k, offs, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")                # exactly what the function asks for
    _C.check(_C.lib.hypad_critic_chain_signals(_C.ptr(critic), _C.ptr(modes), _C.ptr(out), k, offs, w, ws.data_ptr(), nbytes, _C.stream()),
             "critic_chain_signals")
    return modes, out


def _check_chain(counts, w, critic=None, seed=0):
    row_off = [int(v) for v in np.cumsum([0] + list(counts))]
    if critic is None:
        critic = torch.randn(row_off[-1], device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    critic = critic.to("cuda", torch.float32).contiguous()
    want_modes, want = _old_chain(critic, row_off, w)
    modes, got = _new_chain(critic, row_off, w)
    _, got_alone = _new_chain(critic, row_off, w, with_modes=False)
    torch.cuda.synchronize()
    _same_bits(modes, want_modes, (counts[:6], w, "modes"))
    _same_bits(got, want, (counts[:6], w, "scores"))
    _same_bits(got_alone, want, (counts[:6], w, "scores without modes_out"))
    t_off = _toff(row_off, w)
    for s, n in enumerate(counts):                                            # trunc(n * 0.01) = 0: pandas' rolling(0), all NaN
        seg = got[t_off[s]: t_off[s + 1]]
        assert bool(torch.isnan(seg).all()) == (n < 100), (s, n)
    return got


@pytest.mark.parametrize("w", [51, 100, 150])
def test_chain_equals_the_per_segment_launches(w):
    _check_chain([50, 1, 120, 333, 1_500], w, seed=w)                         # (the group of the hyperbolic test: two all-NaN segments)


def test_chain_of_a_ragged_group_of_32_signals():
    rng = np.random.default_rng(0)
    _check_chain([int(v) for v in rng.integers(1_500, 9_001, size=32)], 100, seed=1)


def test_chain_of_70_signals_crosses_the_chunk_of_64():
    rng = np.random.default_rng(2)
    counts = [int(v) for v in rng.integers(1, 700, size=70)]
    counts[3], counts[66] = 1, 40
    _check_chain(counts, 100, seed=2)


def test_chain_with_a_long_segment():
    # 33 000 windows: a smoothing window of 330 (the chunked rolling mean) and 33 slices of the trimmed statistics
    _check_chain([300, 33_000, 2_000], 100, seed=3)


def test_chain_on_clustered_critic_values():
    # trained critics cluster in a band ~2 % wide around a non-zero mean (the case the three pre-levels of the selection exist for)
    counts = [2_500, 400, 12_000, 150]
    g = torch.Generator(device="cuda").manual_seed(4)
    critic = 3.7 * (1.0 + 0.01 * (2.0 * torch.rand(sum(counts), device="cuda", generator=g) - 1.0))
    _check_chain(counts, 100, critic=critic)
    _check_chain(counts, 100, critic=-critic * 1e-3)


def test_chain_meets_the_reference_numbers():
    """The reference's own final_critic_scores output for the fixture's critic values, as one segment among perturbed copies; the
    tolerance is the one tests/test_gpu_parity.py holds the single-signal path to for the same fixture."""
    fx = load("score.npz")
    y, critic = fx["y"], np.asarray(fx["critic"], dtype=np.float32).reshape(-1)
    n, w = len(y), y.reshape(len(y), -1).shape[1]
    assert len(critic) == n
    rng = np.random.default_rng(6)
    segs = [critic + 0.05 * rng.standard_normal(n).astype(np.float32), critic, (critic * 1.1)[: n - 7],
            critic + 0.01 * rng.standard_normal(n).astype(np.float32)]
    counts = [len(c) for c in segs]
    got = _check_chain(counts, w, critic=torch.from_numpy(np.concatenate(segs)))
    t_off = _toff(np.cumsum([0] + counts), w)
    mine = got[t_off[1]: t_off[2]].cpu().numpy()
    assert mine.shape == fx["critic_scores"].shape
    assert np.allclose(mine, fx["critic_scores"], rtol=0, atol=1e-9, equal_nan=True)


# ------------------------------------------------------------------------------------------------ the mirror
def test_mirror_equals_final_critic_scores_per_signal():
    from hypad_amd.utils import anomaly_detection_utils as adu
    w = 100
    counts = [50, 700, 1, 2_345, 100, 99]
    row_off = [int(v) for v in np.cumsum([0] + counts)]
    critic = torch.randn(row_off[-1], device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    out, modes = adu.final_critic_scores_signals(critic, row_off, w, with_modes=True)
    alone = adu.final_critic_scores_signals(critic, row_off, w)
    torch.cuda.synchronize()
    assert out.is_cuda and out.dtype == torch.float64 and modes.is_cuda
    _same_bits(alone, out, "with / without modes")
    t_off = _toff(row_off, w)
    host = critic.cpu().numpy()
    for s, n in enumerate(counts):
        crit = host[row_off[s]: row_off[s + 1]]
        want = adu.final_critic_scores(list(crit), np.empty((n, w)))
        _same_bits(out[t_off[s]: t_off[s + 1]], torch.from_numpy(want), ("final_critic_scores", s))
        _same_bits(modes[t_off[s]: t_off[s + 1]], adu.kde_modes(crit, w), ("kde_modes", s))


def test_mirror_is_capturable_and_replays_to_the_same_bits():
    from hypad_amd.utils import anomaly_detection_utils as adu
    w = 100
    counts = [400, 60, 3_000, 1_200]
    row_off = [int(v) for v in np.cumsum([0] + counts)]
    gen = torch.Generator(device="cuda").manual_seed(9)
    critic = torch.randn(row_off[-1], device="cuda", generator=gen)
    want = adu.final_critic_scores_signals(critic, row_off, w).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = adu.final_critic_scores_signals(critic, row_off, w)
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    g.replay()
    torch.cuda.synchronize()
    second = out.clone()
    _same_bits(first, want, "first replay")
    _same_bits(second, want, "second replay")                                 # (the workspace is zeroed again by the call's own kernels)
    # other values through the same graph: the replay reads the buffer, not what it held at capture
    critic.copy_(2.0 + 0.3 * torch.randn(row_off[-1], device="cuda", generator=gen))
    g.replay()
    torch.cuda.synchronize()
    _same_bits(out.clone(), adu.final_critic_scores_signals(critic, row_off, w), "replay on new values")
