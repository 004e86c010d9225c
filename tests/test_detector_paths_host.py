"""CPU-only checks of what the detector paths share: the combination names and the predicate for the ones that read the critic scores,
the rejection of an unknown combination before anything touches the device, and the writer of the test loop's cache files."""
import os

import numpy as np
import pytest
import torch

from hypad_amd import anomaly_detection as had
from hypad_amd.utils import anomaly_detection_utils as adu

EUCLIDEAN_MESSAGE = 'Unknown combination specified uncertainty, use "mult", "sum", or "rec" instead.'       # score_anomalies' own (:570)


def test_combination_names_and_their_rejection():
    with_critic = ["sum", "mult", "uncertainty", "critic", "critic_uncertainty", "sum_uncertainty"]
    without = ["rec", "rec_uncertainty"]
    assert sorted(adu.COMBINATIONS) == sorted(with_critic + without) and len(adu.COMBINATIONS) == 8
    assert [c for c in adu.COMBINATIONS if adu.uses_critic(c)] == [c for c in adu.COMBINATIONS if c in with_critic]
    assert [c for c in adu.COMBINATIONS if not adu.uses_critic(c)] == [c for c in adu.COMBINATIONS if c in without]
    assert set(adu.COMBINATIONS) <= set(adu._C.COMB) and set(adu.EUCLIDEAN_MODES.values()) <= set(adu._C.COMB)
    # dummy inputs: an unknown name is refused before any of them is looked at, let alone uploaded
    res = {"row_off": [0, 3], "recons": None, "hyper_real": None, "critic": None}
    for call in (lambda: adu.combine_scores("product", [1.0], [1.0], None),
                 lambda: adu.hyperbolic_scores_signals(res, "product"),
                 lambda: adu.multivariate_scores_signals(res, None, "product")):
        with pytest.raises(ValueError, match="^product$"):
            call()
    with pytest.raises(ValueError) as e:
        adu.combine_euclidean("uncertainty", None, None)
    assert str(e.value) == EUCLIDEAN_MESSAGE
    with pytest.raises(ValueError) as e:
        adu.euclidean_scores_signals(res, None, "dtw", "uncertainty")
    assert str(e.value) == EUCLIDEAN_MESSAGE


@pytest.mark.parametrize("hyperbolic", [False, True])
def test_save_test_outputs_writes_the_test_loops_files(tmp_path, hyperbolic):
    g = np.random.default_rng(0)
    recons, eucl, real = (g.standard_normal((7, 5)).astype(np.float32) for _ in range(3))
    gt = g.standard_normal((7, 5, 1))
    critic = g.standard_normal(7).astype(np.float32)
    want = {"recons_signal.pt": recons, "gt_signal.pt": gt, "critic_score.pt": list(critic)}
    if hyperbolic:
        want.update({"eucl_recons.pt": eucl, "real_hyper.pt": real})
        had.save_test_outputs(str(tmp_path), recons, gt, critic, eucl, real)
    else:
        had.save_test_outputs(str(tmp_path), recons, gt, critic)
    assert sorted(os.listdir(tmp_path)) == sorted(want)
    for name, array in want.items():
        got = torch.load(tmp_path / name, weights_only=False)
        if name == "critic_score.pt":
            assert type(got) is list and len(got) == 7 and all(type(v) is np.float32 for v in got)
        else:
            assert type(got) is np.ndarray and got.dtype == array.dtype
        assert np.array_equal(np.asarray(got), np.asarray(array)), name
