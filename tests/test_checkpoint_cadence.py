"""hypad_amd.train._saves_checkpoint: the reference's checkpoint cadence (train.py:381), ONE function for train_tadgan, train_tadgan_resident
and train_signals_resident.  The expectations are literal: worked out from the three lambdas the function replaced,
``(first + e + 1) % 10 == 0 or (first + e + 1) == n_epochs - 1`` over ``e in range(n_epochs)`` -- the reference's quirk included that
``n_epochs`` is the number of epochs still to run (already reduced on resume), while ``first`` counts from the resumed epoch."""
import pytest

from hypad_amd.train import _saves_checkpoint


@pytest.mark.parametrize("first,n_epochs,expected", [
    (0, 24, {9, 19, 22}),
    (0, 3, {1}),
    (0, 2, {0}),
    (8, 3, {1}),            # resume_epoch = 7 of 10: three epochs left, numbered 9, 10, 11 -- only _10 is written
    (0, 0, set()),
    (0, 1, set()),
])
def test_checkpoint_cadence(first, n_epochs, expected):
    assert {e for e in range(n_epochs) if _saves_checkpoint(first, e, n_epochs)} == expected
