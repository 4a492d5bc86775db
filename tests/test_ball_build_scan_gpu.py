"""
The two ball builds (DeviceGoalBall, DeviceSymBall) with a scan of more than one workgroup, at radius 3 (1 195 states, 32 orbits),
against their models (tests/ball_model.py, tests/sym_model.py), bit for bit:
  * pops = 22: 264 children per batch, so the scan's second 256-thread workgroup has an 8-thread tail and one look-back step (the
    plain ball's level 2 has 114 parents: five full batches and one of four);
  * pops = 64: 768 children, three full workgroups.
The symmetry ball's levels 0..2 hold 1, 1 and 5 orbits, so its batches are shorter than the grid: its later workgroups draw a
ticket and leave.
"""
import functools

import numpy as np
import pytest

from librubiks_amd.solving.agents import DeviceGoalBall, DeviceSymBall
from tests import ball_model, sym_model

pytestmark = pytest.mark.gpu

RADIUS = 3
POPS = (22, 64)


@functools.lru_cache(maxsize=None)
def _plain_model():
	want = ball_model.build(RADIUS)
	assert want.len == 1_195
	return want


@functools.lru_cache(maxsize=None)
def _sym_model():
	return sym_model.build(RADIUS)


@pytest.mark.parametrize("pops", POPS)
def test_plain_ball(pops):
	want = _plain_model()
	ball = DeviceGoalBall(RADIUS, pops=pops).build()
	assert len(ball) == want.len and ball.built
	assert ball.level_start.tolist() == want.level_start.tolist()
	states, parents, actions = ball.arrays()
	assert (states == want.states).all() and (parents == want.parents).all() and (actions == want.actions).all()
	assert ball.iterations == sum(-(-n // pops) for n in np.diff(want.level_start).tolist()[:RADIUS])


@pytest.mark.parametrize("pops", POPS)
def test_symmetry_ball(pops):
	want = _sym_model()
	ball = DeviceSymBall(RADIUS, pops=pops).build()
	assert len(ball) == want.len and ball.built
	assert ball.level_start.tolist() == want.level_start.tolist()
	states = ball.arrays()
	assert states.shape == (want.len, 20) and (states == want.states).all()
	assert ball.states_covered.tolist() == want.covered.tolist() == [1, 12, 114, 1_068]
	assert ball.iterations == sum(-(-n // pops) for n in np.diff(want.level_start).tolist()[:RADIUS])
