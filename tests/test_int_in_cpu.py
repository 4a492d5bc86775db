"""
eng.int_in, the one argument checker of the device agents: what it returns for a good value, and the exact message each kind of
bad value has always raised in the agents' constructors (the same check, written out, before it was shared).
"""
import numpy as np
import pytest

from librubiks_amd.solving import _engine as eng

MAX_POPS = 1 << 22
MAX_CAPACITY = 0x3FFFFFF0


def _written_out(name, v, lo, hi):
	"""The check as every constructor used to spell it."""
	if isinstance(v, bool) or int(v) != v or not lo <= int(v) <= hi:
		raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")


@pytest.mark.parametrize("value", [1, 7, MAX_POPS, 16_384.0, np.int64(5), np.float32(64)])
def test_good_values_come_back_as_int(value):
	got = eng.int_in("pops", value, 1, MAX_POPS)
	assert type(got) is int and got == value
	assert eng.int_in("poll", value, 1, what="a positive integer") == value


@pytest.mark.parametrize("value, text", [
	(True, "pops must be an integer in 1..4194304, got True"),
	(False, "pops must be an integer in 1..4194304, got False"),
	(2.5, "pops must be an integer in 1..4194304, got 2.5"),
	(0, "pops must be an integer in 1..4194304, got 0"),
	(-3, "pops must be an integer in 1..4194304, got -3"),
	(MAX_POPS + 1, "pops must be an integer in 1..4194304, got 4194305"),
])
def test_bools_fractions_and_out_of_range(value, text):
	with pytest.raises(ValueError) as e:
		eng.int_in("pops", value, 1, MAX_POPS)
	assert str(e.value) == text
	with pytest.raises(ValueError) as ref:
		_written_out("pops", value, 1, MAX_POPS)
	assert str(ref.value) == text


@pytest.mark.parametrize("name", ["capacity", "max_capacity"])
def test_capacity_texts_and_none(name):
	assert eng.int_in(name, None, 2, MAX_CAPACITY, none_ok=True) is None
	assert eng.int_in(name, 2, 2, MAX_CAPACITY, none_ok=True) == 2
	for bad in (1, True, 3.5, MAX_CAPACITY + 1):
		with pytest.raises(ValueError) as e:
			eng.int_in(name, bad, 2, MAX_CAPACITY, none_ok=True)
		assert str(e.value) == f"{name} must be an integer in 2..1073741808, got {bad!r}"


def test_texts_that_name_their_own_range():
	for bad in (0, True, 1.5, -1):
		with pytest.raises(ValueError) as e:
			eng.int_in("poll", bad, 1, what="a positive integer")
		assert str(e.value) == f"poll must be a positive integer, got {bad!r}"
	with pytest.raises(ValueError) as e:
		eng.int_in("capacity", 0, 1, MAX_CAPACITY, none_ok=True, what=f"an integer in 1..{MAX_CAPACITY} or None")
	assert str(e.value) == "capacity must be an integer in 1..1073741808 or None, got 0"
	with pytest.raises(ValueError) as e:
		eng.int_in("window", 0, 1, none_ok=True, what="an integer >= 1 or None")
	assert str(e.value) == "window must be an integer >= 1 or None, got 0"
	assert eng.int_in("passes", 0, 0, none_ok=True, what="an integer >= 0 or None") == 0
	assert eng.int_in("passes", 10 ** 12, 0, none_ok=True, what="an integer >= 0 or None") == 10 ** 12


def test_none_where_it_is_not_allowed():
	"""The written-out check handed None to int(): a TypeError with int()'s own text.  That stays."""
	with pytest.raises(TypeError) as ref:
		_written_out("pops", None, 1, MAX_POPS)
	for kw in ({}, {"none_ok": False}):
		with pytest.raises(TypeError) as e:
			eng.int_in("pops", None, 1, MAX_POPS, **kw)
		assert str(e.value) == str(ref.value)


def test_the_agents_use_it():
	"""The constructors raise these texts without a GPU."""
	from librubiks_amd.solving import agents
	for make in (agents.DeviceBFS, agents.DeviceBiBFS):
		with pytest.raises(ValueError, match=r"^pops must be an integer in 1\.\.4194304, got True$"):
			make(pops=True)
		with pytest.raises(ValueError, match=r"^max_capacity must be an integer in 2\.\.1073741808, got 1$"):
			make(max_capacity=1)
		with pytest.raises(ValueError, match=r"^poll must be a positive integer, got 0$"):
			make(poll=0)
		assert make(pops=5.0, capacity=2).pops == 5
	with pytest.raises(ValueError, match=r"^radius must be an integer in 0\.\.8, got 9$"):
		agents.DeviceGoalBall(9)
	with pytest.raises(ValueError, match=r"^radius must be an integer in 0\.\.10, got 2\.5$"):
		agents.DeviceSymBall(2.5)
	with pytest.raises(ValueError, match=r"^capacity must be an integer in 1\.\.1073741808 or None, got 0$"):
		agents.DeviceSymBall(2, capacity=0)
	with pytest.raises(ValueError, match=r"^searches must be an integer in 1\.\.1024, got 1025$"):
		agents.DeviceBallSearchBatch(agents.DeviceGoalBall(1), searches=1025)
	with pytest.raises(TypeError, match=r"^ball must be a DeviceGoalBall, got DeviceSymBall$"):
		agents.DeviceBallSearch(agents.DeviceSymBall(1))
