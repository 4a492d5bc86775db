"""
The pattern-database model (tests/pdb_model.py) against something that does not use its ranking: a dictionary breadth-first
search over the tuples of the selected codes from the goal.  For one corner (24 entries), three corners (9 072) and the cross
(190 080): the same distance for every reached tuple, every table entry reached, unrank o rank the identity on the whole space.
For all eight corners only the size and unrank o rank on 100 000 seeded indices, the recovered last twist included.
"""
import numpy as np
import pytest

from oracle import cube_oracle as orc
from tests import pdb_model as M

CROSS_D = tuple(sorted(int(e) for e in orc._FACES[3][1]))


def test_cross_edges_come_from_the_face_definition():
	assert len(CROSS_D) == 4 and all(0 <= e < 12 for e in CROSS_D)


@pytest.mark.parametrize("corners,edges,size", [((5,), (), 24), ((0, 3, 6), (), 9_072), ((), CROSS_D, 190_080)])
def test_model_against_dictionary_search(corners, edges, size):
	p = M.Pattern(corners, edges)
	assert p.size == size
	table, sizes = p.table()
	assert sizes[0] == 1 and sizes.sum() == size and not (table == M.UNREACHED).any()
	everything = np.arange(size)
	codes = p.unrank(everything)
	assert p.valid(codes).all() and (p.rank(codes) == everything).all()
	dist = M.dictionary_bfs(p)
	assert len(dist) == size                                            # every entry is reached, and nothing else
	keys = np.array(list(dist), np.int64)
	assert (table[p.rank(keys)] == np.array(list(dist.values()))).all()
	assert (np.bincount(list(dist.values())) == sizes).all()


def test_all_corners_size_and_rank_round_trip():
	p = M.Pattern(range(8), ())
	assert p.size == 88_179_840
	index = np.random.RandomState(2_501).randint(0, p.size, 100_000)
	codes = p.unrank(index)
	assert p.valid(codes).all() and (p.rank(codes) == index).all()
	# the recovered last twist: every unranked placement is a corner placement some legal state has, as scrambles have
	from tests import group_model
	tau = group_model.tables()[2].astype(np.int64)
	assert not (tau[codes].sum(axis=1) % 3).any()
	rs = np.random.RandomState(2_502)
	s = orc.repeat_state(orc.SOLVED, 2_000)
	for _ in range(30):
		s = orc.multi_rotate(s, rs.randint(0, 6, len(s)), rs.randint(0, 2, len(s)))
	got = p.select(s)
	assert (p.unrank(p.rank(got)) == got).all()
