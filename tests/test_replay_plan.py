"""The schedule of a lockstep replay of recorded walks (csrc/replay_plan.h) through its host-only entry fgdm_replay_plan: which
units share a grouped launch, and in which order everything runs.  No device: a walk here is a list of (key, grid_x, shape)."""
import ctypes as C

import pytest

from fgdm_amd import _lib

A, B_, C_, D = (7, 40, 0), (8, 40, 0), (9, 16, 3), (11, 2, 0)      # four fusable kinds of unit
PLAIN = (0, 0, 0)      # a unit without a grouped form


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def limits(lib):
    """(look-ahead, FGDM_MAX_GROUP) as the library reports them"""
    lim = (C.c_int * 2)()
    assert lib.fgdm_replay_plan(0, None, None, None, None, 1, 0, None, 0, lim) == 0
    return lim[0], lim[1]


def plan(lib, walks, group_max=None, chunk=0):
    """-> (steps, look_ahead); a step is a list of (walk, unit), one member = the unit runs alone.  Checks the invariants that
    hold for every schedule."""
    if group_max is None:
        group_max = limits(lib)[1]
    flat = [u for w in walks for u in w]
    n = max(len(flat), 1)
    lens = (C.c_int32 * max(len(walks), 1))(*[len(w) for w in walks])
    key = (C.c_uint64 * n)(*[u[0] for u in flat])
    grid = (C.c_uint32 * n)(*[u[1] for u in flat])
    shape = (C.c_uint64 * n)(*[u[2] for u in flat])
    cap = 3 * len(flat) + 8
    out = (C.c_int32 * cap)()
    look = (C.c_int * 2)()
    m = lib.fgdm_replay_plan(len(walks), lens, key, grid, shape, group_max, chunk, out, cap, look)
    assert 0 <= m <= cap, m
    steps, i = [], 0
    while i < m:
        k = out[i]
        assert k >= 1 and i + 1 + 2 * k <= m
        steps.append([(out[i + 1 + 2 * j], out[i + 2 + 2 * j]) for j in range(k)])
        i += 1 + 2 * k
    seen = [wu for st in steps for wu in st]
    assert sorted(seen) == [(w, u) for w in range(len(walks)) for u in range(len(walks[w]))]       # every unit exactly once
    for w in range(len(walks)):
        mine = [u for (ww, u) in seen if ww == w]
        assert mine == sorted(mine)                                                              # each walk in its own order
    for st in steps:
        if len(st) > 1:
            assert len(st) <= group_max and len({w for w, _ in st}) == len(st)
            kinds = {walks[w][u] for w, u in st}
            assert len(kinds) == 1 and next(iter(kinds))[0] != 0, kinds
    return steps, look[0]


def groups(steps):
    return [st for st in steps if len(st) > 1]


def test_identical_walks_fuse_unit_by_unit(lib):
    w = [A, B_, C_, A, D, B_]
    steps, _ = plan(lib, [w, w])
    assert steps == [[(0, u), (1, u)] for u in range(6)]


@pytest.mark.parametrize('a,b', [((7, 40, 0), (7, 41, 0)), ((7, 40, 5), (7, 40, 6)), ((0, 40, 0), (0, 40, 0))])
def test_other_grid_other_shape_or_no_key_never_fuse(lib, a, b):
    steps, _ = plan(lib, [[a] * 3, [b] * 3])
    assert not groups(steps)
    assert steps == [[(0, u)] for u in range(3)] + [[(1, u)] for u in range(3)]


def test_look_ahead_limit(lib):
    _, look = plan(lib, [])
    assert look > 1
    for other in (PLAIN, B_):        # what stands in front of the match may itself be fusable, with somebody else
        near, _ = plan(lib, [[A], [other] * (look - 1) + [A]])
        assert groups(near) == [[(0, 0), (1, look - 1)]]
        far, _ = plan(lib, [[A], [other] * look + [A]])
        assert not groups(far)


def test_partner_runs_what_stands_in_front_of_its_member_first(lib):
    steps, _ = plan(lib, [[A, B_], [PLAIN, PLAIN, PLAIN, A, B_]])
    assert steps == [[(1, 0)], [(1, 1)], [(1, 2)], [(0, 0), (1, 3)], [(0, 1), (1, 4)]]


def test_next_walk_leads_when_the_leader_runs_out(lib):
    steps, _ = plan(lib, [[A], [A, B_, PLAIN, C_], [A, B_, C_, PLAIN]])
    assert steps == [[(0, 0), (1, 0), (2, 0)], [(1, 1), (2, 1)], [(1, 2)], [(1, 3), (2, 2)], [(2, 3)]]


def test_walks_beyond_the_group_size_replay_whole_last_first(lib):
    w = [A, PLAIN, B_]
    gm = limits(lib)[1]                  # 5: seven walks, the sixth and seventh are surplus
    steps, _ = plan(lib, [w] * (gm + 2), group_max=gm)
    assert steps[:6] == [[(gm + 1, u)] for u in range(3)] + [[(gm, u)] for u in range(3)]
    every = lambda u: [(k, u) for k in range(gm)]
    assert steps[6:] == [every(0)] + [[(k, 1)] for k in range(gm)] + [every(2)]


def test_chunks_of_group_max_walks(lib):
    """FGDM_GROUP_MAX=2 with the UNet and three ControlNets: apply_model's runs of two walks, each scheduled on its own"""
    w = [A, B_, PLAIN, C_]
    steps, _ = plan(lib, [w] * 4, chunk=2)
    first, _ = plan(lib, [w] * 2)
    assert first == [[(0, 0), (1, 0)], [(0, 1), (1, 1)], [(0, 2)], [(1, 2)], [(0, 3), (1, 3)]]
    assert steps == first + [[(k + 2, u) for k, u in st] for st in first]
    odd, _ = plan(lib, [w] * 3, chunk=2)                 # the last run holds one walk
    assert odd == first + [[(2, u)] for u in range(4)]
    whole, _ = plan(lib, [w] * 4, chunk=0)
    assert groups(whole) == [[(k, u) for k in range(4)] for u in (0, 1, 3)]


def test_single_and_empty_walks(lib):
    assert plan(lib, [])[0] == []
    assert plan(lib, [[], []])[0] == []
    assert plan(lib, [[A, PLAIN, A]])[0] == [[(0, 0)], [(0, 1)], [(0, 2)]]
    steps, _ = plan(lib, [[], [A, B_], [], [A, B_]])
    assert steps == [[(1, 0), (3, 0)], [(1, 1), (3, 1)]]
    assert lib.fgdm_replay_plan(1, None, None, None, None, 5, 0, None, 0, None) < 0
    assert lib.fgdm_replay_plan(0, None, None, None, None, 0, 0, None, 0, None) < 0        # group_max < 1
