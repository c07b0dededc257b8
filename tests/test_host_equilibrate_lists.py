"""CPU tests of the column patterns of tests/test_gpu_equilibrate_lists.py: each pattern, replayed through the compactions
ebm_equilibrate makes (NumPy, with the equilibrium years written beside the member types, which the GPU test asserts of its
reference), really has the waves and rounds it is there for.  compact_active_kernel works on 1024 entries a round, 64 a
wave; at the first compaction (after year 2) the list is still the identity, so wave w holds columns 64 w .. 64 w + 63."""
import numpy as np
import pytest

import test_gpu_equilibrate_lists as L

BIG = ["1024", "1025", "2100"]


def first_compaction(name, model="MIZ"):
    types = L.build_pattern(name)
    year, cur, keep = L.replay(types, L.nominal_years(model))[0]
    assert year == 2 and np.array_equal(cur, np.arange(len(types)))
    return types, keep


def waves(keep):
    """keep flags -> [nwaves, 64] (the last wave padded with False, as the kernel's `i < n`)."""
    n = -(-len(keep) // 64) * 64
    return np.pad(keep, (0, n - len(keep))).reshape(-1, 64)


@pytest.mark.parametrize("name", sorted(L.PATTERNS))
def test_pattern_is_complete(name):
    types = L.build_pattern(name)
    assert len(types) == L.PATTERNS[name][0]
    assert np.array_equal(types, L.build_pattern(name)), "the fill is seeded"
    if name.startswith("tail"):
        return
    assert sorted(set(types.tolist())) == list(range(len(L.TYPE_NAMES))), "every type has a member"
    assert (types == L.NAN).sum() == 1
    for model in ("MIZ", "Classic"):
        Y = L.nominal_years(model)[types]
        assert len(set(Y[Y < L.MAX_YEARS].tolist())) >= 3


@pytest.mark.parametrize("model", ["MIZ", "Classic"])
@pytest.mark.parametrize("name", BIG)
def test_waves_of_the_first_round(name, model):
    types, keep = first_compaction(name, model)
    w = waves(keep)
    count = w.sum(axis=1)
    assert count[0] == 0, "wave 0 is empty: wave_base[1] = 0"
    later_empty = [i for i in range(1, 16) if count[i] == 0 and count[:i].sum() > 0 and count[i + 1:16].sum() > 0]
    assert later_empty, "an empty wave between live ones: wave_base[w + 1] == wave_base[w] != 0"
    only0 = [i for i in range(16) if count[i] == 1 and w[i, 0]]
    only63 = [i for i in range(16) if count[i] == 1 and w[i, 63]]
    but63 = [i for i in range(16) if count[i] == 63 and not w[i, 63]]
    full = [i for i in range(16) if count[i] == 64]
    assert only0 and only63 and but63 and full, (only0, only63, but63, full)
    # the scan: a live wave with more than one non-zero count before it, and a base that is no multiple of 64
    base = np.concatenate([[0], np.cumsum(count[:16])])
    assert any(count[i] and (count[:i] > 0).sum() > 1 and base[i] % 64 for i in range(16))
    # a full wave after a lane-0-only one: its first survivor's slot is the one an off-by-one `below` of the wave before hits
    assert any(i + 1 < 16 and count[i + 1] > 0 for i in only0)
    assert keep[1023] and types[1023] == L.NEVER, "the round's last entry survives"


@pytest.mark.parametrize("name", ["65", "65_tail_dies"])
def test_two_waves_one_of_a_single_lane(name):
    types, keep = first_compaction(name)
    w = waves(keep)
    assert w.shape == (2, 64)
    if name == "65":
        assert w[0, :63].all() and not w[0, 63] and w[1, 0], "every lane but 63 survives; the single lane of wave 1 survives"
    else:
        assert w[0, 63] and 0 < w[0].sum() < 64 and not w[1].any(), "lane 63 survives; nothing survives in wave 1"
    # and the list is longer than one wave at no later compaction: the second wave is this one's only
    assert all(len(cur) <= 64 for _, cur, _ in L.replay(types, L.nominal_years("MIZ"))[1:])


def test_1024_is_exactly_one_round():
    types, keep = first_compaction("1024")
    assert len(keep) == 1024 and waves(keep).shape == (16, 64)


def test_1025_second_round_of_one_entry():
    types, keep = first_compaction("1025")
    assert len(keep) == 1025 and types[1023] != types[1024]
    assert keep[1023] and keep[1024], "both sides of the round boundary survive: slot total + 0 of round 1"
    assert 0 < keep[:1024].sum() < 1024


def test_2100_an_empty_round_between_live_ones():
    types, keep = first_compaction("2100")
    rounds = [keep[0:1024], keep[1024:2048], keep[2048:]]
    assert len(rounds[2]) == 52, "three rounds, the last one short"
    assert rounds[0].sum() > 0 and rounds[1].sum() == 0 and rounds[2].sum() > 0, "total is carried unchanged across round 1"
    assert (types[1024:2048] == L.E2).all() and types[1023] != types[1024]
    assert keep[1023] and keep[2048] and 0 < rounds[2].sum() < 52
    # the compaction after it runs over a list of many waves that is far from the identity, columns of round 2 among them
    year, cur, keep3 = L.replay(types, L.nominal_years("MIZ"))[1]
    assert year == 3 and len(cur) > 512 and len(cur) % 64 and (cur != np.arange(len(cur))).mean() > 0.9
    assert (cur >= 2048).any() and 0 < keep3[cur >= 2048].sum() < (cur >= 2048).sum()


@pytest.mark.parametrize("name", BIG + ["65", "65_tail_dies"])
@pytest.mark.parametrize("model", ["MIZ", "Classic"])
def test_every_compaction_shrinks_the_list(name, model):
    types = L.build_pattern(name)
    steps = L.replay(types, L.nominal_years(model))
    assert [y for y, _, _ in steps] == [2, 3, 4, 5]
    for y, cur, keep in steps:
        assert 0 < keep.sum() < len(cur), (y, keep.sum(), len(cur))
        assert np.all(np.diff(cur) > 0), "stable: the list stays sorted"
    if name in BIG:
        assert all(len(cur) > 64 for _, cur, _ in steps), "more than one wave in every year"


@pytest.mark.parametrize("name, active", [("tail3", [3, 3, 3, 2, 1, 1]), ("tail2", [2, 2, 2, 1, 1])])
def test_tails_pass_through_one_active_column(name, active):
    Y = L.nominal_years("MIZ")[L.build_pattern(name)]
    assert [int((Y >= y).sum()) for y in range(1, int(Y.max()) + 1)] == active
    # half = nactive / 2: 1, 1, 0
    assert [n // 2 for n in sorted(set(active), reverse=True)][-1] == 0


def test_launch_formula():
    years = np.array([2, 3, 6, 6])
    assert L.launches_expected(years, 200, 64, 1) == 4 * 6
    # two chains: 4, 4, 3, 2, 2, 2 active -> two chains every year
    assert L.launches_expected(years, 200, 64, 2) == 4 * 12
    assert L.launches_expected(np.array([3, 5]), 200, 1, 2) == 200 * (2 + 2 + 2 + 1 + 1)
