"""The wide-team cases of tests/wide_team_cases.py do what they are there for, checked on the ORACLE alone (no GPU, no kernel): the
environment counts put every kind of wave into one launch of the PT = 32 and PT = 64 instances, and the episodes collide, capture,
keep running and mix both values in the adjacencies, so that tests/test_wide_teams_gpu.py compares kernels on states worth comparing."""
import numpy as np
import pytest

from tests import guidance_cases as gc
from tests import guidance_ref
from tests import wide_team_cases as wc


@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_environment_counts_reach_every_kind_of_wave(case):
    kind, P, E, N = case
    L = wc.launch(P, E, N)
    assert L.pt == (32 if P <= 32 else 64) and L.pt // 2 < max(P, E) <= L.pt
    assert L.envs_per_block == (64 // L.pt) * 4 and L.blocks == 3
    if L.pt == 32:   # 8 environments per workgroup; the last live wave holds environment 18 beside a group past N
        assert (N, L.envs_per_block) == (19, 8) and L.full_waves == 9 and L.mixed_waves == 1 and L.dead_waves == 2
    else:            # 4 per workgroup, one per wave; the last workgroup has a wave entirely past N
        assert (N, L.envs_per_block) == (11, 4) and L.full_waves == 11 and L.mixed_waves == 0 and L.dead_waves_in_last_block == 1
    assert L.full_waves + L.mixed_waves + L.dead_waves == 12
    if L.pt == 32:   # one environment fewer and no wave holds a live group beside a dead one
        assert wc.launch(P, E, N - 1).mixed_waves == 0


def test_team_sizes_sit_on_both_edges_of_both_widths():
    for cases in (wc.E3D_CASES, wc.N2N_CASES):
        assert [c[0] for c in cases] == [17, 32, 33, 64] and [wc.lanes(c[0], c[1]) for c in cases] == [32, 32, 64, 64]
    assert wc.lanes(16, 8) == 16 and wc.lanes(8, 8) == 8


@pytest.mark.parametrize("case", wc.CASES, ids=wc.IDS)
def test_episode_collides_captures_keeps_running_and_mixes_the_adjacencies(case):
    kind, P, E, N = case
    ep = wc.episode(*case)
    assert wc.min_initial_distance(ep) > wc.KILL_RADIUS
    p_on = ep["p"][:, :, -1, :] != 0                                       # (T + 1, N, P)
    e_on = (ep["e"][:, :, -1] != 0).reshape(wc.T + 1, N, E)
    db = wc.done_before(ep)
    died = p_on[:-1] & ~p_on[1:]
    collided = died & (ep["reward"] < 0)                                   # reward = captures - (team-mates within the kill radius)
    caught = e_on[:-1] & ~e_on[1:]
    running10 = ~db[10]
    live = p_on & ~db[:, :, None]
    rows = ep["pp_adj"][live]                                              # (rows, P)
    mixed = (rows.min(1) == 0) & (rows.max(1) == 1)
    pe = ep["pe_adj"][live]
    print(f"{wc.IDS(case)}: {int(collided.sum())} pursuers culled by collision, {int(caught.sum())} evaders caught, "
          f"{int(running10.sum())} of {N} environments running at tick 10, pp_adj mixed in {mixed.mean():.2f} of {len(rows)} live rows, "
          f"pe_adj ones {pe.mean():.2f}, done at the end {int(db[-1].sum())}")
    assert collided.any() and caught.any()
    assert running10.any()
    assert mixed.mean() >= 0.5
    assert pe.min() == 0 and pe.max() == 1
    assert ep["done"][-1].all()                                            # the time limit ends what is still running
    # two environments are decided by the upper half of their lane group alone: the lower half is out from the start, the episode runs
    half = wc.lanes(P, E) // 2
    for n in wc.upper_half_envs(N):
        assert not p_on[0, n, :half].any() and p_on[0, n, half:].all() and not ep["done"][0, n], n
    assert wc.upper_half_envs(N)[0] % 2 == 1 and wc.upper_half_envs(N)[1] == N - 1


def _left_out(states):
    """share of the rows of env_n2n guidance states whose bearing is within 1e-9 of an octant boundary, over the GPU test's parameters"""
    n = k = 0
    for p, e in states:
        for lead, sr, gain in gc.PARAMS:
            _, b = guidance_ref.n2n_actions(p, e, gc.N2N_P_VMAX, lead, sr, gain, with_bearing=True)
            skip = guidance_ref.near_octant_boundary(b)
            n += skip.size; k += int(skip.sum())
    return k / n


def test_wide_guidance_states_leave_out_no_more_rows_than_the_narrow_ones():
    narrow = _left_out([gc.records(*gc.n2n_case(P, E)[:2]) for P, E in gc.N2N_PE])
    wide = _left_out([(ep["p"][t], ep["e"][t]) for ep in (wc.episode("n2n", *c) for c in wc.N2N_CASES) for t in wc.GUIDANCE_TICKS])
    print(f"rows left out near an octant boundary: narrow cases {narrow:.4f}, wide cases {wide:.4f}")
    assert wide <= narrow
    for c in wc.CASES:   # the states hold what the guidance kernels branch on: inactive pursuers, an environment without an evader
        ep = wc.episode(*c)
        t = wc.GUIDANCE_TICKS[-1]
        assert (ep["p"][t][:, -1] == 0).any() and (ep["p"][t][:, -1] != 0).any()
        e_on = (ep["e"][t][:, -1] != 0).reshape(c[3], -1)
        assert (~e_on.any(1)).any() and e_on.any(1).any()
