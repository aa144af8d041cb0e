"""CPU tests of how the pipelined render kernel hands rays to its workgroups (g-nerf_amd/csrc/pipe_dealing.h, the plain C++ the kernel's
scalar wave runs): tests/cabi/dealing_sim.cpp compiles it for the host and lets W simulated workgroups per XCD make their moves in
an order a seeded scheduler picks.  Whatever the order, every position of every XCD's range must be produced exactly once and
nothing outside it -- the property that makes on-demand dealing a matter of speed only.  Also: the per-launch figures of
tools/wg_lifetimes.py on made-up stamps."""

import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def sim(tmp_path_factory):
    assert shutil.which('g++') is not None, 'the build needs g++ anyway (csrc/build.sh)'
    exe = str(tmp_path_factory.mktemp('dealing') / 'dealing_sim')
    subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'g-nerf_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'cabi', 'dealing_sim.cpp'), '-o', exe], check=True, capture_output=True, text=True)
    return exe


# (total positions, workgroups per XCD, unit): config 2 on pipe<1> / pipe<2>, ragged totals, more workgroups than units, one-ray units
SHAPES = [(65536, 128, 8), (65536, 96, 8), (4 * 10007, 128, 8), (10007, 5, 3), (77, 16, 8), (8, 128, 1), (1, 1, 1), (3 * 4099, 64, 16)]


@pytest.mark.parametrize('on_demand', [1, 0])
@pytest.mark.parametrize('schedule', [0, 1, 2])
@pytest.mark.parametrize('shape', SHAPES)
def test_every_position_is_dealt_exactly_once(sim, shape, schedule, on_demand):
    total, w, unit = shape
    for seed in (1, 2, 3):
        out = subprocess.run([sim, str(total), str(w), str(unit), str(seed), str(schedule), str(on_demand)], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.strip() == f'ok {total}', (shape, schedule, on_demand, seed, out.stdout, out.stderr)


def test_lifetime_summary_on_made_up_stamps():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import wg_lifetimes
    finally:
        sys.path.pop(0)
    # two XCDs of two workgroups; ticks of 10 ns.  Last end 1000, ends 1000, 800, 600, 1000 -> idle (0 + 200 + 400 + 0) / (4 x 1000)
    r = wg_lifetimes.summarize(xcd=[0, 0, 1, 1], cu=[0, 1, 256, 256], start=[0, 0, 100, 0], end=[1000, 800, 600, 1000])
    assert r['workgroups'] == 4 and r['span_us'] == 10.0 and r['start_spread_us'] == 1.0
    assert r['idle_slot_time'] == pytest.approx(0.15)
    assert r['lifetime_us']['max'] == 10.0 and r['lifetime_us']['mean'] == pytest.approx(8.25) and r['lifetime_us']['max_over_mean'] == pytest.approx(1000 / 825)
    assert r['per_xcd']['0']['cus'] == 2 and r['per_xcd']['1']['cus'] == 1
    assert r['per_xcd']['0']['idle_slot_time_in_xcd'] == pytest.approx(200 / 2000) and r['per_xcd']['1']['last_end_us'] == 10.0
