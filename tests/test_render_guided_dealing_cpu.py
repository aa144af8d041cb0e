"""CPU tests of the GUIDED schedule of ray units in the pipelined render kernel (g-nerf_amd/csrc/pipe_dealing.h: units of 8 rays that
shrink to 4, 2 and 1 as an XCD's range runs out).  tests/cabi/guided_dealing_sim.cpp compiles the header for the host, checks the
schedule of every range on its own -- unit_start(k + 1) = unit_start(k) + unit_len(k), lengths never increase, seq() answers -1 only
past x1, an ineligible range gets exactly the uniform schedule -- and then lets W simulated workgroups take units from one counter the
way the kernel's scalar wave does, in random and adversarial orders: every position of [x0, x1) must be produced exactly once."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCHEDULES = {'random': 0, 'one_takes_everything': 1, 'round_robin': 2, 'one_stalls_on_its_first_unit': 3}


@pytest.fixture(scope='module')
def sim(tmp_path_factory):
    assert shutil.which('g++') is not None, 'the build needs g++ anyway (csrc/build.sh)'
    exe = str(tmp_path_factory.mktemp('guided_dealing') / 'guided_dealing_sim')
    subprocess.run(['g++', '-O1', '-std=c++17', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'g-nerf_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'cabi', 'guided_dealing_sim.cpp'), '-o', exe], check=True, capture_output=True, text=True)
    return exe


def _run(sim, *args):
    out = subprocess.run([sim] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith('ok '), (args, out.stdout, out.stderr)
    return int(out.stdout.split()[1])


# (range length of each of the 8 XCDs, workgroups per XCD).  With W = 128 and c = 1 the levels of 1, 2 and 4 rays hold 128, 256 and 512
# rays behind the 1 024 of the workgroups' own units: empty range; shorter than W units; exactly W units; W units and a remainder that
# leaves one extra unit at each level (1, 2, 4 rays, and all three: 7); ranges that end inside the 1-, 2- and 4-ray levels with such
# remainders; all levels full with a remainder in the 8-ray units; config 2's 8 192; the same on pipe<2>'s 96 workgroups.
RANGES = [(0, 128), (5, 128), (1023, 128), (1024, 128), (1025, 128), (1026, 128), (1028, 128), (1031, 128), (1024 + 100, 128),
          (1024 + 128 + 2 * 77 + 1, 128), (1024 + 128 + 256 + 4 * 33 + 3, 128), (1024 + 896 + 8 * 5 + 7, 128), (8192, 128), (2048, 96), (96 * 8 + 3, 96)]


@pytest.mark.parametrize('schedule', sorted(SCHEDULES))
@pytest.mark.parametrize('c,smallest', [(1, 1), (2, 1), (1, 2)])
def test_guided_schedule_deals_every_position_exactly_once(sim, schedule, c, smallest):
    for length, w in RANGES:
        assert _run(sim, 'one', 8 * length, 8, w, 8, c, smallest, SCHEDULES[schedule], 1) == 8 * length


@pytest.mark.parametrize('schedule', sorted(SCHEDULES))
def test_ragged_totals_give_the_xcds_ranges_of_different_lengths(sim, schedule):
    # (total, workgroups per XCD): the GPU test's ragged cases and totals whose eighths differ by one ray around the eligibility threshold
    for total, w in [(10007, 128), (3 * 4099, 128), (9216, 128), (8 * 1024 + 3, 128), (8 * 1024 - 3, 128), (8 * 24 + 5, 3), (1, 1)]:
        for seed in (1, 2):
            assert _run(sim, 'one', total, 8, w, 8, 1, 1, SCHEDULES[schedule], seed) == total


@pytest.mark.parametrize('schedule', sorted(SCHEDULES))
@pytest.mark.parametrize('w', [1, 3, 4])
def test_every_range_length_up_to_all_levels_full_and_beyond(sim, schedule, w):
    for c, smallest in [(1, 1), (2, 1), (2, 2)]:
        top = 8 * w + 7 * c * w + 19
        assert _run(sim, 'sweep', top, w, 8, c, smallest, SCHEDULES[schedule], 5) == top * (top + 1) // 2


@pytest.mark.parametrize('unit,c', [(8, 0), (4, 1), (3, 2), (1, 1), (16, 1)])
def test_other_units_and_c_zero_keep_the_uniform_schedule(sim, unit, c):
    """guided dealing is for 8-ray units: any other unit, or c = 0, must give unit k = rays [k unit, (k + 1) unit) (checked in the sim)"""
    for schedule in sorted(SCHEDULES.values()):
        assert _run(sim, 'one', 4 * 10007, 8, 128, unit, c, 1, schedule, 3) == 4 * 10007
        assert _run(sim, 'sweep', 70, 3, unit, c, 1, schedule, 3) == 70 * 71 // 2
