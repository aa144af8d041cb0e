#!/usr/bin/env python3
"""Record the reference's side of the tests that compare the overlay with a G-NeRF checkout, so that the tests themselves
need only this repository.  Each test module's record_reference() runs that module's scripts on the reference tree: alone
for the API, error-behaviour, renderer, ops and config-1 frame comparisons, and with this repository's overlay in front of it
for generator_reference.npz (the reference's TriPlaneGenerator then renders through the overlay's CPU renderer and ops).
Re-run it when the upstream tree changes, and after a deliberate change to the CPU paths of the overlay's renderer or ops.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_runs.py <G-NeRF checkout>/g_nerf
"""

import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def main():
    ref = os.path.abspath(sys.argv[1])
    assert os.path.isfile(os.path.join(ref, 'training', 'triplane.py')), f'{ref} is not a G-NeRF g_nerf/ directory'
    sys.path.insert(0, os.path.dirname(HERE))
    import test_api_signatures_cpu as api
    import test_gen_videos_cpu as videos
    import test_generator_cpu as gen
    with gzip.open(api.FIXTURE, 'wt') as f:
        json.dump(api.record_reference(ref), f, separators=(',', ':'))
    print('wrote', api.FIXTURE)
    for m in (gen, videos):
        m.record_reference(ref)
        print('wrote', m.FIXTURE)


if __name__ == '__main__':
    main()
