#!/usr/bin/env python
"""split_touching on one 3584 x 3584 tile with each of its growths (nuclei.split_touching; csrc/edt.hip, geodesic.hip, watershed.hip,
reconstruct.hip), on synthetic_tissue(3584, 3584, 8500):
  euclidean  the default: cores grown back by a Euclidean radius
  geodesic   cores grown along chamfer paths inside the mask -- the yardstick of the flood
  flood      the seeded watershed of the negated distance map from the same cores
each with markers='core' (core_radius 3) and, for the two growths along paths, with markers='h_maxima' (h = 1.5 pixels), which puts
morphological reconstruction in front.  The cases take turns, repeat by repeat, so that a drift of the machine falls on all of them
alike.  Per case: the median, the fastest and the slowest of the host-clocked milliseconds per call, a device synchronise before the
clock starts and after the call; the instances found; the relaxation rounds launched by the last call of each stage, and the pointer
jumps of the flood.  'flood_over_geodesic' is the ratio of the medians with the same markers.

    python tools/watershed_bench.py [--repeats 9] [--out profiles/watershed_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cgc_net_amd  # noqa: E402,F401
from cgc_net_amd import kernels, nuclei  # noqa: E402

CASES = (('euclidean', 'core'), ('geodesic', 'core'), ('flood', 'core'), ('geodesic', 'h_maxima'), ('flood', 'h_maxima'))


def call(mask, growth, markers):
    if markers == 'h_maxima':
        return nuclei.split_touching(mask, None, growth=growth, markers='h_maxima', h=1.5)
    return nuclei.split_touching(mask, 3, growth=growth)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8500)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.repeats < 7:
        ap.error('at least seven repeats')
    dev = torch.device('cuda:0')
    mask = torch.from_numpy(nuclei.synthetic_tissue(a.size, a.size, a.nuclei, seed=0)[0] > 0).to(dev)
    table = kernels.get()
    rec = dict(tile='%dx%d' % (a.size, a.size), nuclei=a.nuclei, repeats=a.repeats, device=torch.cuda.get_device_name(0),
               foreground_fraction=round(float(mask.float().mean()), 4), cases={})
    times = {case: [] for case in CASES}
    for case in CASES:                                    # one warm-up each; the launch counts are those of this call
        table.geodesic_rounds = table.reconstruct_rounds = table.watershed_rounds = table.watershed_jumps = None
        _, n = call(mask, *case)
        torch.cuda.synchronize()
        rec['cases']['%s/%s' % case] = dict(instances=n, geodesic_rounds=table.geodesic_rounds, reconstruct_rounds=table.reconstruct_rounds,
                                            watershed_rounds=table.watershed_rounds, watershed_jumps=table.watershed_jumps)
    for _ in range(a.repeats):
        for case in CASES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(mask, *case)
            torch.cuda.synchronize()
            times[case].append((time.perf_counter() - t0) * 1e3)
    for case in CASES:
        ts = times[case]
        rec['cases']['%s/%s' % case].update(ms_median=round(float(np.median(ts)), 3), ms_min=round(min(ts), 3), ms_max=round(max(ts), 3))
    for markers in ('core', 'h_maxima'):
        rec['flood_over_geodesic/' + markers] = round(rec['cases']['flood/' + markers]['ms_median']
                                                      / rec['cases']['geodesic/' + markers]['ms_median'], 3)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
