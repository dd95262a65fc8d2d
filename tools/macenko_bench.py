#!/usr/bin/env python
"""The two reductions of stain estimation (csrc/stain.hip k_od_scan; kernels.KernelSpec.od_moments, angle_histogram) on one 3584 x 3584
rendered two-stain tile, beside stain_separate with one plane -- which reads the same bytes -- and beside the same steps written with
stock torch ops on the same device:
  od_moments       (plain, bool within)          vs  float32 log, a mask, torch.cov
  angle_histogram  (plain, bool within, flat)    vs  a matmul with the two eigenvectors, atan2, histc
  estimate_stains  end to end, wall clock: two launches' worth of device work, two host reads, a 3 x 3 eigh, the percentiles
Device events around ``--batch`` calls in a row, the median over ``--repeats`` (>= 20) such windows after a warm-up; the cases take
turns, window by window.  Per kernel also the compulsory bytes (3 + within bytes per pixel) over the measured time, as a fraction of
the 8 TB/s of HBM, and the ratio to stain_separate with one plane from the same run.

Kernel times come from a kernel trace of a few calls, taken in a run of its own and folded into the record afterwards:
    python tools/macenko_bench.py --out profiles/macenko_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o macenko -- python tools/macenko_bench.py --trace
    python tools/macenko_bench.py --parse-trace DIR/.../macenko_kernel_trace.csv --out profiles/macenko_bench.json"""
import argparse
import collections
import csv
import json
import math
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import cgc_net_amd  # noqa: E402,F401
from cgc_net_amd import kernels, nuclei  # noqa: E402
import macenko_ref  # noqa: E402

HBM_BYTES_PER_S = 8e12
TRACE_CALLS = 40
KERNELS = {r'k_od_scan<(false|0)>|k_od_scanIL[bi]0': 'od_moments', r'k_od_scan<(true|1)>|k_od_scanIL[bi]1': 'angle_histogram',
           'k_put_dirs|k_put_words': 'put_dirs', 'k_stain_separate': 'stain_separate'}


def torch_moments(image, beta):
    od = -torch.log(image.to(torch.float32).clamp_(min=1.0) / 255.0).flip(2).reshape(-1, 3)      # R, G, B
    x = od[(od >= beta).all(dim=1)]
    return x, torch.cov(x.t())


def torch_angles(x, plane):
    p = x @ plane                                                                # [n, 2]
    return torch.histc(torch.atan2(p[:, 1], p[:, 0]), bins=kernels.ANGLE_BINS, min=-0.5 * math.pi, max=0.5 * math.pi)


def parse_trace(path):
    """Median microseconds per launch of the kernels of this tool in a rocprofv3 kernel_trace.csv (the trace mode's launches only)."""
    dur = collections.defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            for key, name in KERNELS.items():
                if re.search(key, r['Kernel_Name']):
                    dur[name].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3)
    out = {k: dict(us_median=round(float(np.median(v)), 2), us_min=round(min(v), 2), launches=len(v)) for k, v in dur.items()}
    out['note'] = 'rocprofv3 --kernel-trace --stats of one --trace case: %d calls of each entry, warm-up calls included' % TRACE_CALLS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--repeats', type=int, default=25)
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--trace', default=None, choices=['plain', 'within', 'flat'], nargs='?', const='plain')
    ap.add_argument('--parse-trace', default=None)
    ap.add_argument('--trace-case', default='plain')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.parse_trace:
        rec = json.load(open(a.out))
        rec.setdefault('rocprofv3_kernel_trace_us', {})[a.trace_case] = parse_trace(a.parse_trace)
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps(rec['rocprofv3_kernel_trace_us'][a.trace_case]))
        return
    if a.repeats < 20:
        ap.error('at least twenty repeats')
    dev = torch.device('cuda:0')
    n = a.size * a.size
    tile = torch.from_numpy(np.array(macenko_ref.rendered_tile((a.size, a.size), 0))).to(dev)
    flat = torch.full((a.size, a.size, 3), 60, dtype=torch.uint8, device=dev)
    within = torch.from_numpy(np.random.RandomState(0).rand(a.size, a.size) < 0.7).to(dev)
    table = kernels.get()
    lut, dirs, od_min = nuclei.OD_LUT, nuclei.ANGLE_DIRS, 154
    S, info = nuclei.estimate_stains(tile, return_info=True)
    _, _, e1, e2 = nuclei._plane_of_moments(table.od_moments(tile, 0, lut, od_min).tolist())
    basis = [[int(v) for v in np.rint(4096.0 * e)] for e in (e1, e2)]
    m = nuclei.stain_matrix(S).tolist()
    plane = torch.from_numpy(np.stack([e1, e2], axis=1)).to(dev, torch.float32)
    x, _ = torch_moments(tile, 0.15)
    if a.trace:                                                                  # a few launches of one case for the kernel trace
        w = within if a.trace == 'within' else None
        img = flat if a.trace == 'flat' else tile
        for _ in range(TRACE_CALLS):
            table.od_moments(img, 0, lut, od_min, w)
            table.angle_histogram(img, 0, lut, od_min, basis, dirs, w)
            table.stain_separate(img, 0, lut, m, 1)
        torch.cuda.synchronize()
        return
    cases = [     # name, callable, compulsory bytes per pixel (None: a stock version)
        ('od_moments', lambda: table.od_moments(tile, 0, lut, od_min), 3),
        ('od_moments/within', lambda: table.od_moments(tile, 0, lut, od_min, within), 4),
        ('od_moments/flat', lambda: table.od_moments(flat, 0, lut, od_min), 3),
        ('angle_histogram', lambda: table.angle_histogram(tile, 0, lut, od_min, basis, dirs), 3),
        ('angle_histogram/within', lambda: table.angle_histogram(tile, 0, lut, od_min, basis, dirs, within), 4),
        ('angle_histogram/flat', lambda: table.angle_histogram(flat, 0, lut, od_min, basis, dirs), 3),
        ('stain_separate/1_plane', lambda: table.stain_separate(tile, 0, lut, m, 1), 4),
        ('torch_log_mask_cov', lambda: torch_moments(tile, 0.15), None),
        ('torch_matmul_atan2_histc', lambda: torch_angles(x, plane), None),
    ]
    for _, fn, _ in cases:                                # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(a.repeats):
        for name, fn, _ in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.batch):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / a.batch)
    whole = []
    for _ in range(a.repeats):                            # end to end: wall clock, the two host reads included
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nuclei.estimate_stains(tile)
        whole.append((time.perf_counter() - t0) * 1e3)
    rec = dict(tile='%dx%d' % (a.size, a.size), repeats=a.repeats, batch=a.batch, device=torch.cuda.get_device_name(0),
               stained_fraction=round(info['n'] / n, 4), skipped=info['skipped'], bins=list(info['bins']), scan_chunk=table.scan_chunk,
               within_fraction=round(float(within.float().mean()), 4), cases={})
    for name, _, bpp in cases:
        ts = times[name]
        row = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if bpp is not None:
            row['compulsory_bytes'] = bpp * n
            row['fraction_of_hbm'] = round(bpp * n / (np.median(ts) * 1e-3) / HBM_BYTES_PER_S, 4)
        rec['cases'][name] = row
    c = rec['cases']
    for name in ('od_moments', 'angle_histogram', 'angle_histogram/flat'):
        c[name]['over_stain_separate_1_plane'] = round(c[name]['ms_median'] / c['stain_separate/1_plane']['ms_median'], 3)
    rec['estimate_stains_wall_ms'] = dict(median=round(float(np.median(whole)), 4), min=round(min(whole), 4), max=round(max(whole), 4),
                                          note='time.perf_counter around one call on an idle stream: both launches, both host reads, eigh, percentiles')
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
