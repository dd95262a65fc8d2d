#!/usr/bin/env python
"""The two kernels of stain normalisation (csrc/stain.hip k_od_scan<SCAN_CONC>, k_od_recolor; kernels.KernelSpec.concentration_histogram,
od_recolor) on one 3584 x 3584 rendered two-stain tile, beside their siblings in the same run and beside the same steps written with
stock torch ops on the same device:
  concentration_histogram (plain, bool within, flat)   beside od_moments and angle_histogram, the other bodies of the scan
  od_recolor              (plain, flat)                beside stain_separate with three planes, which reads and writes the same bytes
  torch: float32 log, a matmul with inv(S)[:, :2], a mask, histc twice   /   float32 log, a matmul with A, exp, round, clamp
  normalize_stains        end to end, wall clock, with given and with estimated stains
Device events around ``--batch`` calls in a row, the median over ``--repeats`` (>= 20) such windows after a warm-up; the cases take
turns, window by window.  Per kernel also the compulsory bytes per pixel (3 read, + within, + 3 written by the recolouring) over the
measured time, as a fraction of the 8 TB/s of HBM.  No time is asserted anywhere.

Kernel times come from a kernel trace of a few calls, taken in a run of its own and folded into the record afterwards:
    python tools/normalize_bench.py --out profiles/normalize_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o normalize -- python tools/normalize_bench.py --trace
    python tools/normalize_bench.py --parse-trace DIR/.../normalize_kernel_trace.csv --out profiles/normalize_bench.json
``--bench-line`` / ``--parent-bench-line`` record the headline of bench.py (a JSON line each) beside the parent commit's: this stage
is not on its path."""
import argparse
import collections
import csv
import json
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
KERNELS = {r'k_od_scan<0>|k_od_scanILi0': 'od_moments', r'k_od_scan<1>|k_od_scanILi1': 'angle_histogram',
           r'k_od_scan<2>|k_od_scanILi2': 'concentration_histogram', 'k_put_words': 'put_words', 'k_stain_separate': 'stain_separate',
           'k_od_recolor': 'od_recolor'}


def torch_concentrations(image, inv2, beta):
    od = -torch.log(image.to(torch.float32).clamp_(min=1.0) / 255.0).flip(2).reshape(-1, 3)      # R, G, B
    C = od[(od >= beta).all(dim=1)] @ inv2                                                       # [n, 2]
    return torch.histc(C[:, 0], bins=512, min=0.0, max=4.0), torch.histc(C[:, 1], bins=512, min=0.0, max=4.0)


def torch_recolor(image, A):
    od = -torch.log(image.to(torch.float32).clamp_(min=1.0) / 255.0).flip(2)
    return (255.0 * torch.exp(-(od @ A))).round_().clamp_(0.0, 255.0).flip(2).to(torch.uint8)


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
    ap.add_argument('--bench-line', default=None, help='a file with the JSON line of bench.py on this commit')
    ap.add_argument('--parent-bench-line', default=None, help='... and on the parent commit')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.parse_trace or a.bench_line or a.parent_bench_line:                     # fold a later run's result into the record
        rec = json.load(open(a.out))
        if a.parse_trace:
            rec.setdefault('rocprofv3_kernel_trace_us', {})[a.trace_case] = parse_trace(a.parse_trace)
        for key, path in (('this_commit', a.bench_line), ('parent_commit', a.parent_bench_line)):
            if path:
                line = [ln for ln in open(path).read().splitlines() if ln.startswith('{')][-1]
                rec.setdefault('bench_py', {})[key] = json.loads(line)
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps({k: rec[k] for k in ('rocprofv3_kernel_trace_us', 'bench_py') if k in rec}))
        return
    if a.repeats < 20:
        ap.error('at least twenty repeats')
    dev = torch.device('cuda:0')
    n = a.size * a.size
    tile = torch.from_numpy(np.array(macenko_ref.rendered_tile((a.size, a.size), 1))).to(dev)
    flat = torch.full((a.size, a.size, 3), 60, dtype=torch.uint8, device=dev)
    within = torch.from_numpy(np.random.RandomState(0).rand(a.size, a.size) < 0.7).to(dev)
    table = kernels.get()
    lut, exp, dirs, od_min = nuclei.OD_LUT, nuclei.EXP_LUT, nuclei.ANGLE_DIRS, 154
    S = nuclei.estimate_stains(tile)
    norm, info = nuclei.normalize_stains(tile, stains=S, return_info=True)
    _, _, e1, e2 = nuclei._plane_of_moments(table.od_moments(tile, 0, lut, od_min).tolist())
    basis = [[int(v) for v in np.rint(4096.0 * e)] for e in (e1, e2)]
    m, mat = nuclei.stain_matrix(S).tolist(), info['matrix'].tolist()
    inv2 = torch.from_numpy(np.linalg.inv(S)[:, :2].copy()).to(dev, torch.float32)
    A = torch.from_numpy(info['matrix'] / 4096.0).to(dev, torch.float32)
    if a.trace:                                                                  # a few launches of one case for the kernel trace
        w = within if a.trace == 'within' else None
        img = flat if a.trace == 'flat' else tile
        for _ in range(TRACE_CALLS):
            table.od_moments(img, 0, lut, od_min, w)
            table.angle_histogram(img, 0, lut, od_min, basis, dirs, w)
            table.concentration_histogram(img, 0, lut, od_min, m, w)
            table.stain_separate(img, 0, lut, m, 7)
            table.od_recolor(img, 0, lut, mat, exp)
        torch.cuda.synchronize()
        return
    cases = [     # name, callable, compulsory bytes per pixel (None: a stock version)
        ('concentration_histogram', lambda: table.concentration_histogram(tile, 0, lut, od_min, m), 3),
        ('concentration_histogram/within', lambda: table.concentration_histogram(tile, 0, lut, od_min, m, within), 4),
        ('concentration_histogram/flat', lambda: table.concentration_histogram(flat, 0, lut, od_min, m), 3),
        ('od_moments', lambda: table.od_moments(tile, 0, lut, od_min), 3),
        ('angle_histogram', lambda: table.angle_histogram(tile, 0, lut, od_min, basis, dirs), 3),
        ('od_recolor', lambda: table.od_recolor(tile, 0, lut, mat, exp), 6),
        ('od_recolor/flat', lambda: table.od_recolor(flat, 0, lut, mat, exp), 6),
        ('stain_separate/3_planes', lambda: table.stain_separate(tile, 0, lut, m, 7), 6),
        ('torch_log_matmul_mask_histc', lambda: torch_concentrations(tile, inv2, 0.15), None),
        ('torch_log_matmul_exp_round', lambda: torch_recolor(tile, A), None),
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
    whole = {'given_stains': [], 'estimated_stains': []}
    for _ in range(a.repeats):                            # end to end: wall clock, the host reads included
        for key, kw in (('given_stains', dict(stains=S)), ('estimated_stains', {})):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nuclei.normalize_stains(tile, **kw)
            torch.cuda.synchronize()
            whole[key].append((time.perf_counter() - t0) * 1e3)
    rec = dict(tile='%dx%d' % (a.size, a.size), repeats=a.repeats, batch=a.batch, device=torch.cuda.get_device_name(0),
               stained_fraction=round(info['n'] / n, 4), bins=list(info['bins']), matrix=mat, scan_chunk=table.scan_chunk,
               within_fraction=round(float(within.float().mean()), 4), cases={})
    for name, _, bpp in cases:
        ts = times[name]
        row = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if bpp is not None:
            row['compulsory_bytes'] = bpp * n
            row['fraction_of_hbm'] = round(bpp * n / (np.median(ts) * 1e-3) / HBM_BYTES_PER_S, 4)
        rec['cases'][name] = row
    c = rec['cases']
    c['od_recolor']['over_stain_separate_3_planes'] = round(c['od_recolor']['ms_median'] / c['stain_separate/3_planes']['ms_median'], 3)
    for sibling in ('od_moments', 'angle_histogram'):
        c['concentration_histogram']['over_' + sibling] = round(c['concentration_histogram']['ms_median'] / c[sibling]['ms_median'], 3)
    rec['normalize_stains_wall_ms'] = {k: dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))
                                       for k, v in whole.items()}
    rec['normalize_stains_wall_ms']['note'] = ('time.perf_counter around one call on an idle stream, synchronised at the end: every launch '
                                               'and host read of the call (one with given stains, three with estimated ones)')
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
