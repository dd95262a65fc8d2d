#!/usr/bin/env python
"""Window sums and the fused local threshold (csrc/window.hip; kernels.KernelSpec.window_sums / local_threshold) on one 3584 x 3584
plane of synthetic_tissue, at window radii 5, 25 and 100, beside the same results from stock torch ops on the same device:
  window_sums                         n, S, Q stored: 1 byte read, 16 written per pixel
  local_threshold                     the fused rule: 1 byte read, 1 written per pixel
  local_threshold + within            1 more byte read per pixel (a bool tissue mask)
  torch: sums                         int64 cumsum tables of the plane and its square (and of the mask), four index_selects each
  torch: sums + rule                  ... and the rule of the contract in int64 elementwise ops
Device events around ``--batch`` calls in a row, the median, minimum and maximum over ``--repeats`` (>= 20) such windows after a
warm-up; the cases take turns, window by window.  Compulsory bytes over the measured time are given as a fraction of the 8 TB/s of HBM
(a 13 MB plane sits in the Infinity Cache).  The two formulations are compared for equality before anything is timed.  No time is
asserted anywhere.

    timeout -k 10 600 python tools/window_bench.py --out profiles/window_bench.json
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o window -- python tools/window_bench.py --trace
    python tools/window_bench.py --parse-trace DIR/.../window_kernel_trace.csv --out profiles/window_bench.json
``--bench-line`` / ``--parent-bench-line`` record the headline of bench.py (a JSON line each) beside the parent commit's: this stage
is not on its path."""
import argparse
import collections
import csv
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cgc_net_amd  # noqa: E402,F401
from cgc_net_amd import kernels, nuclei  # noqa: E402

HBM_BYTES_PER_S = 8e12
RADII = (5, 25, 100)
RULE = dict(k64=13, offset=3, floor=20)
TRACE_CALLS = 10
KERNELS = {r'k_window<false, ?false,|k_windowILb0ELb0E': 'sums', r'k_window<true, ?false,|k_windowILb1ELb0E': 'sums_within',
           r'k_window<false, ?true,|k_windowILb0ELb1E': 'rule', r'k_window<true, ?true,|k_windowILb1ELb1E': 'rule_within'}


def torch_sums(image, r, within=None):
    """window_sums in stock torch ops: summed-area tables in int64, one gather per corner."""
    H, W = image.shape
    dev = image.device
    v = image.to(torch.int64)
    planes = [torch.ones_like(v) if within is None else (within != 0).to(torch.int64)]
    if within is not None:
        v = v * planes[0]
    planes += [v, v * v]
    y, x = torch.arange(H, device=dev), torch.arange(W, device=dev)
    y0, y1 = (y - r).clamp_(min=0), (y + r).clamp_(max=H - 1) + 1
    x0, x1 = (x - r).clamp_(min=0), (x + r).clamp_(max=W - 1) + 1
    out = []
    for p in planes:
        t = torch.zeros(H + 1, W + 1, dtype=torch.int64, device=dev)
        t[1:, 1:] = p.cumsum(0).cumsum(1)
        lo, hi = t.index_select(0, y0), t.index_select(0, y1)
        out.append(hi.index_select(1, x1) - lo.index_select(1, x1) - hi.index_select(1, x0) + lo.index_select(1, x0))
    return out


def torch_rule(image, n, S, Q, k64, offset, floor):
    v = image.to(torch.int64)
    L = 64 * (n * v - S - offset * n)
    D = n * Q - S * S
    L2, k2D = L * L, (k64 * k64) * D
    if k64 >= 0:
        fg = (L > 0) & (L2 > k2D)
    else:
        fg = (L > 0) | ((L == 0) & (D > 0)) | ((L < 0) & (L2 < k2D))
    return fg & (v > floor) & (n >= 1)


def torch_threshold(image, r, within=None):
    return torch_rule(image, *torch_sums(image, r, within), **RULE)


def parse_trace(path):
    """Median microseconds per launch of this stage's kernels in a rocprofv3 kernel_trace.csv (the trace mode's launches only)."""
    dur = collections.defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            for key, name in KERNELS.items():
                if re.search(key, r['Kernel_Name']):
                    dur[name].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3)
                    break
    out = {k: dict(us_median=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_max=round(max(v), 2), launches=len(v))
           for k, v in dur.items()}
    out['note'] = 'rocprofv3 --kernel-trace --stats of one --trace run: %d calls per case at the traced radius, warm-up included' % TRACE_CALLS
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8500)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--batch', type=int, default=5)
    ap.add_argument('--trace', type=int, default=None, nargs='?', const=25, help='a few launches at this radius for a kernel trace')
    ap.add_argument('--parse-trace', default=None)
    ap.add_argument('--trace-radius', type=int, default=25)
    ap.add_argument('--bench-line', default=None, help='a file with the JSON line of bench.py on this commit')
    ap.add_argument('--parent-bench-line', default=None, help='... and on the parent commit')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.parse_trace or a.bench_line or a.parent_bench_line:                     # fold a later run's result into the record
        rec = json.load(open(a.out))
        if a.parse_trace:
            rec.setdefault('rocprofv3_kernel_trace_us', {})['radius_%d' % a.trace_radius] = parse_trace(a.parse_trace)
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
    px = a.size * a.size
    labels_np, gray_np = nuclei.synthetic_tissue(a.size, a.size, a.nuclei)
    plane = torch.from_numpy(gray_np).to(dev)
    within = plane < 170                                                         # a bool mask of the darker two thirds
    table = kernels.get()
    rule = (RULE['k64'], RULE['offset'], RULE['floor'])
    if a.trace is not None:
        for _ in range(TRACE_CALLS):
            table.window_sums(plane, a.trace)
            table.window_sums(plane, a.trace, within)
            table.local_threshold(plane, a.trace, *rule)
            table.local_threshold(plane, a.trace, *rule, within)
        torch.cuda.synchronize()
        return
    cases = []     # name, callable, compulsory bytes per pixel (None: the stock formulation)
    for r in RADII:
        for w, tag in ((None, ''), (within, '+within')):                         # the two formulations agree
            got, want = table.window_sums(plane, r, w), torch_sums(plane, r, w)
            assert all(torch.equal(g.to(torch.int64), x) for g, x in zip(got, want)), r
            assert torch.equal(table.local_threshold(plane, r, *rule, w).bool(), torch_threshold(plane, r, w)), r
        del got, want
        cases += [('window_sums/r%d' % r, lambda r=r: table.window_sums(plane, r), 17),
                  ('local_threshold/r%d' % r, lambda r=r: table.local_threshold(plane, r, *rule), 2),
                  ('local_threshold+within/r%d' % r, lambda r=r: table.local_threshold(plane, r, *rule, within), 3),
                  ('torch_sums/r%d' % r, lambda r=r: torch_sums(plane, r), None),
                  ('torch_sums_rule/r%d' % r, lambda r=r: torch_threshold(plane, r), None),
                  ('torch_sums_rule+within/r%d' % r, lambda r=r: torch_threshold(plane, r, within), None)]
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
    rec = dict(plane='%dx%d' % (a.size, a.size), nuclei=a.nuclei, radii=list(RADII), rule=RULE, repeats=a.repeats, batch=a.batch,
               device=torch.cuda.get_device_name(0), tile_rows=table.window_tile_rows,
               strip_cols={str(r): table.window_strip_cols(r) for r in RADII}, within_fraction=round(float(within.float().mean()), 4),
               hbm_bytes_per_s=HBM_BYTES_PER_S, cases={})
    for name, _, bpp in cases:
        ts = times[name]
        row = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if bpp is not None:
            row['compulsory_bytes'] = bpp * px
            row['floor_us_at_hbm_rate'] = round(bpp * px / HBM_BYTES_PER_S * 1e6, 2)
            row['fraction_of_hbm'] = round(bpp * px / (np.median(ts) * 1e-3) / HBM_BYTES_PER_S, 4)
        rec['cases'][name] = row
    c = rec['cases']
    for r in RADII:
        for ours, stock in (('window_sums/r%d', 'torch_sums/r%d'), ('local_threshold/r%d', 'torch_sums_rule/r%d'),
                            ('local_threshold+within/r%d', 'torch_sums_rule+within/r%d')):
            c[ours % r]['torch_over_this'] = round(c[stock % r]['ms_median'] / c[ours % r]['ms_median'], 2)
    rec['fused_rule_beats_stock_torch_at_every_radius'] = all(
        c['local_threshold/r%d' % r]['ms_max'] < c['torch_sums_rule/r%d' % r]['ms_min'] for r in RADII)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
