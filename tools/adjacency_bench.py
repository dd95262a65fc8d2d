#!/usr/bin/env python
"""Region adjacency (csrc/adjacency.hip; kernels.KernelSpec.region_adjacency) on one 3584 x 3584 tile, beside the same step written
with stock torch ops on the same device and beside the project's scan kernels that move comparable bytes:
  region_adjacency on the Voronoi cells of synthetic_tissue(3584, 3584, 8500) at max_distance 50, with and without value
  region_adjacency on the raw labels, and on the all-distinct worst case at 1024 x 1024 (every contact its own pair)
  torch: shifted compares, stack, torch.unique(dim=0, return_counts=True), scatter_reduce('amin')
  od_moments (3 bytes per pixel) and histogram_u8 (1 byte per pixel)
  voronoi_graph end to end, wall clock, and its parts
Device events around ``--batch`` calls in a row, the median over ``--repeats`` (>= 20) such windows after a warm-up; the cases take
turns, window by window.  Compulsory bytes are 4 H W, plus 4 H W with value; their rate over the measured time is given as a fraction
of the 8 TB/s of HBM (a 51 MB image sits in the Infinity Cache).  No time is asserted anywhere.

Kernel times come from a kernel trace of a few calls, taken in a run of its own and folded into the record afterwards:
    python tools/adjacency_bench.py --out profiles/adjacency_bench.json
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o adjacency -- python tools/adjacency_bench.py --trace
    python tools/adjacency_bench.py --parse-trace DIR/.../adjacency_kernel_trace.csv --out profiles/adjacency_bench.json
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
import cgc_net_amd  # noqa: E402,F401
from cgc_net_amd import kernels, nuclei  # noqa: E402

HBM_BYTES_PER_S = 8e12
TRACE_CALLS = 20
KERNELS = {r'k_adj_tiles<false>|k_adj_tilesILb0': 'tiles_count', r'k_adj_tiles<true>|k_adj_tilesILb1': 'tiles_records',
           'k_adj_scan': 'scan', 'k_adj_heads': 'heads', 'k_adj_init': 'init', 'k_adj_merge': 'merge',
           r'[Ss]ort|[Rr]adix|onesweep|histogram_kernel': 'torch_sort'}
OFFSETS = {1: ((0, 1), (1, 0)), 2: ((0, 1), (1, 0), (1, 1), (1, -1))}


def torch_adjacency(L, V, connectivity):
    """The contract of region_adjacency in stock torch ops (int32 sums: the tissue's values are small)."""
    H, W = L.shape
    a, b, s = [], [], []
    for dy, dx in OFFSETS[connectivity]:
        ys, yq = slice(0, H - dy), slice(dy, H)
        xs, xq = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        p, q = L[ys, xs], L[yq, xq]
        m = (p != q) & (p != 0) & (q != 0)
        a.append(torch.minimum(p, q)[m])
        b.append(torch.maximum(p, q)[m])
        if V is not None:
            s.append((V[ys, xs] + V[yq, xq])[m])
    ab = torch.stack([torch.cat(a), torch.cat(b)], dim=1)
    pairs, inverse, count = torch.unique(ab, dim=0, return_inverse=True, return_counts=True)
    if V is None:
        return pairs, count
    mn = torch.full((pairs.shape[0],), 2 ** 31 - 1, dtype=torch.int32, device=L.device)
    return pairs, count, mn.scatter_reduce(0, inverse, torch.cat(s), 'amin')


def parse_trace(path):
    """Median microseconds per launch of the kernels of this tool in a rocprofv3 kernel_trace.csv (the trace mode's launches only)."""
    dur = collections.defaultdict(list)
    with open(path) as f:
        for r in csv.DictReader(f):
            for key, name in KERNELS.items():
                if re.search(key, r['Kernel_Name']):
                    dur[name].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) * 1e-3)
                    break
    out = {k: dict(us_median=round(float(np.median(v)), 2), us_min=round(min(v), 2), us_sum_per_call=round(sum(v) / TRACE_CALLS, 2),
                   launches=len(v)) for k, v in dur.items()}
    out['note'] = ('rocprofv3 --kernel-trace --stats of one --trace case: %d calls of region_adjacency, warm-up calls included; torch_sort = '
                   'every kernel of torch.sort between the two library calls' % TRACE_CALLS)
    return out


def wall(fn, repeats):
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(float(np.median(ts)), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8500)
    ap.add_argument('--distance', type=float, default=50.0)
    ap.add_argument('--repeats', type=int, default=25)
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--trace', default=None, choices=['cells_value', 'cells', 'raw', 'distinct'], nargs='?', const='cells_value')
    ap.add_argument('--parse-trace', default=None)
    ap.add_argument('--trace-case', default='cells_value')
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
    labels_np, gray_np = nuclei.synthetic_tissue(a.size, a.size, a.nuclei)
    raw = torch.from_numpy(labels_np).to(dev)
    cells, dist2 = nuclei._grow_euclidean(raw, nuclei._d2max(a.distance, 'distance'))
    value = torch.where(dist2 == nuclei.EDT_INF, 0, nuclei._eighths(dist2))
    del dist2
    distinct = (torch.randperm(1024 * 1024, device=dev, generator=torch.Generator(device=dev).manual_seed(0)) + 1).to(torch.int32).reshape(1024, 1024)
    table = kernels.get()
    if a.trace:                                                                  # a few launches of one case for the kernel trace
        lab, val = {'cells_value': (cells, value), 'cells': (cells, None), 'raw': (raw, None), 'distinct': (distinct, None)}[a.trace]
        for _ in range(TRACE_CALLS):
            table.region_adjacency(lab, 1, val)
        torch.cuda.synchronize()
        return
    rgb = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(a.size, a.size, 3)).astype(np.uint8)).to(dev)
    gray = torch.from_numpy(gray_np).to(dev)
    lut = nuclei.OD_LUT
    got, want = table.region_adjacency(cells, 2, value), torch_adjacency(cells, value, 2)      # the two formulations agree
    assert all(torch.equal(g, w.to(torch.int32)) for g, w in zip(got, want))
    cases = [     # name, callable, pixels, compulsory bytes per pixel (None: not a scan of the label image)
        ('region_adjacency/cells', lambda: table.region_adjacency(cells, 1), n, 4),
        ('region_adjacency/cells+value', lambda: table.region_adjacency(cells, 1, value), n, 8),
        ('region_adjacency/cells+value/connectivity2', lambda: table.region_adjacency(cells, 2, value), n, 8),
        ('region_adjacency/raw', lambda: table.region_adjacency(raw, 1), n, 4),
        ('region_adjacency/all_distinct_1024', lambda: table.region_adjacency(distinct, 1), 1024 * 1024, 4),
        ('region_adjacency/all_distinct_1024/connectivity2', lambda: table.region_adjacency(distinct, 2), 1024 * 1024, 4),
        ('torch_unique/cells', lambda: torch_adjacency(cells, None, 1), n, None),
        ('torch_unique_scatter_reduce/cells+value', lambda: torch_adjacency(cells, value, 1), n, None),
        ('torch_unique/raw', lambda: torch_adjacency(raw, None, 1), n, None),
        ('torch_unique/all_distinct_1024', lambda: torch_adjacency(distinct, None, 1), 1024 * 1024, None),
        ('od_moments', lambda: table.od_moments(rgb, 0, lut, 154), n, 3),
        ('histogram_u8', lambda: table.histogram_u8(gray), n, 1),
    ]
    for _, fn, _, _ in cases:                             # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in cases}
    for _ in range(a.repeats):
        for name, fn, _, _ in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(a.batch):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / a.batch)
    pairs, count, _ = table.region_adjacency(cells, 1, value)
    labels_n = int(torch.unique(raw).numel()) - 1
    rec = dict(tile='%dx%d' % (a.size, a.size), nuclei=a.nuclei, labels=labels_n, max_distance=a.distance, repeats=a.repeats,
               batch=a.batch, device=torch.cuda.get_device_name(0), tile_side=table.adjacency_tile,
               cells=dict(pairs=int(pairs.shape[0]), mean_degree=round(2.0 * pairs.shape[0] / max(labels_n, 1), 3),
                          contacts=int(count.sum()), covered_fraction=round(float((cells != 0).float().mean()), 4)),
               raw=dict(pairs=int(table.region_adjacency(raw, 1)[0].shape[0])),
               all_distinct_1024=dict(pairs=int(table.region_adjacency(distinct, 1)[0].shape[0])), cases={})
    for name, _, px, bpp in cases:
        ts = times[name]
        row = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if bpp is not None:
            row['compulsory_bytes'] = bpp * px
            row['fraction_of_hbm'] = round(bpp * px / (np.median(ts) * 1e-3) / HBM_BYTES_PER_S, 4)
        rec['cases'][name] = row
    c = rec['cases']
    for ours, stock in (('region_adjacency/cells', 'torch_unique/cells'), ('region_adjacency/cells+value', 'torch_unique_scatter_reduce/cells+value'),
                        ('region_adjacency/raw', 'torch_unique/raw'), ('region_adjacency/all_distinct_1024', 'torch_unique/all_distinct_1024')):
        c[ours]['torch_over_this'] = round(c[stock]['ms_median'] / c[ours]['ms_median'], 2)
    kept = torch.unique(raw[raw != 0]).to(torch.int32)
    d2max = nuclei._d2max(a.distance, 'distance')
    rec['voronoi_graph_wall_ms'] = dict(
        whole=wall(lambda: nuclei.voronoi_graph(raw, a.distance, kept), a.repeats),
        whole_without_kept_labels=wall(lambda: nuclei.voronoi_graph(raw, a.distance), a.repeats),
        cells_and_dist2=wall(lambda: nuclei._grow_euclidean(raw, d2max), a.repeats),
        eighths=wall(lambda: nuclei._eighths(value), a.repeats),
        region_adjacency=wall(lambda: nuclei.region_adjacency(cells, 1, value), a.repeats),
        note=('time.perf_counter around one call on an idle stream, synchronised at the end: every launch and host read of the call.  '
              'region_adjacency has two host reads; its kernels alone are in rocprofv3_kernel_trace_us'))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
