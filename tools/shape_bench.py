#!/usr/bin/env python
"""Region geometry (csrc/region.hip; kernels.KernelSpec.region_geometry) on the tile of tools/cooc_bench.py: one 3584 x 3584 tile of
synthetic_tissue, labelled by label_instances (labels 1..n), and its uint8 gray plane for the kernel it is reported against:
  geometry                      one table call: init, the tile kernel (pixels and quads in one launch), the extents of empty rows
  geometry/within               ... with within = labels != 0, the background left out
  geometry/one_label            ... on an image of one label: no mixed quad anywhere, the pixel pass alone
  statistics                    region_statistics of the gray plane in the same run, on the same labels: the number to report against
  histogram                     region_histogram, likewise
  region_shape                  the properties off the tables (torch, float64 on the device)
  shape_features                the public function: the table call, the properties, one host read
  torch: geometry               the pixel tables and the bit quads with stock torch (bincount, scatter_reduce, shifted slices)
The stock formulation is compared with this code for equality, bit for bit, before anything is timed.  Device events around
``--batch`` calls in a row, the median, minimum and maximum over ``--repeats`` (>= 20) such windows after a warm-up; the cases take
turns, window by window (the stock formulation takes seconds per call and is timed over three windows).  ``over_statistics`` is the time of a table call over the time of region_statistics.  The clocks the device
reports (torch.cuda.clock_rate, if this build has it) are recorded beside the times.  No time is asserted anywhere.

    python tools/shape_bench.py --out profiles/shape_bench.json
The tool itself never touches the GPU: the measurement is a step, a child process under ``timeout -k 10 --step-limit``, and a step
that fails ends the run with its exit status.  ``--bench-line`` / ``--parent-bench-line`` record the headline of bench.py (a JSON line
each) beside the parent commit's: this stage is not on its path."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SLOW = ('torch_geometry',)          # cases timed over SLOW_WINDOWS windows only
SLOW_WINDOWS = 3


def torch_geometry(labels, rows, directions, within=None):
    """(count, sums [5, R], extents [R, 8, 2], quads [R, 4], border), int64, with stock torch."""
    import torch
    H, W = labels.shape
    dev = labels.device
    lab = labels.to(torch.int64)
    e = lab if within is None else torch.where(within, lab, torch.full_like(lab, -1))
    yy = torch.arange(H, device=dev)[:, None].expand(H, W)
    xx = torch.arange(W, device=dev)[None, :].expand(H, W)
    on = e >= 0
    l, y, x = e[on], yy[on], xx[on]
    count = torch.bincount(l, minlength=rows)
    sums = torch.stack([torch.zeros(rows, dtype=torch.int64, device=dev).scatter_add_(0, l, v) for v in (y, x, y * y, x * y, x * x)])
    ext = torch.zeros(rows, 8, 2, dtype=torch.int64, device=dev)
    some = count > 0
    for k, (a, b) in enumerate(directions):
        v = a * x + b * y
        lo = torch.full((rows,), 2 ** 40, dtype=torch.int64, device=dev).scatter_reduce_(0, l, v, 'amin')
        hi = torch.full((rows,), -2 ** 40, dtype=torch.int64, device=dev).scatter_reduce_(0, l, v, 'amax')
        ext[:, k, 0], ext[:, k, 1] = torch.where(some, lo, 0), torch.where(some, hi, 0)
    frame = (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)
    border = torch.bincount(l[frame], minlength=rows)
    p = torch.full((H + 2, W + 2), -1, dtype=torch.int64, device=dev)
    p[1:H + 1, 1:W + 1] = e
    c = (p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:])
    keys = []
    for i in range(4):
        first = c[i] >= 0
        for j in range(i):
            first &= c[j] != c[i]
        m = [c[j] == c[i] for j in range(4)]
        n = sum(mm.to(torch.int64) for mm in m)
        diagonal = (m[0] & m[3] & ~m[1] & ~m[2]) | (m[1] & m[2] & ~m[0] & ~m[3])
        cls = torch.where(n == 1, 0, torch.where(n == 3, 3, torch.where(diagonal, 2, 1)))
        sel = first & (n < 4)
        keys.append(c[i][sel] * 4 + cls[sel])
    quads = torch.bincount(torch.cat(keys), minlength=rows * 4).view(rows, 4)
    return count, sums, ext, quads, border


def step(a):
    """Every case on the GPU: prints one JSON object."""
    import numpy as np
    import torch
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import kernels, nuclei

    dev = torch.device('cuda:0')
    labels_np, gray_np = nuclei.synthetic_tissue(a.size, a.size, a.nuclei)
    plane = torch.from_numpy(gray_np).to(dev)
    L, n = nuclei.label_instances(torch.from_numpy(labels_np).to(dev))
    kept = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    table = kernels.get()
    rows = n + 1
    inside = L != 0
    one = torch.ones_like(L)

    # the stock formulation agrees with this code, bit for bit
    for within in (None, inside):
        got, meta = table.region_geometry(L, n, within)
        assert int(meta) == 0
        for g, w in zip(got, torch_geometry(L, rows, nuclei.GEOMETRY_DIRECTIONS, within)):
            assert torch.equal(g.to(torch.int64), w)
    geometry = nuclei.region_geometry(L, max_label=n)
    mixed = (L[:-1, :-1] != L[:-1, 1:]) | (L[:-1, :-1] != L[1:, :-1]) | (L[:-1, :-1] != L[1:, 1:])

    cases = [('geometry', lambda: table.region_geometry(L, n), a.batch),
             ('geometry/within', lambda: table.region_geometry(L, n, inside), a.batch),
             ('geometry/one_label', lambda: table.region_geometry(one, n), a.batch),
             ('statistics', lambda: table.region_statistics(L, plane, n), a.batch),
             ('histogram', lambda: table.region_histogram(L, plane, n), a.batch),
             ('region_shape', lambda: nuclei.region_shape(geometry), 1),
             ('shape_features', lambda: nuclei.shape_features(L, kept, max_label=n), 1),
             ('torch_geometry', lambda: torch_geometry(L, rows, nuclei.GEOMETRY_DIRECTIONS), 1)]
    for name, fn, _ in cases:                                                    # warm-up: code objects, the allocator's blocks
        for _ in range(1 if name in SLOW else 3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for window in range(a.repeats):
        for name, fn, batch in cases:
            if name in SLOW and window >= SLOW_WINDOWS:                          # seconds per call: a few windows show the order of magnitude
                continue
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(batch):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / batch)
    try:
        clock_mhz = int(torch.cuda.clock_rate(0))
    except Exception:                                                            # not every build reports it
        clock_mhz = None
    rec = dict(device=torch.cuda.get_device_name(0), clock_mhz_after=clock_mhz, tile_side=table.region_tile, table_slots=table.region_slots,
               labels=n, background_fraction=round(float((L == 0).sum()) / (a.size * a.size), 4),
               mixed_quad_fraction=round(float(mixed.sum()) / mixed.numel(), 4), label_bytes=int(L.numel() * 4), cases={})
    for name, _, _ in cases:
        ts = times[name]
        rec['cases'][name] = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
    c = rec['cases']
    stats = c['statistics']['ms_median']
    for name in ('geometry', 'geometry/within', 'geometry/one_label'):
        c[name]['over_statistics'] = round(c[name]['ms_median'] / stats, 3)
        c[name]['label_gbytes_per_s'] = round(rec['label_bytes'] / c[name]['ms_median'] / 1e6, 1)      # one read of the labels over the call
    c['geometry']['torch_over_this'] = round(c['torch_geometry']['ms_median'] / c['geometry']['ms_median'], 2)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8500)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--batch', type=int, default=5)
    ap.add_argument('--step', action='store_true', help='run the measurement on the GPU (what the tool starts)')
    ap.add_argument('--step-limit', type=int, default=300, help='seconds the step may take')
    ap.add_argument('--bench-line', default=None, help='a file with the JSON line of bench.py on this commit')
    ap.add_argument('--parent-bench-line', default=None, help='... and on the parent commit')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.bench_line or a.parent_bench_line:                                      # fold a later run's result into the record
        rec = json.load(open(a.out))
        for key, path in (('this_commit', a.bench_line), ('parent_commit', a.parent_bench_line)):
            if path:
                line = [ln for ln in open(path).read().splitlines() if ln.startswith('{')][-1]
                rec.setdefault('bench_py', {})[key] = json.loads(line)
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)
        print(json.dumps(rec['bench_py']))
        return
    if a.repeats < 20:
        ap.error('at least twenty repeats')
    if a.step:
        step(a)
        return
    rec = dict(plane='%dx%d' % (a.size, a.size), nuclei=a.nuclei, repeats=a.repeats, batch=a.batch)
    cmd = ['timeout', '-k', '10', str(a.step_limit), sys.executable, os.path.abspath(__file__), '--step', '--size', str(a.size),
           '--nuclei', str(a.nuclei), '--repeats', str(a.repeats), '--batch', str(a.batch)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)   # the GPU step under its own time limit
    if done.returncode != 0:
        sys.stdout.write(done.stdout)
        print('shape_bench: the step ended with status %d; stopping' % done.returncode, file=sys.stderr)
        sys.exit(done.returncode)
    rec.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
