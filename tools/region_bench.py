#!/usr/bin/env python
"""Region statistics (csrc/region.hip; kernels.KernelSpec.region_statistics, region_histogram, region_quantiles) on one 3584 x 3584
tile of synthetic_tissue, labelled by label_instances (labels 1..n), and its uint8 gray plane:
  moments                       init, one pass over the tiles, finish: 4 + 1 bytes read per pixel
  histogram                     memset of the table, one pass: 4 + 1 bytes read per pixel
  histogram+quantiles           ... and one wave per row for three quantiles
  stain_features (ring 0, 6)    the public function on an H&E-like tile: separate_stains, two (four) moments and histogram passes,
                                the ring's distance transform, and its one host read
  torch: moments                bincount (count), bincount with float64 weights (sum, sumsq), scatter_reduce amin / amax -- through
                                int64 copies of the labels and values; no positions
  torch: histogram              bincount(labels * 256 + values)
The stock formulations are compared with this code for equality before anything is timed.  Device events around ``--batch`` calls
in a row, the median, minimum and maximum over ``--repeats`` (>= 20) such windows after a warm-up; the cases take turns, window by
window.  Compulsory bytes over the measured time are given as a fraction of the 8 TB/s of HBM.  No time is asserted anywhere.

    python tools/region_bench.py --out profiles/region_bench.json
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

HBM_BYTES_PER_S = 8e12
BYTES_PER_PIXEL = 5                                                              # an int32 label and a uint8 value
QUANTILES = [1000, 5000, 9000]


def torch_moments(labels, values, rows):
    import torch
    lab, val = labels.reshape(-1).to(torch.int64), values.reshape(-1).to(torch.int64)
    w = val.to(torch.float64)
    count = torch.bincount(lab, minlength=rows)
    total = torch.bincount(lab, weights=w, minlength=rows)
    sumsq = torch.bincount(lab, weights=w * w, minlength=rows)
    mn = torch.full((rows,), 2 ** 31, dtype=torch.int64, device=lab.device).scatter_reduce(0, lab, val, 'amin')
    mx = torch.full((rows,), -2 ** 31, dtype=torch.int64, device=lab.device).scatter_reduce(0, lab, val, 'amax')
    return count, total, sumsq, mn, mx


def torch_histogram(labels, values, rows):
    import torch
    key = labels.reshape(-1).to(torch.int64) * 256 + values.reshape(-1).to(torch.int64)
    return torch.bincount(key, minlength=rows * 256).view(rows, 256)


def step(a):
    """Every case on the GPU: prints one JSON object."""
    import numpy as np
    import torch
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import kernels, nuclei

    dev = torch.device('cuda:0')
    px = a.size * a.size
    labels_np, gray_np = nuclei.synthetic_tissue(a.size, a.size, a.nuclei)
    plane = torch.from_numpy(gray_np).to(dev)
    L, n = nuclei.label_instances(torch.from_numpy(labels_np).to(dev))
    tile = torch.stack([plane, 255 - plane // 2, 128 + plane // 4], dim=2).contiguous()
    kept = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    table = kernels.get()
    rows = n + 1

    # the stock formulations agree with this code
    (count, total, sumsq, mn, mx, _, _), meta = table.region_statistics(L, plane, n)
    hist, _ = table.region_histogram(L, plane, n)
    assert int(meta) == 0
    t_count, t_total, t_sumsq, t_mn, t_mx = torch_moments(L, plane, rows)
    some = count > 0
    assert torch.equal(count.to(torch.int64), t_count) and torch.equal(total, t_total.to(torch.int64))
    assert torch.equal(sumsq, t_sumsq.to(torch.int64))
    assert torch.equal(mn.to(torch.int64)[some], t_mn[some]) and torch.equal(mx.to(torch.int64)[some], t_mx[some])
    assert torch.equal(hist.to(torch.int64), torch_histogram(L, plane, rows))

    cases = [('moments', lambda: table.region_statistics(L, plane, n), a.batch),
             ('histogram', lambda: table.region_histogram(L, plane, n), a.batch),
             ('histogram+quantiles', lambda: table.region_quantiles(table.region_histogram(L, plane, n)[0], QUANTILES), a.batch),
             ('stain_features/ring0', lambda: nuclei.stain_features(L, tile, kept, max_label=n), 1),
             ('stain_features/ring6', lambda: nuclei.stain_features(L, tile, kept, ring=6, max_label=n), 1),
             ('separate_stains', lambda: nuclei.separate_stains(tile, planes=(0, 1)), a.batch),
             ('ring_labels/6', lambda: nuclei.ring_labels(L, 6), 1),
             ('torch_moments', lambda: torch_moments(L, plane, rows), 1),
             ('torch_histogram', lambda: torch_histogram(L, plane, rows), 1)]
    for _, fn, _ in cases:                                                       # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in cases}
    for _ in range(a.repeats):
        for name, fn, batch in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(batch):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / batch)
    rec = dict(device=torch.cuda.get_device_name(0), tile_side=table.region_tile, table_slots=table.region_slots, labels=n,
               background_fraction=round(float((L == 0).sum()) / px, 4), cases={})
    for name, _, _ in cases:
        ts = times[name]
        row = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if name in ('moments', 'histogram', 'histogram+quantiles'):
            row['compulsory_bytes'] = BYTES_PER_PIXEL * px
            row['floor_us_at_hbm_rate'] = round(BYTES_PER_PIXEL * px / HBM_BYTES_PER_S * 1e6, 2)
            row['fraction_of_hbm'] = round(BYTES_PER_PIXEL * px / (np.median(ts) * 1e-3) / HBM_BYTES_PER_S, 5)
            row['ns_per_pixel'] = round(float(np.median(ts)) * 1e6 / px, 4)
        rec['cases'][name] = row
    c = rec['cases']
    c['moments']['torch_over_this'] = round(c['torch_moments']['ms_median'] / c['moments']['ms_median'], 2)
    c['histogram']['torch_over_this'] = round(c['torch_histogram']['ms_median'] / c['histogram']['ms_median'], 2)
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
    rec = dict(plane='%dx%d' % (a.size, a.size), nuclei=a.nuclei, quantiles=QUANTILES, repeats=a.repeats, batch=a.batch,
               hbm_bytes_per_s=HBM_BYTES_PER_S)
    cmd = ['timeout', '-k', '10', str(a.step_limit), sys.executable, os.path.abspath(__file__), '--step', '--size', str(a.size),
           '--nuclei', str(a.nuclei), '--repeats', str(a.repeats), '--batch', str(a.batch)]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)   # the GPU step under its own time limit
    if done.returncode != 0:
        sys.stdout.write(done.stdout)
        print('region_bench: the step ended with status %d; stopping' % done.returncode, file=sys.stderr)
        sys.exit(done.returncode)
    rec.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
