#!/usr/bin/env python
"""Rank filters (csrc/rank.hip; kernels.KernelSpec.rank_filter) on one 3584 x 3584 plane of synthetic_tissue, with the disk and the
square at radii 1, 3, 7, 15 and 63:
  median                              one launch: 1 byte read, 1 written per pixel
  quantile_range (0.05, 0.95)         one launch, both quantiles from one histogram: 1 byte read, 1 written per pixel
  local_entropy (r = 3 and 15)        one launch: 1 byte read, 4 written per pixel
  erode                               csrc/morph.hip with the same footprint on the same plane: the same compulsory bytes -- a floor
  torch: median (square, r = 1, 3)    F.unfold of a replicate-padded float32 copy in strips of rows, then kthvalue over the window;
                                      compared with ``median`` for equality where the footprint is whole before anything is timed
Device events around ``--batch`` calls in a row (one call at r >= 15 and for the stock formulation), the median, minimum and maximum
over ``--repeats`` (>= 20) such windows after a warm-up; the cases take turns, window by window.  Compulsory bytes over the measured
time are given as a fraction of the 8 TB/s of HBM (a 13 MB plane sits in the Infinity Cache).  No time is asserted anywhere.

    python tools/rank_bench.py --out profiles/rank_bench.json
The tool itself never touches the GPU: every footprint is a step, a child process of its own under ``timeout -k 10 --step-limit``, and
the first step that fails ends the run with its exit status.  ``--bench-line`` / ``--parent-bench-line`` record the headline of bench.py
(a JSON line each) beside the parent commit's: this stage is not on its path."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
KINDS = ('disk', 'square')
RADII = (1, 3, 7, 15, 63)
ENTROPY_RADII = (3, 15)
TORCH_RADII = (1, 3)
RANGE = (0.05, 0.95)
BYTES_PER_PIXEL = {'median': 2, 'quantile_range': 2, 'erode': 2, 'local_entropy': 5}
STRIP_ROWS = 512


def width(kind, r, dy):
    if kind == 'square':
        return r
    w = 0
    while (w + 1) ** 2 + dy * dy <= r * r:
        w += 1
    return w


def torch_median(plane, r):
    """The median of the (2 r + 1)^2 square in stock torch ops, in strips of rows; the border is replicated, so the result equals the
    clipped median only where the footprint is whole."""
    import torch
    import torch.nn.functional as F
    H, W = plane.shape
    k = 2 * r + 1
    padded = F.pad(plane.to(torch.float32)[None, None], (r, r, r, r), mode='replicate')
    out = torch.empty(H, W, dtype=torch.uint8, device=plane.device)
    for y0 in range(0, H, STRIP_ROWS):
        y1 = min(y0 + STRIP_ROWS, H)
        cols = F.unfold(padded[:, :, y0:y1 + 2 * r], (k, k))                      # [1, k^2, rows * W]
        out[y0:y1] = cols.kthvalue(k * k // 2 + 1, dim=1).values.view(y1 - y0, W).to(torch.uint8)
    return out


def step(a):
    """One footprint, every radius and operation, on the GPU: prints one JSON object."""
    import numpy as np
    import torch
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import kernels, nuclei

    kind = a.step
    dev = torch.device('cuda:0')
    px = a.size * a.size
    _, gray_np = nuclei.synthetic_tissue(a.size, a.size, a.nuclei)
    plane = torch.from_numpy(gray_np).to(dev)
    table = kernels.get()

    cases = []                                                                   # name, callable, calls per window
    for r in RADII:
        batch = a.batch if r < 15 else 1
        cases += [('median/r%d' % r, lambda r=r: nuclei.median(plane, r, kind), batch),
                  ('quantile_range/r%d' % r, lambda r=r: nuclei.quantile_range(plane, r, RANGE[0], RANGE[1], kind), batch),
                  ('erode/r%d' % r, lambda r=r: nuclei.erode(plane, r, kind), a.batch)]
        if r in ENTROPY_RADII:
            cases.append(('local_entropy/r%d' % r, lambda r=r: nuclei.local_entropy(plane, r, kind, raw=True), batch))
        if kind == 'square' and r in TORCH_RADII:
            inner = (slice(r, a.size - r), slice(r, a.size - r))
            assert torch.equal(nuclei.median(plane, r, kind)[inner], torch_median(plane, r)[inner]), r     # the two formulations agree
            cases.append(('torch_median/r%d' % r, lambda r=r: torch_median(plane, r), 1))
        # the extreme quantiles are the other kernel's results
        assert torch.equal(nuclei.rank_filter(plane, r, 0, kind), nuclei.erode(plane, r, kind)), r
        assert torch.equal(nuclei.quantile_range(plane, r, 0, 1, kind), nuclei.morph_gradient(plane, r, kind)), r
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
    rec = dict(device=torch.cuda.get_device_name(0), tile_rows=table.rank_tile_rows,
               tile_cols={str(r): table.rank_tile_cols(r) for r in RADII}, cases={})
    for name, _, _ in cases:
        ts = times[name]
        row = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if not name.startswith('torch_'):
            op, r = name.split('/r')
            bpp = BYTES_PER_PIXEL[op]
            row['compulsory_bytes'] = bpp * px
            row['floor_us_at_hbm_rate'] = round(bpp * px / HBM_BYTES_PER_S * 1e6, 2)
            row['fraction_of_hbm'] = round(bpp * px / (np.median(ts) * 1e-3) / HBM_BYTES_PER_S, 5)
            row['ns_per_pixel'] = round(float(np.median(ts)) * 1e6 / px, 4)
            row['footprint_pixels'] = sum(2 * width(kind, int(r), dy) + 1 for dy in range(-int(r), int(r) + 1))
        rec['cases'][name] = row
    c = rec['cases']
    for r in RADII:
        for op in ('median', 'quantile_range') + (('local_entropy',) if r in ENTROPY_RADII else ()):
            c['%s/r%d' % (op, r)]['over_erode'] = round(c['%s/r%d' % (op, r)]['ms_median'] / c['erode/r%d' % r]['ms_median'], 2)
        if 'torch_median/r%d' % r in c:
            c['median/r%d' % r]['torch_over_this'] = round(c['torch_median/r%d' % r]['ms_median'] / c['median/r%d' % r]['ms_median'], 2)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8500)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--batch', type=int, default=5)
    ap.add_argument('--step', default=None, choices=KINDS, help='run one footprint on the GPU (what the tool starts for every step)')
    ap.add_argument('--step-limit', type=int, default=240, help='seconds a step may take')
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
    rec = dict(plane='%dx%d' % (a.size, a.size), nuclei=a.nuclei, radii=list(RADII), entropy_radii=list(ENTROPY_RADII),
               footprints=list(KINDS), quantile_range=list(RANGE), repeats=a.repeats, batch=a.batch, hbm_bytes_per_s=HBM_BYTES_PER_S,
               footprints_measured={})
    for kind in KINDS:                                                           # every GPU step under its own time limit
        cmd = ['timeout', '-k', '10', str(a.step_limit), sys.executable, os.path.abspath(__file__), '--step', kind, '--size', str(a.size),
               '--nuclei', str(a.nuclei), '--repeats', str(a.repeats), '--batch', str(a.batch)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if done.returncode != 0:                                                 # the first failure ends the run: nothing more is started
            sys.stdout.write(done.stdout)
            print('rank_bench: step %s ended with status %d; stopping' % (kind, done.returncode), file=sys.stderr)
            sys.exit(done.returncode)
        got = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1])
        for key in ('device', 'tile_rows', 'tile_cols'):
            rec[key] = got.pop(key)
        rec['footprints_measured'][kind] = got['cases']
        print('rank_bench: %s done' % kind, file=sys.stderr, flush=True)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
