#!/usr/bin/env python
"""Region co-occurrence (csrc/region.hip; kernels.KernelSpec.region_cooccurrence) on the tile of tools/region_bench.py: one 3584 x
3584 tile of synthetic_tissue, labelled by label_instances (labels 1..n), and its uint8 gray plane, 16 levels, symmetric:
  cooc/1                        the table call for the offset (0, 1): memset of the tables, one launch
  cooc/4                        ... for the four directions COOC_DIRECTIONS: one launch per offset
  cooc/4/within                 ... with within = labels != 0, the background left out
  properties                    cooccurrence_properties of the four-direction tables (torch, float64 on the device)
  texture_features              the public function on an H&E-like tile: separate_stains, four launches, the properties, one host read
  histogram                     region_histogram in the same run, on the same tile: the same kernel family, the number to report against
  torch: cooc/4                 shifted slices of the label and level planes and bincount((label * noff + k) * L^2 + a * L + b)
The stock formulation is compared with this code for equality, bit for bit, before anything is timed.  Device events around
``--batch`` calls in a row, the median, minimum and maximum over ``--repeats`` (>= 20) such windows after a warm-up; the cases take
turns, window by window.  ``per_offset_over_histogram`` is the time of a table call per offset over the time of region_histogram.
No time is asserted anywhere.

    python tools/cooc_bench.py --out profiles/cooc_bench.json
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

LEVELS = 16


def torch_cooccurrence(labels, level, offsets, rows, levels, symmetric, within=None):
    """int64 [rows, noff, levels, levels] with stock torch: slices for the shift, one bincount for all offsets."""
    import torch
    H, W = labels.shape
    lab, lev = labels.to(torch.int64), level.to(torch.int64)
    noff = len(offsets)
    keys = []
    for k, (dy, dx) in enumerate(offsets):
        ya, yb = (0, H - dy) if dy >= 0 else (-dy, H)
        xa, xb = (0, W - dx) if dx >= 0 else (-dx, W)
        p = (slice(ya, yb), slice(xa, xb))
        q = (slice(ya + dy, yb + dy), slice(xa + dx, xb + dx))
        ok = lab[p] == lab[q]
        if within is not None:
            ok &= within[p] & within[q]
        base = (lab[p][ok] * noff + k) * (levels * levels)
        a, b = lev[p][ok], lev[q][ok]
        keys.append(base + a * levels + b)
        if symmetric:
            keys.append(base + b * levels + a)
    return torch.bincount(torch.cat(keys), minlength=rows * noff * levels * levels).view(rows, noff, levels, levels)


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
    tile = torch.stack([plane, 255 - plane // 2, 128 + plane // 4], dim=2).contiguous()
    kept = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    table = kernels.get()
    rows = n + 1
    lut = nuclei.level_lut(LEVELS)
    dirs = nuclei.COOC_DIRECTIONS
    inside = L != 0
    shape4 = (rows, 4, LEVELS, LEVELS)

    # the stock formulation agrees with this code, bit for bit
    level = torch.tensor(lut, dtype=torch.int64, device=dev)[plane.long()]
    for symmetric in (True, False):
        for within in (None, inside):
            got, meta = table.region_cooccurrence(L, plane, n, lut, LEVELS, dirs, symmetric, within)
            assert int(meta) == 0
            assert torch.equal(got.view(shape4).to(torch.int64), torch_cooccurrence(L, level, dirs, rows, LEVELS, symmetric, within))
    long_offsets = ((3, -16), (-16, 5))
    got, _ = table.region_cooccurrence(L, plane, n, lut, LEVELS, long_offsets, True)
    assert torch.equal(got.view(rows, 2, LEVELS, LEVELS).to(torch.int64), torch_cooccurrence(L, level, long_offsets, rows, LEVELS, True))
    tables4 = table.region_cooccurrence(L, plane, n, lut, LEVELS, dirs, True, inside)[0].view(shape4)

    cases = [('cooc/1', lambda: table.region_cooccurrence(L, plane, n, lut, LEVELS, dirs[:1], True), a.batch),
             ('cooc/4', lambda: table.region_cooccurrence(L, plane, n, lut, LEVELS, dirs, True), a.batch),
             ('cooc/4/within', lambda: table.region_cooccurrence(L, plane, n, lut, LEVELS, dirs, True, inside), a.batch),
             ('cooc/4/plain', lambda: table.region_cooccurrence(L, plane, n, lut, LEVELS, dirs, False), a.batch),
             ('histogram', lambda: table.region_histogram(L, plane, n), a.batch),
             ('properties', lambda: nuclei.cooccurrence_properties(tables4), 1),
             ('texture_features', lambda: nuclei.texture_features(L, tile, kept, hi=159, max_label=n), 1),
             ('torch_cooc/4', lambda: torch_cooccurrence(L, level, dirs, rows, LEVELS, True), 1)]
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
    rec = dict(device=torch.cuda.get_device_name(0), tile_side=table.region_tile, table_slots=table.region_slots, labels=n, levels=LEVELS,
               background_fraction=round(float((L == 0).sum()) / (a.size * a.size), 4), cases={})
    for name, _, _ in cases:
        ts = times[name]
        rec['cases'][name] = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
    c = rec['cases']
    hist = c['histogram']['ms_median']
    c['cooc/1']['per_offset_over_histogram'] = round(c['cooc/1']['ms_median'] / hist, 3)
    for name in ('cooc/4', 'cooc/4/within', 'cooc/4/plain'):
        c[name]['per_offset_over_histogram'] = round(c[name]['ms_median'] / 4 / hist, 3)
    c['cooc/4']['torch_over_this'] = round(c['torch_cooc/4']['ms_median'] / c['cooc/4']['ms_median'], 2)
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
        print('cooc_bench: the step ended with status %d; stopping' % done.returncode, file=sys.stderr)
        sys.exit(done.returncode)
    rec.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
