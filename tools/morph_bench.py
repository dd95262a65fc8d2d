#!/usr/bin/env python
"""Flat grey-scale morphology (csrc/morph.hip; kernels.KernelSpec.flat_morphology) on one 3584 x 3584 plane of synthetic_tissue, with
the three footprints at radii 1, 3, 15 and 63, beside the same results from stock torch ops on the same device:
  erode                               one launch: 1 byte read, 1 written per pixel
  gradient                            one launch, both extrema: 1 byte read, 1 written per pixel
  white_tophat                        two launches, the subtraction fused into the second: 2 + 3 bytes per pixel
  torch: square                       F.max_pool2d on a float16 copy padded with the neutral value, as a row pass and a column pass
  torch: disk, diamond                for every |dy| the row-run maximum F.max_pool2d(., (1, 2 w + 1)) of the padded copy, then the
                                      maximum over the 2 r + 1 row-shifted views of those planes (r + 1 pools, 2 r + 1 elementwise maxima);
                                      erosion as 255 - dilate(255 - x); the conversions to float16 and back are part of the call
Device events around ``--batch`` calls in a row (one call for the stock formulation), the median, minimum and maximum over
``--repeats`` (>= 20) such windows after a warm-up; the cases take turns, window by window.  Compulsory bytes over the measured time
are given as a fraction of the 8 TB/s of HBM (a 13 MB plane sits in the Infinity Cache).  The two formulations are compared for
equality before anything is timed.  No time is asserted anywhere.

    python tools/morph_bench.py --out profiles/morph_bench.json
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
KINDS = ('square', 'disk', 'diamond')
RADII = (1, 3, 15, 63)
OPS = ('erode', 'gradient', 'white_tophat')
BYTES_PER_PIXEL = {'erode': 2, 'gradient': 2, 'white_tophat': 5}


def width(kind, r, dy):
    if kind == 'square':
        return r
    if kind == 'diamond':
        return r - abs(dy)
    w = 0
    while (w + 1) ** 2 + dy * dy <= r * r:
        w += 1
    return w


def torch_dilate(x, kind, r):
    """Dilation in stock torch ops.  x: float16 (any float type) [H, W]; padding with 0 is the clipped footprint."""
    import torch
    import torch.nn.functional as F
    if r == 0:
        return x
    H, W = x.shape
    p = F.pad(x[None, None], (r, r, r, r), value=0.0)
    if kind == 'square':
        return F.max_pool2d(F.max_pool2d(p, (1, 2 * r + 1), 1), (2 * r + 1, 1), 1)[0, 0]
    out = None
    for dy in range(0, r + 1):
        w = width(kind, r, dy)
        run = F.max_pool2d(p[:, :, :, r - w:r + W + w], (1, 2 * w + 1), 1)[0, 0]          # [H + 2 r, W]
        for s in ((0,) if dy == 0 else (dy, -dy)):
            view = run[r + s:r + s + H]
            out = view.clone() if out is None else torch.maximum(out, view)
    return out


def torch_op(plane, kind, op, r, dtype=None):
    import torch
    x = plane.to(dtype or torch.float16)
    if op == 'erode':
        res = 255 - torch_dilate(255 - x, kind, r)
    elif op == 'gradient':
        res = torch_dilate(x, kind, r) - (255 - torch_dilate(255 - x, kind, r))
    else:
        res = x - torch_dilate(255 - torch_dilate(255 - x, kind, r), kind, r)
    return res.to(torch.uint8)


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

    ours = {'erode': lambda r: nuclei.erode(plane, r, kind), 'gradient': lambda r: nuclei.morph_gradient(plane, r, kind),
            'white_tophat': lambda r: nuclei.white_tophat(plane, r, kind)}
    cases = []                                                                   # name, callable, calls per window
    for r in RADII:
        for op in OPS:                                                           # the two formulations agree
            assert torch.equal(ours[op](r), torch_op(plane, kind, op, r)), (kind, op, r)
            cases += [('%s/r%d' % (op, r), lambda op=op, r=r: ours[op](r), a.batch),
                      ('torch_%s/r%d' % (op, r), lambda op=op, r=r: torch_op(plane, kind, op, r), 1)]
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
    rec = dict(device=torch.cuda.get_device_name(0), tile_rows=table.morph_tile_rows,
               tile_cols={str(r): table.morph_tile_cols(r) for r in RADII}, cases={})
    for name, _, _ in cases:
        ts = times[name]
        row = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if not name.startswith('torch_'):
            bpp = BYTES_PER_PIXEL[name.split('/')[0]]
            row['compulsory_bytes'] = bpp * px
            row['floor_us_at_hbm_rate'] = round(bpp * px / HBM_BYTES_PER_S * 1e6, 2)
            row['fraction_of_hbm'] = round(bpp * px / (np.median(ts) * 1e-3) / HBM_BYTES_PER_S, 4)
            row['footprint_pixels'] = sum(2 * width(kind, int(name.split('/r')[1]), dy) + 1
                                          for dy in range(-int(name.split('/r')[1]), int(name.split('/r')[1]) + 1))
        rec['cases'][name] = row
    c = rec['cases']
    for r in RADII:
        for op in OPS:
            c['%s/r%d' % (op, r)]['torch_over_this'] = round(c['torch_%s/r%d' % (op, r)]['ms_median'] / c['%s/r%d' % (op, r)]['ms_median'], 2)
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
    rec = dict(plane='%dx%d' % (a.size, a.size), nuclei=a.nuclei, radii=list(RADII), footprints=list(KINDS), ops=list(OPS),
               repeats=a.repeats, batch=a.batch, hbm_bytes_per_s=HBM_BYTES_PER_S, footprints_measured={})
    for kind in KINDS:                                                           # every GPU step under its own time limit
        cmd = ['timeout', '-k', '10', str(a.step_limit), sys.executable, os.path.abspath(__file__), '--step', kind, '--size', str(a.size),
               '--nuclei', str(a.nuclei), '--repeats', str(a.repeats), '--batch', str(a.batch)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        if done.returncode != 0:                                                 # the first failure ends the run: nothing more is started
            sys.stdout.write(done.stdout)
            print('morph_bench: step %s ended with status %d; stopping' % (kind, done.returncode), file=sys.stderr)
            sys.exit(done.returncode)
        got = json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1])
        for key in ('device', 'tile_rows', 'tile_cols'):
            rec[key] = got.pop(key)
        rec['footprints_measured'][kind] = got['cases']
        print('morph_bench: %s done' % kind, file=sys.stderr, flush=True)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
