#!/usr/bin/env python
"""The three kernels of the stain front end (csrc/stain.hip, csrc/smooth.hip) on one 3584 x 3584 tile, the reference's tile size,
each beside the same step written with stock torch ops on the same device:
  stain_separate (3 planes, 1 plane)   vs  float32 log, matmul with inv(S), clamp
  histogram_u8 on (a) uniform random values, (b) a flat image -- every lane on one bin, the contention case --, (c) the smoothed
      haematoxylin plane of the rendered tissue tile, (d) the same with a ``within`` mask   vs  torch.bincount
  binomial_smooth, radius 2 and 5      vs  two float32 conv2d with replicated padding
Device events around ``--batch`` calls in a row, the median over ``--repeats`` (>= 20) such windows after a warm-up; the cases take
turns, window by window.  Per kernel also the compulsory bytes (3 + planes, 1 + within bytes, and 2 bytes per pixel) over the
measured time, as a fraction of the 8 TB/s of HBM.  The stock versions are timed, not compared bit for bit: they round differently.

    python tools/stain_bench.py [--repeats 25] [--out profiles/stain_bench.json]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import cgc_net_amd  # noqa: E402,F401
from cgc_net_amd import kernels, nuclei  # noqa: E402
import stain_ref  # noqa: E402

HBM_BYTES_PER_S = 8e12


def torch_separate(image, inv_s, planes):
    od = torch.log(255.0 / image.to(torch.float32).clamp_(min=1.0))            # [H, W, 3] B, G, R
    c = od.flip(2).reshape(-1, 3) @ inv_s[:, planes]
    return (64.0 * c + 0.5).floor_().clamp_(0.0, 255.0).to(torch.uint8).t().reshape((len(planes),) + tuple(image.shape[:2]))


def torch_histogram(img, within=None):
    sel = img.reshape(-1) if within is None else img[within]
    return torch.bincount(sel.to(torch.int64), minlength=256)


def torch_smooth(img, w):
    x = img.to(torch.float32)[None, None]
    r = (w.numel() - 1) // 2
    x = F.conv2d(F.pad(x, (r, r, 0, 0), mode='replicate'), w.view(1, 1, 1, -1))
    x = F.conv2d(F.pad(x, (0, 0, r, r), mode='replicate'), w.view(1, 1, -1, 1))
    return (x / float(w.sum()) ** 2 + 0.5).floor_().clamp_(0, 255).to(torch.uint8)[0, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=3584)
    ap.add_argument('--nuclei', type=int, default=8500)
    ap.add_argument('--repeats', type=int, default=25)
    ap.add_argument('--batch', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error('at least twenty repeats')
    dev = torch.device('cuda:0')
    n = a.size * a.size
    rng = np.random.RandomState(0)
    labels = nuclei.synthetic_tissue(a.size, a.size, a.nuclei, seed=0)[0]
    tile = torch.from_numpy(stain_ref.render_tile(labels)).to(dev)
    tile = (tile.to(torch.int16) + torch.randint(-12, 13, tile.shape, device=dev, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
    plane = nuclei.smooth(nuclei.separate_stains(tile, planes=(0,))[0], 2)
    uniform = torch.from_numpy(rng.randint(0, 256, (a.size, a.size)).astype(np.uint8)).to(dev)
    flat = torch.full((a.size, a.size), 137, dtype=torch.uint8, device=dev)
    within = torch.from_numpy(labels > 0).to(dev)
    S = np.array(nuclei.DEFAULT_STAINS)
    inv_s = torch.from_numpy(np.linalg.inv(S / np.sqrt((S * S).sum(axis=1))[:, None])).to(dev, torch.float32)
    weights = {r: torch.tensor([float(math.comb(2 * r, k)) for k in range(2 * r + 1)], device=dev) for r in (2, 5)}
    table = kernels.get()
    m, lut = nuclei.stain_matrix().tolist(), nuclei.OD_LUT
    cases = [     # name, callable, compulsory bytes per pixel (None: a stock version)
        ('stain_separate/3_planes', lambda: table.stain_separate(tile, 0, lut, m, 7), 6),
        ('stain_separate/1_plane', lambda: table.stain_separate(tile, 0, lut, m, 1), 4),
        ('torch_separate/3_planes', lambda: torch_separate(tile, inv_s, [0, 1, 2]), None),
        ('torch_separate/1_plane', lambda: torch_separate(tile, inv_s, [0]), None),
        ('histogram_u8/uniform', lambda: table.histogram_u8(uniform), 1),
        ('histogram_u8/flat', lambda: table.histogram_u8(flat), 1),
        ('histogram_u8/tissue', lambda: table.histogram_u8(plane), 1),
        ('histogram_u8/tissue_within', lambda: table.histogram_u8(plane, within), 2),
        ('torch_bincount/uniform', lambda: torch_histogram(uniform), None),
        ('torch_bincount/flat', lambda: torch_histogram(flat), None),
        ('torch_bincount/tissue', lambda: torch_histogram(plane), None),
        ('torch_bincount/tissue_within', lambda: torch_histogram(plane, within), None),
        ('binomial_smooth/r2', lambda: table.binomial_smooth(plane, 2), 2),
        ('binomial_smooth/r5', lambda: table.binomial_smooth(plane, 5), 2),
        ('torch_conv2d/r2', lambda: torch_smooth(plane, weights[2]), None),
        ('torch_conv2d/r5', lambda: torch_smooth(plane, weights[5]), None),
    ]
    for _, fn, _ in cases:                                # warm-up: code objects, the allocator's blocks, the library's choices
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
    rec = dict(tile='%dx%d' % (a.size, a.size), repeats=a.repeats, batch=a.batch, device=torch.cuda.get_device_name(0),
               foreground_fraction=round(float(within.float().mean()), 4), histogram_chunk=table.histogram_chunk, cases={})
    for name, _, bpp in cases:
        ts = times[name]
        row = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if bpp is not None:
            row['compulsory_bytes'] = bpp * n
            row['fraction_of_hbm'] = round(bpp * n / (np.median(ts) * 1e-3) / HBM_BYTES_PER_S, 4)
        rec['cases'][name] = row
    c = rec['cases']
    rec['histogram_flat_over_uniform'] = round(c['histogram_u8/flat']['ms_median'] / c['histogram_u8/uniform']['ms_median'], 3)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
