#!/usr/bin/env python
"""Superpixels (csrc/slic.hip; kernels.KernelSpec.slic_iterate, slic_merge): a whole call, the clustering, a round of it, and the same
rounds written with stock torch.
  <image>/S<step>/superpixels   nuclei.superpixels: clustering, pieces, contacts, merge, relabel, with its host reads
  <image>/S<step>/iterate       kernels.slic_iterate, ``--iters`` rounds: 1 + 2 * iters launches, no host read
  <image>/S<step>/iterate1      ... one round: init, assign + accumulate, finalize.  ``round_ms`` beside ``iterate`` is (iterate -
                                iterate1) / (iters - 1): one fused assign + accumulate launch and its finalize launch
  <image>/S<step>/relabel       kernels.slic_relabel: one launch over the pixels (some ten microseconds: a window of one call is mostly
                                launch and event overhead, so the figure only says that the launch is small)
  <image>/S<step>/torch         the same ``--iters`` rounds in torch: per candidate cell a gather of the centres and a 64-bit distance,
                                nine of them folded by ``torch.where`` in ascending k, then ``index_add_`` and an integer division
The images: a smoothed noise tile of ``--planes`` uint8 planes at every ``--sizes``, steps ``--steps``.  Before anything is timed the torch
rounds are compared with the library's for equality (labels, centres, counts).  Device events around each case, the median, minimum and
maximum over ``--repeats`` (>= 20) windows after a warm-up (the torch case: ``--torch-repeats``); the cases take turns, window by window.
No time is asserted anywhere.

    python tools/slic_bench.py --out profiles/slic_bench.json
The tool itself never touches the GPU: the measurement is a step, a child process under ``timeout -k 10 --step-limit``, and a step
that fails ends the run with its exit status."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tile_planes(C, size, seed):
    """uint8 [C, size, size] on the GPU: noise smoothed by a 9 x 9 box twice, stretched to the full range (blobs of tens of pixels)."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    a = torch.rand(1, C, size, size, device='cuda', generator=g)
    for _ in range(2):
        a = torch.nn.functional.avg_pool2d(a, 9, 1, 4, count_include_pad=False)
    a = a[0]
    lo, hi = a.amin((1, 2), keepdim=True), a.amax((1, 2), keepdim=True)
    return ((a - lo) / (hi - lo) * 255).round().to(torch.uint8).contiguous()


def torch_rounds(planes, S, m, n_iter):
    """KernelSpec.slic_iterate in stock torch, int64 throughout: (labels int32 [H, W], centres int32 [K, 2 + C], count int32 [K])."""
    import torch
    C, H, W = planes.shape
    dev = planes.device
    ny, nx = max(1, (2 * H + S) // (2 * S)), max(1, (2 * W + S) // (2 * S))
    K = ny * nx
    ys, xs = torch.arange(H, device=dev), torch.arange(W, device=dev)
    hy, hx = ys * ny // H, xs * nx // W
    cy = ((2 * torch.arange(ny, device=dev) + 1) * H) // (2 * ny)
    cx = ((2 * torch.arange(nx, device=dev) + 1) * W) // (2 * nx)
    p = planes.to(torch.int64)
    cen = torch.cat([cy[:, None].expand(ny, nx).reshape(K, 1), cx[None, :].expand(ny, nx).reshape(K, 1),
                     p[:, cy][:, :, cx].reshape(C, K).t()], 1)
    feats = torch.cat([ys[:, None].expand(H, W).reshape(-1, 1), xs[None, :].expand(H, W).reshape(-1, 1), p.reshape(C, -1).t()], 1)
    big = torch.iinfo(torch.int64).max
    for _ in range(n_iter):
        best = torch.full((H, W), big, dtype=torch.int64, device=dev)
        best_k = torch.zeros(H, W, dtype=torch.int64, device=dev)
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):                                       # ascending k: of equal D the first one stays
                ci, cj = hy + di, hx + dj
                valid = ((ci >= 0) & (ci < ny))[:, None] & ((cj >= 0) & (cj < nx))[None, :]
                k = ci.clamp(0, ny - 1)[:, None] * nx + cj.clamp(0, nx - 1)[None, :]
                c = cen[k]                                              # [H, W, 2 + C]
                d = m * m * ((ys[:, None] - c[..., 0]) ** 2 + (xs[None, :] - c[..., 1]) ** 2)
                d = d + S * S * ((p.permute(1, 2, 0) - c[..., 2:]) ** 2).sum(-1)
                d = torch.where(valid, d, big)
                better = d < best
                best, best_k = torch.where(better, d, best), torch.where(better, k, best_k)
        flat = best_k.reshape(-1)
        n = torch.zeros(K, dtype=torch.int64, device=dev).index_add_(0, flat, torch.ones_like(flat))
        sums = torch.zeros(K, 2 + C, dtype=torch.int64, device=dev).index_add_(0, flat, feats)
        den = n.clamp(min=1)[:, None]
        cen = torch.where(n[:, None] > 0, (2 * sums + n[:, None]) // (2 * den), cen)
    return (best_k + 1).to(torch.int32), cen.to(torch.int32), n.to(torch.int32)


def step(a):
    """Every case on the GPU: prints one JSON object."""
    import numpy as np
    import torch
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import kernels, nuclei

    table = kernels.get()
    cases, facts, slow = [], {}, set()
    for size in a.sizes:
        planes = tile_planes(a.planes, size, size)
        for S in a.steps:
            name = 'noise/%d/S%d' % (size, S)
            lib_out = table.slic_iterate(planes, S, a.compactness, a.iters)
            for x, y in zip(lib_out, torch_rounds(planes, S, a.compactness, a.iters)):
                assert torch.equal(x, y), name                               # the torch rounds are the library's
            final, n = nuclei.superpixels(planes, S, a.compactness, a.iters)
            pieces, P = nuclei.label_instances(lib_out[0], 1)
            table_in = torch.arange(P + 1, dtype=torch.int32, device=planes.device)
            facts[name] = dict(centres=int(lib_out[2].numel()), pieces=P, regions=n, launches=1 + 2 * a.iters)
            cases += [
                (name + '/superpixels', lambda planes=planes, S=S: nuclei.superpixels(planes, S, a.compactness, a.iters)),
                (name + '/iterate', lambda planes=planes, S=S: table.slic_iterate(planes, S, a.compactness, a.iters)),
                (name + '/iterate1', lambda planes=planes, S=S: table.slic_iterate(planes, S, a.compactness, 1)),
                (name + '/relabel', lambda pieces=pieces, table_in=table_in: table.slic_relabel(pieces, table_in)),
                (name + '/torch', lambda planes=planes, S=S: torch_rounds(planes, S, a.compactness, a.iters)),
            ]
            slow.add(name + '/torch')
    for _, fn in cases:                                                      # warm-up: code objects, the allocator's blocks
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for window in range(a.repeats):
        for name, fn in cases:
            if name in slow and window >= a.torch_repeats:
                continue
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop))
    rec = dict(device=torch.cuda.get_device_name(0), images=facts, cases={})
    for name, _ in cases:
        ts = times[name]
        rec['cases'][name] = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), windows=len(ts))
    for name in facts:
        whole, one = rec['cases'][name + '/iterate']['ms_median'], rec['cases'][name + '/iterate1']['ms_median']
        if a.iters > 1:
            rec['cases'][name + '/iterate']['round_ms'] = round((whole - one) / (a.iters - 1), 5)
        rec['cases'][name + '/torch']['ratio_to_iterate'] = round(rec['cases'][name + '/torch']['ms_median'] / whole, 2)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[1024, 3584])
    ap.add_argument('--steps', type=int, nargs='+', default=[16, 32, 64])
    ap.add_argument('--planes', type=int, default=3)
    ap.add_argument('--compactness', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--torch-repeats', type=int, default=5)
    ap.add_argument('--step', action='store_true', help='run the measurement on the GPU (what the tool starts)')
    ap.add_argument('--step-limit', type=int, default=420, help='seconds the step may take')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error('at least twenty repeats')
    if a.torch_repeats < 3:
        ap.error('at least three repeats of the torch rounds')
    if a.step:
        step(a)
        return
    rec = dict(sizes=a.sizes, steps=a.steps, planes=a.planes, compactness=a.compactness, iters=a.iters, repeats=a.repeats,
               torch_repeats=a.torch_repeats)
    cmd = ['timeout', '-k', '10', str(a.step_limit), sys.executable, os.path.abspath(__file__), '--step', '--planes', str(a.planes),
           '--compactness', str(a.compactness), '--iters', str(a.iters), '--repeats', str(a.repeats), '--torch-repeats', str(a.torch_repeats),
           '--sizes'] + [str(s) for s in a.sizes] + ['--steps'] + [str(s) for s in a.steps]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)   # the GPU step under its own time limit
    if done.returncode != 0:
        sys.stdout.write(done.stdout)
        print('slic_bench: the step ended with status %d; stopping' % done.returncode, file=sys.stderr)
        sys.exit(done.returncode)
    rec.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
