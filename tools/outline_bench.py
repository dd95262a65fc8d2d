#!/usr/bin/env python
"""Region outlines (csrc/outline.hip; kernels.KernelSpec.region_outlines): a whole call and each of its launches.
  <image>/call/corners|cracks   nuclei.region_outlines, connectivity 1, with its two host reads
  <image>/count                 cgc_region_outline_count: a thread per pixel, the crack sides of every pixel
  <image>/prefix                torch.cumsum over the pixels' counts
  <image>/cracks                cgc_region_outline_cracks: the compact crack list and the successors
  <image>/loops                 cgc_region_outline_loops: both doubling phases, 2 rounds + 3 launches; ``loops_per_launch`` beside it
  <image>/keys, sort, tables    the loop keys, torch.sort of them, the loop tables
  <image>/scatter, compact      the tails to their slots with the areas and the keep flags; the kept vertices to their places
The images: ``synthetic_tissue(size, size, size^2 / 1024 nuclei)`` as it comes (sparse ids) at every ``--sizes``, and the serpentine
of the tests (one region, one very long loop) at ``--serpentine``.  Before anything is timed the staged run is compared with the public
call for equality.  Device events around each case, the median, minimum and maximum over ``--repeats`` (>= 20) windows after a
warm-up; the cases take turns, window by window.  No time is asserted anywhere.

    python tools/outline_bench.py --out profiles/outline_bench.json
The tool itself never touches the GPU: the measurement is a step, a child process under ``timeout -k 10 --step-limit``, and a step
that fails ends the run with its exit status."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def serpentine(H, W):
    """Rows 1, 3, 5, ... over columns 1 .. W - 2, joined alternately at the right and the left end (tests/outline_ref.py)."""
    import numpy as np
    a = np.zeros((H, W), np.int32)
    rows = list(range(1, H - 1, 2))
    for y in rows:
        a[y, 1:W - 1] = 1
    for k, y in enumerate(rows[:-1]):
        a[y + 1, W - 2 if k % 2 == 0 else 1] = 1
    return a


def staged(table, L, top):
    """The launches of a 'corners' call, connectivity 1, one by one: (the cases [(name, fn)], facts, the outputs)."""
    import torch
    from cgc_net_amd.kernels import _ptr
    lib, st, dev = table.lib, table._stream(), L.device
    H, W = L.shape
    i32, i64, u8 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev), dict(dtype=torch.uint8, device=dev)
    C = ctypes.c_int64
    image = (_ptr(L), None, 0, H, W, top)
    sides, meta = torch.empty(2, H * W, **u8), torch.empty(1, **i32)
    t = {}

    def ok(rc):
        assert rc == 0, rc

    def count():
        ok(lib.cgc_region_outline_count(*image, 0, _ptr(sides[0]), _ptr(sides[1]), _ptr(meta), st))

    def prefix():
        t['off'] = torch.cumsum(sides[1], 0, dtype=torch.int32)

    count(), prefix()
    n = int(t['off'][-1])
    lists = torch.empty(4, n, **i32)
    crack, succ, start, steps = lists
    ws = torch.empty(int(lib.cgc_region_outlines_ws_bytes(C(n))), **u8)

    def cracks():
        ok(lib.cgc_region_outline_cracks(*image, 1, _ptr(sides[0]), _ptr(t['off']), C(n), _ptr(crack), _ptr(succ), st))

    def loops():
        ok(lib.cgc_region_outline_loops(C(n), _ptr(succ), _ptr(ws), _ptr(start), _ptr(steps), st))

    cracks(), loops()
    rank = torch.cumsum(start == torch.arange(n, **i32), 0, dtype=torch.int32)
    n_loops = int(rank[-1])
    n_vertices = int((((crack ^ crack[succ.to(torch.int64)]) & 3) != 0).sum())
    keys, loop_of = torch.empty(n_loops, **i64), torch.empty(n, **i32)
    tables, area2 = torch.empty(3, n_loops, **i32), torch.empty(n_loops, **i64)
    crack_ptr = torch.zeros(n_loops + 1, **i64)
    slots, keep, place = torch.empty(n, 2, **i32), torch.empty(n, **u8), torch.zeros(n + 1, **i32)
    vertices = torch.empty(n_vertices, 2, **i32)

    def make_keys():
        ok(lib.cgc_region_outline_keys(C(n), C(n_loops), _ptr(L), _ptr(crack), _ptr(start), _ptr(rank), _ptr(keys), st))

    def sort():
        t['keys'] = torch.sort(keys).values

    def make_tables():
        ok(lib.cgc_region_outline_tables(C(n), C(n_loops), _ptr(t['keys']), _ptr(crack), _ptr(steps), _ptr(tables[0]), _ptr(tables[1]),
                                         _ptr(tables[2]), _ptr(area2), _ptr(loop_of), st))
        torch.cumsum(tables[2], 0, out=crack_ptr[1:])

    def scatter():
        area2.zero_()
        ok(lib.cgc_region_outline_scatter(C(n), C(n_loops), W, _ptr(crack), _ptr(succ), _ptr(start), _ptr(steps), _ptr(loop_of),
                                          _ptr(crack_ptr), _ptr(area2), _ptr(slots), _ptr(keep), st))

    def compact():
        torch.cumsum(keep, 0, dtype=torch.int32, out=place[1:])
        ok(lib.cgc_region_outline_compact(C(n), C(n_vertices), _ptr(keep), _ptr(place[1:]), _ptr(slots), _ptr(vertices), st))

    make_keys(), sort(), make_tables(), scatter(), compact()
    cases = [('count', count), ('prefix', prefix), ('cracks', cracks), ('loops', loops), ('keys', make_keys), ('sort', sort),
             ('tables', make_tables), ('scatter', scatter), ('compact', compact)]
    rounds = table.region_outline_rounds(n)
    facts = dict(cracks=n, loops=n_loops, vertices=n_vertices, rounds=rounds, loop_launches=2 * rounds + 3,
                 longest_loop=int(tables[2].max()) if n_loops else 0)
    return cases, facts, (place[crack_ptr].to(torch.int64), tables[0], tables[1], tables[2], area2, vertices)


def step(a):
    """Every case on the GPU: prints one JSON object."""
    import numpy as np
    import torch
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import kernels, nuclei

    dev = torch.device('cuda:0')
    table = kernels.get()
    images = {}
    for size in a.sizes:
        images['tissue/%d' % size] = nuclei.synthetic_tissue(size, size, max(size * size // 1024, 4))[0]
    images['serpentine/%d' % a.serpentine] = serpentine(a.serpentine, a.serpentine)
    cases, facts = [], {}
    for name, lab in images.items():
        L = torch.from_numpy(np.asarray(lab, np.int32)).to(dev)
        top = int(L.max())
        parts, facts[name], out = staged(table, L, top)
        whole = nuclei.region_outlines(L, max_label=top)
        assert all(torch.equal(x, y) for x, y in zip(out, whole[1:7]))       # the staged run is the public call
        cases += [('%s/%s' % (name, k), fn) for k, fn in parts]
        for mode in ('corners', 'cracks'):
            cases.append(('%s/call/%s' % (name, mode), lambda L=L, top=top, mode=mode: nuclei.region_outlines(L, max_label=top, mode=mode)))
    for _, fn in cases:                                                          # warm-up: code objects, the allocator's blocks
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for window in range(a.repeats):
        for name, fn in cases:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop))
    rec = dict(device=torch.cuda.get_device_name(0), images=facts, cases={})
    for name, _ in cases:
        ts = times[name]
        rec['cases'][name] = dict(ms_median=round(float(np.median(ts)), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4))
        if name.endswith('/loops'):
            rec['cases'][name]['loops_per_launch_ms_median'] = round(float(np.median(ts)) / facts[name[:-6]]['loop_launches'], 5)
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[512, 2048, 3584])
    ap.add_argument('--serpentine', type=int, default=2048)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--step', action='store_true', help='run the measurement on the GPU (what the tool starts)')
    ap.add_argument('--step-limit', type=int, default=420, help='seconds the step may take')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error('at least twenty repeats')
    if a.step:
        step(a)
        return
    rec = dict(sizes=a.sizes, serpentine=a.serpentine, repeats=a.repeats, connectivity=1)
    cmd = ['timeout', '-k', '10', str(a.step_limit), sys.executable, os.path.abspath(__file__), '--step', '--serpentine', str(a.serpentine),
           '--repeats', str(a.repeats), '--sizes'] + [str(s) for s in a.sizes]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)   # the GPU step under its own time limit
    if done.returncode != 0:
        sys.stdout.write(done.stdout)
        print('outline_bench: the step ended with status %d; stopping' % done.returncode, file=sys.stderr)
        sys.exit(done.returncode)
    rec.update(json.loads([ln for ln in done.stdout.splitlines() if ln.startswith('{')][-1]))
    print(json.dumps(rec))
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


if __name__ == '__main__':
    main()
