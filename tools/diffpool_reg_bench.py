"""Cost of the DiffPool regularisers (SoftPoolingGcnEncoder(diffpool_loss=True), csrc/diffpool_reg.hip) on the C3 workload of bench.py:
32 graphs of ~1800 nodes, 16 features, max_num_nodes 11404 (C1 = 1140, C2 = 114), shipped flags (norm_adj, jk, dropout 0.2).

    python tools/diffpool_reg_bench.py [--steps 20] [--warmup 5] [--runs 3]

A step is forward + backward + the library's Adam, as in bench.py.  For each GEMM mode (0 exact, 1 bf16 x6, 2 fp16 x3) the flag-off
and flag-on steps run alternately, ``--runs`` times each; one JSON line per mode: ms/step of every run and the medians.  With the flag
on, the loss is ``cls_loss + sum(link_loss) + sum(ent_loss)``.

The new kernels' own times come from a separate trace run of this script:
    rocprofv3 --kernel-trace --stats -d DIR -o reg -- python tools/diffpool_reg_bench.py --steps 5 --warmup 2 --runs 1 --modes 0 --only-on
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--runs', type=int, default=3)
    p.add_argument('--modes', default='0,1,2')
    p.add_argument('--only-on', action='store_true', help='flag-on runs only (for a trace)')
    args = p.parse_args()

    import torch
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import network
    from cgc_net_amd.data import Batch, SyntheticCellGraphs
    from cgc_net_amd.optim import Adam

    dev = torch.device('cuda:0')
    ds = SyntheticCellGraphs(4 * 32, 1800, 16, base_seed=0)
    batches = [Batch.from_data_list([ds[b * 32 + i] for i in range(32)]).to(dev) for b in range(4)]
    torch.manual_seed(0)
    model = network.SoftPoolingGcnEncoder(11404, 16, 20, 20, True, True, 20, 3, 0.1, [50], concat=True, gcn_name='SAGE',
                                          load_data_sparse=True, norm_adj=True, jk=True, drop_out=0.2).to(dev).train()
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4, model=model)
    torch.autograd.set_multithreading_enabled(False)

    def step(b):
        _, loss = model(b)
        if model.diffpool_loss:
            loss = loss + sum(model.link_loss) + sum(model.ent_loss)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def timed(flag):
        model.diffpool_loss = flag
        for i in range(args.warmup):
            step(batches[i % len(batches)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(batches[i % len(batches)])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    for mode in [int(m) for m in args.modes.split(',')]:
        model.gemm_mode = mode
        res = {False: [], True: []}
        for _ in range(args.runs):
            for flag in ((True,) if args.only_on else (False, True)):
                res[flag].append(timed(flag))
        line = {'mode': mode, 'off_ms': [round(v, 3) for v in res[False]], 'on_ms': [round(v, 3) for v in res[True]]}
        if res[False] and res[True]:
            off, on = statistics.median(res[False]), statistics.median(res[True])
            line.update(off_median=round(off, 3), on_median=round(on, 3), cost_ms=round(on - off, 3))
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
