"""The optimiser update alone, for the three optimisers of the reference's init_optim (adam, sgd, rmsprop), each in three forms:

  torch       torch.optim.Adam(fused=True) / SGD(fused=True) / RMSprop(foreach=True): torch's own step()
  lists       cgc_net_amd.optim.<class>(model=None): torch's kernels on lists built once
  one_launch  cgc_net_amd.optim.<class>(model=encoder): one launch of cgc_adam_step / cgc_sgd_step / cgc_rmsprop_step

on the bench.py model (C3, shipped flags) with the gradients of one forward + backward at B graphs (default: the C3 batch of 32
and the 4-graph shard of an 8-GPU step).  Per form, with the same gradients left in place:

  enqueue_us  host time of one step() call, no synchronise inside the window (N back-to-back calls / N): the enqueue cost
  device_us   HIP events recorded around one step(), then a synchronise: the median over N of the update's device time

  python tools/optim_step_bench.py [--batches 32 4] [--reps 200] [--out profiles/optim_step_bench.json]

Kernels and launches per update come from a run under the profiler of its own (tracing slows the host):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o optim -- \
      python tools/optim_step_bench.py --trace-steps 20 --out RUN_OUT
  python tools/optim_step_bench.py --parse-trace DIR/optim_kernel_trace.csv --order RUN_OUT --trace-steps 20 [--out FILE]

With --trace-steps each form runs its warm-up, then `torch.cuda._sleep` (a kernel named spin_kernel, used nowhere else) as a
delimiter, the given number of step() calls, and another delimiter; --parse-trace counts the kernels between each pair of
delimiters, in dispatch order (Dispatch_Id).
"""
import argparse
import collections
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPTIMS = ('adam', 'sgd', 'rmsprop')
FORMS = ('torch', 'lists', 'one_launch')


def make_optimiser(name, form, model):
    import torch
    from cgc_net_amd import optim
    ps = model.parameters()
    hp = dict(adam=dict(lr=1e-3, weight_decay=1e-4), sgd=dict(lr=1e-3, momentum=0.9, weight_decay=1e-4),
              rmsprop=dict(lr=1e-3, momentum=0.9, weight_decay=1e-4))[name]
    if form == 'torch':
        cls = dict(adam=torch.optim.Adam, sgd=torch.optim.SGD, rmsprop=torch.optim.RMSprop)[name]
        return cls(ps, **hp, **(dict(foreach=True) if name == 'rmsprop' else dict(fused=True)))
    cls = dict(adam=optim.Adam, sgd=optim.SGD, rmsprop=optim.RMSprop)[name]
    return cls(ps, **hp, model=model if form == 'one_launch' else None)


def setup(batch, nodes=1800):
    import torch
    import cgc_net_amd  # noqa: F401
    from cgc_net_amd import network
    from cgc_net_amd.data import Batch, SyntheticCellGraphs
    torch.manual_seed(0)
    model = network.SoftPoolingGcnEncoder(11404, 16, 20, 20, True, True, 20, 3, 0.1, [50], concat=True, gcn_name='SAGE',
                                          load_data_sparse=True, norm_adj=True, jk=True, drop_out=0.2).cuda().train()
    ds = SyntheticCellGraphs(batch, nodes, 16, base_seed=0)
    b = Batch.from_data_list([ds[i] for i in range(batch)]).to('cuda')
    return model, b


def prepare(name, form, model, b, warm=3):
    """A new optimiser on the model: `warm` full steps (the first creates the state), then one forward + backward whose gradients
    the timed step() calls reuse."""
    import torch
    opt = make_optimiser(name, form, model)
    for i in range(warm + 1):
        opt.zero_grad()
        loss = model(b)[1]
        loss.backward()
        if i < warm:
            opt.step()
    if form == 'one_launch':
        assert opt._fast_ready(), 'one-launch path not ready'
    for _ in range(3):
        opt.step()                # (warm the exact call)
    torch.cuda.synchronize()
    return opt


def measure(opt, reps):
    import torch
    t0 = time.perf_counter()
    for _ in range(reps):
        opt.step()
    enq = (time.perf_counter() - t0) / reps * 1e6
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        opt.step()
        e.record()
    torch.cuda.synchronize()
    dev = [s.elapsed_time(e) * 1e3 for s, e in ev]
    return enq, statistics.median(dev)


def run(args):
    import torch
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    torch.autograd.set_multithreading_enabled(False)
    rows = []
    for batch in args.batches:
        model, b = setup(batch)
        for name in OPTIMS:
            for form in FORMS:
                opt = prepare(name, form, model, b)
                if args.trace_steps:
                    torch.cuda._sleep(1000)
                    for _ in range(args.trace_steps):
                        opt.step()
                    torch.cuda._sleep(1000)
                    torch.cuda.synchronize()
                    rows.append(dict(batch=batch, optim=name, form=form))
                    continue
                enq, dev = measure(opt, args.reps)
                rows.append(dict(batch=batch, optim=name, form=form, enqueue_us=round(enq, 1), device_us=round(dev, 1)))
                print(json.dumps(rows[-1]), flush=True)
        del model, b
    out = dict(tool='tools/optim_step_bench.py', device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=args.reps,
               trace_steps=args.trace_steps, rows=rows)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)
    return out


def short(name):
    name = name.replace('at::native::(anonymous namespace)::', '').replace('void ', '')
    return name if len(name) <= 200 else name[:197] + '...'


def parse_trace(path, steps, order_file):
    """Kernels between consecutive spin_kernel pairs, per form (the order of the forms is read from the run's --out file)."""
    with open(path) as f:
        recs = sorted(csv.DictReader(f), key=lambda r: int(r['Dispatch_Id']))
    forms = json.load(open(order_file))['rows']
    spans, cur = [], None
    for r in recs:
        if 'spin_kernel' in r['Kernel_Name']:
            if cur is None:
                cur = collections.Counter()
            else:
                spans.append(cur)
                cur = None
        elif cur is not None:
            cur[r['Kernel_Name']] += 1
    assert len(spans) == len(forms), (len(spans), len(forms))
    rows = []
    for f_, c in zip(forms, spans):
        total = sum(c.values())
        rows.append(dict(f_, launches_per_step=total / steps,
                         kernels={short(k): n / steps for k, n in c.most_common()}))
    return rows


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--batches', type=int, nargs='+', default=[32, 4])
    p.add_argument('--reps', type=int, default=200)
    p.add_argument('--trace-steps', type=int, default=0, help='profiler run: delimited step() calls per form, no timing')
    p.add_argument('--parse-trace', default=None, help='a rocprofv3 *_kernel_trace.csv of a --trace-steps run')
    p.add_argument('--order', default=None, help='with --parse-trace: the --out file of the --trace-steps run')
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if args.parse_trace:
        rows = parse_trace(args.parse_trace, args.trace_steps, args.order)
        text = json.dumps(dict(tool='tools/optim_step_bench.py --parse-trace', trace_steps=args.trace_steps, rows=rows), indent=1)
        print(text)
        if args.out:
            with open(args.out, 'w') as f:
                f.write(text)
        return
    run(args)


if __name__ == '__main__':
    main()
