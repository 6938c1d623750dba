"""Host-side cost of enqueueing one denoiser forward (python + ctypes + HIP launch calls) vs its device time: how many lanes one
python thread can feed.  t23d: DiT-L/2 as the EulerEDM loop calls it (prepared context and timesteps, c_in, [uc ; c]); i23d:
DiT-PixArt-L/2 as the flow-matching loop calls it (prepared context, [c ; uc]).
usage: python tools/host_launch_cost.py [network_batch] [--workload t23d|i23d] [--tree OTHER_CHECKOUT]"""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument('batch', nargs='?', type=int, default=16)
ap.add_argument('--workload', default='t23d', choices=['t23d', 'i23d'])
ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='checkout to import bench.py and ln3diff_amd from')
ap.add_argument('--forwards', type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import torch
import bench
dev = torch.device('cuda', 0)
Bn = args.batch
t = torch.full((Bn,), 500.0, device=dev)
if args.workload == 't23d':
    dit, _ = bench.build_models(dev, 'DiT-L/2', 'DiT2-L/2')
    x = torch.randn(Bn // 2, 12, 32, 32, device=dev)
    ctx = torch.cat([torch.zeros(Bn // 2, 77, 768, device=dev), torch.randn(Bn // 2, 77, 768, device=dev)])
    kw = dict(context_cache=dit.prepare_context(ctx), in_scale=torch.ones(Bn, device=dev), mod_cache=(dit.prepare_timesteps(torch.full((4, Bn), 500.0)), 0))
else:
    dit = bench.build_i23d(dev, 'DiT-PixArt-L/2')
    x = torch.randn(Bn, 12, 32, 32, device=dev)
    cond = lambda *shape: torch.cat([torch.randn(Bn // 2, *shape, device=dev), torch.zeros(Bn // 2, *shape, device=dev)])
    kw = dict(context_cache=dit.prepare_context({'crossattn': cond(256, 2048), 'vector': cond(768)}))
    t = t / 1000
for _ in range(3):
    dit(x, t, **kw)
torch.cuda.synchronize()
n = args.forwards
t0 = time.perf_counter()
for _ in range(n):
    dit(x, t, **kw)
t_host = (time.perf_counter() - t0) / n
torch.cuda.synchronize()
t_all = (time.perf_counter() - t0) / n
print("%s network batch %d: host enqueue %.3f ms per forward, device %.2f ms per forward (%d forwards back to back)" % (args.workload, Bn, t_host * 1e3, t_all * 1e3, n))
