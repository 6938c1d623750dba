"""Times the mesh smoothing of include/ln3d_meshsmooth.h on the level set of a 192^3 grid and writes profiles/mesh_smooth.md.

    python tools/mesh_smooth_bench.py [--out profiles/mesh_smooth.md] [--iters 20] [--grid 192] [--commit SHA]

The field is the one of tools/mesh_clean_bench.py and profiles/mesh_simplify.md.  Per simplify_cell 0 (full density) and 3: the adjacency build
(mesh._adjacency: two kernels around torch's unique, sort and searchsorted, one read-back) and smooth_mesh at 10 iterations (the finiteness
read-back, the adjacency, 20 passes) with a host clock around calls that end synchronised; one pass (ln3d_smooth_step) with device events
around `iters` back-to-back ping-pong calls after 3 warm-up calls - at these sizes that is launch throughput, an upper bound on the kernel's
own time; an iteration is two passes.  Before anything is reported the device result is compared with the numpy reference of
tests/mesh_smooth_refs.py on a small mesh."""
import argparse
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_smooth.md'))
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--grid', type=int, default=192)
    ap.add_argument('--commit', default=None, help="the commit the measured tree sits on (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_smooth_bench measures on the GPU; there is none here")
    import numpy as np
    import mesh_smooth_refs as R
    from mesh_clean_bench import events, clocked, field
    from ln3diff_amd import ops
    from ln3diff_amd.mesh import SMOOTH_LAMBDA, SMOOTH_MU, _adjacency, extract_isosurface, smooth_mesh
    dev, G, thr, it = 'cuda', args.grid, 10.0, args.iters

    # ---- the same code on a mesh small enough for the numpy reference
    sv, sf = extract_isosurface(torch.from_numpy(field(16)).to(dev), thr)
    got = smooth_mesh(sv, sf, 3)[0].cpu().numpy()
    if not np.array_equal(R.bits(got), R.bits(R.smooth(sv.cpu().numpy(), sf.cpu().numpy(), 3))):
        raise SystemExit("the device result differs from the reference's: nothing is reported")

    sigma = torch.from_numpy(field(G)).to(dev)
    rows = []
    for cell in (0.0, 3.0):
        verts, faces = extract_isosurface(sigma, thr, simplify_cell=cell)
        nv, nf = verts.shape[0], faces.shape[0]
        start, nbr, pinned = _adjacency(faces, nv)
        free = int(((pinned == 0) & (start[1:] > start[:-1])).sum())
        t_adj = clocked(lambda: _adjacency(faces, nv), it)
        bufs = [verts.clone(), torch.empty_like(verts)]
        state = {'k': 0}

        def one_pass():
            k = state['k']
            ops.smooth_step(bufs[k], start, nbr, pinned, SMOOTH_LAMBDA if k == 0 else SMOOTH_MU, bufs[1 - k], check=False)
            state['k'] = 1 - k
        t_pass = events(one_pass, 2 * it)
        t_all = clocked(lambda: smooth_mesh(verts, faces, 10, check=False), max(3, it // 2))
        t_checked = clocked(lambda: smooth_mesh(verts, faces, 10), max(3, it // 2))
        rows.append((cell, nv, nf, nbr.shape[0] // 2, free, t_adj, t_pass, 2 * t_pass, t_all, t_checked))

    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True, timeout=60).stdout.strip()
        except Exception:                        # noqa: BLE001
            commit = ''
        commit = commit or 'an unknown commit (no git checkout here)'
    with open(args.out, 'w') as f:
        f.write("# Mesh smoothing: measured times\n\n")
        f.write(f"`python tools/mesh_smooth_bench.py --iters {it} --grid {G}` on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}, "
                f"on top of commit {commit}.  The adjacency build and smooth_mesh: a host clock around {it} / {max(3, it // 2)} calls that end "
                f"synchronised, after 3 warm-up calls.  One pass: device events around {2 * it} back-to-back ln3d_smooth_step calls between two "
                "buffers after 3 warm-up calls - launch throughput at these sizes, an upper bound on the kernel's own time; an iteration is a "
                "lambda pass and a mu pass.\n\n")
        f.write(f"Field: the five-blob field rescaled to {G}^3 plus Gaussian noise (sigma 2) and 2000 single-node specks, level {thr:g}, marching "
                "cubes, no clean-up (the mesh of profiles/mesh_simplify.md), at full density and simplified to cell 3.  On a small mesh the "
                "device's coordinates after 3 iterations equal the numpy reference's bit for bit (checked by this run).\n\n")
        f.write("| simplify_cell | vertices | faces | edges | free vertices | adjacency build ms | one pass ms | one iteration ms | "
                "smooth_mesh, 10 iterations, check=False ms | the same with the face-index check ms |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for cell, nv, nf, ne, free, t_adj, t_pass, t_iter, t_all, t_checked in rows:
            f.write(f"| {cell:g} | {nv} | {nf} | {ne} | {free} | {t_adj:.3f} | {t_pass:.4f} | {t_iter:.4f} | {t_all:.3f} | {t_checked:.3f} |\n")
        f.write("\nFree vertices are those a pass moves: not an end of a boundary edge and with at least one neighbour.  Vertex clustering drops "
                "collapsed and duplicate faces, and wherever that leaves an edge with a single face both its ends are pinned: compare the "
                "free counts of the two rows.  Smoothing a simplified mesh moves only its free vertices.\n")
        f.write("\nNot measured: kernel-level counters, the kernel's own time apart from launch throughput, other iteration counts, a sampled "
                "latent's own level set, clock and power during the run.  Nothing is gated on these numbers.\n")
    print(open(args.out).read())


if __name__ == "__main__":
    main()
