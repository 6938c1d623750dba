"""Which kernel a shape gets, without a GPU.  ln3diff_amd/csrc/kernel_plan.h holds the bf16 GEMM's tile table and the two dispatch
decisions as pure functions; a host program compiled from it with the build's compiler prints the table and both plans over a grid:
  (a) every grid point equals what the dispatch code before the plan header decided (tests/golden/kernel_plan_grid.npz, recorded from
      that code with its launches replaced by their tile ids - profiles/kernel_plan_refactor.md);
  (b) the grid reaches every outcome: each tile unforced, both cross-attention tiles, both fall-backs to 256x256, all nine attention
      kernels, both error codes;
  (c) tests/kernel_refs.py::TILE_SHAPE is the table's tile sizes;
and the benchmark's GEMM shapes are pinned to their tiles at 256 CUs, so that a retuned threshold shows up as a diff here."""
import os
import subprocess

import numpy as np
import pytest

import kernel_refs as kr
from conftest import ROOT

GRID = os.path.join(ROOT, 'tests', 'golden', 'kernel_plan_grid.npz')
BAD_ARG, UNSUPPORTED = -1, -3
ATTN_KERNELS = ['short', 'kres', 'stream', 'ring64_occ4', 'ring64_occ2', 'ring80', 'ring80_t72', 'ring128', 'ring128_t72']   # codes of the fixture
# GEMM cases of the grid: (epilogue, how the LN3D_EPI_HEADS arguments are set)
#   heads64: head_dim 64, tokens 32 - the split is stageable wherever M % 32 == 0 and N % 64 == 0; heads4: head_dim 4, never stageable;
#   norm: heads64 with a qk_norm weight, the result is the tile or LN3D_ERR_UNSUPPORTED
GEMM_CASES = ['F32', 'BF16', 'GELU_ERF', 'GATE_RES', 'HEADS heads64', 'HEADS heads4', 'SILU', 'HEADS norm']

# The grid driver: reads the axes (one `name v v v ...` line each) and prints one integer per point, last axis fastest.  The three
# decisions come from the adaptor in front of it, so the same driver ran over the dispatch code this header replaced.
DRIVER = r'''
#include <stdio.h>
#include <string.h>
#include <vector>
#include <map>
#include <string>
static std::map<std::string, std::vector<int>> read_axes(const char* path) {
  std::map<std::string, std::vector<int>> ax;
  FILE* f = fopen(path, "r");
  char line[4096];
  while (f && fgets(line, sizeof line, f)) {
    char* tok = strtok(line, " \n");
    if (!tok) continue;
    std::vector<int>& v = ax[tok];
    while ((tok = strtok(nullptr, " \n"))) v.push_back(atoi(tok));
  }
  if (f) fclose(f);
  return ax;
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  auto ax = read_axes(argv[1]);
  print_table();
  printf("gemm\n");
  for (int M : ax["M"]) for (int N : ax["N"]) for (int K : ax["K"]) for (int c : ax["gemm_case"]) for (int al : ax["aligned"])
    for (int cus : ax["cus"]) for (int fo : ax["forced"]) printf("%d\n", gemm_decision(M, N, K, c, al, cus, fo));
  printf("cross\n");
  for (int M : ax["cross_M"]) for (int N : ax["cross_N"]) for (int cus : ax["cus"]) for (int fo : ax["forced"])
    printf("%d\n", cross_decision(M, N, cus, fo));
  printf("fusable\n");
  for (int M : ax["M"]) for (int N : ax["N"]) for (int cus : ax["cus"]) for (int fo : ax["forced"]) printf("%d\n", fusable_decision(M, N, cus, fo));
  printf("attn\n");
  for (int Dh : ax["Dh"]) for (int dt : ax["Dh_true"]) for (int Nk : ax["Nk"]) for (int kp : ax["Nk_pad_mode"]) for (int Nq : ax["Nq"])
    for (int qp : ax["Nq_pad_mode"]) for (int BH : ax["BH"]) for (int ca : ax["causal"]) for (int cus : ax["attn_cus"]) {
      // Dh_true -1 = Dh; key padding: 0 = Nk itself, 1 = up to 64, 2 = 64 more than that; query padding: 0 = Nq, 1 = up to 256
      const int k64 = (Nk + 63) / 64 * 64;
      printf("%d\n", attn_decision(Dh, dt < 0 ? Dh : dt, Nq, qp ? (Nq + 255) / 256 * 256 : Nq, Nk, kp == 0 ? Nk : (kp == 1 ? k64 : k64 + 64), BH, ca, cus));
    }
  return 0;
}
'''

ADAPTOR = r'''
#include <stdio.h>
#include <stdlib.h>
#include "kernel_plan.h"
static void print_table() {
  for (const Ln3dGemmTile& t : ln3d_gemm_tiles)
    printf("tile %d %d %d %d %d %d %d %d %g %d %u %s\n", t.id, t.kind, t.nw, t.wgt, t.ni, t.nj, t.bf, t.bt, t.speed, (int)t.head_row, t.epis, t.name);
}
static int gemm_decision(int M, int N, int K, int c, int aligned, int cus, int forced) {
  static const int epi[8] = {LN3D_EPI_F32, LN3D_EPI_BF16, LN3D_EPI_GELU_ERF, LN3D_EPI_GATE_RES, LN3D_EPI_HEADS, LN3D_EPI_HEADS, LN3D_EPI_SILU, LN3D_EPI_HEADS};
  const bool heads64 = (c == 4 || c == 7) && (M % 32) == 0 && (N % 64) == 0;
  const Ln3dGemmTile& t = ln3d_gemm_tiles[ln3d_plan_gemm(M, N, K, epi[c], heads64, aligned != 0, cus, forced)];
  if (c == 7 && !(t.head_row && heads64)) return LN3D_ERR_UNSUPPORTED;     // what ln3d_gemm_bf16 makes of the head_row flag
  return t.id;
}
static int cross_decision(int M, int N, int cus, int forced) { return ln3d_gemm_tiles[ln3d_plan_gemm(M, N, 1024, LN3D_EPI_CROSS_ATTN, false, true, cus, forced)].id; }
static int fusable_decision(int M, int N, int cus, int forced) {        // ln3d_gemm_heads_norm_fusable(M, N, 32, 64, 64)
  if ((M % 32) != 0 || (N % 64) != 0) return 0;
  return ln3d_gemm_tiles[ln3d_plan_gemm(M, N, 0, LN3D_EPI_HEADS, true, true, cus, forced)].head_row ? 1 : 0;
}
static int attn_decision(int Dh, int Dh_true, int Nq, int Nq_pad, int Nk, int Nk_pad, int BH, int causal, int cus) {
  const int k = ln3d_plan_attention(Dh, Dh_true, Nq, Nq_pad, Nk, Nk_pad, BH, causal != 0, cus);
  switch (k) {                                                            // the fixture's codes, in ATTN_KERNELS' order
    case LN3D_ATTN_SHORT: return 0;
    case LN3D_ATTN_KRES: return 1;
    case LN3D_ATTN_STREAM: return 2;
    case LN3D_ATTN_RING64_OCC4: return 3;
    case LN3D_ATTN_RING64_OCC2: return 4;
    case LN3D_ATTN_RING80: return 5;
    case LN3D_ATTN_RING80_T72: return 6;
    case LN3D_ATTN_RING128: return 7;
    case LN3D_ATTN_RING128_T72: return 8;
    default: return k;
  }
}
'''
AXES = ['M', 'N', 'K', 'gemm_case', 'aligned', 'cus', 'forced', 'cross_M', 'cross_N', 'Dh', 'Dh_true', 'Nk', 'Nk_pad_mode', 'Nq', 'Nq_pad_mode', 'BH',
        'causal', 'attn_cus']
SHAPES = {'gemm': ['M', 'N', 'K', 'gemm_case', 'aligned', 'cus', 'forced'], 'cross': ['cross_M', 'cross_N', 'cus', 'forced'],
          'fusable': ['M', 'N', 'cus', 'forced'],
          'attn': ['Dh', 'Dh_true', 'Nk', 'Nk_pad_mode', 'Nq', 'Nq_pad_mode', 'BH', 'causal', 'attn_cus']}


def run_probe(workdir, adaptor, axes, flags=()):
    """compile adaptor + DRIVER on the host side with the build's compiler, run it over `axes`: (table lines, {section: int array})"""
    workdir = str(workdir)
    with open(os.path.join(workdir, 'probe.cpp'), 'w') as f:
        f.write(adaptor + DRIVER)
    with open(os.path.join(workdir, 'axes.txt'), 'w') as f:
        f.write(''.join('%s %s\n' % (k, ' '.join(str(int(v)) for v in axes[k])) for k in AXES))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-O1', '-I', os.path.join(ROOT, 'ln3diff_amd', 'csrc'), *flags, 'probe.cpp', '-o', 'probe'],
                          cwd=workdir)
    lines = subprocess.check_output([os.path.join(workdir, 'probe'), 'axes.txt'], cwd=workdir, text=True).split('\n')
    table = [ln.split(' ', 12)[1:] for ln in lines if ln.startswith('tile ')]
    out, at = {}, lines.index('gemm')
    for name, dims in SHAPES.items():
        assert lines[at] == name, (lines[at], name)
        n = int(np.prod([len(axes[d]) for d in dims]))
        out[name] = np.array(lines[at + 1:at + 1 + n], dtype=np.int64).reshape([len(axes[d]) for d in dims])
        at += 1 + n
    return table, out


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    golden = np.load(GRID)
    axes = {k: golden[k] for k in AXES}
    table, got = run_probe(tmp_path_factory.mktemp('kernel_plan'), ADAPTOR, axes)
    tiles = [dict(id=int(r[0]), kind=int(r[1]), nw=int(r[2]), wgt=int(r[3]), ni=int(r[4]), nj=int(r[5]), bf=int(r[6]), bt=int(r[7]),
                  speed=float(r[8]), head_row=bool(int(r[9])), epis=int(r[10]), name=r[11]) for r in table]
    return golden, axes, tiles, got


def test_plan_equals_the_dispatch_it_replaced(plan):
    golden, axes, _, got = plan
    assert list(golden['attn_kernels']) == ATTN_KERNELS and list(golden['gemm_cases']) == GEMM_CASES
    for name, dims in SHAPES.items():
        want = golden[name].astype(np.int64)
        assert want.shape == got[name].shape, name
        bad = np.argwhere(want != got[name])
        assert len(bad) == 0, "%s: %d of %d differ, first at %s: recorded %d, plan %d" % (
            name, len(bad), want.size, {d: int(axes[d][i]) for d, i in zip(dims, bad[0])}, want[tuple(bad[0])], got[name][tuple(bad[0])])


def test_grid_reaches_every_outcome(plan):
    _, axes, tiles, got = plan
    ids = sorted(t['id'] for t in tiles)
    assert ids == [0, 7, 8, 9, 12, 13, 14, 16]
    forced = list(axes['forced'])
    unforced = [i for i, f in enumerate(forced) if f < 0]
    assert len(unforced) == 1 and set(ids) < set(forced) and any(f >= 0 and f not in ids for f in forced)     # none, every id, an unknown one
    gemm = got['gemm']
    plain = gemm[:, :, :, :7]                                                                    # the cases that always return a tile
    assert sorted(np.unique(plain[..., unforced[0]])) == ids, "every tile occurs unforced"
    assert sorted(np.unique(got['cross'][..., unforced[0]])) == [9, 14] and sorted(np.unique(got['cross'])) == [9, 14]
    bf16, gelu, silu = GEMM_CASES.index('BF16'), GEMM_CASES.index('GELU_ERF'), GEMM_CASES.index('SILU')
    ok, off = list(axes['aligned']).index(1), list(axes['aligned']).index(0)
    # 16 -> 7: the unforced pick is the persistent tile where the output is aligned, and the 256x256 ring at the same point where it is not
    moved = (gemm[:, :, :, bf16, ok, :, unforced[0]] == 16) & (gemm[:, :, :, bf16, off, :, unforced[0]] == 7)
    assert moved.any() and ((gemm[:, :, :, gelu, ok, :, unforced[0]] == 16) & (gemm[:, :, :, gelu, off, :, unforced[0]] == 7)).any()
    assert (gemm[:, :, :, :, off] != 16).all()
    # 13 -> 7: only a forced 13 meets an epilogue the 4-wave 256x256 tile is not instantiated for
    f13 = forced.index(13)
    assert (gemm[:, :, :, silu, :, :, f13] == 7).all() and (gemm[:, :, :, bf16, :, :, f13] == 13).all()
    assert (plain[..., unforced[0]] == 13).any()
    assert (gemm[:, :, :, GEMM_CASES.index('HEADS norm')] == UNSUPPORTED).any() and set(np.unique(got['fusable'])) == {0, 1}
    assert set(np.unique(plain[..., [i for i, f in enumerate(forced) if f >= 0 and f not in ids]])) == {0}   # an unknown id: the 128x128 kernel
    assert sorted(np.unique(got['attn'])) == [UNSUPPORTED, BAD_ARG] + list(range(len(ATTN_KERNELS)))


def test_python_tile_shapes_equal_the_table(plan):
    _, _, tiles, _ = plan
    by_id = {t['id']: (t['bf'], t['bt']) for t in tiles}
    want = {'auto': by_id[0], 's': by_id[0]}
    want.update({'x%d' % i: s for i, s in by_id.items() if i != 0})
    assert kr.TILE_SHAPE == want
    for t in tiles:
        assert (t['bf'], t['bt']) == (32 * t['ni'] * (t['nw'] // t['wgt']), 32 * t['nj'] * t['wgt']), t['name']
        assert t['head_row'] == (t['kind'] == 1 and t['ni'] == 2), t['name']


# tokens x features x K, case of GEMM_CASES -> tile id at 256 CUs, nothing forced, aligned outputs
BENCH_SHAPES = {
    'T23D QKV': ((12288, 3072, 1024, 'HEADS heads64'), 12),
    'T23D fc1': ((12288, 4096, 1024, 'GELU_ERF'), 16),
    'T23D fc2': ((12288, 1024, 4096, 'GATE_RES'), 9),
    'T23D output projection': ((12288, 1024, 1024, 'GATE_RES'), 9),
    'half-batch to_q': ((6144, 1024, 1024, 'BF16'), 14),
    'I23D QKV': ((49152, 3072, 1024, 'HEADS heads64'), 12),
    'I23D fc1': ((49152, 4096, 1024, 'GELU_ERF'), 16),
    'I23D fc2': ((49152, 1024, 4096, 'GATE_RES'), 13),
}


def test_benchmark_shapes_keep_their_tiles(plan):
    _, axes, _, got = plan
    at = lambda name, v: list(axes[name]).index(v)                                               # noqa: E731
    for what, ((M, N, K, case), tile) in BENCH_SHAPES.items():
        i = (at('M', M), at('N', N), at('K', K), GEMM_CASES.index(case), at('aligned', 1), at('cus', 256), at('forced', -1))
        assert got['gemm'][i] == tile, (what, int(got['gemm'][i]), tile)
